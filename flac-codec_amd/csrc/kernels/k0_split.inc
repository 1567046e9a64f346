// k0_split.inc -- K0: channel split + OR of every candidate (wasted bits), candidate info.
// Part of flacenc_gpu.hip (one translation unit; included inside its anonymous namespace).

// ---------------------------------------------------------------------------------
// K0: de-interleave (audio.rs:190-199)  [pcm_frame][ch] -> [flac_frame][ch][ldb]
// also used to re-stride planar input whose block size is not a multiple of 4
// ---------------------------------------------------------------------------------
// the frame length rule of frame_len() (common.inc) for the kernels that take no Params; frame_n: a ragged batch's table
__device__ __forceinline__ uint32_t k0_frame_len(const uint32_t *frame_n, uint32_t frame, uint32_t n_frames, uint32_t last_len,
                                                 uint32_t block_size) {
    if (frame_n) return frame_n[frame];
    return (frame + 1 == n_frames) ? last_len : block_size;
}

__global__ void __launch_bounds__(WG) k_deinterleave(const int32_t *__restrict__ in,
                                                     int32_t *__restrict__ out, uint32_t channels,
                                                     uint32_t block_size, uint32_t ldb,
                                                     uint32_t n_frames, uint32_t last_len,
                                                     int planar_in, uint32_t f0, const uint32_t *__restrict__ frame_n) {
    const uint32_t frame = f0 + blockIdx.y;
    const uint32_t n = k0_frame_len(frame_n, frame, n_frames, last_len, block_size);
    const size_t in_base = (size_t)frame * block_size * channels;
    int32_t *o = out + (size_t)frame * channels * ldb;
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        for (uint32_t c = 0; c < channels; c++) {
            int32_t v = planar_in ? in[in_base + (size_t)c * n + i]
                                  : in[in_base + (size_t)i * channels + c];
            o[(size_t)c * ldb + i] = v;
        }
    }
}

// stereo fast path: both channels of an interleaved pair in one 8-byte load.  Also ORs together
// all samples of L, R, mid, side per frame (orbits[frame*ncand + c]): trailing zeros of the OR =
// wasted bits (encode.rs:2878-2898), OR == 0 = all-zero candidate.
__global__ void __launch_bounds__(WG) k_deinterleave2(const int2 *__restrict__ in,
                                                      int32_t *__restrict__ out,
                                                      uint32_t block_size, uint32_t ldb,
                                                      uint32_t n_frames, uint32_t last_len,
                                                      uint32_t *__restrict__ orbits, uint32_t ncand,
                                                      uint32_t f0, unsigned long long *__restrict__ abs_sums,
                                                      const uint32_t *__restrict__ frame_n) {
    const uint32_t frame = f0 + blockIdx.y;
    const uint32_t n = k0_frame_len(frame_n, frame, n_frames, last_len, block_size);
    const int2 *src = in + (size_t)frame * block_size;
    int32_t *o = out + (size_t)frame * 2 * ldb;
    uint32_t ol = 0, orr = 0, om = 0, os = 0;
    // abs_sums (fast channel choice, encode.rs:2463-2674): sum |l|, |r|, |mid|, |side| of the frame while the
    // samples pass through anyway.  64-bit partial sums like the reference's (encode.rs:2463-2674 sums in u64): at
    // 29..31 bits per sample a lane's handful of |side| values already wraps a u32
    uint64_t al = 0, ar = 0, am = 0, as = 0;
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        int2 v = src[i];
        o[i] = v.x;
        o[ldb + i] = v.y;
        const int32_t m = combine(1, v.x, v.y), sd = combine(2, v.x, v.y);
        ol |= (uint32_t)v.x;
        orr |= (uint32_t)v.y;
        om |= (uint32_t)m;
        os |= (uint32_t)sd;
        if (abs_sums) {
            al += uabs(v.x);
            ar += uabs(v.y);
            am += uabs(m);
            as += uabs(sd);
        }
    }
    if (abs_sums) {
        const uint64_t tl = wave_sum_u64(al), tr = wave_sum_u64(ar), tm = wave_sum_u64(am), ts = wave_sum_u64(as);
        if ((threadIdx.x & 63) == 0) {
            unsigned long long *a = abs_sums + (size_t)frame * 4;
            atomicAdd(&a[0], (unsigned long long)tl);
            atomicAdd(&a[1], (unsigned long long)tr);
            atomicAdd(&a[2], (unsigned long long)tm);
            atomicAdd(&a[3], (unsigned long long)ts);
        }
    }
    ol = wave_or_u32(ol);
    orr = wave_or_u32(orr);
    om = wave_or_u32(om);
    os = wave_or_u32(os);
    if ((threadIdx.x & 63) == 0) {
        uint32_t *ob = orbits + (size_t)frame * ncand;
        if (ol) atomicOr(&ob[0], ol);
        if (orr) atomicOr(&ob[1], orr);
        if (ncand == 4) {
            if (om) atomicOr(&ob[2], om);
            if (os) atomicOr(&ob[3], os);
        }
    }
}

// the same ORs from the planar buffer (every layout but interleaved stereo)
__global__ void __launch_bounds__(WG) k_orbits(Params p, uint32_t *__restrict__ orbits) {
    const uint32_t frame = p.f0 + blockIdx.y;
    const uint32_t n = frame_len(p, frame);
    const int32_t *base = p.planar + (size_t)frame * p.channels * p.ldb;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        if (p.stereo4) {
            const int32_t l = base[i], r = base[p.ldb + i];
            acc[0] |= (uint32_t)l;
            acc[1] |= (uint32_t)r;
            acc[2] |= (uint32_t)combine(1, l, r);
            acc[3] |= (uint32_t)combine(2, l, r);
        } else {
#pragma unroll
            for (uint32_t c = 0; c < 8; c++)
                if (c < p.channels) acc[c] |= (uint32_t)base[(size_t)c * p.ldb + i];
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        const uint32_t v = wave_or_u32(acc[c]);
        if ((threadIdx.x & 63) == 0 && c < p.ncand && v) atomicOr(&orbits[(size_t)frame * p.ncand + c], v);
    }
}

// interleaved input with C independent channels (ncand == C): one pass splits the channels into
// planar rows and ORs every channel's samples (orbits -> wasted bits / all-zero)
template <int C>
__global__ void __launch_bounds__(WG) k_deinterleave_n(const int32_t *__restrict__ in,
                                                       int32_t *__restrict__ out, uint32_t block_size,
                                                       uint32_t ldb, uint32_t n_frames, uint32_t last_len,
                                                       uint32_t *__restrict__ orbits, uint32_t f0,
                                                       const uint32_t *__restrict__ frame_n) {
    const uint32_t frame = f0 + blockIdx.y;
    const uint32_t n = k0_frame_len(frame_n, frame, n_frames, last_len, block_size);
    const int32_t *src = in + (size_t)frame * block_size * C;
    int32_t *o = out + (size_t)frame * C * ldb;
    uint32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0;
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        int32_t v[C];
        if constexpr (C % 4 == 0) {
#pragma unroll
            for (int q = 0; q < C / 4; q++) {
                const int4 t = reinterpret_cast<const int4 *>(src + (size_t)i * C)[q];
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
        } else if constexpr (C % 2 == 0) {
#pragma unroll
            for (int q = 0; q < C / 2; q++) {
                const int2 t = reinterpret_cast<const int2 *>(src + (size_t)i * C)[q];
                v[2 * q] = t.x; v[2 * q + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = src[(size_t)i * C + c];
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            o[(size_t)c * ldb + i] = v[c];
            acc[c] |= (uint32_t)v[c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t v = wave_or_u32(acc[c]);
        if ((threadIdx.x & 63) == 0 && v) atomicOr(&orbits[(size_t)frame * C + c], v);
    }
}

// Interleaved input at its STREAM width: little-endian samples of BYTES = ceil(bps / 8) bytes, the
// bytes FlacByteWriter::write receives (encode.rs:359) and update_md5 hashes (encode.rs:1292-1318,
// byteorder.rs:60-72).  The samples are widened here instead of on the host, so that a stream
// crosses PCIe at 2 or 3 bytes per sample.  A lane takes 4 PCM frames = C * BYTES dwords (the host
// checks that a block is a whole number of dwords) and writes C planar 16-byte runs; the ORs of
// every candidate's samples are accumulated as in k_deinterleave2 / k_deinterleave_n.
template <int C, int BYTES>
__global__ void __launch_bounds__(WG) k_deinterleave_packed(const uint32_t *__restrict__ in,
                                                            int32_t *__restrict__ out, uint32_t block_size,
                                                            uint32_t ldb, uint32_t n_frames, uint32_t last_len,
                                                            uint32_t *__restrict__ orbits, uint32_t f0,
                                                            unsigned long long *__restrict__ abs_sums) {
    constexpr int ND = C * BYTES;                // dwords per group of 4 PCM frames
    constexpr bool S4 = C == 2;                  // L, R, mid, side candidates (bps <= 24 < 32)
    constexpr int NC = S4 ? 4 : C;
    const uint32_t frame = f0 + blockIdx.y;
    const uint32_t n = (frame + 1 == n_frames) ? last_len : block_size;   // (a ragged batch's samples are int32: it never comes this way)
    const uint32_t *src = in + (size_t)frame * ((size_t)block_size * ND / 4);
    int32_t *o = out + (size_t)frame * C * ldb;
    uint32_t acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0;
    uint64_t ab[4] = {0, 0, 0, 0};   // abs sums of L, R, mid, side (stereo, fast channel choice; see k_deinterleave2)
    for (uint32_t g = blockIdx.x * WG + threadIdx.x; 4 * g < n; g += gridDim.x * WG) {
        uint32_t w[ND + 1];
        const uint32_t *q = src + (size_t)g * ND;   // reads past a short last frame stay inside the buffer's slack
        if constexpr (ND % 4 == 0) {
#pragma unroll
            for (int k = 0; k < ND / 4; k++) {
                const uint4 t = reinterpret_cast<const uint4 *>(q)[k];
                w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w;
            }
        } else if constexpr (ND % 2 == 0) {
#pragma unroll
            for (int k = 0; k < ND / 2; k++) {
                const uint2 t = reinterpret_cast<const uint2 *>(q)[k];
                w[2 * k] = t.x; w[2 * k + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < ND; k++) w[k] = q[k];
        }
        w[ND] = 0;
        int32_t v[4][C];
#pragma unroll
        for (int s = 0; s < 4 * C; s++) {
            constexpr int SH = 32 - 8 * BYTES;
            const int b = s * BYTES, d = b / 4, sh = (b % 4) * 8;
            const uint32_t raw = sh ? __funnelshift_r(w[d], w[d + 1], sh) : w[d];   // bytes b .. b+3
            v[s / C][s % C] = (int32_t)(raw << SH) >> SH;                             // sign-extend BYTES bytes
        }
        const uint32_t i0 = 4 * g;
#pragma unroll
        for (int c = 0; c < C; c++) {
            if (i0 + 3 < n) {
                *reinterpret_cast<int4 *>(o + (size_t)c * ldb + i0) = make_int4(v[0][c], v[1][c], v[2][c], v[3][c]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (i0 + k < n) o[(size_t)c * ldb + i0 + k] = v[k][c];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) {
                if constexpr (S4) {
                    const int32_t m = combine(1, v[k][0], v[k][1]), sd = combine(2, v[k][0], v[k][1]);
                    acc[0] |= (uint32_t)v[k][0];
                    acc[1] |= (uint32_t)v[k][1];
                    acc[2] |= (uint32_t)m;
                    acc[3] |= (uint32_t)sd;
                    if (abs_sums) {
                        ab[0] += uabs(v[k][0]);
                        ab[1] += uabs(v[k][1]);
                        ab[2] += uabs(m);
                        ab[3] += uabs(sd);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < C; c++) acc[c] |= (uint32_t)v[k][c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const uint32_t t = wave_or_u32(acc[c]);
        if ((threadIdx.x & 63) == 0 && t) atomicOr(&orbits[(size_t)frame * NC + c], t);
    }
    if constexpr (S4) {
        if (abs_sums) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint64_t t = wave_sum_u64(ab[c]);
                if ((threadIdx.x & 63) == 0) atomicAdd(&abs_sums[(size_t)frame * 4 + c], (unsigned long long)t);
            }
        }
    }
}

// per (frame, candidate): activity, wasted bits, effective bps (encode.rs:2870-2898)
// abs_sums != nullptr (stereo, fast channel choice): K0 summed |l|, |r|, |mid|, |side| per frame; the choice
// of correlate_channels (encode.rs:2506-2514 / 2600-2607: first minimum in the reference's candidate order) is
// made here instead of by a k_stereo_stats pass over the rows
__global__ void __launch_bounds__(WG) k_candinfo(Params p, const uint32_t *__restrict__ orbits,
                                                 const unsigned long long *__restrict__ abs_sums) {
    const uint32_t idx = p.f0 * p.ncand + blockIdx.x * WG + threadIdx.x;
    if (idx >= (p.f0 + p.fcount) * p.ncand) return;
    const uint32_t cand = idx % p.ncand;
    bool active = p.cinfo[idx].active;
    if (abs_sums && p.stereo4 && !p.exhaustive) {
        const uint32_t frame = idx / p.ncand;
        const unsigned long long *a = abs_sums + (size_t)frame * 4;
        const uint64_t ls = a[0], rs = a[1], ms = a[2], ss = a[3];
        uint8_t assign;
        if (p.mid_side) {
            const uint64_t tot[4] = {ls + rs, ls + ss, ss + rs, ms + ss};
            int b = 0;
            for (int i = 1; i < 4; i++)
                if (tot[i] < tot[b]) b = i;
            assign = b == 0 ? FLACGPU_ASSIGN_INDEPENDENT : b == 1 ? FLACGPU_ASSIGN_LEFT_SIDE
                   : b == 2 ? FLACGPU_ASSIGN_SIDE_RIGHT : FLACGPU_ASSIGN_MID_SIDE;
        } else {
            const uint64_t tot[3] = {ls + ss, ss + rs, ls + rs};
            int b = 0;
            for (int i = 1; i < 3; i++)
                if (tot[i] < tot[b]) b = i;
            assign = b == 0 ? FLACGPU_ASSIGN_LEFT_SIDE : b == 1 ? FLACGPU_ASSIGN_SIDE_RIGHT : FLACGPU_ASSIGN_INDEPENDENT;
        }
        active = cand == 0 ? (assign == FLACGPU_ASSIGN_INDEPENDENT || assign == FLACGPU_ASSIGN_LEFT_SIDE)
               : cand == 1 ? (assign == FLACGPU_ASSIGN_INDEPENDENT || assign == FLACGPU_ASSIGN_SIDE_RIGHT)
               : cand == 2 ? (assign == FLACGPU_ASSIGN_MID_SIDE) : (assign != FLACGPU_ASSIGN_INDEPENDENT);
        if (cand == 0) p.finfo[frame].assignment = assign;
    }
    const CandInfo ci = cand_info_from_or(p, cand, orbits[idx], active);
    p.cinfo[idx] = ci;
}
