// pack.inc -- K8 layout, generic K9 k_pack + K10 k_crc, wave-per-subframe frame assembly k_frame64.
#ifndef FRAME_TIMELINE
#define FRAME_TIMELINE 0
#endif
// Part of flacenc_gpu.hip (one translation unit; included inside its anonymous namespace).

// ---------------------------------------------------------------------------------
// Device-side frame assembly (SURVEY.md 8(f) N1).
//   K8  k_layout  frame sizes (header + ceil(body/8) + 2) -> exclusive prefix sum
//   K9  k_pack    one workgroup per (frame, subframe): the subframe's bits are built in LDS
//                 (header, warm-up, LPC parameters by a few lanes; residual codes at bit
//                 offsets from a workgroup prefix scan of the code lengths) and copied to
//                 the frame's position in HBM with a funnel shift; words shared with a
//                 neighbouring subframe / frame are OR-ed atomically (the buffer is zeroed
//                 first, so byte-alignment padding is free)
//   K10 k_crc     CRC-16 of every frame: 256 lanes each fold a slice, partial CRCs are
//                 combined with x^(8*len) mod P multiplications (GF(2) linearity)
// Replaces stream.rs:242-276 (FrameHeader::build + CRC-8), stream.rs:1390-1413,
// 1603-1619, encode.rs:3078-3135 (subframe serialisation), 3834-3907 (residual block),
// 2408-2409 (align + CRC-16).
// ---------------------------------------------------------------------------------
struct HeaderCodes {
    uint32_t bcode, bextra_bits, rcode, rextra_bits, rextra, fn_bytes;
};
__device__ __forceinline__ HeaderCodes header_codes(uint32_t n, uint32_t rate, uint64_t fn) {
    HeaderCodes h;
    h.bextra_bits = 0;
    switch (n) {  // BlockSize::try_from, stream.rs:531-558
    case 192: h.bcode = 1; break;
    case 576: h.bcode = 2; break;
    case 1152: h.bcode = 3; break;
    case 2304: h.bcode = 4; break;
    case 4608: h.bcode = 5; break;
    case 256: h.bcode = 8; break;
    case 512: h.bcode = 9; break;
    case 1024: h.bcode = 10; break;
    case 2048: h.bcode = 11; break;
    case 4096: h.bcode = 12; break;
    case 8192: h.bcode = 13; break;
    case 16384: h.bcode = 14; break;
    case 32768: h.bcode = 15; break;
    default:
        if (n <= 256) { h.bcode = 6; h.bextra_bits = 8; }
        else { h.bcode = 7; h.bextra_bits = 16; }
    }
    h.rextra_bits = 0;
    h.rextra = 0;
    switch (rate) {  // SampleRate::try_from, stream.rs:767-800
    case 88200: h.rcode = 1; break;
    case 176400: h.rcode = 2; break;
    case 192000: h.rcode = 3; break;
    case 8000: h.rcode = 4; break;
    case 16000: h.rcode = 5; break;
    case 22050: h.rcode = 6; break;
    case 24000: h.rcode = 7; break;
    case 32000: h.rcode = 8; break;
    case 44100: h.rcode = 9; break;
    case 48000: h.rcode = 10; break;
    case 96000: h.rcode = 11; break;
    default:
        if (rate % 1000 == 0 && rate / 1000 < 255) { h.rcode = 12; h.rextra_bits = 8; h.rextra = rate / 1000; }
        else if (rate % 10 == 0 && rate / 10 < 65535) { h.rcode = 14; h.rextra_bits = 16; h.rextra = rate / 10; }
        else if (rate < 65535) { h.rcode = 13; h.rextra_bits = 16; h.rextra = rate; }
        else h.rcode = 0;
    }
    h.fn_bytes = fn <= 0x7F ? 1 : fn <= 0x7FF ? 2 : fn <= 0xFFFF ? 3 : fn <= 0x1FFFFF ? 4
               : fn <= 0x3FFFFFF ? 5 : fn <= 0x7FFFFFFFull ? 6 : 7;
    return h;
}
__device__ __forceinline__ uint32_t header_bytes(const HeaderCodes &h) {
    return 4 + h.fn_bytes + h.bextra_bits / 8 + h.rextra_bits / 8 + 1;
}

// frames [p.f0, p.f0 + p.fcount): byte offsets continue from frame_off[p.f0] (0 for the first
// range; written by the previous range's launch otherwise).
// One frame per thread, one workgroup per tile of 1024 frames.  A tile scans its sizes, publishes its byte count
// (PackParams::tile_sync, tagged with the launch's epoch) and adds up the counts of the tiles before it as they appear
// (decoupled look-back: every tile publishes BEFORE it waits, so a waiting tile only ever waits for tiles that are
// running or still to be dispatched; the launcher keeps a launch at <= 256 tiles -- one 1024-thread workgroup per CU,
// half of what is resident at once -- so that whatever order the dispatcher picks, no undispatched tile is ever kept
// out by spinning ones; ADVICE r03).  As ONE workgroup walking 8 (29 for 1152-sample blocks) frames per lane this kernel took 17 (50) us.
__global__ void __launch_bounds__(1024) k_layout(Params p, PackParams q) {
    __shared__ uint64_t wave_tot[16];
    __shared__ uint64_t tile_base;
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint32_t end = p.f0 + p.fcount;
    const uint32_t f = p.f0 + tile * 1024u + tid;
    uint64_t mine = 0;
    if (f < end) {
        const flacgpu_frame_plan fp = p.frame_plan[f];
        HeaderCodes h = header_codes(fp.block_size, q.sample_rate, frame_number_of(q, f));
        mine = header_bytes(h) + ((uint64_t)fp.body_bits + 7) / 8 + 2;
    }
    uint64_t v = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint64_t t = __shfl_up(v, off, 64);
        if ((tid & 63) >= (uint32_t)off) v += t;
    }
    if ((tid & 63) == 63) wave_tot[tid >> 6] = v;
    __syncthreads();
    uint64_t wprefix = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) {
        const uint64_t t = wave_tot[w];
        wprefix += w < (tid >> 6) ? t : 0ull;
        total += t;
    }
    constexpr unsigned long long LOW = (1ull << 40) - 1ull;
    if (tid == 0)
        __hip_atomic_store(&q.tile_sync[tile], ((unsigned long long)q.epoch << 40) | (total & LOW), __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {   // the tiles before this one (<= 64 for 65 536 frames; more take turns)
        uint64_t acc = 0;
        for (uint32_t t = tid; t < tile; t += 64) {
            unsigned long long w;
            uint32_t polls = 0;
            do {
                w = __hip_atomic_load(&q.tile_sync[t], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                // a publish that never comes (a faulted tile, two launches sharing one context's tile words) must not
                // hang the stream: ~seconds of polling, then the kernel aborts and the next HIP call reports it
                if (++polls == (1u << 27)) __builtin_trap();
            } while ((uint32_t)(w >> 40) != q.epoch);
            acc += w & LOW;
        }
        acc = wave_sum_u64(acc);
        if (tid == 0) tile_base = (p.f0 ? q.frame_off[p.f0] : 0ull) + acc;
    }
    __syncthreads();
    const uint64_t prefix = tile_base + wprefix + v - mine;
    if (f < end) {
        if (f != p.f0 || p.f0 == 0) q.frame_off[f] = prefix;
        if (f + 1 == end) q.frame_off[end] = prefix + mine;
    }
}

// zero the part of the output buffer the frames will occupy (16 bytes per lane)
__global__ void __launch_bounds__(WG) k_zero(PackParams q, uint32_t n_frames) {
    const uint64_t total = q.frame_off[n_frames];
    const uint64_t n16 = (total + 15) / 16 + 1;
    uint4 *o = reinterpret_cast<uint4 *>(q.out_words);
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * WG)
        o[i] = make_uint4(0, 0, 0, 0);
}

// OR a field of nbits (<= 32) at bit position pos of an MSB-first bit string held in LDS words
__device__ __forceinline__ void lds_put(uint32_t *sb, uint32_t pos, uint32_t v, uint32_t nbits) {
    if (nbits == 0) return;
    if (nbits < 32) v &= (1u << nbits) - 1u;
    const uint32_t w = pos >> 5, off = pos & 31;
    if (off + nbits <= 32) {
        atomicOr(&sb[w], v << (32 - off - nbits));
    } else {
        const uint32_t lo = off + nbits - 32;  // bits spilling into the next word
        atomicOr(&sb[w], v >> lo);
        atomicOr(&sb[w + 1], v << (32 - lo));
    }
}

// FrameHeader::build (stream.rs:242-276) with its CRC-8 (crc.rs:99-128: x^8 + x^2 + x + 1, so c x^8 = c (x^2 + x + 1) with two
// overflow bits folded once more) written at bit `pos0` of the LDS bit string by ONE lane, from wave-uniform inputs: the bytes
// are gathered in two 64-bit words (no byte array in LDS, no bit-serial CRC loop -- the old header cost its wave a dozen
// dependent LDS round trips and ~250 instructions before the subframe could start) and leave with at most five ORs.
__device__ __forceinline__ uint32_t crc8_byte(uint32_t crc, uint32_t b) {
    const uint32_t c = (crc ^ b) & 0xFFu;
    const uint32_t t = (c << 2) ^ (c << 1) ^ c;   // c (x^2 + x + 1): 10 bits
    const uint32_t h = t >> 8;
    return (t ^ (h << 2) ^ (h << 1) ^ h) & 0xFFu;
}
__device__ __forceinline__ void put_frame_header(uint32_t *fb, uint32_t pos0, const HeaderCodes &hc, uint64_t fn, uint32_t N,
                                                 uint32_t acode, uint32_t pcode) {
    const uint32_t b2 = (hc.bcode << 4) | hc.rcode, b3 = (acode << 4) | (pcode << 1);
    uint32_t crc = crc8_byte(crc8_byte(crc8_byte(crc8_byte(0u, 0xFFu), 0xF8u), b2), b3);   // sync + blocking strategy 0, codes
    lds_put(fb, pos0, 0xFFF80000u | (b2 << 8) | b3, 32);
    uint64_t hi = 0, lo = 0;   // the bytes behind the first four: the first eight of them in hi, the rest in lo (right-aligned)
    uint32_t nb = 0;
    auto add = [&](uint32_t b) {
        b &= 0xFFu;
        crc = crc8_byte(crc, b);
        if (nb < 8) hi = (hi << 8) | b;
        else lo = (lo << 8) | b;
        nb++;
    };
    if (hc.fn_bytes == 1) {
        add((uint32_t)fn);
    } else {  // UTF-8-like frame number, stream.rs:1264-1325
        const uint32_t n = hc.fn_bytes;
        add(((0xFFu << (8 - n)) & 0xFFu) | (uint32_t)(fn >> (6 * (n - 1))));
        for (int b = (int)n - 2; b >= 0; b--) add(0x80u | (uint32_t)((fn >> (6 * b)) & 0x3F));
    }
    if (hc.bextra_bits == 8) add(N - 1);
    else if (hc.bextra_bits == 16) { add((N - 1) >> 8); add(N - 1); }
    if (hc.rextra_bits == 8) add(hc.rextra);
    else if (hc.rextra_bits == 16) { add(hc.rextra >> 8); add(hc.rextra); }
    const uint32_t c8 = crc;
    if (nb < 8) hi = (hi << 8) | c8;
    else lo = (lo << 8) | c8;
    nb++;
    const uint32_t nh = nb < 8 ? nb : 8, nl = nb - nh;   // bytes in hi / lo
    uint32_t pos = pos0 + 32;
    if (nh > 4) {
        lds_put(fb, pos, (uint32_t)(hi >> (8 * (nh - 4))), 32);
        lds_put(fb, pos + 32, (uint32_t)hi, 8 * (nh - 4));
    } else {
        lds_put(fb, pos, (uint32_t)hi, 8 * nh);
    }
    pos += 8 * nh;
    if (nl) lds_put(fb, pos, (uint32_t)lo, 8 * nl);
}

// Generic subframe writer (any block length): residual rows read from HBM (written by k_emit).
// One subframe's bits are written into the MSB-first LDS bit string `sb` (zeroed by the caller, which
// has NOT synchronised yet) starting at bit `base`; `with_header` also writes the frame header at
// bit 0.  Ends WITHOUT a barrier.
__device__ __forceinline__ void pack_subframe(const Params &p, const PackParams &q, uint32_t frame,
                                              uint32_t ch, uint32_t n, uint32_t *sb, uint32_t base,
                                              bool with_header, const HeaderCodes &hc, uint64_t fn) {
    __shared__ uint32_t wave_tot[4];
    const uint32_t tid = threadIdx.x;
    const SubPlan *sp = p.out_plan + (size_t)frame * p.channels + ch;
    const uint32_t type = sp->type, order = sp->order, wasted = sp->wasted, bps = sp->bps;
    // residual row: every lane reads its own contiguous run straight from HBM/L2 (twice:
    // lengths, then codes; the second pass hits L1/L2)
    const int32_t *__restrict__ r = p.residuals + ((size_t)frame * p.channels + ch) * p.block_size;
    auto rd = [&](uint32_t i) -> int32_t { return r[i]; };
    __syncthreads();

    if (tid == 0) {
        if (with_header) {  // FrameHeader::build, stream.rs:242-276 (+ CRC-8, :194-197)
            const flacgpu_frame_plan fp = p.frame_plan[frame];
            const uint32_t acode = fp.assignment == FLACGPU_ASSIGN_INDEPENDENT ? p.channels - 1 : fp.assignment;
            const uint32_t pcode = p.bps == 8 ? 1 : p.bps == 12 ? 2 : p.bps == 16 ? 4 : p.bps == 20 ? 5
                                 : p.bps == 24 ? 6 : p.bps == 32 ? 7 : 0;
            put_frame_header(sb, 0u, hc, fn, n, acode, pcode);
        }
        // SubframeHeader, stream.rs:1390-1413
        const uint32_t tcode = type == FLACGPU_SUB_CONSTANT ? 0u : type == FLACGPU_SUB_VERBATIM ? 1u
                             : type == FLACGPU_SUB_FIXED ? 8u + order : 31u + order;
        lds_put(sb, base, tcode, 7);
        if (wasted) {
            lds_put(sb, base + 7, 1, 1);
            lds_put(sb, base + 8 + (wasted - 1), 1, 1);  // wasted-1 zeros then a one
        }
        if (type == FLACGPU_SUB_CONSTANT) lds_put(sb, base + 8 + wasted, (uint32_t)rd(0), bps);
    }
    const uint32_t body0 = base + 8 + wasted;
    if (type == FLACGPU_SUB_VERBATIM) {
        for (uint32_t i = tid; i < n; i += WG) lds_put(sb, body0 + i * bps, (uint32_t)rd(i), bps);
    } else if (type == FLACGPU_SUB_FIXED || type == FLACGPU_SUB_LPC) {
        // warm-up, precision, shift, coefficients (encode.rs:3083-3085, 3118-3133)
        if (tid < order) lds_put(sb, body0 + tid * bps, (uint32_t)rd(tid), bps);
        uint32_t pos = body0 + order * bps;
        if (type == FLACGPU_SUB_LPC) {
            const uint32_t prec = sp->precision;
            if (tid == 32) {
                lds_put(sb, pos, prec - 1, 4);
                lds_put(sb, pos + 4, sp->shift, 5);
            }
            if (tid >= 64 && tid < 64 + order) lds_put(sb, pos + 9 + (tid - 64) * prec, (uint32_t)sp->coeffs[tid - 64], prec);
            pos += 9 + order * prec;
        }
        // residual block (encode.rs:3944-3961, 3898-3907)
        const uint32_t method = sp->coding_method, hb = method ? 5u : 4u, esc_code = method ? 31u : 15u;
        if (tid == 96) {
            lds_put(sb, pos, method, 2);
            lds_put(sb, pos + 2, sp->partition_order, 4);
        }
        pos += 6;
        const uint32_t np = sp->n_partitions, plen = sp->part_len;
        const uint32_t first_j = plen ? n / plen - np : 0;  // chunks lying inside the warm-up
        const uint32_t ept = (n + WG - 1) / WG;
        const uint32_t lo = tid * ept > order ? tid * ept : order;
        const uint32_t hi = (tid + 1) * ept < n ? (tid + 1) * ept : n;
        // pass 1: code lengths of this lane's residuals (+ partition headers)
        uint32_t mybits = 0;
        if (lo < hi) {
            uint32_t pj = lo / plen;                 // partition (block-aligned index)
            uint32_t bound = (pj + 1) * plen;
            uint32_t k = sp->rice[pj - first_j], eb = sp->escape_bits[pj - first_j];
            const uint32_t pstart0 = pj * plen > order ? pj * plen : order;
            if (lo == pstart0) mybits += hb + (k == 0xFF ? 5u : 0u);
            // an EMPTY first partition (order == part_len: 1024-sample blocks, order 16, partition order 6 -- a caller's plan,
            // the encoder never chooses it) has no residual to bring its header along: the first residual's lane writes it
            if (lo == order && order == plen && np > 1) mybits += hb + (sp->rice[0] == 0xFF ? 5u : 0u);
            for (uint32_t i = lo; i < hi; i++) {
                if (i == bound) {
                    pj++;
                    bound += plen;
                    k = sp->rice[pj - first_j];
                    eb = sp->escape_bits[pj - first_j];
                    mybits += hb + (k == 0xFF ? 5u : 0u);
                }
                mybits += (k != 0xFF) ? (zigzag(r[i]) >> k) + 1u + k : eb;
            }
        }
        // exclusive scan of mybits over the workgroup
        uint32_t v = mybits;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t t = __shfl_up(v, off, 64);
            if ((tid & 63) >= (uint32_t)off) v += t;
        }
        if ((tid & 63) == 63) wave_tot[tid >> 6] = v;
        __syncthreads();
        uint32_t mypos = pos + v - mybits;
        for (uint32_t w = 0; w < (tid >> 6); w++) mypos += wave_tot[w];
        // pass 2: emit
        if (lo < hi) {
            uint32_t pj = lo / plen;
            uint32_t bound = (pj + 1) * plen;
            uint32_t k = sp->rice[pj - first_j], eb = sp->escape_bits[pj - first_j];
            const uint32_t pstart0 = pj * plen > order ? pj * plen : order;
            if (lo == order && order == plen && np > 1) {   // the header of an empty first partition
                const uint32_t k0 = sp->rice[0];
                if (k0 != 0xFF) { lds_put(sb, mypos, k0, hb); mypos += hb; }
                else { lds_put(sb, mypos, esc_code, hb); lds_put(sb, mypos + hb, sp->escape_bits[0], 5); mypos += hb + 5; }
            }
            if (lo == pstart0) {
                if (k != 0xFF) { lds_put(sb, mypos, k, hb); mypos += hb; }
                else { lds_put(sb, mypos, esc_code, hb); lds_put(sb, mypos + hb, eb, 5); mypos += hb + 5; }
            }
            for (uint32_t i = lo; i < hi; i++) {
                if (i == bound) {
                    pj++;
                    bound += plen;
                    k = sp->rice[pj - first_j];
                    eb = sp->escape_bits[pj - first_j];
                    if (k != 0xFF) { lds_put(sb, mypos, k, hb); mypos += hb; }
                    else { lds_put(sb, mypos, esc_code, hb); lds_put(sb, mypos + hb, eb, 5); mypos += hb + 5; }
                }
                if (k != 0xFF) {
                    const uint32_t u = zigzag(r[i]);
                    const uint32_t qn = u >> k;
                    mypos += qn;  // unary zeros (buffer is pre-zeroed)
                    lds_put(sb, mypos, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
                    mypos += k + 1;
                } else if (eb) {
                    lds_put(sb, mypos, (uint32_t)r[i], eb);
                    mypos += eb;
                }
            }
        }
        if (n == order && tid == 0) {  // no residuals at all: lone partition header
            const uint32_t k = sp->rice[0], eb = sp->escape_bits[0];
            if (k != 0xFF) lds_put(sb, pos, k, hb);
            else { lds_put(sb, pos, esc_code, hb); lds_put(sb, pos + hb, eb, 5); }
        }
    }
}

// BIG: blocks above LDS_BLOCK_LIMIT, the subframe's bit string lives in HBM (p.big_scratch, global
// atomics) instead of dynamic LDS
template <bool BIG>
__global__ void __launch_bounds__(WG) k_pack_t(Params p, PackParams q) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    uint32_t frame, ch;
    map_block(blockIdx.x, p.channels, p.fcount, frame, ch);
    frame += p.f0;
    const uint32_t tid = threadIdx.x;
    const uint32_t n = frame_len(p, frame);
    const uint32_t sub_bits = p.out_plan[(size_t)frame * p.channels + ch].bits;

    // position of this subframe inside the frame
    const uint64_t fn = frame_number_of(q, frame);
    const HeaderCodes hc = header_codes(n, q.sample_rate, fn);
    const uint32_t hbytes = header_bytes(hc);
    uint32_t start_bit = hbytes * 8;
    for (uint32_t c = 0; c < ch; c++) start_bit += p.out_plan[(size_t)frame * p.channels + c].bits;
    const uint32_t prefix_bits = ch == 0 ? hbytes * 8 : 0;  // subframe 0 also carries the header
    const uint32_t total_bits = prefix_bits + sub_bits;
    const uint32_t nwords = (total_bits + 31) / 32 + 1;

    uint32_t *sb = reinterpret_cast<uint32_t *>(lds);  // the subframe's bit string
    if constexpr (BIG) sb = reinterpret_cast<uint32_t *>(p.big_scratch + (size_t)blockIdx.x * p.big_stride);
    for (uint32_t i = tid; i < nwords; i += WG) sb[i] = 0;
    pack_subframe(p, q, frame, ch, n, sb, prefix_bits, ch == 0, hc, fn);
    __syncthreads();
    // copy out: absolute bit position of sb[0] in the output stream
    const uint64_t abs_bit = q.frame_off[frame] * 8ull + (ch == 0 ? 0u : start_bit);
    const uint64_t w0 = abs_bit >> 5;
    const uint32_t s = (uint32_t)(abs_bit & 31);
    const uint32_t nout = (s + total_bits + 31) / 32;
    for (uint32_t j = tid; j < nout; j += WG) {
        uint32_t val;
        if (s == 0) val = sb[j];
        else val = (j ? (sb[j - 1] << (32 - s)) : 0u) | (sb[j] >> s);
        const uint32_t be = __builtin_bswap32(val);
        if (j == 0 || j + 1 == nout) atomicOr(&q.out_words[w0 + j], be);
        else q.out_words[w0 + j] = be;
    }
}

// CRC-16 (poly 0x8005, MSB first, init 0; crc.rs:142-188) of every packed frame
#include "crc16.inc"
constexpr uint32_t CRC_CHUNK = 16384;  // bytes staged in LDS per pass: 256 lanes x 64 B

// ---- CRC-16 of the whole words fb[0 .. nw4) of an MSB-first LDS bit string by NT cooperating lanes (crc.rs:142-188).
// The words, left-padded with zero WORDS (they leave a zero CRC state unchanged) to S * NT slices of 17 words, slice
// g = s * NT + tid: a lane runs its SC = S table-lookup chains interleaved (each step is one LDS round trip), folds them with
// Horner in x^(544 NT) and weights the result with x^(544 (NT - 1 - tid)): the XOR of the lanes' return values is the CRC
// (GF(2) linearity).  Word granularity -- the <= 3 bytes behind the last whole word go through crc16_tail -- keeps every
// slice word-aligned: a step is the word, t = crc ^ (word >> 16), four byte-indexed lookups and three XORs (the byte-aligned
// version this replaces funnel-shifted two words per step and cost 19 instructions instead of 11).
// SW: words per slice, 17 (odd: the lanes' word reads spread over the banks).  Shorter slices = more chains per lane = fewer
// DEPENDENT table round trips (a frame of 16 KB: 2 chains x 17 steps or 4 chains x 9), paid for with one more Horner fold
// (gf_mulmod_t) per chain.
template <int NT, int SC, int SW = 17>
__device__ __forceinline__ uint32_t crc16_words_share(const uint32_t *fb, uint32_t padw, uint32_t tid, const uint16_t (*T)[256]) {
    static_assert(SW == 17, "weights table");
    uint32_t crc[SC];
    int32_t w0[SC];
#pragma unroll
    for (int c = 0; c < SC; c++) {
        w0[c] = (int32_t)((c * NT + tid) * (uint32_t)SW) - (int32_t)padw;   // first word of the slice (negative: padding)
        crc[c] = 0;
    }
#pragma unroll
    for (int kk = 0; kk < SW; kk++) {
#pragma unroll
        for (int c = 0; c < SC; c++) {
            const int32_t wi = w0[c] + kk;
            const uint32_t m = wi >= 0 ? fb[wi >= 0 ? wi : 0] : 0u;
            const uint32_t t = crc[c] ^ (m >> 16);
            crc[c] = T[3][(t >> 8) & 0xFF] ^ T[2][t & 0xFF] ^ T[1][(m >> 8) & 0xFF] ^ T[0][m & 0xFF];
        }
    }
    static_assert(SW == 17, "kCrcW17: weights of 17-word slices");
    const uint16_t *wt = kCrcW17.w;
    const uint32_t xrow = wt[NT];          // x^(32 SW NT)
    uint32_t acc = crc[0];
#pragma unroll
    for (int c = 1; c < SC; c++) acc = gf_mulmod_t(acc, xrow, T) ^ crc[c];
    return gf_mulmod_t(acc, wt[NT - 1 - tid], T);
}
// the CRC continued over the first `nbytes` (<= 3) bytes of `word` (MSB first)
__device__ __forceinline__ uint32_t crc16_tail(uint32_t crc, uint32_t word, uint32_t nbytes, const uint16_t (*T)[256]) {
    for (uint32_t j = 0; j < nbytes; j++) {
        const uint32_t b = (word >> (24 - 8 * j)) & 0xFFu;
        crc = ((crc << 8) & 0xFFFFu) ^ T[0][((crc >> 8) ^ b) & 0xFFu];   // T[0][b] = b x^16 mod P: the byte-wise table
    }
    return crc;
}

// ---------------------------------------------------------------------------------
// Wave-per-subframe frame assembly (4096-sample frames, LPC order <= 16, <= 4 channels): the
// workgroup is one frame, wave c is subframe c.  Lane l owns samples [64 l, 64 l + 64) in
// registers as in k_cand64: the residual is recomputed in place (FIR with wave-uniform
// coefficients / iterated differences), the code lengths of a lane's run are summed, one DPP scan
// gives every lane its bit offset, and the lane then streams its codes through a 64-bit shift
// register into the frame's LDS bit string one finished 32-bit word at a time.  The only workgroup
// barriers are the ones around the CRC-16.
// ---------------------------------------------------------------------------------
struct BitRun {  // a lane's contiguous MSB-first bit run inside an LDS word array
    uint32_t *word;   // next word to complete
    uint64_t acc;     // pending bits, right-aligned; bits above `fill` are stale and never read
    uint32_t fill;    // pending bit count (< 32 between calls); starts at the run's bit offset
    __device__ __forceinline__ void init(uint32_t *sb, uint32_t pos) {
        word = sb + (pos >> 5);
        fill = pos & 31;  // the bits before the run belong to someone else: contribute zeros
        acc = 0;
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t nb) {  // nb <= 32, v < 2^nb
        acc = (acc << nb) | v;
        fill += nb;
        if (fill >= 32) {
            fill -= 32;
            atomicOr(word, (uint32_t)(acc >> fill));  // words at the ends of a run are shared
            word++;
        }
    }
    __device__ __forceinline__ void finish() {
        if (fill) atomicOr(word, (uint32_t)(acc << (32 - fill)));
    }
};

// DIRECT: stereo frames read from the caller's interleaved PCM (Params::inter) instead of planar rows
// S4: the instantiation may meet stereo L/R/M/S candidates (two-channel frames only)
// Place: called once the plan and sample loads are under way and before the first LDS access; it may still change where
// the subframe goes (k_sub64 prepares its LDS image and finds the subframe's position while the loads travel)
struct PlaceAsGiven {
    __device__ __forceinline__ void operator()(uint32_t *&, uint32_t &) const {}
};
// Load: brings the lane's samples itself (k_sub64's transposing load of an interleaved batch) instead of the planar row
struct LoadRow {
    static constexpr bool ON = false;
    template <int SPL> __device__ __forceinline__ void operator()(int32_t (&)[SPL]) const {}
};
template <class F>
struct LoadWith {
    static constexpr bool ON = true;
    F f;
    template <int SPL> __device__ __forceinline__ void operator()(int32_t (&x)[SPL]) const { f(x); }
};
template <int SPL, int MAXO, bool DIRECT = false, bool S4 = true, class Place = PlaceAsGiven, class Load = LoadRow>
__device__ __forceinline__ void wave_subframe(const Params &p, uint32_t frame, uint32_t ch,
                                              uint32_t *sb, uint32_t base, Place &&place = Place(), Load &&load = Load()) {
    const uint32_t lane = threadIdx.x & 63;
    const SubPlan *sp = p.out_plan + (size_t)frame * p.channels + ch;
    // One memory round trip: the whole 280-byte plan as one dword per lane (fields, coefficients
    // and partition parameters are handed out with readlane / bpermute) and, at the same time,
    // the samples -- for stereo frames both input rows, whatever candidate the plan names.
    static_assert(sizeof(SubPlan) == 280, "plan layout");
    const uint32_t *d = reinterpret_cast<const uint32_t *>(sp);
    const uint32_t pw = d[lane];                       // dwords 0..63
    const uint32_t pw2 = lane < 6 ? d[64 + lane] : 0;  // dwords 64..69
    const int32_t *rowa, *rowb;
    if (p.stereo4) {
        rowa = p.planar + (size_t)frame * 2 * p.ldb;
        rowb = rowa + p.ldb;
    } else {
        rowa = p.planar + ((size_t)frame * p.channels + ch) * p.ldb;  // source == ch
        rowb = rowa;
    }
    int32_t x[SPL];
    // independent channels: the row is requested first thing, together with the plan (one round trip)
    if constexpr (std::remove_reference_t<Load>::ON) {
        static_assert(!DIRECT && !S4, "independent channels");
        load(x);
    } else if constexpr (!DIRECT) {
        if (!S4 || !p.stereo4) load_lane<SPL>(rowa, lane, x);
    }
    // THE RESIDUAL HANDED OVER (Params::hand_meta; 4096-sample direct stereo frames): the subframe's row of Params::residuals
    // holds what the winning candidate wave of k_cand64p had in its registers -- zigzag(r) rotated right by one, sample e of
    // lane l at dword 256 (e / 4) + 4 l + e % 4 (16-byte pieces, a kilobyte per instruction), zeros for the warm-up -- and
    // hand_meta says whether it does (an LPC winner whose wave did not have to re-fetch).  The row is requested together with the plan and the flag, on the expectation that it is there (it is
    // for nearly every subframe of ordinary audio); where it is not, the samples are fetched behind it as before.  A handed
    // subframe needs no second channel, no pick, no shift, no history and no FIR: its warm-up samples come from one (l, r) pair
    // per lane.
    constexpr bool CAN_HAND = DIRECT && SPL == 64;
    bool handed = false, placed = false;
    int2 warm_pair = make_int2(0, 0);
    if constexpr (CAN_HAND) {
        if (p.hand_meta) {   // (a kernel argument: the same for the whole workgroup)
            const uint32_t sub = __builtin_amdgcn_readfirstlane(frame * 2u + ch);
            const uint32_t hflag = p.hand_meta[sub];
            const int32_t *row = p.residuals + (size_t)sub * (64u * SPL);
            typedef int v4i __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int j = 0; j < SPL / 4; j++) {   // (read once: non-temporal, like the stores that made the row)
                const v4i v = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(row) + 64 * j + lane);
                x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
            }
            if (lane < (uint32_t)MAXO) warm_pair = reinterpret_cast<const int2 *>(inter_frame(p, frame, 128 * SPL))[lane];
            place(sb, base);   // (k_frame64 prepares its LDS image here, under the loads' round trip)
            placed = true;
            __builtin_amdgcn_sched_barrier(0);
            handed = __builtin_amdgcn_readfirstlane(hflag) != 0u;
        }
    }
    // (not handed, but the plan -- it came with the flag -- says VERBATIM or CONSTANT: nothing to fetch either.  A VERBATIM
    // subframe fetches its samples itself further down, a CONSTANT one needs sample 0, which lane 0's warm-up pair holds.  Without
    // this a batch of noise paid the wasted row AND a wasted fetch: + 5.7 %, tools/hand_worstcase.py)
    bool fetch = !handed;
    if constexpr (CAN_HAND) {
        if (placed && !handed) {
            const uint32_t ty = sread(pw, 0) & 0xFF;
            fetch = !(ty == FLACGPU_SUB_VERBATIM || ty == FLACGPU_SUB_CONSTANT);
            if (!fetch) {
                const uint32_t srcid0 = sread(pw, 2) & 0xFF;
                const int32_t l0 = warm_pair.x, r0 = warm_pair.y;
                x[0] = srcid0 == 1 ? r0 : srcid0 == FLACGPU_SRC_MID ? (int32_t)((uint32_t)l0 + (uint32_t)r0)
                     : srcid0 == FLACGPU_SRC_SIDE ? (int32_t)((uint32_t)l0 - (uint32_t)r0) : l0;   // (lane 0: sample 0; shifted below)
            }
        }
    }
    if constexpr (DIRECT) {
      if (fetch) {
        // the lane's SPL (l, r) pairs are SPL / 2 contiguous 16-byte pieces.  They are fetched in TWO halves, each
        // picked into x (l, r, l + r or l - r: wave-uniform) before the next is requested: 64 registers of input in
        // flight instead of 128, which is the difference between two and three waves per SIMD for this kernel.
        // (1152-sample blocks: 9 pieces per lane, fetched in one go)
        const int4 *f = reinterpret_cast<const int4 *>(inter_frame(p, frame, 128 * SPL)) + (SPL / 2) * lane;
        uint32_t srcid = 0;
        constexpr int NH = SPL % 4 == 0 ? 2 : 1, HP = SPL / 2 / NH;   // passes, pieces per pass
        // (touching one dword of every line of the second half behind the first half's pieces, so that its own round trip ends
        // in the L2: measured slower, profiles/r05_frame_timeline.json)
#pragma unroll
        for (int h = 0; h < NH; h++) {
            int4 v[HP];
#pragma unroll
            for (int k = 0; k < HP; k++) v[k] = f[h * HP + k];   // (plain loads: a line is shared by eight of these; non-temporal they ran at half speed)
            if (h == 0) {   // the plan word is looked at only now: the first half travels together with the plan
                if (!placed) place(sb, base);   // (k_frame64 prepares its LDS image here, under the loads' round trip)
                __builtin_amdgcn_sched_barrier(0);
                srcid = sread(pw, 2) & 0xFF;
            }
#define PICKF(E0, E1)                                                                     \
    _Pragma("unroll") for (int k = 0; k < HP; k++) {                                     \
        x[h * (2 * HP) + 2 * k] = (E0);                                                   \
        x[h * (2 * HP) + 2 * k + 1] = (E1);                                               \
    }
            if (srcid == 1) { PICKF(v[k].y, v[k].w) }
            else if (srcid == FLACGPU_SRC_MID) { PICKF((int32_t)((uint32_t)v[k].x + (uint32_t)v[k].y), (int32_t)((uint32_t)v[k].z + (uint32_t)v[k].w)) }
            else if (srcid == FLACGPU_SRC_SIDE) { PICKF((int32_t)((uint32_t)v[k].x - (uint32_t)v[k].y), (int32_t)((uint32_t)v[k].z - (uint32_t)v[k].w)) }
            else { PICKF(v[k].x, v[k].z) }
#undef PICKF
            __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else if (S4 && p.stereo4) {
        // planar L / R rows, two halves as above (SPL a multiple of 8: 16-byte pieces per half)
        uint32_t srcid = 0;
        if constexpr (SPL % 8 == 0) {
            const int4 *fa = reinterpret_cast<const int4 *>(rowa) + (SPL / 4) * lane;
            const int4 *fb = reinterpret_cast<const int4 *>(rowb) + (SPL / 4) * lane;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                int4 a[SPL / 8], b[SPL / 8];
#pragma unroll
                for (int k = 0; k < SPL / 8; k++) {
                    a[k] = fa[h * (SPL / 8) + k];
                    b[k] = fb[h * (SPL / 8) + k];
                }
                if (h == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    srcid = sread(pw, 2) & 0xFF;
                }
#define PICKP(OP)                                                                                   \
    _Pragma("unroll") for (int k = 0; k < SPL / 8; k++) {                                           \
        const int e0 = h * (SPL / 2) + 4 * k;                                                        \
        x[e0] = OP(a[k].x, b[k].x); x[e0 + 1] = OP(a[k].y, b[k].y);                                 \
        x[e0 + 2] = OP(a[k].z, b[k].z); x[e0 + 3] = OP(a[k].w, b[k].w);                             \
    }
#define SEL_A(u, v) (u)
#define SEL_B(u, v) (v)
#define SEL_M(u, v) ((int32_t)((uint32_t)(u) + (uint32_t)(v)))
#define SEL_S(u, v) ((int32_t)((uint32_t)(u) - (uint32_t)(v)))
                if (srcid == 1) { PICKP(SEL_B) }
                else if (srcid == FLACGPU_SRC_MID) { PICKP(SEL_M) }
                else if (srcid == FLACGPU_SRC_SIDE) { PICKP(SEL_S) }
                else { PICKP(SEL_A) }
#undef PICKP
#undef SEL_A
#undef SEL_B
#undef SEL_M
#undef SEL_S
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            load_lane<SPL>(rowa, lane, x);
            int32_t xb[SPL];
            load_lane<SPL>(rowb, lane, xb);
            srcid = sread(pw, 2) & 0xFF;
            // L: a, R: b, mid: a + b (>> 1 below), side: a - b; wave-uniform branches
            if (srcid == 1) {
#pragma unroll
                for (int e = 0; e < SPL; e++) x[e] = xb[e];
            } else if (srcid == FLACGPU_SRC_MID) {
#pragma unroll
                for (int e = 0; e < SPL; e++) x[e] = (int32_t)((uint32_t)x[e] + (uint32_t)xb[e]);
            } else if (srcid == FLACGPU_SRC_SIDE) {
#pragma unroll
                for (int e = 0; e < SPL; e++) x[e] = (int32_t)((uint32_t)x[e] - (uint32_t)xb[e]);
            }
        }
    }
    if constexpr (!DIRECT) place(sb, base);
    const uint32_t d0 = sread(pw, 0), d1 = sread(pw, 1), d2 = sread(pw, 2);
    const uint32_t type = d0 & 0xFF, wasted = (d0 >> 8) & 0xFF, bps = (d0 >> 16) & 0xFF, order = d0 >> 24;
    const uint32_t prec = d1 & 0xFF, shift = (d1 >> 8) & 0xFF, method = (d1 >> 16) & 0xFF, porder = d1 >> 24;
    const uint32_t sh_all = wasted + ((p.stereo4 && (d2 & 0xFF) == FLACGPU_SRC_MID) ? 1u : 0u);
    if (!handed) {
#pragma unroll
        for (int e = 0; e < SPL; e++) x[e] >>= sh_all;
    }
    // Rice parameters of the partition this lane's samples lie in (a partition is 2^(6 - porder)
    // lanes; the warm-up never swallows a whole partition since order <= 16 <= SPL):
    // rice[pj] is byte pj of dwords 38..53, escape_bits[pj] byte pj of dwords 54..69
    const uint32_t lpp = 6u - (porder < 6u ? porder : 6u);  // log2(lanes per partition)
    const uint32_t pj = lane >> lpp;
    const bool coded = type == FLACGPU_SUB_FIXED || type == FLACGPU_SUB_LPC;
    const uint32_t rw = __shfl(pw, (int)(38 + (pj >> 2)), 64);
    const uint32_t ei = 54 + (pj >> 2);
    const uint32_t ew1 = __shfl(pw, (int)(ei & 63), 64), ew2 = __shfl(pw2, (int)(ei & 63), 64);
    const uint32_t ew = ei < 64 ? ew1 : ew2;
    const uint32_t k = coded ? (rw >> (8 * (pj & 3))) & 0xFF : 0u;
    const uint32_t eb = coded ? (ew >> (8 * (pj & 3))) & 0xFF : 0u;
    const uint32_t cw = pw;  // LPC coefficient j sits on lane 6 + j
    const uint32_t smask = bps >= 32 ? 0xFFFFFFFFu : (1u << bps) - 1u;
    // SubframeHeader, stream.rs:1390-1413
    if (lane == 0) {
        const uint32_t tcode = type == FLACGPU_SUB_CONSTANT ? 0u : type == FLACGPU_SUB_VERBATIM ? 1u
                             : type == FLACGPU_SUB_FIXED ? 8u + order : 31u + order;
        lds_put(sb, base, tcode, 7);
        if (wasted) {
            lds_put(sb, base + 7, 1, 1);
            lds_put(sb, base + 8 + (wasted - 1), 1, 1);  // wasted-1 zeros then a one
        }
        if (type == FLACGPU_SUB_CONSTANT) lds_put(sb, base + 8 + wasted, (uint32_t)x[0], bps);
    }
    const uint32_t body0 = base + 8 + wasted;
    if (type == FLACGPU_SUB_CONSTANT) return;
    BitRun br;
    if (type == FLACGPU_SUB_VERBATIM) {
        // The samples are FETCHED AGAIN here (plain loads; a rare path: noise).  This region sits inside a structurised
        // part of the kernel's control flow, where a uniform `if (...) { ...; return; }` becomes a flag tested BEHIND the
        // coded path: emitted from `x`, all 64 original samples stayed alive through the in-place FIR beside its 64
        // results (165-168 VGPRs, and scratch at order 32).
        int32_t xv[SPL];
        {
            const uint32_t srcid = d2 & 0xFF;
            const uint32_t s0 = (uint32_t)SPL * lane;
            if constexpr (std::remove_reference_t<Load>::ON) {
                const int32_t *src = split_frame(p, frame, 64u * SPL * p.channels) + (size_t)s0 * p.channels + ch;
                asm volatile("" : "+v"(src));   // (not to be merged with the first fetch)
#pragma unroll
                for (int e = 0; e < SPL; e++) xv[e] = src[(size_t)e * p.channels];
            } else if constexpr (DIRECT) {
                const int32_t *src = inter_frame(p, frame, 128 * SPL) + 2 * s0;
                asm volatile("" : "+v"(src));
#pragma unroll
                for (int e = 0; e < SPL; e++) {
                    const int32_t l = src[2 * e], r = src[2 * e + 1];
                    xv[e] = srcid == 1 ? r : srcid == FLACGPU_SRC_MID ? (int32_t)((uint32_t)l + (uint32_t)r)
                          : srcid == FLACGPU_SRC_SIDE ? (int32_t)((uint32_t)l - (uint32_t)r) : l;
                }
            } else {
                const int32_t *ra = rowa + s0, *rb = rowb + s0;
                asm volatile("" : "+v"(ra), "+v"(rb));
                const bool two = S4 && p.stereo4;
#pragma unroll
                for (int e = 0; e < SPL; e++) {
                    const int32_t l = ra[e], r = two ? rb[e] : 0;
                    xv[e] = !two ? l : srcid == 1 ? r : srcid == FLACGPU_SRC_MID ? (int32_t)((uint32_t)l + (uint32_t)r)
                          : srcid == FLACGPU_SRC_SIDE ? (int32_t)((uint32_t)l - (uint32_t)r) : l;
                }
            }
            const uint32_t sh = wasted + ((p.stereo4 && srcid == FLACGPU_SRC_MID) ? 1u : 0u);
#pragma unroll
            for (int e = 0; e < SPL; e++) xv[e] >>= sh;
        }
        br.init(sb, body0 + lane * (uint32_t)SPL * bps);
#pragma unroll
        for (int e = 0; e < SPL; e++) br.put((uint32_t)xv[e] & smask, bps);
        br.finish();
        return;
    }
    // warm-up samples (encode.rs:3083-3085, 3118-3133): the first `order` samples of lane 0
    if (handed) {   // ... of the subframe: sample `lane` from the lane's (l, r) pair
        const uint32_t srcid = d2 & 0xFF;
        const int32_t l = warm_pair.x, r = warm_pair.y;
        const int32_t v = srcid == 1 ? r : srcid == FLACGPU_SRC_MID ? (int32_t)((uint32_t)l + (uint32_t)r)
                        : srcid == FLACGPU_SRC_SIDE ? (int32_t)((uint32_t)l - (uint32_t)r) : l;
        if (lane < order) lds_put(sb, body0 + lane * bps, (uint32_t)(v >> sh_all) & smask, bps);
    }
    if (!handed && lane == 0) {
        br.init(sb, body0);
#pragma unroll
        for (int e = 0; e < MAXO; e++)
            if ((uint32_t)e < order) br.put((uint32_t)x[e] & smask, bps);
        br.finish();
    }
    // Code lengths are summed where each residual is produced; Rice-coded lanes keep zigzag(r)
    // in place of r.  Warm-up samples (lane 0, e < order) carry no residual.
    const uint32_t first = lane == 0 ? order : 0u;
    const bool rice = k != 0xFF;
    struct LenAcc {
        uint32_t qsum, ks, first;
        bool lane0;
        uint32_t order;
        __device__ __forceinline__ int32_t operator()(int e, int32_t r) {
            uint32_t u = zigzag(r);
            if (e < MAXO) u = (lane0 && (uint32_t)e < order) ? 0u : u;   // scalar-conditioned mask
            qsum += u >> ks;
            // pinned every fourth sample: left alone, the 64 quotients are all formed first and summed at the end of the
            // pass (64 more live registers: the difference between two and three waves per SIMD)
            if ((e & 3) == 0) asm volatile("" : "+v"(qsum));
            return (int32_t)u;   // zigzag(r) in place of r for every lane (an escaped partition unfolds it again below)
        }
    } len{0u, rice ? k : 0u, first, lane == 0, order};
    uint32_t resid_pos = body0 + order * bps;
    if (type == FLACGPU_SUB_LPC) {
        if (lane == 32) {
            lds_put(sb, resid_pos, prec - 1, 4);
            lds_put(sb, resid_pos + 4, shift, 5);
        }
        if (lane >= 6 && lane < 6 + order) lds_put(sb, resid_pos + 9 + (lane - 6) * prec, cw, prec);
        resid_pos += 9 + order * prec;
        if (!handed) {
            int32_t hp[MAXO];
#pragma unroll
            for (int kk = 0; kk < MAXO; kk++) hp[kk] = lane_prev(x[SPL - MAXO + kk]);
            // the residual, in place (encode.rs:3181-3197); taps rounded up to a multiple of 2 (the tap behind an odd order
            // is zeroed by fir_coeffs_from itself: a caller's plan may hold anything in coeffs[order ..]): one region
            // with a run-time tap count (fir64_dyn, wave_cand.inc)
            fir64_dyn<SPL, MAXO, 6, FIR_TURN(SPL)>(x, hp, cw, order, shift);
        }
    }
    // (two independent regions, not if / else: structurised, an if / else is a chain of two regions that BOTH read the
    // original samples, which then stay alive beside the first region's results)
    if (type != FLACGPU_SUB_LPC) {  // FIXED: iterated differences in place (encode.rs:3039-3060)
        // The residual of order K = the K-th iterated difference, formed by K IN-PLACE passes x[e] -= x[e - 1] (descending;
        // the sample before the lane's first comes from the previous lane at the same level), each under a uniform
        // `order > k`: K subtractions per sample, like the per-order chains this replaces -- but ONE definition per sample
        // and pass.  (The five per-order loops behind a switch were, once structurised, a chain of regions each reading the
        // original samples: originals and results alive together, 152 VGPRs.)
        uint32_t order_s = order;
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            asm volatile("" : "+s"(order_s));   // (one condition for all passes would merge them)
            if (order_s > (uint32_t)kk) {
                const int32_t hk = lane_prev(x[SPL - 1]);
#pragma unroll
                for (int e = SPL - 1; e >= 1; e--) x[e] = (int32_t)((uint32_t)x[e] - (uint32_t)x[e - 1]);
                x[0] = (int32_t)((uint32_t)x[0] - (uint32_t)hk);
                asm volatile("" : "+v"(x[0]));   // the pass ends here (no difference is carried into the next one)
            }
        }
    }
    // code lengths in ONE pass behind both (fused into the residual loops, every instantiation carried its own copy of the
    // length code and their results met in different registers: 223 VGPRs)
    if (!handed) {
#pragma unroll
        for (int e = 0; e < SPL; e++) {
            x[e] = len(e, x[e]);
            if ((e & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (CAN_HAND) {
        if (handed) {   // the handed word rotated left by one is zigzag(r) (zero for the warm-up): one instruction per sample
#pragma unroll
            for (int e = 0; e < SPL; e++) {
                const uint32_t u = __builtin_amdgcn_alignbit((uint32_t)x[e], (uint32_t)x[e], 31);
                len.qsum += u >> len.ks;
                if ((e & 3) == 0) asm volatile("" : "+v"(len.qsum));
                x[e] = (int32_t)u;
                if ((e & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // residual block (encode.rs:3944-3961, 3898-3907)
    const uint32_t hb = method ? 5u : 4u, esc_code = method ? 31u : 15u;
    if (lane == 1) {
        lds_put(sb, resid_pos, method, 2);
        lds_put(sb, resid_pos + 2, porder, 4);
    }
    const uint32_t pos = resid_pos + 6;
    const bool head = (lane & ((1u << lpp) - 1u)) == 0;   // this lane starts a partition
    const uint32_t cnt = (uint32_t)SPL - first;
    const uint32_t mybits = (head ? hb + (rice ? 0u : 5u) : 0u) + (rice ? len.qsum + cnt * (k + 1u) : cnt * eb);
    const uint32_t incl = wave_scan_u32(mybits);
    // Rice codes placed DIRECTLY: the image is zero, so the q zeros of a code need no write at all -- only its k + 1 low
    // bits (the stop bit and the remainder), a field that ENDS at the lane's running bit position.  With r = end & 31 the
    // field's last r bits are the top of word end >> 5 (alignbit(v, 0, end): v << (32 - r), 0 for r = 0) and the rest the
    // bottom of the word before it (v >> r): two LDS ORs and seven VALU instructions per sample, whatever the quotient
    // (the 64-bit shift register this replaces took thirteen, tracked the longest code of the wave and had a slow path
    // for codes beyond 32 bits).  (sb[-1] is never reached: a subframe's codes start behind its header bits, and
    // k_sub64's image has a guard word in front.)
    if (rice) {
        // the bit position is kept LDS-absolute and one word early (8 x the byte address of sb[-1] added once), so that the
        // byte address of word W - 1 is (end >> 3) & ~3 and word W the same + 4 (an immediate offset): two address
        // instructions per code, and both shifts take `end` unmasked (v_alignbit_b32 uses its low five bits)
        typedef __attribute__((address_space(3))) uint32_t lds_u32;
        const uint32_t sb_addr = (uint32_t)(uintptr_t)(lds_u32 *)sb;
        auto put_end = [&](uint32_t end, uint32_t v) {   // field v ending at bit `end` (exclusive)
            lds_u32 *w = (lds_u32 *)(uintptr_t)((end >> 3) & ~3u);
            (void)__hip_atomic_fetch_or(w, __builtin_amdgcn_alignbit(0u, v, end), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            (void)__hip_atomic_fetch_or(w + 1, __builtin_amdgcn_alignbit(v, 0u, end), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        uint32_t pe = pos + incl - mybits + 8u * sb_addr - 32u;
        if (head) {
            pe += hb;
            put_end(pe, k);
        }
        const uint32_t stop = 1u << k, lowmask = stop - 1u, k1 = k + 1u;
#pragma unroll
        for (int e = 0; e < SPL; e++) {
            const uint32_t u = (uint32_t)x[e];
            uint32_t q = u >> k, add = k1;
            uint32_t v = stop | (u & lowmask);
            if (e < MAXO) {  // warm-up samples of lane 0 carry no residual
                const bool warm = lane == 0 && (uint32_t)e < order;
                q = warm ? 0u : q;
                add = warm ? 0u : add;
                v = warm ? 0u : v;
            }
            pe += q + add;
            put_end(pe, v);
            if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
    // an escaped partition (encode.rs:3898-3907): raw residuals of `eb` bits through the lane's shift register
    br.init(sb, pos + incl - mybits);
    if (head) { br.put(esc_code, hb); br.put(eb, 5); }
    if (eb) {
        const uint32_t emask = eb >= 32 ? 0xFFFFFFFFu : (1u << eb) - 1u;
#pragma unroll
        for (int e = 0; e < SPL; e++)
            if (e >= MAXO || (uint32_t)e >= first) {
                const uint32_t u = (uint32_t)x[e];
                br.put(((u >> 1) ^ (0u - (u & 1u))) & emask, eb);   // the residual back from its zigzag form
            }
    }
    br.finish();
}

// Register budget per instantiation, as waves per SIMD: 3 for the stereo 4096-sample instantiations (<= 168 VGPRs with
// the frame fetched in two halves; six workgroups per CU by their LDS frame); no request for the other 4096-sample shapes
// (160 VGPRs = three waves as well; 8 channels: the 102 KB LDS frame allows one workgroup per CU anyway); the frames of
// the shorter wave block lengths are latency bound -- a frame is one dependent chain of plan load, sample load, barriers
// and CRC lookups -- and get the budget their code needs anyway (88 / 102-127 VGPRs: 5 / 4 waves).  The second number of
// amdgpu_waves_per_eu is a CAP the compiler enforces by padding the register count: until r03 every instantiation but
// the stereo one carried "1, 2" and ran two waves per SIMD whatever it used (1152-sample frames: 0.258 -> 0.134 ms
// per 67 M samples without it, 1024: 0.316 -> 0.142).
#define F64_W18 5
#define F64_W36 4
#define F64_W64 3
#define F64_WAVES(nt, spl) (((nt) == 128 && (spl) == 64) ? F64_W64 : ((nt) <= 256 && (spl) <= 18) ? F64_W18 : ((nt) <= 256 && (spl) <= 36) ? F64_W36 : 1)
// XP (NT = 192 / 256: three / four independent channels, the batch interleaved in Params::split_src): the waves fetch their samples
// together through load_lane_xpose (wave_cand.inc) -- no planar rows exist; the transposing buffer is the frame's image area,
// which is therefore zeroed (and given its header) only after the load
template <int NT, int SPL, int MAXO, bool DIRECT = false, bool XP = false>
__global__ void __launch_bounds__(NT)
__attribute__((amdgpu_waves_per_eu((!DIRECT && SPL == 36) ? 3 : F64_WAVES(NT, SPL), (NT == 128 && SPL == 64) ? F64_WAVES(NT, SPL) : 8))) k_frame64(Params p, PackParams q) {   // (2304-sample blocks from planar rows: 132 registers since the direct Rice emitter; the in-place instantiation needs 104)
    static_assert(!DIRECT || NT == 128, "direct input: interleaved stereo");
    static_assert(!XP || ((NT == 192 || NT == 256) && !DIRECT), "transposing load: a whole frame of three or four channels");
    constexpr uint32_t N = 64u * SPL;
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    __shared__ __attribute__((aligned(16))) uint16_t T[4][256];  // slicing-by-4 tables
    __shared__ uint32_t part[NT / 64];
    const uint32_t frame = p.f0 + blockIdx.x, tid = threadIdx.x;
    const uint32_t ch = __builtin_amdgcn_readfirstlane(tid >> 6);
#if FRAME_TIMELINE   // measurement builds (tools/cand_timeline.py --kernel frame): 100 MHz stamps of the wave's phases in its candidate's autocorrelation row
    uint64_t *const tl_row = (DIRECT && p.ncand >= NT / 64) ? reinterpret_cast<uint64_t *>(p.ac) + ((size_t)frame * p.ncand + ch) * AC_LD : nullptr;
#define FRAME_STAMP(k) do { if (tl_row) { const uint64_t t_ = __builtin_amdgcn_s_memrealtime(); if ((tid & 63) == 0) tl_row[k] = t_; } } while (0)
#else
#define FRAME_STAMP(k) do { } while (0)
#endif
    FRAME_STAMP(0);
    uint32_t *fb = reinterpret_cast<uint32_t *>(lds);
    const uint64_t fn = frame_number_of(q, frame);
    const HeaderCodes hc = header_codes(N, q.sample_rate, fn);
    const uint64_t begin = q.frame_off[frame];
    const uint32_t flen = (uint32_t)(q.frame_off[frame + 1] - begin);  // bytes, CRC-16 included
    const uint32_t nwords = (flen + 3) / 4 + 1;
    // DIRECT: the image is prepared INSIDE wave_subframe, while the plan and the first half of the samples travel --
    // before, the table copy, the frame's length and the earlier subframe's bit count each cost the workgroup a round trip of
    // their own in front of the one the samples need (tools/frame_timeline.py: 2.9 us of a workgroup's 18.7)
    constexpr bool EARLY = DIRECT && !XP && NT == 128;
    if constexpr (!EARLY) {
    for (uint32_t i = tid; i < 128; i += NT)
        reinterpret_cast<uint4 *>(&T[0][0])[i] = reinterpret_cast<const uint4 *>(&kCrcT.t[0][0])[i];
    }
    auto begin_image = [&]() {
    // (the whole image as launched -- a few stores more, but the frame's length, which comes from memory, is first needed
    // behind the subframes)
    const uint32_t zq = q.fb_words ? q.fb_words / 4 : (nwords + 3) / 4;
    for (uint32_t i = tid; i < zq; i += NT) reinterpret_cast<uint4 *>(fb)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (tid == 0) {  // FrameHeader::build, stream.rs:242-276 (+ CRC-8, :194-197)
        const flacgpu_frame_plan fp = p.frame_plan[frame];
        const uint32_t acode = fp.assignment == FLACGPU_ASSIGN_INDEPENDENT ? p.channels - 1 : fp.assignment;
        const uint32_t pcode = p.bps == 8 ? 1 : p.bps == 12 ? 2 : p.bps == 16 ? 4 : p.bps == 20 ? 5
                             : p.bps == 24 ? 6 : p.bps == 32 ? 7 : 0;
        put_frame_header(fb, 0u, hc, fn, N, acode, pcode);
    }
    };
    if constexpr (EARLY) {
        const uint4 tl = reinterpret_cast<const uint4 *>(&kCrcT.t[0][0])[tid];   // (2048 bytes: one piece per thread)
        uint32_t prev_bits = 0;
        if (ch) prev_bits = p.out_plan[(size_t)frame * p.channels].bits;          // (wave 1 follows subframe 0)
        flacgpu_frame_plan fp{};
        if (tid == 0) fp = p.frame_plan[frame];
        auto prepare = [&](uint32_t *&, uint32_t &base) {
            const uint32_t zq = q.fb_words ? q.fb_words / 4 : (nwords + 3) / 4;
            for (uint32_t i = tid; i < zq; i += NT) reinterpret_cast<uint4 *>(fb)[i] = make_uint4(0, 0, 0, 0);
            reinterpret_cast<uint4 *>(&T[0][0])[tid] = tl;
            // (a bare barrier: __syncthreads() would wait for the samples as well)
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (tid == 0) {  // FrameHeader::build, stream.rs:242-276 (+ CRC-8, :194-197)
                const uint32_t acode = fp.assignment == FLACGPU_ASSIGN_INDEPENDENT ? p.channels - 1 : fp.assignment;
                const uint32_t pcode = p.bps == 8 ? 1 : p.bps == 12 ? 2 : p.bps == 16 ? 4 : p.bps == 20 ? 5
                                     : p.bps == 24 ? 6 : p.bps == 32 ? 7 : 0;
                put_frame_header(fb, 0u, hc, fn, N, acode, pcode);
            }
            base = header_bytes(hc) * 8 + prev_bits;
            FRAME_STAMP(1);   // image zeroed, tables copied, header written
        };
        wave_subframe<SPL, MAXO, true, true>(p, frame, ch, fb, 0u, prepare);
    } else {
    if constexpr (!XP) begin_image();
    FRAME_STAMP(1);   // image zeroed, tables copied, header written
    uint32_t start_bit = header_bytes(hc) * 8;
    for (uint32_t c = 0; c < ch; c++) start_bit += p.out_plan[(size_t)frame * p.channels + c].bits;
    if constexpr (XP) {
        auto fetch = [&](int32_t (&x)[SPL]) {
            load_lane_xpose_cw<SPL, NT / 64>(split_frame(p, frame, 64u * SPL * (NT / 64)), 0u, 0u, NT / 64, lds, tid, x);
            __syncthreads();   // every wave has read its last turn out of the buffer
            begin_image();
        };
        wave_subframe<SPL, MAXO, false, false>(p, frame, ch, fb, start_bit, PlaceAsGiven(), LoadWith<decltype(fetch)>{fetch});
    } else {
        wave_subframe<SPL, MAXO, DIRECT, NT == 128>(p, frame, ch, fb, start_bit);
    }
    }
    FRAME_STAMP(2);   // subframe emitted
    __syncthreads();
    FRAME_STAMP(3);
    // ---- CRC-16 of bytes [0, len) (crc.rs:142-188); byte i = fb[i / 4] >> (24 - 8 (i % 4)): the whole words by all lanes
    // (crc16_words_share), the <= 3 bytes behind them by the lane that writes the result
    const uint32_t len = flen - 2;
    const uint32_t nw4 = len >> 2;
    constexpr int SW = 17;
    constexpr uint32_t CHW = NT * SW;                // words per slice row
    const uint32_t S = (nw4 + CHW - 1) / CHW;        // 0..3 (frame_fb_words bounds the frame; slices of 9 words -- half the
                                                     // dependent table round trips, two more folds -- measured slower)
    const uint32_t padw = S * CHW - nw4;
    uint32_t running = 0;
    if (S) {
        uint32_t c;
        c = S == 1 ? crc16_words_share<NT, 1>(fb, padw, tid, T)
          : S == 2 ? crc16_words_share<NT, 2>(fb, padw, tid, T)
                   : crc16_words_share<NT, 3>(fb, padw, tid, T);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c ^= __shfl_xor(c, off, 64);
        if ((tid & 63) == 0) part[tid >> 6] = c;
        __syncthreads();
#pragma unroll
        for (int wv = 0; wv < NT / 64; wv++) running ^= part[wv];
    }
    if (tid == 0) running = crc16_tail(running, fb[nw4], len & 3u, T);
    if (tid == 0) {  // the two CRC bytes follow byte len - 1 (still zero there)
        atomicOr(&fb[len >> 2], ((running >> 8) & 0xFF) << (24 - 8 * (len & 3)));
        atomicOr(&fb[(len + 1) >> 2], (running & 0xFF) << (24 - 8 * ((len + 1) & 3)));
    }
    __syncthreads();
    FRAME_STAMP(4);   // CRC-16 done
    // ---- copy out: output dword j covers frame bytes [4 j - r, 4 j - r + 4)
    uint8_t *ob = reinterpret_cast<uint8_t *>(q.out_words);
    const uint32_t r = (uint32_t)(begin & 3);
    uint32_t *og = reinterpret_cast<uint32_t *>(ob + (begin - r));
    const uint32_t nout = (r + flen + 3) / 4;
    auto emit = [&](uint32_t j, uint32_t m) {   // m: MSB-first window of output dword j
        const int32_t fbyte = (int32_t)(4 * j) - (int32_t)r;
        if (fbyte >= 0 && fbyte + 4 <= (int32_t)flen) {
            og[j] = __builtin_bswap32(m);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int32_t fbk = fbyte + e;
                if (fbk >= 0 && fbk < (int32_t)flen) ob[begin + fbk] = (uint8_t)(m >> (24 - 8 * e));
            }
        }
    };
    // a lane moves FOUR consecutive output dwords per turn: one 16-byte LDS read (+ the dword before it for the
    // byte shift), four funnel shifts, one 16-byte store -- a wave writes 1 KB of contiguous output per instruction
    // (dword by dword this loop was ~15 % of the kernel's instructions)
    // (COPY_AHEAD turns' LDS reads requested together: four measured no faster than one, profiles/r05_frame_timeline.json)
    constexpr uint32_t COPY_AHEAD = 1;
    for (uint32_t jb = 4 * tid; jb < nout; jb += 4 * NT * COPY_AHEAD) {
    uint4 wq[COPY_AHEAD];
    uint32_t pq[COPY_AHEAD];
#pragma unroll
    for (uint32_t u = 0; u < COPY_AHEAD; u++) {
        const uint32_t jj = jb + 4 * NT * u;
        const uint32_t jc = jj < nout ? jj : jb;                          // (a turn past the end repeats the first one's reads)
        wq[u] = *reinterpret_cast<const uint4 *>(fb + jc);               // (16-byte aligned; words past the frame are read, never stored)
        pq[u] = (r && jc) ? fb[jc - 1] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < COPY_AHEAD; u++) {
        const uint32_t j0 = jb + 4 * NT * u;
        if (j0 >= nout) break;
        const uint4 w = wq[u];
        const uint32_t prev = pq[u];
        const int32_t fbyte = (int32_t)(4 * j0) - (int32_t)r;
        const uint32_t sh = 8 * r;                                       // alignbit(hi, lo, 0) = lo
        const uint32_t m0 = __builtin_amdgcn_alignbit(prev, w.x, sh), m1 = __builtin_amdgcn_alignbit(w.x, w.y, sh),
                       m2 = __builtin_amdgcn_alignbit(w.y, w.z, sh), m3 = __builtin_amdgcn_alignbit(w.z, w.w, sh);
        if (fbyte >= 0 && fbyte + 16 <= (int32_t)flen) {
            // (4-byte aligned only: a frame starts at any byte of the output)
            struct __attribute__((packed, aligned(4))) Out4 { uint32_t x, y, z, w; };
            *reinterpret_cast<Out4 *>(og + j0) = Out4{__builtin_bswap32(m0), __builtin_bswap32(m1), __builtin_bswap32(m2),
                                                     __builtin_bswap32(m3)};
        } else {   // the frame's first and last dwords: byte by byte where they stick out
            const uint32_t ms[4] = {m0, m1, m2, m3};
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (j0 + e < nout) emit(j0 + e, ms[e]);
        }
    }
    }
    FRAME_STAMP(5);   // copied out
#undef FRAME_STAMP
}

// VERIFY = false: store the CRC-16 behind the frame; true: compare with the stored one and
// count mismatching frames in verify_counts[1]
template <bool VERIFY>
__global__ void __launch_bounds__(WG) k_crc(Params p, PackParams q, uint32_t *verify_counts) {
    __shared__ uint16_t T[4][256];                 // slicing-by-4 tables
    __shared__ uint32_t buf[CRC_CHUNK / 4 + WG];   // one pad dword per 64-byte slice
    __shared__ uint32_t part[4];
    const uint32_t frame = p.f0 + blockIdx.x, tid = threadIdx.x;
    {
        uint32_t c = tid << 8;
        for (int k = 0; k < 4; k++) {  // T[k][b] = CRC state after byte b followed by k zero bytes
            for (int b = 0; b < 8; b++) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
            T[k][tid] = (uint16_t)c;
        }
    }
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(q.out_words);
    const uint64_t begin = q.frame_off[frame];
    const uint32_t len = (uint32_t)(q.frame_off[frame + 1] - begin) - 2;  // all but the CRC itself
    const uint32_t my_weight = kCrcW.w[WG - 1 - tid];   // slices to the right of mine
    const uint32_t xchunk = kCrcW.w[WG];                // x^(8 * CRC_CHUNK)
    uint32_t running = 0;
    uint32_t pos = 0;
    while (pos < len) {
        // the FIRST pass takes the odd-sized head so every later pass is a full chunk; a chunk
        // is right-aligned in the LDS window, i.e. left-padded with zero bytes, which leave a
        // zero CRC state unchanged -- all 256 slices then have the same length
        const uint32_t clen = (pos == 0 && (len % CRC_CHUNK)) ? len % CRC_CHUNK : CRC_CHUNK;
        const uint32_t padb = CRC_CHUNK - clen;
        __syncthreads();
        for (uint32_t d = tid; d < CRC_CHUNK / 4; d += WG) {
            uint32_t v = 0;
            const int64_t j0 = (int64_t)4 * d - padb;  // chunk byte index of this dword's first byte
            if (j0 + 3 >= 0) {
                const uint64_t src = begin + pos;
                if (j0 >= 0 && ((src + j0) & 3) == 0) {
                    v = *reinterpret_cast<const uint32_t *>(bytes + src + j0);
                } else {
                    for (int e = 0; e < 4; e++)
                        if (j0 + e >= 0) v |= (uint32_t)bytes[src + j0 + e] << (8 * e);
                }
            }
            buf[d + (d >> 4)] = v;
        }
        __syncthreads();
        uint32_t crc = 0;
        const uint32_t *sl = buf + tid * 17;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const uint32_t v = sl[w];
            crc = T[3][((crc >> 8) ^ v) & 0xFF] ^ T[2][(crc ^ (v >> 8)) & 0xFF] ^
                  T[1][(v >> 16) & 0xFF] ^ T[0][v >> 24];
        }
        // CRC (init 0) is GF(2)-linear: crc(chunk) = XOR_t crc(slice_t) * x^(512 * slices after t)
        uint32_t c = gf_mulmod(crc, my_weight);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c ^= __shfl_xor(c, off, 64);
        if ((tid & 63) == 0) part[tid >> 6] = c;
        __syncthreads();
        running = gf_mulmod(running, xchunk) ^ part[0] ^ part[1] ^ part[2] ^ part[3];
        pos += clen;
    }
    if (tid == 0) {
        uint8_t *ob = reinterpret_cast<uint8_t *>(q.out_words);
        if constexpr (VERIFY) {
            const uint32_t stored = ((uint32_t)ob[begin + len] << 8) | ob[begin + len + 1];
            if (stored != running) atomicAdd(&verify_counts[1], 1u);
        } else {
            ob[begin + len] = (uint8_t)(running >> 8);
            ob[begin + len + 1] = (uint8_t)running;
        }
    }
}
