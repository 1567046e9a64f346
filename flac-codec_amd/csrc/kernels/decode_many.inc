// decode_many.inc -- the batch decoder's frame kernels and MD5 (decode_many.hip).
// Included inside decode_many.hip's anonymous namespace, after decode.inc, crc16.inc and frame_scan.inc.
//   K_d1 k_decode_many   lane per frame: k_decode_frames with a per-frame descriptor (streams of any shape in one
//                        launch), planar scratch of exactly channels x roundup4(n) samples per frame
//   K_d2 k_frame_crc     wave per frame: CRC-16 of the frame, stored CRC included, must be 0
//   K_d3 k_finish_many   workgroup per frame: undoes the stereo decorrelation (k_decode_finish's arithmetic) and
//                        writes interleaved int32 at the stream's output offset
//   K_d4 k_md5_many      lane per stream: MD5 of the stream's interleaved samples as ceil(bps / 8)-byte
//                        little-endian values (decode.rs:1282-1310 `verify`)
//   K_d5 k_finish_as     workgroup per frame: k_finish_many's arithmetic, the samples converted in registers to
//                        int16 / packed 24-bit / float32 (or left int32) and written flat or into padded planar rows;
//                        with MD5 also
//                        the interleaved int32 that k_md5_many reads
//   K_d6 k_pad_rows      workgroup per (stream, channel row) of a padded batch: zeroes what no frame writes
//   K_d7 k_finish_window workgroup per selected frame of a sample window (flacgpu_decoder_decode_windows): k_finish_as's
//                        arithmetic and conversions on the part of the frame the window keeps, into the window's rows
//   K_d8 k_fill_runs     workgroup per run of a timeline (flacgpu_decoder_decode_timeline): a byte value over a run of
//                        elements that begins and ends anywhere in a row -- the gaps, and, decided by the per-frame
//                        counts, the frames that did not decode; the mask likewise

struct ManyFrame {
    uint64_t start, end;   // byte offsets in the batch buffer: header .. CRC-16 inclusive
    uint64_t cap;          // the slot's end - 4: the bit reader never leaves the slot's zero tail
    uint64_t scratch;      // first planar sample of the frame (channel rows of roundup4(n) samples)
    uint64_t out;          // first interleaved sample of the frame in the output
    uint32_t n, slot, channels, bps;   // n: the scan's block size; channels / bps: STREAMINFO
};

template <int MAXO>
__global__ void __launch_bounds__(64) k_decode_many(const uint32_t *__restrict__ words,
                                                    const ManyFrame *__restrict__ frames, uint32_t n_frames,
                                                    int32_t *__restrict__ scratch, uint32_t *__restrict__ codes) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    const ManyFrame fr = frames[f];
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
    const uint32_t end_bit = (uint32_t)(fr.end - fr.start) * 8;
    const uint32_t ldb = (fr.n + 3u) & ~3u;
    BitReader r;
    r.init(words, fr.start, fr.cap, 0);
    FrameHead fh;
    bool bad = !parse_frame_header(r, bytes, fr.start, fh);
    const uint32_t n = fh.n, acode = fh.acode;
    const uint32_t bps = bps_of_code(fh.bps_code, fr.bps);
    const uint32_t nch = acode < 8 ? acode + 1 : 2;
    if (n != fr.n || bps != fr.bps || nch != fr.channels) bad = true;
    for (uint32_t c = 0; c < nch && !bad; c++) {
        int32_t *__restrict__ x = scratch + fr.scratch + (size_t)c * ldb;
        int32_t *mid = (c == 1 && wide_mid_side(bps, acode)) ? x - ldb : nullptr;
        if (!decode_subframe<MAXO>(r, subframe_bps(bps, acode, c), n, x, end_bit, mid)) bad = true;
    }
    if (!bad && ((r.pos() + 7) & ~7u) + 16 != end_bit) bad = true;
    if (!bad && (r.pos() & 7) && r.get(8 - (r.pos() & 7)) != 0) bad = true;
    codes[f] = (bad ? 0x100u : 0u) | (wide_mid_side(bps, acode) ? 1u : acode);   // 1: nothing left to undo
}

// the CRC-16 of the whole frame, its stored CRC included, is 0 exactly when the stored CRC is right
__global__ void __launch_bounds__(64) k_frame_crc(const uint8_t *__restrict__ bytes,
                                                  const ManyFrame *__restrict__ frames,
                                                  uint32_t *__restrict__ slot_counts) {
    __shared__ uint16_t T[256];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 256; i += 64) {
        uint32_t c = i << 8;
        for (int b = 0; b < 8; b++) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
        T[i] = (uint16_t)c;
    }
    __syncthreads();
    const ManyFrame fr = frames[blockIdx.x];
    const uint64_t len = fr.end - fr.start;
    const uint64_t per = (len + 63) / 64;
    const uint64_t a = min(len, tid * per), e = min(len, a + per);
    uint32_t crc = 0;
    for (uint64_t i = a; i < e; i++) crc = ((crc << 8) & 0xFFFFu) ^ T[((crc >> 8) ^ bytes[fr.start + i]) & 0xFFu];
    uint32_t c = gf_mulmod(crc, gf_xpow_bytes(len - e));   // weighted by the bytes behind the slice
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c ^= __shfl_xor(c, off, 64);
    if (tid == 0 && c) atomicAdd(&slot_counts[2 * fr.slot + 1], 1u);
}

// k_decode_finish's decorrelation (decode.inc), planar scratch -> interleaved output.  A frame that did not parse is
// counted and written as decoded (what flacgpu_decode_stream leaves for it: not defined by the stream).
__global__ void __launch_bounds__(WG) k_finish_many(const ManyFrame *__restrict__ frames,
                                                    const int32_t *__restrict__ scratch,
                                                    const uint32_t *__restrict__ codes, int32_t *__restrict__ out,
                                                    uint32_t *__restrict__ slot_counts) {
    const uint32_t f = blockIdx.x;
    const ManyFrame fr = frames[f];
    const uint32_t code = codes[f], acode = code & 0xFFu;
    const bool bad = code & 0x100u;
    if (bad && threadIdx.x == 0) atomicAdd(&slot_counts[2 * fr.slot], 1u);
    const uint32_t n = fr.n, C = fr.channels, ldb = (n + 3u) & ~3u;
    const int32_t *rows = scratch + fr.scratch;
    int32_t *o = out + fr.out;
    if (!bad && acode >= 8) {
        for (uint32_t i = threadIdx.x; i < n; i += WG) {
            const long long a = rows[i], b = rows[ldb + i];
            long long l, rr;
            if (acode == 8) { l = a; rr = a - b; }
            else if (acode == 9) { l = a + b; rr = b; }
            else {
                const long long sum = a * 2 + ((b < 0 ? -b : b) & 1);
                l = (sum + b) >> 1;
                rr = (sum - b) >> 1;
            }
            o[2 * (size_t)i] = (int32_t)l;
            o[2 * (size_t)i + 1] = (int32_t)rr;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += WG)
            for (uint32_t c = 0; c < C; c++) o[(size_t)i * C + c] = rows[(size_t)c * ldb + i];
    }
}

// ---- other sample formats and layouts (flacgpu_decoder_decode_as) ----
constexpr uint32_t DT_I32 = 0, DT_I16 = 1, DT_F32 = 2, DT_S24 = 24;   // FLACGPU_SAMPLE_*
// bytes per element; S24 elements are 3 bytes, little-endian, packed
template <uint32_t DT> constexpr uint32_t elem_bytes() { return DT == DT_I16 ? 2 : DT == DT_S24 ? 3 : 4; }

// One sample of a frame, the stereo decorrelation undone: k_finish_many's arithmetic (64-bit mid/side; a code of 1
// means that nothing is left to undo), kept apart from it so that its code stays as it is.
__device__ __forceinline__ int32_t frame_sample(const int32_t *__restrict__ rows, uint32_t ldb, uint32_t acode,
                                                uint32_t i, uint32_t c) {
    if (acode < 8) return rows[(size_t)c * ldb + i];
    const long long a = rows[i], b = rows[ldb + i];
    long long l, rr;
    if (acode == 8) { l = a; rr = a - b; }
    else if (acode == 9) { l = a + b; rr = b; }
    else {
        const long long sum = a * 2 + ((b < 0 ? -b : b) & 1);
        l = (sum + b) >> 1;
        rr = (sum - b) >> 1;
    }
    return (int32_t)(c ? rr : l);
}

// The bits of one output element: I16 sample << (16 - bps) in the low half, S24 sample << (24 - bps) in the low 24
// bits (bits 24-31 zero: store_run3 ORs neighbours together), F32 (float)sample * 2^-(bps - 1)
// (the int -> float conversion rounds to nearest even, the scale is a power of two and so exact).
template <uint32_t DT> __device__ __forceinline__ uint32_t sample_bits(int32_t v, uint32_t bps) {
    if (DT == DT_S24) return ((uint32_t)v << ((24u - bps) & 31u)) & 0xFFFFFFu;
    if (DT == DT_I16) return ((uint32_t)v << ((16u - bps) & 15u)) & 0xFFFFu;
    if (DT == DT_F32) return __float_as_uint(__int2float_rn(v) * __uint_as_float((128u - bps) << 23));
    return (uint32_t)v;
}

// n elements of ES bytes to dst (ES-aligned), element e = get(e) in the low bits of a dword: single elements up to
// the first 16-byte boundary, then 16 bytes per lane (consecutive lanes, consecutive 16 bytes), then single elements.
template <uint32_t ES, class Get>
__device__ __forceinline__ void store_run(uint8_t *dst, uint32_t n, uint32_t tid, uint32_t nthreads, Get get) {
    constexpr uint32_t V = 16 / ES;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u) / ES;
    const uint32_t head = min(n, (V - mis) % V);
    const uint32_t nv = (n - head) / V, tail_at = head + nv * V;
    if (tid < head) {
        if (ES == 2) reinterpret_cast<uint16_t *>(dst)[tid] = (uint16_t)get(tid);
        else reinterpret_cast<uint32_t *>(dst)[tid] = get(tid);
    }
    uint4 *body = reinterpret_cast<uint4 *>(dst + (size_t)head * ES);
    for (uint32_t v = tid; v < nv; v += nthreads) {
        const uint32_t e = head + v * V;
        uint4 w;
        if (ES == 2) {
            w.x = get(e) | get(e + 1) << 16;
            w.y = get(e + 2) | get(e + 3) << 16;
            w.z = get(e + 4) | get(e + 5) << 16;
            w.w = get(e + 6) | get(e + 7) << 16;
        } else {
            w.x = get(e);
            w.y = get(e + 1);
            w.z = get(e + 2);
            w.w = get(e + 3);
        }
        body[v] = w;
    }
    if (tid < n - tail_at) {
        const uint32_t e = tail_at + tid;
        if (ES == 2) reinterpret_cast<uint16_t *>(dst)[e] = (uint16_t)get(e);
        else reinterpret_cast<uint32_t *>(dst)[e] = get(e);
    }
}

// n packed 3-byte elements to dst (any byte address), element e = get(e) in the low 24 bits of a dword, bits 24-31
// zero.  The run is the 3n bytes [dst, dst + 3n): byte b belongs to element b / 3 and is its byte b % 3.  Single bytes
// up to the first 16-byte boundary (at most 15; an element may straddle the boundary), then 16 bytes per lane
// (consecutive lanes, consecutive 16 bytes), then single bytes (at most 15).  Every byte of the run is stored exactly
// once and no other byte is touched: two runs that meet at any byte (adjacent frames of a FLAT stream) never write the
// same byte.  Indices are 32-bit (3n < 2^32: n <= 65535 * 8), so that / 3 is a multiply-high.
// A 16-byte group at run byte B (B + 16 <= 3n), with e0 = B / 3 and r = B % 3, holds bytes of elements e0 .. e0 + 5 and
// of no other: its last byte B + 15 belongs to element (B + 15) / 3 = e0 + (r + 15) / 3 = e0 + 5 for r = 0, 1, 2.  That
// byte lies inside the run, B + 15 <= 3n - 1, hence e0 + 5 <= (3n - 1) / 3 = n - 1: get(n) is never needed, nor any
// element whose bytes the group does not hold.  The 18 bytes of the six elements are put together from e0's first byte
// on (u0 .. u4) and shifted down by r bytes; dword k of the group is then get-bits of run bytes B + 4k .. B + 4k + 3,
// which is get(e) >> 8r' | get(e + 1) << (24 - 8r') for e = (B + 4k) / 3, r' = (B + 4k) % 3.
template <class Get>
__device__ __forceinline__ void store_run3(uint8_t *dst, uint32_t n, uint32_t tid, uint32_t nthreads, Get get) {
    const uint32_t bytes = 3u * n;
    const uint32_t head = min(bytes, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    const uint32_t nv = (bytes - head) / 16u, tail_at = head + nv * 16u;
    if (tid < head) dst[tid] = (uint8_t)(get(tid / 3u) >> (8u * (tid % 3u)));
    uint4 *body = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t v = tid; v < nv; v += nthreads) {
        const uint32_t at = head + v * 16u, e = at / 3u, sh = 8u * (at - 3u * e);
        const uint32_t g0 = get(e), g1 = get(e + 1), g2 = get(e + 2), g3 = get(e + 3), g4 = get(e + 4), g5 = get(e + 5);
        const uint64_t u10 = (uint64_t)(g0 | g1 << 24) | (uint64_t)(g1 >> 8 | g2 << 16) << 32;
        const uint64_t u21 = (u10 >> 32) | (uint64_t)(g2 >> 16 | g3 << 8) << 32;
        const uint64_t u32 = (u21 >> 32) | (uint64_t)(g4 | g5 << 24) << 32;
        const uint64_t u43 = (u32 >> 32) | (uint64_t)(g5 >> 8) << 32;
        body[v] = make_uint4((uint32_t)(u10 >> sh), (uint32_t)(u21 >> sh), (uint32_t)(u32 >> sh),
                             (uint32_t)(u43 >> sh));
    }
    if (tid < bytes - tail_at) {
        const uint32_t b = tail_at + tid;
        dst[b] = (uint8_t)(get(b / 3u) >> (8u * (b % 3u)));
    }
}

// a run of n elements of DT: store_run, or store_run3 for the packed 3-byte elements
template <uint32_t ES, class Get>
__device__ __forceinline__ void store_elems(uint8_t *dst, uint32_t n, uint32_t tid, uint32_t nthreads, Get get) {
    if constexpr (ES == 3) store_run3(dst, n, tid, nthreads, get);
    else store_run<ES>(dst, n, tid, nthreads, get);
}

// pad_out (PADDED only): the frame's first element of channel 0, row + the frame's first sample; channel c is
// samples_padded elements further per channel.  side (MD5 only): interleaved int32 at the frame's flat offset,
// written as k_finish_many writes it.
template <uint32_t DT, bool PADDED, bool SIDE>
__global__ void __launch_bounds__(WG) k_finish_as(const ManyFrame *__restrict__ frames,
                                                  const int32_t *__restrict__ scratch,
                                                  const uint32_t *__restrict__ codes, uint8_t *__restrict__ out,
                                                  const uint64_t *__restrict__ pad_out, uint64_t samples_padded,
                                                  int32_t *__restrict__ side, uint32_t *__restrict__ slot_counts) {
    constexpr uint32_t ES = elem_bytes<DT>();
    const uint32_t f = blockIdx.x;
    const ManyFrame fr = frames[f];
    const uint32_t code = codes[f];
    const bool bad = code & 0x100u;
    const uint32_t acode = bad ? 0u : (code & 0xFFu);   // a frame that did not parse is written as decoded
    if (bad && threadIdx.x == 0) atomicAdd(&slot_counts[2 * fr.slot], 1u);
    const uint32_t n = fr.n, C = fr.channels, bps = fr.bps, ldb = (n + 3u) & ~3u;
    const int32_t *rows = scratch + fr.scratch;
    if (PADDED) {
        for (uint32_t c = 0; c < C; c++)
            store_elems<ES>(out + (pad_out[f] + (uint64_t)c * samples_padded) * ES, n, threadIdx.x, WG, [&](uint32_t i) {
                return sample_bits<DT>(frame_sample(rows, ldb, acode, i, c), bps);
            });
    } else {
        uint8_t *o = out + fr.out * ES;
        if (C == 1)
            store_elems<ES>(o, n, threadIdx.x, WG,
                          [&](uint32_t e) { return sample_bits<DT>(rows[e], bps); });
        else if (C == 2)
            store_elems<ES>(o, 2 * n, threadIdx.x, WG, [&](uint32_t e) {
                return sample_bits<DT>(frame_sample(rows, ldb, acode, e >> 1, e & 1u), bps);
            });
        else
            store_elems<ES>(o, C * n, threadIdx.x, WG, [&](uint32_t e) {
                return sample_bits<DT>(rows[(size_t)(e % C) * ldb + e / C], bps);
            });
    }
    if (SIDE) {
        int32_t *o = side + fr.out;
        for (uint32_t i = threadIdx.x; i < n; i += WG)
            for (uint32_t c = 0; c < C; c++) o[(size_t)i * C + c] = frame_sample(rows, ldb, acode, i, c);
    }
}

struct PadStream {
    uint64_t samples;    // decoded samples per channel; 0 for a stream with rc != 0
    uint32_t channels;   // 0 for a stream with rc != 0
    uint32_t reserved;
};
// `bytes` bytes from p, every one the low byte of w (w: that byte four times), by one workgroup: single elements of ES
// bytes up to the first 16-byte boundary (ES == 1 and ES == 3: single bytes, such a run begins and ends at any byte), 16
// bytes per lane, consecutive lanes consecutive groups, single elements behind the last whole group.  Exactly these
// bytes are written.  For ES == 2 and 4 p is ES-aligned, so that head and tail are whole elements.  Len: uint64_t for a
// row of a padded batch, uint32_t for a run of at most kFillPiece bytes.
template <uint32_t ES, class Len> __device__ __forceinline__ void fill_bytes(uint8_t *p, Len bytes, uint32_t w) {
    const Len head = min(bytes, (Len)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u));
    const Len nv = (bytes - head) / 16, tail_at = head + nv * 16;
    constexpr bool BYTES = ES == 1 || ES == 3;
    if (BYTES) {
        if (threadIdx.x < head) p[threadIdx.x] = (uint8_t)w;
    } else if (threadIdx.x * ES < head) {
        if (ES == 2) reinterpret_cast<uint16_t *>(p)[threadIdx.x] = (uint16_t)w;
        else reinterpret_cast<uint32_t *>(p)[threadIdx.x] = w;
    }
    uint4 *body = reinterpret_cast<uint4 *>(p + head);
    for (Len v = threadIdx.x; v < nv; v += WG) body[v] = make_uint4(w, w, w, w);
    if (BYTES) {
        if (threadIdx.x < bytes - tail_at) p[tail_at + threadIdx.x] = (uint8_t)w;
    } else if (threadIdx.x * ES < bytes - tail_at) {
        if (ES == 2) reinterpret_cast<uint16_t *>(p + tail_at)[threadIdx.x] = (uint16_t)w;
        else reinterpret_cast<uint32_t *>(p + tail_at)[threadIdx.x] = w;
    }
}
// Workgroup per (stream, channel row): zeroes [decoded_samples, samples_padded) of a channel the stream has and the
// whole row of one it has not (fill_bytes: a row of packed 24-bit elements begins and ends at any byte).
template <uint32_t ES>
__global__ void __launch_bounds__(WG) k_pad_rows(const PadStream *__restrict__ streams, uint32_t channels_padded,
                                                 uint64_t samples_padded, uint8_t *__restrict__ out) {
    const uint32_t s = blockIdx.x / channels_padded, c = blockIdx.x % channels_padded;
    const PadStream ps = streams[s];
    const uint64_t from = c < ps.channels ? ps.samples : 0;
    fill_bytes<ES, uint64_t>(out + ((uint64_t)blockIdx.x * samples_padded + from) * ES, (samples_padded - from) * ES, 0u);
}

// ---- MD5 (RFC 1321) ----
struct Md5Job {
    uint64_t off;        // first interleaved sample of the stream in the output
    uint64_t count;      // interleaved samples
    uint32_t width;      // bytes per sample: ceil(bps / 8)
    uint32_t reserved;
    uint32_t expect[4];  // STREAMINFO's MD5
};
struct Md5Consts {
    uint32_t k[64];
    constexpr Md5Consts() : k() {
        const uint32_t t[64] = {
            0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
            0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
            0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
            0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
            0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
            0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
            0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
            0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
        for (int i = 0; i < 64; i++) k[i] = t[i];
    }
};
constexpr Md5Consts kMd5 = Md5Consts();
__device__ __forceinline__ void md5_block(uint32_t (&s)[4], const uint32_t (&m)[16]) {
    constexpr int R[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        uint32_t f;
        int g;
        if (i < 16) { f = (b & c) | (~b & d); g = i; }
        else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
        else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
        else { f = c ^ (b | ~d); g = (7 * i) & 15; }
        const uint32_t t = a + f + kMd5.k[i] + m[g];
        a = d;
        d = c;
        c = b;
        b = b + __builtin_rotateleft32(t, R[i >> 4][i & 3]);
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d;
}
// Lane per stream.  The message words are built in registers from the int32 samples: a 64-bit accumulator takes
// `width` bytes per sample and gives one word per 4 bytes; the 0x80 byte, zeros and the bit length follow the data.
// digest[5 * s]: the 16 digest bytes as 4 little-endian words, then md5_status (1 equal, 0 different, 2 no MD5).
__global__ void __launch_bounds__(64) k_md5_many(const int32_t *__restrict__ out, const Md5Job *__restrict__ jobs,
                                                 uint32_t n_jobs, uint32_t *__restrict__ digest) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_jobs) return;
    const Md5Job jb = jobs[s];
    const int32_t *src = out + jb.off;
    uint64_t left = jb.count;
    const uint32_t width = jb.width;
    const uint64_t wmask = (1ull << (8 * width)) - 1;
    const uint64_t bits = jb.count * width * 8;
    const uint64_t nblocks = (jb.count * width + 8) / 64 + 1;
    uint64_t acc = 0;
    uint32_t nb = 0;
    bool padded = false;
    uint32_t st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    for (uint64_t blk = 0; blk < nblocks; blk++) {
        const bool last = blk + 1 == nblocks;
        uint32_t m[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k >= 14 && last) {
                m[k] = k == 14 ? (uint32_t)bits : (uint32_t)(bits >> 32);
                continue;
            }
            while (nb < 4) {
                if (left) {
                    acc |= ((uint64_t)(uint32_t)*src++ & wmask) << (8 * nb);
                    nb += width;
                    left--;
                } else if (!padded) {
                    acc |= 0x80ull << (8 * nb);
                    nb += 1;
                    padded = true;
                } else {
                    nb = 4;
                }
            }
            m[k] = (uint32_t)acc;
            acc >>= 32;
            nb -= 4;
        }
        md5_block(st, m);
    }
    const bool none = (jb.expect[0] | jb.expect[1] | jb.expect[2] | jb.expect[3]) == 0;
    const bool same = st[0] == jb.expect[0] && st[1] == jb.expect[1] && st[2] == jb.expect[2] && st[3] == jb.expect[3];
    digest[5 * (size_t)s + 0] = st[0];
    digest[5 * (size_t)s + 1] = st[1];
    digest[5 * (size_t)s + 2] = st[2];
    digest[5 * (size_t)s + 3] = st[3];
    digest[5 * (size_t)s + 4] = none ? 2u : (same ? 1u : 0u);
}

// ---- sample windows (flacgpu_decoder_decode_windows) ----
// One selected frame of one window.  The frame's ManyFrame stands at the same index of the compact frame array; its
// `slot` is the window index there, so that k_frame_crc counts per window.
struct WinFrame {
    uint64_t row;          // first element of the window's channel 0 row in the output
    uint64_t at;           // the row position of the first kept sample: frame start + keep_first - window start
    uint32_t keep_first;   // samples [keep_first, keep_last) of the frame lie inside the window
    uint32_t keep_last;
    uint32_t channels, bps;
    uint32_t window;
    uint32_t reserved;
};
// Workgroup per selected frame: frame_sample's decorrelation and sample_bits' conversion of the kept samples, planar
// into the window's rows.  A row position is arbitrary, hence store_run / store_run3.  A frame that did not parse is counted for
// its window (win_counts[2 * window]) and written as decoded, as k_finish_as does.
template <uint32_t DT>
__global__ void __launch_bounds__(WG) k_finish_window(const ManyFrame *__restrict__ frames,
                                                      const WinFrame *__restrict__ win,
                                                      const int32_t *__restrict__ scratch,
                                                      const uint32_t *__restrict__ codes, uint8_t *__restrict__ out,
                                                      uint64_t samples_padded, uint32_t *__restrict__ win_counts) {
    constexpr uint32_t ES = elem_bytes<DT>();
    const uint32_t f = blockIdx.x;
    const ManyFrame fr = frames[f];
    const WinFrame w = win[f];
    const uint32_t code = codes[f];
    const bool bad = code & 0x100u;
    const uint32_t acode = bad ? 0u : (code & 0xFFu);
    if (bad && threadIdx.x == 0) atomicAdd(&win_counts[2 * w.window], 1u);
    const uint32_t ldb = (fr.n + 3u) & ~3u, bps = w.bps;
    const int32_t *rows = scratch + fr.scratch + w.keep_first;   // sample i of the run is sample keep_first + i
    for (uint32_t c = 0; c < w.channels; c++)
        store_elems<ES>(out + (w.row + (uint64_t)c * samples_padded + w.at) * ES, w.keep_last - w.keep_first, threadIdx.x,
                      WG, [&](uint32_t i) { return sample_bits<DT>(frame_sample(rows, ldb, acode, i, c), bps); });
}

// ---- frames on a timeline (flacgpu_decoder_decode_timeline) ----
// One run of a fill: `count` elements of ES bytes from element `first` of the output, every byte of them `value`
// (0 for samples; 0 or 1 for the mask, whose elements are bytes).  cond == FILL_ALWAYS: the run is always written (a gap,
// a row's tail in the mask, the 1s of a placed frame); else it is written only when frame `cond` of the compact table did
// not parse or failed its CRC-16 (counts[2 cond] / counts[2 cond + 1], as decode_frames reads them): the concealment.
// The host cuts a run into pieces of at most kFillPiece bytes (FLACGPU_TIMELINE_PIECE_BYTES) before it gets here.
constexpr uint32_t FILL_ALWAYS = 0xFFFFFFFFu;
constexpr uint32_t kFillPiece = FLACGPU_TIMELINE_PIECE_BYTES;
static_assert(kFillPiece % 48 == 0, "a piece is whole elements of 2, 3 and 4 bytes and whole 16-byte groups");
struct FillRun {
    uint64_t first;   // element index in the output
    uint32_t count;   // elements; count * ES <= kFillPiece
    uint32_t cond;    // FILL_ALWAYS, or the frame whose counts decide
    uint32_t value;   // the byte
    uint32_t reserved;
};
// K_d8 k_fill_runs  workgroup per run, k_pad_rows' shape (fill_bytes).  Exactly the run's bytes are written: its
// neighbours belong to other workgroups and to k_finish_window and k_pad_rows.  `out` is ES-aligned for ES == 2 and 4,
// hence so is every run.
template <uint32_t ES>
__global__ void __launch_bounds__(WG) k_fill_runs(const FillRun *__restrict__ runs, const uint32_t *__restrict__ counts,
                                                  uint8_t *__restrict__ out) {
    const FillRun r = runs[blockIdx.x];
    if (r.cond != FILL_ALWAYS && (counts[2 * (size_t)r.cond] | counts[2 * (size_t)r.cond + 1]) == 0) return;
    fill_bytes<ES, uint32_t>(out + r.first * ES, r.count * ES, (r.value & 0xFFu) * 0x01010101u);
}
