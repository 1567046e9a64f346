// frame_extent.h -- where a FLAC frame ends by its own bits: the walk over its subframes that finds the byte behind its
// CRC-16 without the header of a next frame (DESIGN.md 4b "A frame's own extent", FLACGPU_SCAN_SPECULATIVE).  One function
// for the host scan (scan_raw_frames, host/flac_stream.cpp) and the device scan (k_spec_end, kernels/spec_end.inc), so
// that the rule is tested without a GPU.  No sample is reconstructed and nothing is stored: VERBATIM bodies, warm-up
// samples, coefficients and escaped partitions are stepped over in one move, only Rice codes are walked one by one.
//
// The tests are those under which k_decode_many (decode_subframe, decode_subframe_wide, decode_residuals, the padding
// and the end check) accepts a frame, with the end unknown:
//   per coded channel   1 pad bit (0), 6 bits type, 1 bit wasted flag; flag set: wasted = zeros before the next 1, + 1;
//                       wasted >= sbps fails (sbps = bps, + 1 for the side channel); eb = sbps - wasted
//   type 0 / 1          eb / n * eb bits
//   types 8-12, 32-63   order = type - 8 / type - 31 (order > n fails), order * eb bits of warm-up; LPC: 4 bits
//                       precision - 1 (15 fails), 5 bits shift (negative fails), order * precision bits
//   residual            2 bits method (> 1 fails), 4 bits po; plen = n >> po, plen < order or (plen << po) != n fails;
//                       per partition 4 / 5 bits parameter, all ones: 5 bits w and count * w bits, else count codes of
//                       zeros, a 1 and `parameter` bits; count = plen, less order in partition 0
//   every other type    fails
//   frame end           zero bits up to the byte boundary, then 16 bits: the frame is [0, pos / 8)
// Bit positions count from the frame's first byte.  A read that would pass bit 8 * window_bytes fails: the caller's
// window is min(bytes left in the input, kFrameExtentWindow), and a frame larger than that is not found by its own bits.
// The CRC-16 of the extent is the caller's test.
//
// The bit source `Src` (bytes behind its input read as 0, so that a walk into them ends at the window test):
//   uint32_t pos() const               bits consumed so far
//   void seek(uint32_t bit)            continue at this bit, in O(1)
//   uint32_t get(uint32_t n)           the next n bits, 1 <= n <= 32
//   uint32_t zeros(uint32_t limit)     the zeros before the next 1 bit, that bit consumed; may give up once pos() > limit
//   void rice(uint32_t k, uint32_t limit)   one Rice code consumed: zeros(limit), then k (<= 30) bits
#ifndef FLACGPU_FRAME_EXTENT_H
#define FLACGPU_FRAME_EXTENT_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLACGPU_FX __host__ __device__ __attribute__((always_inline)) inline
#else
#define FLACGPU_FX inline
#endif

// 4 MiB: any frame of 8 channels x 65535 samples x 32 bits coded VERBATIM fits
constexpr uint64_t kFrameExtentWindow = (uint64_t)1 << 22;

template <class Src> FLACGPU_FX bool fx_take(Src &r, uint64_t limit, uint32_t nbits, uint32_t &v) {
    if (r.pos() + (uint64_t)nbits > limit) return false;
    v = r.get(nbits);
    return true;
}
template <class Src> FLACGPU_FX bool fx_skip(Src &r, uint64_t limit, uint64_t nbits) {
    const uint64_t to = r.pos() + nbits;   // n * eb and count * w are formed in 64 bits by the caller
    if (to > limit) return false;
    if (nbits > 32) r.seek((uint32_t)to);
    else if (nbits) r.get((uint32_t)nbits);
    return true;
}

// The frame at the source's bit 0, whose accepted header says header_bytes, n (block size), acode (channel assignment
// code, <= 10) and bps (8 .. 32): its length in bytes, CRC-16 included, or 0 when it has none inside the window.
template <class Src>
FLACGPU_FX uint32_t frame_extent(Src &r, uint32_t header_bytes, uint32_t n, uint32_t acode, uint32_t bps,
                                 uint64_t window_bytes) {
    const uint64_t limit = 8 * window_bytes;   // <= 2^25: positions fit 32 bits
    if (8ull * header_bytes > limit) return 0;
    r.seek(8u * header_bytes);
    const uint32_t channels = acode < 8 ? acode + 1u : 2u;
    for (uint32_t c = 0; c < channels; c++) {
        const uint32_t sbps = bps + (((acode == 8 && c == 1) || (acode == 9 && c == 0) || (acode == 10 && c == 1)) ? 1u : 0u);
        uint32_t v;
        if (!fx_take(r, limit, 8, v) || (v & 0x80u)) return 0;
        const uint32_t type = (v >> 1) & 63u;
        uint32_t wasted = 0;
        if (v & 1u) {
            wasted = r.zeros((uint32_t)limit) + 1u;
            if (r.pos() > limit) return 0;
        }
        if (wasted >= sbps) return 0;
        const uint32_t eb = sbps - wasted;
        if (type == 0) {
            if (!fx_skip(r, limit, eb)) return 0;
            continue;
        }
        if (type == 1) {
            if (!fx_skip(r, limit, (uint64_t)n * eb)) return 0;
            continue;
        }
        const bool lpc = type >= 32;
        if (!lpc && (type < 8 || type > 12)) return 0;
        const uint32_t order = lpc ? type - 31u : type - 8u;
        if (order > n || !fx_skip(r, limit, (uint64_t)order * eb)) return 0;
        if (lpc) {
            if (!fx_take(r, limit, 9, v)) return 0;
            const uint32_t precision = (v >> 5) + 1u;
            if (precision == 16 || (v & 0x10u)) return 0;   // bit 4: the sign of the shift
            if (!fx_skip(r, limit, (uint64_t)order * precision)) return 0;
        }
        if (!fx_take(r, limit, 6, v) || (v >> 4) > 1u) return 0;
        const uint32_t hb = (v >> 4) ? 5u : 4u, esc = (v >> 4) ? 31u : 15u, po = v & 15u;
        const uint32_t plen = n >> po;
        if (plen < order || (plen << po) != n) return 0;
        for (uint32_t part = 0; part < (1u << po); part++) {
            const uint32_t count = plen - (part ? 0u : order);
            uint32_t k;
            if (!fx_take(r, limit, hb, k)) return 0;
            if (k == esc) {
                uint32_t w;
                if (!fx_take(r, limit, 5, w) || !fx_skip(r, limit, (uint64_t)count * w)) return 0;
                continue;
            }
            for (uint32_t i = 0; i < count; i++) {
                r.rice(k, (uint32_t)limit);
                if (r.pos() > limit) return 0;
            }
        }
    }
    const uint32_t odd = r.pos() & 7u;
    uint32_t v;
    if (odd && (!fx_take(r, limit, 8u - odd, v) || v)) return 0;
    if (!fx_skip(r, limit, 16)) return 0;
    return r.pos() >> 3;
}
#endif
