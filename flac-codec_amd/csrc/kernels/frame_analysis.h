// frame_analysis.h -- what a FLAC frame is made of: the walk over its subframes that records every decision the encoder
// took (type, order, wasted bits, predictor, Rice method, partition order and parameters, exact bit lengths) and,
// when asked, the residual rows as they are coded (DESIGN.md 4b "Frame analysis", include/flacenc_gpu.h "frame
// analysis").  One function for the host (flacgpu_analyze_frame_host, host/frame_analysis.cpp) and the device
// (k_analyze_many, kernels/analyze_many.inc), so that the rule is tested without a GPU.  It has frame_extent.h's shape
// and makes frame_extent.h's tests, which are k_decode_many's (the head of that file spells them out), with the end
// known: the frame is `end_bit` bits long, a read that would pass it fails, and behind the last subframe the bits up to
// the byte boundary must be 0 and exactly 16 bits (the CRC-16, the caller's test) must be left.
//
// Nothing is synthesised: a row holds what the bit stream holds.  Every field is stored where it belongs as soon as it
// is read -- no record is collected in registers, and no per-lane array is indexed at run time -- into records that the
// caller has cleared, so that every entry a subframe does not use stays 0.  Stores are bounded whatever the bits say:
// records 0 .. channels - 1, rice[] / escape_bits[] entries below FLACGPU_MAX_PARTITIONS, coeffs[] below the order
// (<= 32), row elements below n.
//
// The bit source `Src` is frame_extent.h's with one change: rice() gives the code's value.
//   uint32_t pos() const               bits consumed so far
//   void seek(uint32_t bit)            continue at this bit, in O(1)
//   uint32_t get(uint32_t n)           the next n bits, 1 <= n <= 32
//   uint32_t zeros(uint32_t limit)     the zeros before the next 1 bit, that bit consumed; may give up once pos() > limit
//   uint32_t rice(uint32_t k, uint32_t limit)   one Rice code: (zeros(limit) << k) | the next k (<= 30) bits
#ifndef FLACGPU_FRAME_ANALYSIS_H
#define FLACGPU_FRAME_ANALYSIS_H
#include "flacenc_gpu.h"
#include "frame_extent.h"

// a signed value of 0 .. 33 bits (0 bits: the value 0); the 33rd is what the side channel of 32-bit stereo adds
template <class Src> FLACGPU_FX bool fa_signed(Src &r, uint64_t limit, uint32_t nbits, int64_t &v) {
    v = 0;
    if (!nbits) return true;
    if (r.pos() + (uint64_t)nbits > limit) return false;
    if (nbits > 32) {
        const uint32_t top = r.get(nbits - 32);
        v = (int64_t)(((uint64_t)(0u - (top & 1u)) << 32) | r.get(32));
    } else {
        v = (int32_t)(r.get(nbits) << (32u - nbits)) >> (32u - nbits);
    }
    return true;
}

// `count` values of `nbits` bits each: to x[0 .. count) when ROWS, else stepped over in one move
template <bool ROWS, class Src, class RowT>
FLACGPU_FX bool fa_values(Src &r, uint64_t limit, uint32_t nbits, uint32_t count, RowT *x) {
    if (!ROWS) return fx_skip(r, limit, (uint64_t)count * nbits);
    for (uint32_t i = 0; i < count; i++) {
        int64_t v;
        if (!fa_signed(r, limit, nbits, v)) return false;
        x[i] = (RowT)v;
    }
    return true;
}

FLACGPU_FX uint32_t fa_source(uint32_t acode, uint32_t c) {
    if (acode < 8) return c;
    if (acode == 8) return c ? FLACGPU_SRC_SIDE : 0u;
    if (acode == 9) return c ? 1u : FLACGPU_SRC_SIDE;
    return c ? FLACGPU_SRC_SIDE : FLACGPU_SRC_MID;
}

// The subframes of the frame whose accepted header ends at the source's position and says n (block size, >= 1), acode
// (<= 10) and bps (<= 32): records subs[0 .. channels), cleared by the caller, and, when ROWS, the row of channel c at
// rows + c * ld (ld >= n).  *body_bits: the sum of the subframes' bits.  Returns false when the frame does not parse;
// the records and rows are then unspecified.
template <bool ROWS, class Src, class RowT>
FLACGPU_FX bool analyze_subframes(Src &r, uint32_t n, uint32_t acode, uint32_t bps, uint32_t end_bit,
                                  flacgpu_subframe_plan *subs, RowT *rows, uint32_t ld, uint32_t *body_bits) {
    const uint64_t limit = end_bit;
    const uint32_t channels = acode < 8 ? acode + 1u : 2u;
    const uint32_t body_at = r.pos();
    for (uint32_t c = 0; c < channels; c++) {
        flacgpu_subframe_plan *s = subs + c;
        RowT *x = ROWS ? rows + (size_t)c * ld : rows;
        const uint32_t at = r.pos();
        const uint32_t sbps = bps + (((acode == 8 && c == 1) || (acode == 9 && c == 0) || (acode == 10 && c == 1)) ? 1u : 0u);
        uint32_t v;
        if (!fx_take(r, limit, 8, v) || (v & 0x80u)) return false;
        const uint32_t type = (v >> 1) & 63u;
        uint32_t wasted = 0;
        if (v & 1u) {
            wasted = r.zeros((uint32_t)limit) + 1u;
            if (r.pos() > limit) return false;
        }
        if (wasted >= sbps) return false;
        const uint32_t eb = sbps - wasted;
        s->source = (uint8_t)fa_source(acode, c);
        s->wasted = (uint8_t)wasted;
        s->bps = (uint8_t)eb;
        s->reserved[0] = sbps > 32 ? FLACGPU_AN_WIDE : 0;
        if (type == 0) {
            s->type = FLACGPU_SUB_CONSTANT;
            if (!fa_values<ROWS>(r, limit, eb, 1, x)) return false;
        } else if (type == 1) {
            s->type = FLACGPU_SUB_VERBATIM;
            if (!fa_values<ROWS>(r, limit, eb, n, x)) return false;
        } else {
            const bool lpc = type >= 32;
            if (!lpc && (type < 8 || type > 12)) return false;
            const uint32_t order = lpc ? type - 31u : type - 8u;
            s->type = lpc ? FLACGPU_SUB_LPC : FLACGPU_SUB_FIXED;
            s->order = (uint8_t)order;
            if (order > n || !fa_values<ROWS>(r, limit, eb, order, x)) return false;
            if (lpc) {
                if (!fx_take(r, limit, 9, v)) return false;
                const uint32_t precision = (v >> 5) + 1u;
                if (precision == 16 || (v & 0x10u)) return false;   // bit 4: the sign of the shift
                s->precision = (uint8_t)precision;
                s->shift = (uint8_t)(v & 15u);
                for (uint32_t j = 0; j < order; j++) {   // order <= 32 = FLACGPU_MAX_LPC_ORDER
                    int64_t q;
                    if (!fa_signed(r, limit, precision, q)) return false;
                    s->coeffs[j] = (int32_t)q;
                }
            }
            if (!fx_take(r, limit, 6, v) || (v >> 4) > 1u) return false;
            const uint32_t hb = (v >> 4) ? 5u : 4u, esc = (v >> 4) ? 31u : 15u, po = v & 15u;
            const uint32_t plen = n >> po;
            if (plen < order || (plen << po) != n) return false;
            s->coding_method = (uint8_t)(v >> 4);
            s->partition_order = (uint8_t)po;
            s->n_partitions = 1u << po;
            s->part_len = plen;
            if ((1u << po) > (uint32_t)FLACGPU_MAX_PARTITIONS) s->reserved[0] |= FLACGPU_AN_PARTS_CLIPPED;
            uint32_t i = order;
            for (uint32_t part = 0; part < (1u << po); part++) {
                const uint32_t count = plen - (part ? 0u : order);   // i + count <= n: the partitions tile [order, n)
                uint32_t k;
                if (!fx_take(r, limit, hb, k)) return false;
                if (k == esc) {
                    uint32_t w;
                    if (!fx_take(r, limit, 5, w)) return false;
                    if (part < (uint32_t)FLACGPU_MAX_PARTITIONS) {
                        s->rice[part] = 0xFF;
                        s->escape_bits[part] = (uint8_t)w;
                    }
                    if (!fa_values<ROWS>(r, limit, w, count, x + (ROWS ? i : 0u))) return false;
                    i += count;
                    continue;
                }
                if (part < (uint32_t)FLACGPU_MAX_PARTITIONS) s->rice[part] = (uint8_t)k;
                for (uint32_t e = i + count; i < e; i++) {
                    const uint32_t u = r.rice(k, (uint32_t)limit);
                    if (r.pos() > limit) return false;
                    if (ROWS) x[i] = (RowT)((int32_t)(u >> 1) ^ -(int32_t)(u & 1u));
                }
            }
        }
        s->bits = r.pos() - at;
    }
    *body_bits = r.pos() - body_at;
    const uint32_t odd = r.pos() & 7u;
    uint32_t v;
    if (odd && (!fx_take(r, limit, 8u - odd, v) || v)) return false;
    return (uint64_t)r.pos() + 16 == limit;
}
#endif
