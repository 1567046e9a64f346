// frame_analysis.cpp -- flacgpu_analyze_frame_host: the frame analysis rule (kernels/frame_analysis.h, shared with
// k_analyze_many) on the host, for one frame.  Plain C++: no HIP call, no global state; every byte read is bounded by
// the length given, every store by the rule's own bounds.
#include <cstring>

#include "../kernels/frame_analysis.h"
#include "checksums.h"
#include "flac_stream.h"

namespace {
// analyze_subframes' bit source over data[0, len): MSB first, the bytes behind `len` read as 0
struct AnalysisBits {
    const uint8_t *d;
    size_t len;
    uint64_t p = 0;
    uint32_t byte(size_t i) const { return i < len ? d[i] : 0u; }
    uint32_t pos() const { return (uint32_t)p; }
    void seek(uint32_t bit) { p = bit; }
    uint32_t get(uint32_t n) {   // 1 <= n <= 32: five bytes hold the 7 odd bits in front and the n
        const size_t b = (size_t)(p >> 3);
        uint64_t v = 0;
        for (size_t i = 0; i < 5; i++) v = v << 8 | byte(b + i);
        v = (v >> (40 - (uint32_t)(p & 7) - n)) & (((uint64_t)1 << n) - 1);
        p += n;
        return (uint32_t)v;
    }
    uint32_t zeros(uint32_t limit) {
        uint32_t q = 0;
        for (;;) {
            const uint32_t odd = (uint32_t)(p & 7);
            const uint32_t cur = (byte((size_t)(p >> 3)) << odd) & 0xFFu;
            if (cur) {
                const uint32_t z = (uint32_t)__builtin_clz(cur) - 24u;
                p += z + 1;
                return q + z;
            }
            q += 8 - odd;
            p += 8 - odd;
            if (p > limit) return q;   // no 1 bit inside the frame
        }
    }
    uint32_t rice(uint32_t k, uint32_t limit) {
        const uint32_t q = zeros(limit);
        return (q << k) | (k ? get(k) : 0u);
    }
};
}  // namespace

extern "C" int flacgpu_analyze_frame_host(const uint8_t *frame, size_t len, uint32_t streaminfo_bps,
                                          flacgpu_frame_analysis *analysis, flacgpu_subframe_plan *subframes,
                                          int64_t *rows64, size_t rows64_cap) {
    if (!analysis || !subframes || (len && !frame)) return FLACGPU_ERR_INVALID_ARG;
    flacenc::HostFrameInfo h;
    // a frame is at most 8 channels x 65536 samples x 33 bits and its header: positions fit 32 bits
    const bool head = len < ((size_t)1 << 28) && flacenc::host_parse_frame_info(frame, len, h);
    const uint32_t ld = head ? (h.n + 3u) & ~3u : 0;
    if (head && rows64 && rows64_cap < (size_t)h.channels * ld) return FLACGPU_ERR_BUFFER_TOO_SMALL;
    memset(analysis, 0, sizeof *analysis);
    memset(subframes, 0, sizeof(flacgpu_subframe_plan) * FLACGPU_MAX_CHANNELS);
    const uint32_t crc_bit = flacenc::crc16(frame, len) ? 2u : 0u;
    analysis->status = 1u | crc_bit;
    if (!head) return FLACGPU_OK;
    const uint32_t bps = h.bits_per_sample ? h.bits_per_sample : streaminfo_bps;
    analysis->block_size = h.n;
    analysis->header_bytes = h.header_bytes;
    analysis->assignment_code = h.acode;
    analysis->plan.assignment = (uint8_t)(h.acode >= 8 ? h.acode : FLACGPU_ASSIGN_INDEPENDENT);
    analysis->plan.channels = (uint8_t)h.channels;
    analysis->plan.block_size = (uint16_t)(h.n & 0xFFFFu);
    if (bps < 4 || bps > 32) return FLACGPU_OK;
    AnalysisBits bits{frame, len};
    bits.seek(8u * h.header_bytes);
    uint32_t body = 0;
    const uint32_t end_bit = (uint32_t)(8 * len);
    const bool ok = rows64 ? analyze_subframes<true>(bits, h.n, h.acode, bps, end_bit, subframes, rows64, ld, &body)
                           : analyze_subframes<false>(bits, h.n, h.acode, bps, end_bit, subframes, (int64_t *)nullptr, ld, &body);
    analysis->plan.body_bits = body;
    analysis->status = (ok ? 0u : 1u) | crc_bit;
    return FLACGPU_OK;
}
