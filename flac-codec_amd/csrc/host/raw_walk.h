// raw_walk.h -- the walk that turns a raw frame stream's candidate headers into kept frames (DESIGN.md 4b "Raw frame
// streams", "Decoder sessions"), stated once for its four callers: the host rules (scan_raw_frames, flac_stream.cpp;
// session_decide, session_rule.cpp), which find a candidate's end with CRC-16 loops, and the batch decoder's two
// (scan_raw_impl, session_step: decode_many.hip, through walk_slot), which read it from the device scan's tables.
// Beside it what those callers build around a walk alike, and regular_walk, the chain of a regular stream's frames, for
// its three: container_decide (session_rule.cpp) with CRC-16 loops, scan_impl and container_step (decode_many.hip,
// through walk_regular_slot) from the device's links.  The rest of a container session's rule is container_rule.h's.
// Header only, plain C++: no HIP call, no global state.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "checksums.h"
#include "flac_stream.h"
#include "flacenc_gpu.h"

namespace flacenc {
constexpr uint32_t kSessionHead = 16;   // a session judges a position once this many bytes follow it

// One stream's cumulative counts.  A gap is a maximal run of bytes in no kept frame over the whole byte string: a run
// that goes on from the feed before is not counted again.
struct SessionCount {
    uint64_t skipped = 0;
    uint32_t frames = 0, gaps = 0;
    bool in_gap = false;   // the last decided byte lies in no kept frame
    void skip(uint64_t n) {
        if (!n) return;
        skipped += n;
        if (!in_gap) gaps++;
        in_gap = true;
    }
    void keep() {
        frames++;
        in_gap = false;
    }
};

// Where a candidate ends: a position behind it, kRawNone (no end: passed over) or kRawHold (not decided yet: a session
// stops here).  own: the end is the frame's own extent (FLACGPU_SCAN_SPECULATIVE), not a header or the input's end.
constexpr uint64_t kRawNone = 0, kRawHold = ~(uint64_t)0;
struct RawEnd {
    uint64_t end = kRawNone;
    bool own = false;
};

struct RawWalk {
    uint64_t cursor;   // the end of the last kept frame (`begin`: none kept)
    uint64_t hold;     // the candidate that answered kRawHold (`limit`: none did)
};

// The walk over one stream's candidates pos[k0, k1), ascending positions in [begin, limit): one below the cursor is
// ignored, one without an end is passed over, one with an end is kept -- keep(k, at, end, own) -- and the cursor moves
// to that end; the first undecided one stops the walk.  end_of(k, at) is asked only for a candidate at or behind the
// cursor (the host rules checksum up to a frame's length to answer).  count (a session's; may be null) is told the
// bytes skipped in front of every kept frame, and the frame.
template <class Pos, class EndOf, class Keep>
RawWalk raw_walk(const Pos *pos, size_t k0, size_t k1, uint64_t begin, uint64_t limit, EndOf end_of, Keep keep,
                 SessionCount *count = nullptr) {
    RawWalk w{begin, limit};
    for (size_t k = k0; k < k1; k++) {
        const uint64_t at = pos[k];
        if (at < w.cursor) continue;
        const RawEnd e = end_of(k, at);
        if (e.end == kRawNone) continue;
        if (e.end == kRawHold) {
            w.hold = at;
            break;
        }
        if (count) {
            count->skip(at - w.cursor);
            count->keep();
        }
        keep(k, at, e.end, e.own);
        w.cursor = e.end;
    }
    return w;
}

// Where a session's segment [begin, begin + len) is held from after walk `w`: a flushed one is decided to its end; in
// an open one nothing from len - kSessionHead + 1 on is judged.  `count` is told the bytes skipped in front of it.
static inline uint64_t session_hold(const RawWalk &w, uint64_t begin, uint64_t len, bool final, SessionCount &count) {
    const uint64_t at_most = begin + (len >= kSessionHead ? len - kSessionHead + 1 : 0);
    const uint64_t h = final ? begin + len : std::max(w.cursor, std::min(w.hold, at_most));
    count.skip(h - w.cursor);
    return h;
}

// ---- a regular stream's walk: the one-shot scan's, and a container session's (DESIGN.md 4b "Container sessions") ----
// A regular stream's frames are a chain from the cursor: the frame at the cursor ends where the next begins, and a
// cursor that is no candidate, or a frame without an end, loses the stream for good.
struct RegularWalk {
    uint64_t cursor;   // the end of the last kept frame (`begin`: none kept): an open stream is held from here
    bool lost;         // synchronisation was lost at the cursor: nothing from there on is kept, in this feed or later
};

// The walk over one stream's candidates pos[k0, k1), ascending positions in [begin, limit); the positions below `judged`
// have been judged (a session judges a position once kSessionHead bytes follow it, or the input has ended).  end_of(k, at)
// answers for the candidate at the cursor: a position behind it, kRawNone (no end, and none can come) or kRawHold (not
// decided yet).  keep(k, at, end) is told every kept frame.  The walk stops at `limit`, at a cursor not judged yet, at a
// held candidate, or where synchronisation is lost.
template <class Pos, class EndOf, class Keep>
RegularWalk regular_walk(const Pos *pos, size_t k0, size_t k1, uint64_t begin, uint64_t limit, uint64_t judged,
                         EndOf end_of, Keep keep) {
    RegularWalk w{begin, false};
    size_t k = k0;
    while (w.cursor < limit && w.cursor < judged) {
        while (k < k1 && pos[k] < w.cursor) k++;
        if (k == k1 || pos[k] != w.cursor) {
            w.lost = true;
            break;
        }
        const RawEnd e = end_of(k, w.cursor);
        if (e.end == kRawHold) break;
        if (e.end == kRawNone) {
            w.lost = true;
            break;
        }
        keep(k, w.cursor, e.end);
        w.cursor = e.end;
    }
    return w;
}

// the first position of a session's segment [begin, begin + len) that is not judged yet
static inline uint64_t session_judged(uint64_t begin, uint64_t len, bool final) {
    return final ? begin + len : begin + (len >= kSessionHead ? len - kSessionHead + 1 : 0);
}

// The record of a kept frame of `bytes` bytes with the header `h` (status 0)
static inline flacgpu_frame_record raw_frame_record(const HostFrameInfo &h, uint32_t stream, uint64_t byte_offset,
                                                    uint64_t bytes, uint64_t out_offset, bool own) {
    flacgpu_frame_record f{};
    f.byte_offset = byte_offset;
    f.number = h.number;
    f.out_offset = out_offset;
    f.stream = stream;
    f.bytes = (uint32_t)bytes;
    f.block_size = h.n;
    f.sample_rate = h.sample_rate;
    f.channels = h.channels;
    f.bits_per_sample = h.bits_per_sample;
    f.assignment = h.acode;
    f.blocking = h.blocking;
    f.reserved = own ? FLACGPU_FRAME_SPECULATIVE : 0u;
    return f;
}

// at least one frame, and all share sample rate, channels and sample size
static inline bool raw_frames_uniform(const flacgpu_frame_record *frames, size_t n) {
    for (size_t k = 1; k < n; k++)
        if (frames[k].sample_rate != frames[0].sample_rate || frames[k].channels != frames[0].channels ||
            frames[k].bits_per_sample != frames[0].bits_per_sample)
            return false;
    return n > 0;
}

// A session's summary of one stream: the cumulative counts, and this feed's `n` records, which begin at `first_frame`
static inline flacgpu_raw_stream session_summary(const SessionCount &count, size_t first_frame,
                                                 const flacgpu_frame_record *frames, size_t n) {
    flacgpu_raw_stream sum{};
    sum.first_frame = first_frame;
    sum.skipped_bytes = count.skipped;
    sum.frames = count.frames;
    sum.gaps = count.gaps;
    sum.uniform = raw_frames_uniform(frames, n);
    return sum;
}

// ---- the host rules' candidates and ends (the batch decoder has both from the device) ----
// The candidates among d[0, judged) of the input d[0, L): a header that parses, with a sample rate and a sample size
// of its own
static inline void raw_candidates(const uint8_t *d, size_t L, size_t judged, std::vector<size_t> &cand,
                                  std::vector<HostFrameInfo> &head) {
    for (size_t q = 0; q < judged; q++) {
        HostFrameInfo h;
        if (d[q] == 0xFF && host_parse_frame_info(d + q, L - q, h) && h.rcode != 0 && h.bps_code != 0) {
            cand.push_back(q);
            head.push_back(h);
        }
    }
}
// Where candidate i (header h) ends by its CRC-16, at most W bytes behind it: at the first later candidate, or
// (final: no byte follows the input) at the input's end L; 0: at neither.  With init 0 and no final XOR, bytes
// [q - 2, q) are the CRC-16 of [s, q - 2) exactly when the CRC-16 of [s, q) is 0.
static inline size_t raw_end_by_crc(const uint8_t *d, size_t L, const std::vector<size_t> &cand, size_t i,
                                    const HostFrameInfo &h, size_t W, bool final) {
    const uint16_t *const T = crc16_table();
    const size_t s = cand[i], min_end = s + h.header_bytes + 2 + h.channels;
    uint16_t crc = 0;   // of [s, at)
    size_t at = s;
    for (size_t j = i + 1; j < cand.size() && cand[j] - s <= W; j++) {
        for (; at < cand[j]; at++) crc = crc16_step(T, crc, d[at]);
        if (cand[j] >= min_end && crc == 0) return cand[j];
    }
    if (final && L - s >= 2 && L - s <= W) {
        for (; at < L; at++) crc = crc16_step(T, crc, d[at]);
        if (crc == 0) return L;
    }
    return 0;
}
}  // namespace flacenc
