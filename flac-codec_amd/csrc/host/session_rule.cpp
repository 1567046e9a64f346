#include "session_rule.h"

#include <algorithm>
#include <new>

#include "raw_walk.h"

namespace flacenc {
size_t session_decide(const uint8_t *d, size_t L, bool final, uint32_t W, uint64_t base, uint32_t stream,
                      SessionCount &count, std::vector<flacgpu_frame_record> &out, uint64_t *elements) {
    // the positions judged so far: all of a flushed stream, else those with kSessionHead bytes behind them
    const size_t judged = final ? L : (L >= kSessionHead ? L - kSessionHead + 1 : 0);
    std::vector<size_t> cand;
    std::vector<HostFrameInfo> head;
    raw_candidates(d, L, judged, cand, head);
    const RawWalk w = raw_walk(
        cand.data(), 0, cand.size(), 0, L,
        [&](size_t i, uint64_t s) {
            if (const size_t end = raw_end_by_crc(d, L, cand, i, head[i], W, final)) return RawEnd{end, false};
            // no end within W: passed over; in an open stream with less than that behind it, an end may still arrive
            return RawEnd{final || L - s >= (size_t)W + kSessionHead ? kRawNone : kRawHold, false};
        },
        [&](size_t i, uint64_t s, uint64_t end, bool) {
            const flacgpu_frame_record f = raw_frame_record(head[i], stream, base + s, end - s, *elements, false);
            out.push_back(f);
            *elements += (uint64_t)head[i].n * head[i].channels;
        },
        &count);
    return session_hold(w, 0, L, final, count);
}
}  // namespace flacenc

struct flacgpu_session_host {
    struct Stream {
        std::vector<uint8_t> held;   // the bytes that cannot be judged yet
        uint64_t base = 0;           // offset of held[0] from the stream's first byte
        flacenc::SessionCount count;
    };
    std::vector<Stream> streams;
    uint32_t W = 0;
    bool finished = false;
};

int flacgpu_session_host_open(uint32_t n_streams, uint32_t max_frame_bytes, flacgpu_session_host **out) {
    if (!out) return FLACGPU_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_frame_bytes < flacenc::kSessionMinW || max_frame_bytes > flacenc::kSessionMaxW) return FLACGPU_ERR_INVALID_ARG;
    try {
        flacgpu_session_host *s = new flacgpu_session_host();
        s->streams.resize(n_streams);
        s->W = max_frame_bytes;
        *out = s;
    } catch (const std::bad_alloc &) {
        return FLACGPU_ERR_UNSUPPORTED;
    }
    return FLACGPU_OK;
}

// one feed into copies of the streams; committed only when the records fit
static int session_host_step(flacgpu_session_host *s, const uint8_t *const *data, const size_t *len, const uint8_t *flush,
                             bool finish, flacgpu_frame_record *records, size_t cap, flacgpu_raw_stream *raw,
                             uint64_t *held_bytes, uint64_t *total_frames) {
    if (!s || !total_frames || s->finished) return FLACGPU_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)s->streams.size();
    if (!finish && n && (!data || !len)) return FLACGPU_ERR_INVALID_ARG;
    try {
        std::vector<flacgpu_session_host::Stream> next(n);
        std::vector<flacgpu_frame_record> recs;
        std::vector<flacgpu_raw_stream> sums(n);
        uint64_t elements = 0;
        for (uint32_t i = 0; i < n; i++) {
            const flacgpu_session_host::Stream &cur = s->streams[i];
            std::vector<uint8_t> buf = cur.held;
            if (!finish && data[i] && len[i]) buf.insert(buf.end(), data[i], data[i] + len[i]);
            const bool final = finish || (flush && flush[i]);
            const size_t first = recs.size();
            next[i].count = cur.count;
            const size_t h = flacenc::session_decide(buf.data(), buf.size(), final, s->W, cur.base, i, next[i].count, recs,
                                                     &elements);
            next[i].base = cur.base + h;
            next[i].held.assign(buf.begin() + h, buf.end());
            sums[i] = flacenc::session_summary(next[i].count, first, recs.data() + first, recs.size() - first);
        }
        *total_frames = recs.size();
        if (recs.size() > cap || (!recs.empty() && !records)) return FLACGPU_ERR_BUFFER_TOO_SMALL;
        for (size_t k = 0; k < recs.size(); k++) records[k] = recs[k];
        for (uint32_t i = 0; i < n; i++) {
            if (raw) raw[i] = sums[i];
            if (held_bytes) held_bytes[i] = next[i].held.size();
        }
        s->streams.swap(next);
        s->finished = finish;
    } catch (const std::bad_alloc &) {
        return FLACGPU_ERR_UNSUPPORTED;
    }
    return FLACGPU_OK;
}

int flacgpu_session_host_feed(flacgpu_session_host *s, const uint8_t *const *data, const size_t *len, const uint8_t *flush,
                              flacgpu_frame_record *records, size_t cap, flacgpu_raw_stream *raw, uint64_t *held_bytes,
                              uint64_t *total_frames) {
    return session_host_step(s, data, len, flush, false, records, cap, raw, held_bytes, total_frames);
}

int flacgpu_session_host_finish(flacgpu_session_host *s, flacgpu_frame_record *records, size_t cap, flacgpu_raw_stream *raw,
                                uint64_t *total_frames) {
    return session_host_step(s, nullptr, nullptr, nullptr, true, records, cap, raw, nullptr, total_frames);
}

void flacgpu_session_host_close(flacgpu_session_host *s) { delete s; }
