#include "session_rule.h"

#include <algorithm>
#include <new>

#include "checksums.h"

namespace flacenc {
size_t session_decide(const uint8_t *d, size_t L, bool final, uint32_t W, uint64_t base, uint32_t stream,
                      SessionCount &count, std::vector<flacgpu_frame_record> &out, uint64_t *elements) {
    const uint16_t *const T = crc16_table();
    // the positions judged so far: all of a flushed stream, else those with kSessionHead bytes behind them
    const size_t judged = final ? L : (L >= kSessionHead ? L - kSessionHead + 1 : 0);
    std::vector<size_t> cand;
    std::vector<HostFrameInfo> head;
    for (size_t q = 0; q < judged; q++) {
        HostFrameInfo h;
        if (d[q] == 0xFF && host_parse_frame_info(d + q, L - q, h) && h.rcode != 0 && h.bps_code != 0) {
            cand.push_back(q);
            head.push_back(h);
        }
    }
    size_t cursor = 0, hold = L;   // hold: the first candidate whose link is not decided
    for (size_t i = 0; i < cand.size(); i++) {
        const size_t s = cand[i];
        if (s < cursor) continue;
        const HostFrameInfo &h = head[i];
        const size_t min_end = s + h.header_bytes + 2 + h.channels;
        uint16_t crc = 0;   // of [s, at): 0 at an end (flac_stream.cpp scan_raw_frames)
        size_t at = s, end = 0;
        for (size_t j = i + 1; j < cand.size() && !end && cand[j] - s <= W; j++) {
            for (; at < cand[j]; at++) crc = crc16_step(T, crc, d[at]);
            if (cand[j] >= min_end && crc == 0) end = cand[j];
        }
        if (!end && final && L - s >= 2 && L - s <= W) {   // the frame ends with the flushed input
            for (; at < L; at++) crc = crc16_step(T, crc, d[at]);
            if (crc == 0) end = L;
        }
        if (!end) {
            if (final || L - s >= (size_t)W + kSessionHead) continue;   // no end within W: passed over
            hold = s;   // an end may still arrive
            break;
        }
        count.skip(s - cursor);
        count.keep();
        flacgpu_frame_record f{};
        f.byte_offset = base + s;
        f.number = h.number;
        f.out_offset = *elements;
        f.stream = stream;
        f.bytes = (uint32_t)(end - s);
        f.block_size = h.n;
        f.sample_rate = h.sample_rate;
        f.channels = h.channels;
        f.bits_per_sample = h.bits_per_sample;
        f.assignment = h.acode;
        f.blocking = h.blocking;
        out.push_back(f);
        *elements += (uint64_t)h.n * h.channels;
        cursor = end;
    }
    const size_t at_most = L >= kSessionHead ? L - kSessionHead + 1 : 0;   // L - 15: nothing behind it is judged
    const size_t hpos = final ? L : std::max(cursor, std::min(hold, at_most));
    count.skip(hpos - cursor);
    return hpos;
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
            flacgpu_raw_stream &sum = sums[i];
            sum.first_frame = first;
            sum.skipped_bytes = next[i].count.skipped;
            sum.frames = next[i].count.frames;
            sum.gaps = next[i].count.gaps;
            sum.uniform = recs.size() > first;
            for (size_t k = first; k < recs.size(); k++)
                if (recs[k].sample_rate != recs[first].sample_rate || recs[k].channels != recs[first].channels ||
                    recs[k].bits_per_sample != recs[first].bits_per_sample)
                    sum.uniform = 0;
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
