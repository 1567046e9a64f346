#include "session_rule.h"

#include <string.h>

#include <algorithm>
#include <new>

#include "container_rule.h"

namespace flacenc {
RegularWalk container_decide(const uint8_t *d, size_t L, bool final, uint32_t W, const flacgpu_stream_info &info,
                             uint32_t min_frame, uint64_t base, uint32_t stream, std::vector<flacgpu_frame_record> &out,
                             uint64_t *elements) {
    const size_t judged = (size_t)session_judged(0, L, final);
    // the regular candidate test: every header that parses, those that defer to STREAMINFO included
    std::vector<size_t> cand;
    std::vector<HostFrameInfo> head;
    for (size_t q = 0; q < judged; q++) {
        HostFrameInfo h;
        if (d[q] == 0xFF && host_parse_frame_info(d + q, L - q, h)) {
            cand.push_back(q);
            head.push_back(h);
        }
    }
    const uint16_t *const T = crc16_table();
    return regular_walk(
        cand.data(), 0, cand.size(), 0, L, judged,
        [&](size_t k, uint64_t s) {
            const HostFrameInfo &h = head[k];
            const size_t min_end = s + std::max<size_t>(h.header_bytes + 2 + info.channels, min_frame);
            uint16_t crc = 0;   // of [s, at)
            size_t at = s;
            for (size_t j = k + 1; j < cand.size() && cand[j] - s <= W; j++) {
                for (; at < cand[j]; at++) crc = crc16_step(T, crc, d[at]);
                if (cand[j] >= min_end && crc == 0 && head[j].blocking == h.blocking) return RawEnd{cand[j], false};
            }
            if (final) {
                if (L - s < 2 || L - s > W) return RawEnd{kRawNone, false};
                for (; at < L; at++) crc = crc16_step(T, crc, d[at]);
                return RawEnd{crc == 0 ? L : kRawNone, false};
            }
            // every position up to s + W judged and none fits: no end can come
            return RawEnd{L - s >= (size_t)W + kSessionHead ? kRawNone : kRawHold, false};
        },
        [&](size_t k, uint64_t s, uint64_t end) {
            HostFrameInfo h = head[k];
            if (!h.rcode) h.sample_rate = info.sample_rate;
            if (!h.bps_code) h.bits_per_sample = info.bits_per_sample;
            out.push_back(raw_frame_record(h, stream, base + s, end - s, *elements, false));
            *elements += (uint64_t)h.n * h.channels;
        });
}

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
        flacenc::SessionCount count;     // a raw session's
        flacenc::ContainerStream rule;   // a container session's (host/container_rule.h)
    };
    std::vector<Stream> streams;
    uint32_t W = 0;
    bool finished = false, container = false;
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

int flacgpu_session_host_open_container(uint32_t n_streams, uint32_t max_frame_bytes, flacgpu_session_host **out) {
    if (int rc = flacgpu_session_host_open(n_streams, max_frame_bytes, out)) return rc;
    (*out)->container = true;
    for (flacgpu_session_host::Stream &st : (*out)->streams) meta_feed_init(st.rule.meta);
    return FLACGPU_OK;
}

int flacgpu_meta_feed_host(flacgpu_meta_feed *state, const uint8_t *chunk, size_t len, size_t *consumed) {
    static_assert(sizeof(flacgpu_meta_feed) == sizeof(MetaFeed), "flacgpu_meta_feed is MetaFeed");
    if (!state || !consumed || (len && !chunk)) return FLACGPU_ERR_INVALID_ARG;
    MetaFeed m;
    memcpy(&m, state, sizeof m);
    if (m.phase > MF_REFUSED || m.have >= kStreamInfoBytes) return FLACGPU_ERR_INVALID_ARG;   // not a state of ours
    *consumed = (size_t)meta_feed(m, chunk, len);
    memcpy(state, &m, sizeof m);
    return FLACGPU_OK;
}

void flacgpu_meta_feed_init_host(flacgpu_meta_feed *state) {
    if (!state) return;
    MetaFeed m;
    meta_feed_init(m);
    memcpy(state, &m, sizeof m);
}

int flacgpu_meta_feed_result_host(const flacgpu_meta_feed *state, uint64_t total_bytes, flacgpu_stream_info *info,
                                  uint32_t *min_frame, uint64_t *frames_at) {
    if (!state || !info || !min_frame || !frames_at) return FLACGPU_ERR_INVALID_ARG;
    *frames_at = 0;
    MetaFeed m;
    memcpy(&m, state, sizeof m);
    MetaRecord rec;
    meta_feed_record(m, total_bytes, rec);
    size_t pos = 0;
    if (flacenc::metadata_of_record(rec, info, min_frame, &pos)) return FLACGPU_ERR_INVALID_ARG;
    *frames_at = pos;
    return FLACGPU_OK;
}

// one feed of a container session into copies of the streams; committed only when the records fit
static int container_host_step(flacgpu_session_host *s, const uint8_t *const *data, const size_t *len, bool finish,
                               flacgpu_frame_record *records, size_t cap, flacgpu_raw_stream *raw, uint64_t *held_bytes,
                               uint64_t *total_frames) {
    const uint32_t n = (uint32_t)s->streams.size();
    try {
        std::vector<flacgpu_session_host::Stream> next(s->streams);
        std::vector<flacgpu_frame_record> recs;
        std::vector<flacgpu_raw_stream> sums(n);
        uint64_t elements = 0;
        for (uint32_t i = 0; i < n; i++) {
            flacgpu_session_host::Stream &st = next[i];
            flacenc::ContainerStream &k = st.rule;
            const uint8_t *chunk = !finish && data[i] && len[i] ? data[i] : nullptr;
            const size_t fresh = chunk ? len[i] : 0;
            const size_t first = recs.size();
            MetaFeed meta = k.meta;
            const size_t used = k.phase == flacenc::CS_META ? (size_t)meta_feed(meta, chunk, fresh) : 0;
            flacenc::container_begin(k, meta, fresh, finish, &st.base);
            if (k.phase == flacenc::CS_FRAMES) {
                if (fresh > used) st.held.insert(st.held.end(), chunk + used, chunk + fresh);   // metadata is never held
                const size_t L = st.held.size();
                const flacenc::RegularWalk w =
                    flacenc::container_decide(st.held.data(), L, finish, s->W, k.info, k.min_frame, st.base, i, recs, &elements);
                uint64_t samples = 0;
                for (size_t q = first; q < recs.size(); q++) samples += recs[q].block_size;
                st.base += w.cursor;
                st.held.erase(st.held.begin(), st.held.begin() + w.cursor);
                st.held.resize((size_t)flacenc::container_end(k, w, L, recs.size() - first, samples));
            }
            sums[i] = flacenc::container_summary(k, first);
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

// one feed into copies of the streams; committed only when the records fit
static int session_host_step(flacgpu_session_host *s, const uint8_t *const *data, const size_t *len, const uint8_t *flush,
                             bool finish, flacgpu_frame_record *records, size_t cap, flacgpu_raw_stream *raw,
                             uint64_t *held_bytes, uint64_t *total_frames) {
    if (!s || !total_frames || s->finished) return FLACGPU_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)s->streams.size();
    if (!finish && n && (!data || !len)) return FLACGPU_ERR_INVALID_ARG;
    if (s->container) {
        for (uint32_t i = 0; flush && i < n; i++)   // a container's sender knows no frame boundary
            if (flush[i]) return FLACGPU_ERR_INVALID_ARG;
        return container_host_step(s, data, len, finish, records, cap, raw, held_bytes, total_frames);
    }
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
