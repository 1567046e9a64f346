// device_session.cpp -- flacenc_device_session_*: flacenc_encode_many_device's batch taken chunk by chunk (include/
// flacenc_stream.h "sessions"; DESIGN.md 4c "Sessions").  Everything but the hash reuses what the one-shot call uses:
//   * staging: an ingest handle of the session's own, kept for its whole life, whose staging buffer has a constant size
//     (it is never reallocated, so its contents survive between submits) and is laid out as two halves.  In the half in
//     use stream i owns a region: its chunk is ingested at the fixed 16-byte-aligned element A_i, its carry of
//     c_i < block_size samples sits directly in front, in [A_i - c_i ch, A_i), so the pending samples are contiguous;
//   * whole blocks: plan_stream_batches over what every stream's pending samples complete, through encode_whole_blocks
//     (device_blocks.h, the loop of the one-shot call) with the frame numbers continued per stream.  A segment starts on a
//     16-byte boundary only when c_i ch is a multiple of 4: flacgpu_encode_segments_device reads aligned segments in
//     place and gathers the others (plan_route), the same bytes either way;
//   * the new remainder of every stream is then copied into the OTHER half's [A_i - r_i ch, A_i) by one k_place_runs
//     launch (flacgpu_ingest_move) -- two halves, so that source and destination never overlap when a chunk is shorter
//     than a block -- after the contexts that read the old half have been waited for and before the next submit;
//   * MD5: the ingest runs without FLACGPU_INGEST_MD5, and the chunk at A_i is appended to the stream's resumable chain
//     (flacgpu_md5_chains_update) on the handle's stream, beside the analysis; finalize pads and downloads;
//   * finalize: the short last block through the one-frame path, the header from flacenc_stream_header;
//   * a stream opened WITHOUT a total (flacenc_device_session_open_ex, total_known[i] == 0) is FlacSampleWriter::new(..,
//     None): no placeholder SEEKTABLE in front of its frames, no bound on what it may be fed, and at finalize the header
//     of flacenc_stream_header_unknown_total with total = the samples received.  Its frames and tail are a known-total
//     stream's: nothing in a frame depends on the total.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../kernels/sample_types.h"
#include "device_blocks.h"
#include "host_internal.h"

using namespace flacenc_host;

namespace {

int refuse(int rc, const std::string &why) {
    set_last_error("flacenc_device_session: " + why);
    return rc;
}

// elements (int32) of the staging buffer: carry_room in front of every chunk's place, `region` per stream and half
struct Layout {
    uint64_t carry_room = 0, region = 0, half = 0;
};
bool layout_of(uint32_t block_size, uint32_t channels, uint64_t max_chunk, size_t n_streams, Layout *l) {
    uint64_t chunk = 0, total = 0;
    l->carry_room = ((uint64_t)(block_size - 1) * channels + 3u) & ~(uint64_t)3;
    if (__builtin_mul_overflow(max_chunk, (uint64_t)channels, &chunk) || __builtin_add_overflow(chunk, (uint64_t)3, &chunk)) return false;
    chunk &= ~(uint64_t)3;
    if (__builtin_add_overflow(chunk, l->carry_room, &l->region) || __builtin_mul_overflow(l->region, (uint64_t)n_streams, &l->half) ||
        __builtin_mul_overflow(l->half, (uint64_t)8, &total))   // two halves of 4-byte elements
        return false;
    return true;
}

int plan_shape(const flacenc_options *o, uint32_t bps, uint32_t channels, size_t n_streams, uint64_t max_chunk, uint32_t flags,
               Layout *l) {
    if (!o) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    if (flags & ~FLACENC_DEVICE_NO_MD5) return refuse(FLACENC_ERR_INVALID_ARG, "unknown flags");
    if (!max_chunk) return refuse(FLACENC_ERR_INVALID_ARG, "max_chunk is 0");
    // the shape through the one-shot plan: a FLAT int32 batch of n_streams chunks of one sample
    const flacenc_tensor_format fmt{FLACGPU_SAMPLE_I32, FLACGPU_LAYOUT_FLAT, 0, 0, 0};
    if (n_streams > 0xFFFFFFFFull) return refuse(FLACENC_ERR_UNSUPPORTED, "more than 2^32 - 1 streams");
    std::vector<flacenc_device_job> jobs(n_streams);
    for (size_t i = 0; i < n_streams; i++) {
        jobs[i] = flacenc_device_job{};
        jobs[i].in_offset = (uint64_t)i * FLACGPU_MAX_CHANNELS;
        jobs[i].samples = 1;
    }
    if (int rc = flacenc_device_batch_plan(o, &fmt, bps, channels, jobs.data(), n_streams, nullptr, nullptr)) return rc;
    if (!layout_of(o->block_size, channels, max_chunk, n_streams, l))
        return refuse(FLACENC_ERR_UNSUPPORTED, "the staging buffer exceeds 2^64 bytes");
    return 0;
}

struct Stream {
    uint64_t total = 0, fed = 0;    // samples per channel: declared, received
    bool known = true;              // the total was declared at open (false: `total` is unused)
    uint32_t carry = 0;             // c_i: pending samples in front of A_i in the half in use
    size_t hlen = 0;
    int status = 0;                 // sticky
    uint64_t altered = 0;
    std::vector<uint32_t> sizes;    // per frame so far (4 bytes a frame, for flacenc_stream_header)
};

}  // namespace

struct flacenc_device_session {
    flacenc_options o;
    flacgpu_options g;
    uint32_t sample_rate = 0, bps = 0, ch = 0, flags = 0;
    uint64_t max_chunk = 0;
    int device = 0;
    Layout lay;
    uint32_t half = 0;              // the half the carries lie in and the next chunk goes to
    uint32_t ctx_frames = 0;        // what a write's contexts hold: the batch cap of the fullest possible write
    flacgpu_ingest *ing = nullptr;
    flacgpu_md5_chains *chains = nullptr;
    int32_t *d_staging = nullptr;
    std::vector<Stream> st;
    bool finalized = false;
    int gpu_rc = 0;                 // sticky
    uint64_t place(size_t i, uint32_t h) const { return h * lay.half + i * lay.region + lay.carry_room; }   // A_i
};

extern "C" {

int flacenc_device_session_plan(const flacenc_options *opts, uint32_t bits_per_sample, uint32_t channels, size_t n_streams,
                                uint64_t max_chunk, uint32_t flags, size_t *device_bytes) {
    Layout l;
    if (int rc = plan_shape(opts, bits_per_sample, channels, n_streams, max_chunk, flags, &l)) return rc;
    if (device_bytes) *device_bytes = (size_t)(8 * l.half + ((flags & FLACENC_DEVICE_NO_MD5) ? 0 : 128 * (uint64_t)n_streams));
    return 0;
}

int flacenc_device_session_open(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                uint32_t channels, const uint64_t *totals, size_t n_streams, uint64_t max_chunk,
                                uint32_t flags, flacenc_device_session **session) {
    return flacenc_device_session_open_ex(opts, sample_rate, bits_per_sample, channels, totals, nullptr, n_streams, max_chunk,
                                          flags, session);
}

int flacenc_device_session_open_ex(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                   uint32_t channels, const uint64_t *totals, const uint8_t *total_known, size_t n_streams,
                                   uint64_t max_chunk, uint32_t flags, flacenc_device_session **session) {
    if (!session) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    *session = nullptr;
    Layout l;
    if (int rc = plan_shape(opts, bits_per_sample, channels, n_streams, max_chunk, flags, &l)) return rc;
    bool any_known = !total_known;
    for (size_t i = 0; total_known && i < n_streams; i++) any_known |= total_known[i] != 0;
    if (!totals && n_streams && any_known) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    flacenc_device_session *s = new (std::nothrow) flacenc_device_session();
    if (!s) return refuse(FLACENC_ERR_UNSUPPORTED, "out of memory");
    s->o = *opts;
    s->g = gpu_options(*opts, opts->block_size);
    s->sample_rate = sample_rate;
    s->bps = bits_per_sample;
    s->ch = channels;
    s->flags = flags;
    s->max_chunk = max_chunk;
    s->lay = l;
    s->device = opts->device >= 0 ? opts->device : flacgpu_current_device();
    s->st.resize(n_streams);
    const uint32_t B = opts->block_size;
    std::vector<uint64_t> most(n_streams, 0);   // the blocks one write can complete
    for (size_t i = 0; i < n_streams; i++) {
        Stream &m = s->st[i];
        m.known = !total_known || total_known[i];
        m.total = m.known ? totals[i] : 0;
        if (m.known && !m.total) {
            m.status = FLACENC_ERR_INVALID_ARG;
            continue;
        }
        if (int rc = stream_header_len(s->o, sample_rate, bits_per_sample, channels, m.total, &m.hlen, m.known)) {
            m.status = rc;
            m.hlen = 0;
            continue;
        }
        // (without a total only max_chunk bounds what one write completes)
        most[i] = (max_chunk + B - 1) / B + 1;
        if (m.known) most[i] = std::min<uint64_t>(most[i], (m.total + B - 1) / B);
    }
    (void)plan_stream_batches(most, s->o.batch_frames, (size_t)B * channels, &s->ctx_frames);
    int rc = flacgpu_ingest_create(s->device, &s->ing);
    if (!rc && !(flags & FLACENC_DEVICE_NO_MD5)) rc = flacgpu_md5_chains_create(s->device, (uint32_t)n_streams, &s->chains);
    if (rc) {
        const int e = device_gpu_error(rc);
        flacenc_device_session_close(s);
        return e;
    }
    *session = s;
    return 0;
}

size_t flacenc_device_session_header_len(const flacenc_device_session *s, size_t i) {
    return s && i < s->st.size() ? s->st[i].hlen : 0;
}

int flacenc_device_session_write(flacenc_device_session *s, const void *d_pcm, const flacenc_tensor_format *fmt,
                                 flacenc_session_chunk *chunks, void *stream) {
    if (!s || !fmt || (!chunks && !s->st.empty())) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    if (s->finalized) return refuse(FLACENC_ERR_FINALIZED, "write after finalize");
    if (s->gpu_rc) return s->gpu_rc;
    const size_t n = s->st.size();
    const uint32_t B = s->o.block_size, ch = s->ch;
    const size_t per = (size_t)B * ch;
    // ---- the checks: nothing is launched or written, and the session stays as it is, when one fails
    std::vector<flacenc_device_job> jobs(n);
    uint64_t fed_now = 0;
    for (size_t i = 0; i < n; i++) {
        const Stream &m = s->st[i];
        if (chunks[i].samples > s->max_chunk) return refuse(FLACENC_ERR_INVALID_ARG, "chunk " + std::to_string(i) + " is longer than max_chunk");
        if (!m.status && m.known && chunks[i].samples > m.total - m.fed)
            return refuse(FLACENC_ERR_INVALID_ARG, "chunk " + std::to_string(i) + " passes the stream's declared total");
        jobs[i] = flacenc_device_job{};
        jobs[i].in_offset = chunks[i].in_offset;
        jobs[i].samples = m.status ? 0 : chunks[i].samples;   // a dead stream's chunk is ignored
        fed_now += jobs[i].samples;
    }
    size_t in_elements = 0;
    if (int rc = flacenc_device_batch_plan(&s->o, fmt, s->bps, ch, jobs.data(), n, &in_elements, nullptr)) return rc;
    if ((in_elements && !d_pcm) || reinterpret_cast<uintptr_t>(d_pcm) % sample_type_align(fmt->dtype))
        return refuse(FLACENC_ERR_INVALID_ARG, "no tensor, or a tensor not aligned to its element size");
    for (size_t i = 0; i < n; i++) {
        chunks[i].out_len = 0;
        chunks[i].altered = 0;
        chunks[i].status = s->st[i].status;
    }
    if (!fed_now) return 0;   // (no stream can complete a block without a sample)
    const auto fail_gpu = [&](int rc) {
        s->gpu_rc = device_gpu_error(rc);
        for (size_t i = 0; i < n; i++)
            if (!s->st[i].status) chunks[i].status = s->gpu_rc;
        return s->gpu_rc;
    };

    // ---- ingest at A_i of the half in use, then the chains, which run beside the analysis
    std::vector<flacgpu_ingest_stream> is(n);
    for (size_t i = 0; i < n; i++) is[i] = flacgpu_ingest_stream{jobs[i].in_offset, jobs[i].samples, s->place(i, s->half)};
    if (int rc = flacgpu_ingest_submit(s->ing, d_pcm, fmt, s->bps, ch, is.data(), (uint32_t)n, 2 * s->lay.half, 0u, stream, &s->d_staging))
        return fail_gpu(rc);
    std::vector<uint32_t> altered(n, 0);
    if (int rc = flacgpu_ingest_finish(s->ing, altered.data(), nullptr)) return fail_gpu(rc);
    if (s->chains) {
        std::vector<flacgpu_md5_piece> pieces;
        for (size_t i = 0; i < n; i++)
            if (jobs[i].samples) pieces.push_back(flacgpu_md5_piece{(uint32_t)i, 0u, s->place(i, s->half), jobs[i].samples * ch});
        if (int rc = flacgpu_md5_chains_update(s->chains, s->d_staging, pieces.data(), (uint32_t)pieces.size(), (s->bps + 7) / 8,
                                               flacgpu_ingest_stream_of(s->ing)))
            return fail_gpu(rc);
    }

    // ---- the blocks that the carried samples and the chunks complete
    std::vector<uint64_t> whole(n, 0), frame0(n, 0);
    std::vector<size_t> pos(n, 0);
    for (size_t i = 0; i < n; i++) {
        Stream &m = s->st[i];
        if (m.status) continue;
        m.altered += altered[i];
        chunks[i].altered = altered[i];
        whole[i] = (m.carry + jobs[i].samples) / B;
        frame0[i] = m.sizes.size();
        m.sizes.resize(m.sizes.size() + (size_t)whole[i], 0);
    }
    uint32_t batch_cap = 0;
    const std::vector<std::vector<PlanSeg>> batches = plan_stream_batches(whole, s->o.batch_frames, per, &batch_cap);
    const int whole_rc = encode_whole_blocks(
        s->g, s->bps, ch, s->device, s->sample_rate, batches, std::max(batch_cap, s->ctx_frames), true,
        [&](const PlanSeg &p) { return s->d_staging + s->place(p.stream, s->half) - (size_t)s->st[p.stream].carry * ch + p.first * per; },
        [&](const PlanSeg &p) { return frame0[p.stream] + p.first; },
        [&](const PooledContext &c, const std::vector<PlanSeg> &batch, const std::vector<uint64_t> &off) {
            uint32_t f = 0;
            for (const PlanSeg &p : batch) {
                Stream &m = s->st[p.stream];
                flacenc_session_chunk &k = chunks[p.stream];
                const uint64_t bytes = off[f + p.n] - off[f];
                for (uint32_t q = 0; q < p.n; q++) m.sizes[frame0[p.stream] + p.first + q] = (uint32_t)(off[f + q + 1] - off[f + q]);
                if (!m.status) {
                    if (!k.out || pos[p.stream] + bytes > k.out_cap) m.status = FLACENC_ERR_IO;
                    else std::memcpy(k.out + pos[p.stream], c.out + off[f], (size_t)bytes);
                    pos[p.stream] += (size_t)bytes;
                }
                f += p.n;
            }
            return (int)FLACGPU_OK;
        });
    if (whole_rc) {   // (encode_whole_blocks has set the text)
        s->gpu_rc = whole_rc;
        for (size_t i = 0; i < n; i++)
            if (!s->st[i].status) chunks[i].status = whole_rc;
        return whole_rc;
    }

    // ---- every stream's new remainder to the other half (the contexts that read this half have been waited for)
    std::vector<flacgpu_place_run> runs;
    for (size_t i = 0; i < n; i++) {
        Stream &m = s->st[i];
        if (m.status) {
            chunks[i].status = m.status;
            chunks[i].out_len = 0;
            continue;
        }
        const uint64_t pending = m.carry + jobs[i].samples, rest = pending - whole[i] * B;
        const int32_t *src = s->d_staging + s->place(i, s->half) - (size_t)m.carry * ch + (size_t)whole[i] * per;
        const int32_t *dst = s->d_staging + s->place(i, s->half ^ 1u) - (size_t)rest * ch;
        if (rest) runs.push_back(flacgpu_place_run{(uint64_t)reinterpret_cast<uintptr_t>(src), (uint64_t)reinterpret_cast<uintptr_t>(dst), rest * ch * 4});
        m.carry = (uint32_t)rest;
        m.fed += jobs[i].samples;
        chunks[i].out_len = pos[i];
    }
    if (int rc = flacgpu_ingest_move(s->ing, runs.data(), (uint32_t)runs.size())) return fail_gpu(rc);
    s->half ^= 1u;
    return 0;   // (a stream's own failure is in its chunk's status)
}

int flacenc_device_session_finalize(flacenc_device_session *s, flacenc_session_final *finals) {
    tail_stats_reset();   // (flacenc_device_tail_stats: this call's, also when it is refused)
    if (!s || (!finals && !s->st.empty())) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    if (s->finalized) return refuse(FLACENC_ERR_FINALIZED, "finalize after finalize");
    if (s->gpu_rc) return s->gpu_rc;
    s->finalized = true;
    const size_t n = s->st.size();
    const uint32_t B = s->o.block_size, ch = s->ch;
    std::vector<size_t> tails;
    for (size_t i = 0; i < n; i++) {
        Stream &m = s->st[i];
        flacenc_session_final &f = finals[i];
        f.header_len = f.tail_len = 0;
        f.altered = (uint32_t)std::min<uint64_t>(m.altered, 0xFFFFFFFFull);
        std::memset(f.md5, 0, 16);
        if (!m.status) m.status = totals_verdict(m.known, m.total, m.fed);   // Encoder::finalize_inner (encode.rs:2079-2097)
        f.status = m.status;
        if (!m.status && m.carry) tails.push_back(i);
    }
    // ---- the short last blocks: one frame each, two one-frame contexts in rotation (encode_tail_blocks, device_blocks.h,
    // with one_by_one set).  NOT as ragged batches like the one-shot call: with them the 256-tracks session measured above
    // the parent commit's maximum (DESIGN.md 4c "Short last blocks as one batch", the regression condition), and a front
    // end whose leg fails that condition keeps the one-frame loop
    if (!tails.empty()) {
        std::vector<TailFrame> tail_frames;
        for (size_t i : tails) {
            const Stream &m = s->st[i];
            tail_frames.push_back(TailFrame{s->d_staging + s->place(i, s->half) - (size_t)m.carry * ch, m.carry, m.sizes.size()});
        }
        const int tail_rc = encode_tail_blocks(
            s->g, s->bps, ch, s->device, s->sample_rate, tail_frames, true, true, true,
            [&](const PooledContext &c, size_t t0, size_t count, const std::vector<uint64_t> &off) {
                for (size_t k = 0; k < count; k++) {
                    flacenc_session_final &f = finals[tails[t0 + k]];
                    const uint64_t total = off[k + 1] - off[k];
                    if (!f.tail || total > f.tail_cap) {
                        s->st[tails[t0 + k]].status = f.status = FLACENC_ERR_IO;
                        continue;
                    }
                    std::memcpy(f.tail, c.out + off[k], (size_t)total);
                    f.tail_len = (size_t)total;
                }
                return (int)FLACGPU_OK;
            });
        if (tail_rc) s->gpu_rc = tail_rc;
    }
    // ---- the digests, then every stream's metadata
    std::vector<uint8_t> digests(16 * std::max<size_t>(n, 1), 0);
    if (!s->gpu_rc && s->chains)
        if (int rc = flacgpu_md5_chains_final(s->chains, digests.data())) s->gpu_rc = device_gpu_error(rc);
    if (s->gpu_rc) {
        for (size_t i = 0; i < n; i++)
            if (!finals[i].status) {
                finals[i].status = s->gpu_rc;
                finals[i].tail_len = 0;
            }
        return s->gpu_rc;
    }
    for (size_t i = 0; i < n; i++) {
        Stream &m = s->st[i];
        flacenc_session_final &f = finals[i];
        if (m.status) {
            f.tail_len = 0;
            continue;
        }
        std::memcpy(f.md5, &digests[16 * i], 16);
        std::vector<uint32_t> sizes = m.sizes;
        if (m.carry) sizes.push_back((uint32_t)f.tail_len);
        size_t hlen = 0;
        int rc = FLACENC_ERR_IO;
        if (f.header && m.known)
            rc = flacenc_stream_header(&s->o, s->sample_rate, s->bps, ch, m.total, f.md5, sizes.size(), sizes.data(),
                                       m.carry ? m.carry : B, f.header, f.header_cap, &hlen);
        else if (f.header)
            rc = flacenc_stream_header_unknown_total(&s->o, s->sample_rate, s->bps, ch, f.md5, sizes.size(), sizes.data(),
                                                     m.carry ? m.carry : B, f.header, f.header_cap, &hlen);
        if (!rc && hlen != m.hlen) rc = FLACENC_ERR_IO;   // (cannot happen: the header's size is fixed at open, with or without a total)
        if (rc) {
            m.status = f.status = rc != FLACENC_ERR_INVALID_ARG ? rc : FLACENC_ERR_IO;
            f.tail_len = 0;
            std::memset(f.md5, 0, 16);
            continue;
        }
        f.header_len = hlen;
    }
    for (size_t i = 0; i < n; i++)
        if (finals[i].status) return finals[i].status;
    return 0;
}

void flacenc_device_session_close(flacenc_device_session *s) {
    if (!s) return;
    flacgpu_md5_chains_destroy(s->chains);   // (waits for the chains still running on the ingest handle's stream)
    flacgpu_ingest_destroy(s->ing);
    delete s;
}

}  // extern "C"
