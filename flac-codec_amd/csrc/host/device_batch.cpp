// device_batch.cpp -- flacenc_encode_many_device: a batch of streams of one shape held in DEVICE memory (int32, int16, packed
// 24-bit or float32; planar and padded, or interleaved and flat) -> finished .flac files in the callers' host buffers, the samples
// never visiting the host.  The mirror image of flacgpu_decoder_decode_as.  flacenc_encode_many_device_out is the same loop
// (encode_impl, below) with the files left in DEVICE memory, in slots of one buffer of the caller's: there a retired batch's
// frames are not fetched but placed by k_place_runs (flacgpu_frame_offsets + flacgpu_place_frames) beside the next batch's
// analysis, and the headers, built on the host, go up in one copy and to their places in one launch (flacgpu_ingest_place).
//
//   * plan (pure host code): the checks, the elements the tensor must hold, the staging bytes;
//   * ingest (ingest.hip, kernels/ingest.inc): one kernel pass converts the tensor by ingest_sample (kernels/ingest_rule.h)
//     into interleaved int32 in the ingest handle's staging buffer, every stream from a 16-byte boundary -- what
//     flacgpu_encode_segments_device reads in place.  This version always ingests (an aligned FLAT I32 batch could be read
//     in place: a follow-up);
//   * MD5 on the device, one k_md5_many lane per stream (about 15 MB/s per stream, DESIGN.md section 4b: fine for many
//     clips, poor for one long stream -- FLACENC_DEVICE_NO_MD5 is the way round it today), queued behind the ingest on
//     the handle's stream, so that it runs beside the analysis;
//   * whole blocks: batches of segments planned as flacenc_encode_many_coalesced plans them (plan_stream_batches), on two
//     pooled contexts in rotation -- batch i + 1 is submitted before batch i's frames are fetched into its pinned buffer,
//     so one batch's kernels run while the other's frames cross the link -- and copied once to their places in `out`;
//   * the streams' short last blocks: ragged batches (flacgpu_encode_ragged_device) on the staging pointers, each of up
//     to a pooled context's frames -- all the tails of a call of up to a few thousand streams in ONE batch
//     (encode_tail_blocks, device_blocks.h).  FLACGPU_NO_RAGGED=1 keeps the loop this replaced, a one-frame
//     flacgpu_encode_device call per stream on two one-frame contexts in rotation (what coalesce.cpp does from host PCM);
//   * everything in front of the first frame: flacenc_stream_header, as in coalesce.cpp.
// The whole-block loop (encode_whole_blocks, device_blocks.h) is shared with the chunk-by-chunk sessions of
// device_session.cpp.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../kernels/ingest_rule.h"
#include "../kernels/sample_types.h"
#include "../kernels/shape.h"   // Knobs
#include "device_blocks.h"
#include "host_internal.h"

using namespace flacenc_host;

namespace {

// idle ingest handles (a stream, an event and the staging buffer: kept between calls like the analysis contexts)
struct IngestPool {
    std::mutex mu;
    std::vector<flacgpu_ingest *> idle;
    static IngestPool &get() {
        static IngestPool *p = new IngestPool();   // leaked on purpose: no HIP calls during static destruction
        return *p;
    }
    int take(int device, flacgpu_ingest **out) {
        {
            std::lock_guard<std::mutex> l(mu);
            for (size_t i = 0; i < idle.size(); i++)
                if (flacgpu_ingest_device(idle[i]) == device) {
                    *out = idle[i];
                    idle.erase(idle.begin() + (ptrdiff_t)i);
                    return 0;
                }
        }
        return flacgpu_ingest_create(device, out);
    }
    void give(flacgpu_ingest *g) {
        flacgpu_ingest *drop = nullptr;
        {
            std::lock_guard<std::mutex> l(mu);
            idle.push_back(g);
            if (idle.size() > 2) {   // the oldest goes
                drop = idle.front();
                idle.erase(idle.begin());
            }
        }
        flacgpu_ingest_destroy(drop);
    }
    void release_all() {
        std::vector<flacgpu_ingest *> all;
        {
            std::lock_guard<std::mutex> l(mu);
            all.swap(idle);
        }
        for (flacgpu_ingest *g : all) flacgpu_ingest_destroy(g);
    }
};

int gpu_error(int rc) { return device_gpu_error(rc); }
int refuse(int rc, const std::string &why) {
    set_last_error("flacenc_device_batch_plan: " + why);
    return rc;
}

// The checks of plan / encode (Job: flacenc_device_job or flacenc_device_out_job); staging_off (may be null) receives every stream's first int32 in the staging buffer.
template <class Job>
int plan_impl(const flacenc_options *o, const flacenc_tensor_format *fmt, uint32_t bps, uint32_t channels,
              const Job *jobs, size_t n_jobs, uint64_t *in_elements, uint64_t *staging_elements,
              std::vector<uint64_t> *staging_off) {
    if (!o || !fmt || (!jobs && n_jobs)) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    if (int e = options_error(*o)) return e;
    const bool padded = fmt->layout == FLACGPU_LAYOUT_PADDED;
    if (!sample_type_known(fmt->dtype) || fmt->layout > FLACGPU_LAYOUT_PADDED || fmt->reserved ||
        (!padded && (fmt->channels_padded || fmt->samples_padded)))
        return refuse(FLACENC_ERR_INVALID_ARG, "unknown dtype or layout, reserved not 0, or padded fields under FLAT");
    if (channels < 1 || channels > FLACGPU_MAX_CHANNELS || bps < 1 || bps > 32)
        return refuse(FLACENC_ERR_INVALID_ARG, "channels outside 1..8 or bits per sample outside 1..32");
    if (sample_type_max_bits(fmt->dtype) && bps > sample_type_max_bits(fmt->dtype))
        return refuse(FLACENC_ERR_UNSUPPORTED, std::string(sample_type_name(fmt->dtype)) + " input, but " + std::to_string(bps) +
                                                   " bits per sample");
    if (n_jobs > 0xFFFFFFFFull) return refuse(FLACENC_ERR_UNSUPPORTED, "more than 2^32 - 1 streams");
    if (padded && fmt->channels_padded < channels)
        return refuse(FLACENC_ERR_INVALID_ARG, "channels_padded is less than channels");
    uint64_t in_end = 0, staging = 0;
    if (staging_off) staging_off->assign(n_jobs, 0);
    std::vector<std::pair<uint64_t, uint64_t>> spans;   // FLAT: [first element, end) of every stream with samples
    for (size_t i = 0; i < n_jobs; i++) {
        uint64_t count = 0, rounded = 0;
        if (__builtin_mul_overflow(jobs[i].samples, (uint64_t)channels, &count) ||
            __builtin_add_overflow(count, (uint64_t)3, &rounded) ||
            __builtin_add_overflow(staging, rounded & ~(uint64_t)3, &rounded))
            return refuse(FLACENC_ERR_UNSUPPORTED, "the batch exceeds 2^64 samples");
        if (staging_off) (*staging_off)[i] = staging;
        staging = rounded;
        if (padded) {
            if (jobs[i].samples > fmt->samples_padded)
                return refuse(FLACENC_ERR_INVALID_ARG, "stream " + std::to_string(i) + " is longer than samples_padded");
        } else if (count) {
            uint64_t end = 0;
            if (__builtin_add_overflow(jobs[i].in_offset, count, &end))
                return refuse(FLACENC_ERR_INVALID_ARG, "stream " + std::to_string(i) + ": in_offset + its elements overflows");
            spans.emplace_back(jobs[i].in_offset, end);
            in_end = std::max(in_end, end);
        }
    }
    if (padded) {
        if (__builtin_mul_overflow((uint64_t)n_jobs * fmt->channels_padded, fmt->samples_padded, &in_end))
            return refuse(FLACENC_ERR_UNSUPPORTED, "the padded batch exceeds 2^64 elements");
    } else {
        std::sort(spans.begin(), spans.end());
        for (size_t k = 1; k < spans.size(); k++)
            if (spans[k].first < spans[k - 1].second) return refuse(FLACENC_ERR_INVALID_ARG, "FLAT streams overlap");
    }
    if (staging > (~(uint64_t)0) / 4) return refuse(FLACENC_ERR_UNSUPPORTED, "the staging buffer exceeds 2^64 bytes");
    *in_elements = in_end;
    *staging_elements = staging;
    return 0;
}

struct Stream {
    uint64_t whole = 0;             // whole blocks
    uint32_t tail = 0;              // samples of the short last block (0: none)
    size_t hlen = 0;                // bytes in front of the first frame
    uint64_t pos = 0;               // bytes of the frames placed so far
    std::vector<uint32_t> sizes;    // per frame
    std::vector<uint8_t> tail_bytes;   // host output: the short last block's frame until the header is written
    size_t tail_len = 0;               // its size
    bool tail_done = false;            // ... is known
    bool tail_placed = false;          // device output: it is in its place
};
struct CopyJob {
    const uint8_t *src;
    uint8_t *dst;
    size_t n;
};

// the frames of a retired batch to their places, a few threads side by side (one copy per output byte)
void run_copies(const std::vector<CopyJob> &cj) {
    size_t bytes = 0;
    for (const CopyJob &c : cj) bytes += c.n;
    std::atomic<size_t> next{0};
    const auto work = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < cj.size();) std::memcpy(cj[i].dst, cj[i].src, cj[i].n);
    };
    const unsigned helpers = (unsigned)std::min<size_t>({bytes >> 20, cj.size() ? cj.size() - 1 : 0, (size_t)std::min(usable_cpus(), 8u) - 1});
    run_parallel(helpers, work);
}

// where a stream's file begins: a host address (flacenc_device_job) or a device address (flacenc_device_out_job: never
// dereferenced here)
inline bool has_place(const flacenc_device_job &j) { return j.out != nullptr; }
inline bool has_place(const flacenc_device_out_job &) { return true; }
inline uint8_t *place_of(const flacenc_device_job &j, uint8_t *) { return j.out; }
inline uint8_t *place_of(const flacenc_device_out_job &j, uint8_t *d_out) { return d_out + j.out_offset; }
inline uint64_t address(const uint8_t *p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }

// The slots of flacenc_device_out_plan: every one inside [0, d_out_bytes), no two with bytes overlapping.
int slots_error(const flacenc_device_out_job *jobs, size_t n_jobs, size_t d_out_bytes) {
    const auto refuse_slot = [](const std::string &why) {
        set_last_error("flacenc_device_out_plan: " + why);
        return FLACENC_ERR_INVALID_ARG;
    };
    std::vector<std::pair<uint64_t, uint64_t>> spans;   // [first byte, end) of every slot that holds bytes
    for (size_t i = 0; i < n_jobs; i++) {
        uint64_t end = 0;
        if (__builtin_add_overflow(jobs[i].out_offset, jobs[i].out_cap, &end))
            return refuse_slot("stream " + std::to_string(i) + ": out_offset + out_cap overflows");
        if (end > d_out_bytes) return refuse_slot("stream " + std::to_string(i) + ": its slot reaches past d_out_bytes");
        if (jobs[i].out_cap) spans.emplace_back(jobs[i].out_offset, end);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); k++)
        if (spans[k].first < spans[k - 1].second) return refuse_slot("two slots overlap");
    return 0;
}

template <class Job>
int encode_impl(const flacenc_options *opts, const void *d_pcm, const flacenc_tensor_format *fmt, uint32_t sample_rate,
                uint32_t bits_per_sample, uint32_t channels, Job *jobs, size_t n_jobs, uint8_t *d_out, uint32_t flags,
                void *stream, const std::vector<uint64_t> &staging_off, uint64_t staging_elements);

}  // namespace

Knobs read_knobs();   // flacenc_gpu.hip: every FLACGPU_* selector is read there

namespace flacenc_host {
void release_device_batch_pool() { IngestPool::get().release_all(); }

bool tails_one_by_one() {
    static const bool v = read_knobs().no_ragged;   // (once: knobs do not change under a running process)
    return v;
}
namespace {
thread_local uint64_t g_tail_frames = 0, g_tail_batches = 0;
}
void tail_stats_reset() { g_tail_frames = g_tail_batches = 0; }
void tail_stats_add(uint64_t frames, uint64_t batches) {
    g_tail_frames += frames;
    g_tail_batches += batches;
}
}  // namespace flacenc_host

extern "C" {

int32_t flacenc_ingest_sample(uint32_t sample_type, uint32_t raw_bits, uint32_t bits_per_sample, int *altered) {
    int a = 1;
    int32_t v = 0;
    if (sample_type_known(sample_type) && bits_per_sample >= 1 && bits_per_sample <= 32 &&
        !(sample_type_max_bits(sample_type) && bits_per_sample > sample_type_max_bits(sample_type)))
        v = ingest_sample(sample_type, raw_bits, bits_per_sample, &a);
    if (altered) *altered = a;
    return v;
}

void flacenc_device_tail_stats(uint64_t *tail_frames, uint64_t *tail_batches) {
    if (tail_frames) *tail_frames = flacenc_host::g_tail_frames;
    if (tail_batches) *tail_batches = flacenc_host::g_tail_batches;
}

int flacenc_device_batch_plan(const flacenc_options *opts, const flacenc_tensor_format *fmt, uint32_t bits_per_sample,
                              uint32_t channels, const flacenc_device_job *jobs, size_t n_jobs, size_t *in_elements,
                              size_t *staging_bytes) {
    uint64_t in = 0, st = 0;
    if (int rc = plan_impl(opts, fmt, bits_per_sample, channels, jobs, n_jobs, &in, &st, nullptr)) return rc;
    if (in_elements) *in_elements = (size_t)in;
    if (staging_bytes) *staging_bytes = (size_t)(4 * st);
    return 0;
}

int flacenc_encode_many_device(const flacenc_options *opts, const void *d_pcm, const flacenc_tensor_format *fmt,
                               uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels, flacenc_device_job *jobs,
                               size_t n_jobs, uint32_t flags, void *stream) {
    tail_stats_reset();   // (flacenc_device_tail_stats: this call's, also when it is refused or ends before its tails)
    uint64_t in_elements = 0, staging_elements = 0;
    std::vector<uint64_t> staging_off;
    if (int rc = plan_impl(opts, fmt, bits_per_sample, channels, jobs, n_jobs, &in_elements, &staging_elements, &staging_off))
        return rc;
    if ((flags & ~FLACENC_DEVICE_NO_MD5) || (in_elements && !d_pcm) ||
        reinterpret_cast<uintptr_t>(d_pcm) % sample_type_align(fmt->dtype)) {
        set_last_error("flacenc_encode_many_device: unknown flags, no tensor, or a tensor not aligned to its element size");
        return FLACENC_ERR_INVALID_ARG;
    }
    return encode_impl(opts, d_pcm, fmt, sample_rate, bits_per_sample, channels, jobs, n_jobs, nullptr, flags, stream, staging_off,
                       staging_elements);
}

int flacenc_device_out_plan(const flacenc_options *opts, const flacenc_tensor_format *fmt, uint32_t bits_per_sample,
                            uint32_t channels, const flacenc_device_out_job *jobs, size_t n_jobs, size_t d_out_bytes,
                            size_t *in_elements, size_t *staging_bytes) {
    uint64_t in = 0, st = 0;
    if (int rc = plan_impl(opts, fmt, bits_per_sample, channels, jobs, n_jobs, &in, &st, nullptr)) return rc;
    if (int rc = slots_error(jobs, n_jobs, d_out_bytes)) return rc;
    if (in_elements) *in_elements = (size_t)in;
    if (staging_bytes) *staging_bytes = (size_t)(4 * st);
    return 0;
}

int flacenc_encode_many_device_out(const flacenc_options *opts, const void *d_pcm, const flacenc_tensor_format *fmt,
                                   uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels,
                                   flacenc_device_out_job *jobs, size_t n_jobs, void *d_out, size_t d_out_bytes, uint32_t flags,
                                   void *stream) {
    tail_stats_reset();
    uint64_t in_elements = 0, staging_elements = 0;
    std::vector<uint64_t> staging_off;
    if (int rc = plan_impl(opts, fmt, bits_per_sample, channels, jobs, n_jobs, &in_elements, &staging_elements, &staging_off))
        return rc;
    if (int rc = slots_error(jobs, n_jobs, d_out_bytes)) return rc;
    if ((flags & ~FLACENC_DEVICE_NO_MD5) || (in_elements && !d_pcm) || (d_out_bytes && !d_out) ||
        reinterpret_cast<uintptr_t>(d_pcm) % sample_type_align(fmt->dtype)) {
        set_last_error("flacenc_encode_many_device_out: unknown flags, no tensor, no output buffer, or a tensor not aligned to its "
                       "element size");
        return FLACENC_ERR_INVALID_ARG;
    }
    return encode_impl(opts, d_pcm, fmt, sample_rate, bits_per_sample, channels, jobs, n_jobs, static_cast<uint8_t *>(d_out), flags,
                       stream, staging_off, staging_elements);
}

}  // extern "C"

namespace {

// The loop of both entry points, behind their checks.  Job = flacenc_device_job: every file to jobs[i].out in host memory.
// Job = flacenc_device_out_job: every file to d_out + jobs[i].out_offset in device memory.
template <class Job>
int encode_impl(const flacenc_options *opts, const void *d_pcm, const flacenc_tensor_format *fmt, uint32_t sample_rate,
                uint32_t bits_per_sample, uint32_t channels, Job *jobs, size_t n_jobs, uint8_t *d_out, uint32_t flags,
                void *stream, const std::vector<uint64_t> &staging_off, uint64_t staging_elements) {
    constexpr bool kDeviceOut = std::is_same<Job, flacenc_device_out_job>::value;
    const flacenc_options &o = *opts;
    const uint32_t B = o.block_size, ch = channels, bps = bits_per_sample;
    const size_t per = (size_t)B * ch;
    const bool md5 = !(flags & FLACENC_DEVICE_NO_MD5);
    const int device = o.device >= 0 ? o.device : flacgpu_current_device();
    const flacgpu_options g = gpu_options(o, B);

    // ---- the streams: what flacenc_encode_many checks per job, and the size of what stands in front of the first frame
    std::vector<Stream> st(n_jobs);
    std::map<uint64_t, std::pair<int, size_t>> header_memo;   // (streams of one length share their header's size)
    for (size_t i = 0; i < n_jobs; i++) {
        Job &j = jobs[i];
        j.out_len = 0;
        j.status = 0;
        j.altered = 0;
        std::memset(j.md5, 0, 16);
        if (!j.samples || !has_place(j)) {
            j.status = FLACENC_ERR_INVALID_ARG;
            continue;
        }
        auto it = header_memo.find(j.samples);
        if (it == header_memo.end()) {
            size_t l = 0;
            const int rc = stream_header_len(o, sample_rate, bps, ch, j.samples, &l);
            it = header_memo.emplace(j.samples, std::make_pair(rc, l)).first;
        }
        if (it->second.first) {
            j.status = it->second.first;
            continue;
        }
        Stream &s = st[i];
        s.hlen = it->second.second;
        if (s.hlen > j.out_cap) {
            j.status = FLACENC_ERR_IO;
            continue;
        }
        s.whole = j.samples / B;
        s.tail = (uint32_t)(j.samples % B);
        s.sizes.assign(s.whole + (s.tail ? 1 : 0), 0);
    }
    const auto fail = [&](size_t i, int rc) {
        if (!jobs[i].status) jobs[i].status = rc;
    };
    const auto fail_all = [&](int rc) {
        for (size_t i = 0; i < n_jobs; i++) fail(i, rc);
        return rc;
    };

    // ---- ingest (and the MD5 chains behind it)
    flacgpu_ingest *ing = nullptr;
    if (int rc = IngestPool::get().take(device, &ing)) return fail_all(gpu_error(rc));
    struct Giver {
        flacgpu_ingest *g;
        ~Giver() { IngestPool::get().give(g); }
    } giver{ing};
    std::vector<flacgpu_ingest_stream> is(n_jobs);
    for (size_t i = 0; i < n_jobs; i++) is[i] = flacgpu_ingest_stream{jobs[i].in_offset, jobs[i].samples, staging_off[i]};
    int32_t *d_staging = nullptr;
    if (int rc = flacgpu_ingest_submit(ing, d_pcm, fmt, bps, ch, is.data(), (uint32_t)n_jobs, staging_elements,
                                       md5 ? FLACGPU_INGEST_MD5 : 0u, stream, &d_staging))
        return fail_all(gpu_error(rc));

    // ---- whole blocks: batches of segments, two contexts in rotation
    std::vector<uint64_t> whole(n_jobs);
    for (size_t i = 0; i < n_jobs; i++) whole[i] = jobs[i].status ? 0 : st[i].whole;
    uint32_t batch_cap = 0;
    const std::vector<std::vector<PlanSeg>> batches = plan_stream_batches(whole, o.batch_frames, per, &batch_cap);
    std::vector<CopyJob> cj;
    std::vector<flacgpu_place_run> runs;
    const int whole_rc = encode_whole_blocks(
        g, bps, ch, device, sample_rate, batches, batch_cap, !kDeviceOut,
        [&](const PlanSeg &p) { return d_staging + staging_off[p.stream] + p.first * per; },
        [&](const PlanSeg &p) { return p.first; },
        [&](const PooledContext &s, const std::vector<PlanSeg> &batch, const std::vector<uint64_t> &off) {
            cj.clear();
            runs.clear();
            uint32_t f = 0;
            for (const PlanSeg &p : batch) {
                Stream &sm = st[p.stream];
                Job &j = jobs[p.stream];
                const uint64_t bytes = off[f + p.n] - off[f];
                for (uint32_t k = 0; k < p.n; k++) sm.sizes[p.first + k] = (uint32_t)(off[f + k + 1] - off[f + k]);
                uint8_t *const to = place_of(j, d_out) + sm.hlen + sm.pos;
                if (sm.hlen + sm.pos + bytes > j.out_cap) fail(p.stream, FLACENC_ERR_IO);
                else if (j.status) ;
                else if (kDeviceOut) runs.push_back(flacgpu_place_run{off[f], address(to), bytes});
                else cj.push_back(CopyJob{s.out + off[f], to, (size_t)bytes});
                sm.pos += bytes;
                f += p.n;
            }
            // (device output: the kernel runs on this context's stream, beside the next batch's analysis on the other's)
            if (kDeviceOut) return flacgpu_place_frames(s.ctx, runs.data(), (uint32_t)runs.size());
            run_copies(cj);
            return (int)FLACGPU_OK;
        });
    if (whole_rc)
        for (size_t i = 0; i < n_jobs; i++)
            if (whole[i]) fail(i, whole_rc);

    // ---- the short last blocks: ragged batches of up to a pooled context's frames (encode_tail_blocks; under
    // FLACGPU_NO_RAGGED one frame each on two one-frame contexts in rotation).  Host output: the batch is fetched once and
    // every tail copied out; device output: all its tails placed by ONE flacgpu_place_frames call, one run per tail
    std::vector<size_t> tails;
    std::vector<TailFrame> tail_frames;
    for (size_t i = 0; i < n_jobs; i++)
        if (!jobs[i].status && st[i].tail) {
            tails.push_back(i);
            tail_frames.push_back(TailFrame{d_staging + staging_off[i] + st[i].whole * per, st[i].tail, st[i].whole});
        }
    if (!tails.empty()) {
        std::vector<size_t> placing;
        const int tail_rc = encode_tail_blocks(
            g, bps, ch, device, sample_rate, tail_frames, !kDeviceOut, false, true,
            [&](const PooledContext &s, size_t t0, size_t count, const std::vector<uint64_t> &off) {
                runs.clear();
                placing.clear();
                for (size_t k = 0; k < count; k++) {
                    const size_t i = tails[t0 + k];
                    Stream &sm = st[i];
                    const uint64_t total = off[k + 1] - off[k];
                    sm.sizes[sm.whole] = (uint32_t)total;
                    sm.tail_len = (size_t)total;
                    sm.tail_done = true;
                    if (!kDeviceOut) {
                        sm.tail_bytes.assign(s.out + off[k], s.out + off[k + 1]);
                    } else if (sm.hlen + sm.pos + total <= jobs[i].out_cap) {   // (else: FLACENC_ERR_IO where the header is built)
                        runs.push_back(flacgpu_place_run{off[k], address(place_of(jobs[i], d_out) + sm.hlen + sm.pos), total});
                        placing.push_back(i);
                    }
                }
                if (!kDeviceOut || runs.empty()) return (int)FLACGPU_OK;
                const int rc = flacgpu_place_frames(s.ctx, runs.data(), (uint32_t)runs.size());
                if (!rc)
                    for (size_t i : placing) st[i].tail_placed = true;
                return rc;
            });
        if (tail_rc)
            for (size_t i : tails)
                if (!st[i].tail_done || (kDeviceOut && !st[i].tail_placed && !jobs[i].status)) fail(i, tail_rc);
    }

    // ---- the digests, then every stream's metadata and its last frame
    std::vector<uint32_t> altered(n_jobs);
    std::vector<uint8_t> digests(16 * n_jobs, 0);
    if (int rc = flacgpu_ingest_finish(ing, altered.data(), md5 ? digests.data() : nullptr)) return fail_all(gpu_error(rc));
    // device output: the headers are built one behind another in a pinned buffer of the ingest handle's
    uint8_t *headers = nullptr;
    size_t headers_len = 0;
    std::vector<flacgpu_place_run> header_runs;
    if (kDeviceOut) {
        size_t sum = 0;
        for (size_t i = 0; i < n_jobs; i++)
            if (!jobs[i].status) sum += st[i].hlen;
        if (int rc = flacgpu_ingest_scratch(ing, sum, &headers)) return fail_all(gpu_error(rc));
    }
    for (size_t i = 0; i < n_jobs; i++) {
        Job &j = jobs[i];
        j.altered = altered[i];
        std::memcpy(j.md5, &digests[16 * i], 16);
        if (j.status) continue;
        Stream &s = st[i];
        size_t hlen = 0;
        const uint32_t last_len = s.tail ? s.tail : B;
        uint8_t *const to = place_of(j, d_out);
        int rc = flacenc_stream_header(&o, sample_rate, bps, ch, j.samples, j.md5, s.sizes.size(), s.sizes.data(), last_len,
                                       kDeviceOut ? headers + headers_len : to, kDeviceOut ? s.hlen : (size_t)j.out_cap, &hlen);
        if (!rc && hlen != s.hlen) rc = FLACENC_ERR_IO;   // (cannot happen: the header's size is fixed at `new`)
        if (rc || s.hlen + s.pos + s.tail_len > j.out_cap) {
            fail(i, rc && rc != FLACENC_ERR_INVALID_ARG ? rc : FLACENC_ERR_IO);
            continue;
        }
        if (kDeviceOut) {
            header_runs.push_back(flacgpu_place_run{headers_len, address(to), s.hlen});
            headers_len += s.hlen;
        } else if (s.tail_len) {
            std::memcpy(to + s.hlen + s.pos, s.tail_bytes.data(), s.tail_len);
        }
        j.out_len = s.hlen + s.pos + s.tail_len;
    }
    if (kDeviceOut)   // one upload, one launch, and the handle's stream waited for: the files are complete
        if (int rc = flacgpu_ingest_place(ing, headers_len, header_runs.data(), (uint32_t)header_runs.size())) {
            const int e = gpu_error(rc);
            for (size_t i = 0; i < n_jobs; i++)
                if (!jobs[i].status) {
                    jobs[i].status = e;
                    jobs[i].out_len = 0;
                }
        }
    for (size_t i = 0; i < n_jobs; i++)
        if (jobs[i].status) return jobs[i].status;
    return 0;
}

}  // namespace
