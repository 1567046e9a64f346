// device_stream_writer.cpp -- flacenc_device_stream_writer_*: FlacStreamWriter::write (encode.rs:1094-1274) for n streams of
// one shape whose samples lie in device memory -- every call ONE raw subset frame per stream that brings samples, of as many
// samples as it brings, numbered with that stream's own count (include/flacenc_stream.h "device stream writer"; DESIGN.md 4c
// "Device stream writer").  No metadata, no MD5: what comes out is what flacenc_stream_writer_write writes, and what
// decode_frames / decode_timeline / FlacStreamReader read.  Nothing here is new on the device:
//   * staging: an ingest handle of the writer's own whose staging buffer has a constant size; stream i's chunk is ingested
//     at int32 element i * roundup4(max_block * channels), a 16-byte boundary;
//   * the frames: one TailFrame{place, samples, number} per stream with samples through encode_tail_blocks (device_blocks.h):
//     frames of any length from many streams as ragged batches (flacgpu_encode_ragged_device) on pooled contexts of
//     gpu_options(opts, max(16, max_block)) -- a context's block size is at least 16, and flacenc_stream_writer_write too
//     encodes a frame of 1..15 samples on a context of 16 --, or under FLACGPU_NO_RAGGED=1 the one-frame loop -- the same
//     bytes; the frames go to the host.  The calls do not count into flacenc_device_tail_stats: a writer's frames are no stream's short last block.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../kernels/sample_types.h"
#include "../kernels/shape.h"   // MAXP
#include "device_blocks.h"
#include "host_internal.h"

using namespace flacenc_host;

namespace {

int refuse(int rc, const std::string &why) {
    set_last_error("flacenc_device_stream_writer: " + why);
    return rc;
}

// int32 elements of one stream's place in the staging buffer
uint64_t slot_of(uint32_t max_block, uint32_t channels) { return ((uint64_t)max_block * channels + 3u) & ~(uint64_t)3; }

// The checks of plan / open.  First what FlacStreamWriter::new and ::write check, in their order and with their codes
// (flacenc_stream_writer_new / _write): the options, bits per sample outside 1..32, the channel count, the block size, the
// subset sample rate, the subset bits per sample; then what flacenc_device_batch_plan refuses for the shape.
int plan_shape(const flacenc_options *o, uint32_t sample_rate, uint32_t bps, uint32_t channels, size_t n_streams,
               uint32_t max_block) {
    if (!o) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    if (int e = options_error(*o)) return refuse(e, "invalid options");
    if (bps < 1 || bps > 32) return refuse(FLACENC_ERR_NON_SUBSET_BITS_PER_SAMPLE, "bits per sample outside 1..32");
    if (channels < 1 || channels > 8) return refuse(FLACENC_ERR_EXCESSIVE_CHANNELS, "channels outside 1..8");
    if (max_block < 1 || max_block > 65535) return refuse(FLACENC_ERR_INVALID_BLOCK_SIZE, "max_block outside 1..65535");
    if (int e = subset_frame_error(sample_rate, bps)) return refuse(e, "a sample rate or bits per sample no subset frame header codes");
    // what is left of flacenc_device_batch_plan's refusals for a shape once the above has passed: the stream count.  (The
    // staging buffer, at most 2^32 x 2^21 bytes, cannot overflow 64 bits.)
    if (n_streams > 0xFFFFFFFFull) return refuse(FLACENC_ERR_UNSUPPORTED, "more than 2^32 - 1 streams");
    return 0;
}

// a flacgpu_* refusal of arguments: the call did nothing on the device, so it is the call's error and not the writer's
bool is_refusal(int flacgpu_rc) { return flacgpu_rc == FLACGPU_ERR_INVALID_ARG || flacgpu_rc == FLACGPU_ERR_UNSUPPORTED; }

}  // namespace

struct flacenc_device_stream_writer {
    flacenc_options o;
    flacgpu_options g;
    uint32_t sample_rate = 0, bps = 0, ch = 0, max_block = 0;
    int device = 0;
    uint64_t slot = 0;              // int32 elements per stream in the staging buffer
    flacgpu_ingest *ing = nullptr;
    int32_t *d_staging = nullptr;
    std::vector<uint64_t> number;   // every stream's next frame number
    int gpu_rc = 0;                 // sticky
};

extern "C" {

int flacenc_device_stream_writer_plan(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                      uint32_t channels, size_t n_streams, uint32_t max_block, size_t *device_bytes) {
    if (int rc = plan_shape(opts, sample_rate, bits_per_sample, channels, n_streams, max_block)) return rc;
    if (device_bytes) *device_bytes = (size_t)(4 * slot_of(max_block, channels) * (uint64_t)n_streams);
    return 0;
}

int flacenc_device_stream_writer_open(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                      uint32_t channels, size_t n_streams, uint32_t max_block, const uint64_t *first_numbers,
                                      flacenc_device_stream_writer **writer) try {
    if (!writer) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    *writer = nullptr;
    if (int rc = plan_shape(opts, sample_rate, bits_per_sample, channels, n_streams, max_block)) return rc;
    for (size_t i = 0; first_numbers && i < n_streams; i++)
        if (first_numbers[i] > kMaxFrameNumber)
            return refuse(FLACENC_ERR_EXCESSIVE_FRAME_NUMBER, "stream " + std::to_string(i) + ": its first frame number exceeds 2^36 - 1");
    std::unique_ptr<flacenc_device_stream_writer, void (*)(flacenc_device_stream_writer *)> w(
        new (std::nothrow) flacenc_device_stream_writer(), flacenc_device_stream_writer_close);   // (closed on every early return)
    if (!w) return refuse(FLACENC_ERR_UNSUPPORTED, "out of memory");
    w->o = *opts;
    w->o.vendor_string = nullptr;   // (no metadata: the writer keeps no pointers into caller memory)
    w->o.comment_fields = nullptr;
    w->o.n_comment_fields = 0;
    w->g = gpu_options(*opts, std::max(16u, max_block));   // (flacgpu_create: block sizes from 16)
    w->sample_rate = sample_rate;
    w->bps = bits_per_sample;
    w->ch = channels;
    w->max_block = max_block;
    w->slot = slot_of(max_block, channels);
    w->device = opts->device >= 0 ? opts->device : flacgpu_current_device();
    w->number.assign(n_streams, 0);
    if (first_numbers) w->number.assign(first_numbers, first_numbers + n_streams);
    // the handle, and the staging buffer at its final size now (a submit without streams allocates it): a buffer the
    // device cannot hold is open's error, not the first write's
    const flacenc_tensor_format none{FLACGPU_SAMPLE_I32, FLACGPU_LAYOUT_FLAT, 0, 0, 0};
    int rc = flacgpu_ingest_create(w->device, &w->ing);
    if (!rc) rc = flacgpu_ingest_submit(w->ing, nullptr, &none, w->bps, w->ch, nullptr, 0, w->slot * n_streams, 0u, nullptr, &w->d_staging);
    if (rc) return device_gpu_error(rc);
    *writer = w.release();
    return 0;
} catch (const std::bad_alloc &) {
    return refuse(FLACENC_ERR_UNSUPPORTED, "out of memory");
}

uint64_t flacenc_device_stream_writer_frame_number(const flacenc_device_stream_writer *w, size_t i) {
    return w && i < w->number.size() ? w->number[i] : 0;
}

int flacenc_device_stream_writer_write(flacenc_device_stream_writer *w, const void *d_pcm, const flacenc_tensor_format *fmt,
                                       flacenc_session_chunk *chunks, void *stream) try {
    if (!w || !fmt || (!chunks && !w->number.empty())) return refuse(FLACENC_ERR_INVALID_ARG, "a null argument");
    if (w->gpu_rc) return w->gpu_rc;
    const size_t n = w->number.size();
    const uint32_t ch = w->ch;
    // ---- the checks: nothing is launched or written, and no number advances, when one fails
    std::vector<flacenc_device_job> jobs(n);
    uint64_t fed_now = 0;
    for (size_t i = 0; i < n; i++) {
        if (chunks[i].samples > w->max_block)
            return refuse(FLACENC_ERR_INVALID_ARG, "chunk " + std::to_string(i) + " is longer than max_block");
        jobs[i] = flacenc_device_job{};
        jobs[i].in_offset = chunks[i].in_offset;
        jobs[i].samples = chunks[i].samples;
        fed_now += jobs[i].samples;
    }
    size_t in_elements = 0;
    if (int rc = flacenc_device_batch_plan(&w->o, fmt, w->bps, ch, jobs.data(), n, &in_elements, nullptr)) return rc;
    if ((in_elements && !d_pcm) || reinterpret_cast<uintptr_t>(d_pcm) % sample_type_align(fmt->dtype))
        return refuse(FLACENC_ERR_INVALID_ARG, "no tensor, or a tensor not aligned to its element size");
    // the ragged plan's rule (ragged_plan.h), and the one-frame path's: the reference collects partitions into
    // ArrayVec<_, 64> and panics beyond (encode.rs:3880)
    for (size_t i = 0; i < n; i++) {
        if (!jobs[i].samples) continue;
        const uint32_t tz = (uint32_t)__builtin_ctzll(jobs[i].samples);
        if (std::min(tz, w->o.max_partition_order) > (uint32_t)MAXP)
            return refuse(FLACENC_ERR_UNSUPPORTED, "stream " + std::to_string(i) + " (" + std::to_string(jobs[i].samples) +
                                                       " samples): effective partition order > " + std::to_string((int)MAXP) +
                                                       ": the reference panics (MAX_PARTITIONS = 64)");
    }
    for (size_t i = 0; i < n; i++) {
        chunks[i].out_len = 0;
        chunks[i].altered = 0;
        chunks[i].status = 0;
    }
    if (!fed_now) return 0;
    const auto fail_gpu = [&](int code) {
        w->gpu_rc = code;
        for (size_t i = 0; i < n; i++) {
            chunks[i].status = code;
            chunks[i].out_len = 0;
        }
        return code;
    };

    // ---- every chunk to its stream's place
    std::vector<flacgpu_ingest_stream> is(n);
    for (size_t i = 0; i < n; i++) is[i] = flacgpu_ingest_stream{jobs[i].in_offset, jobs[i].samples, i * w->slot};
    if (int rc = flacgpu_ingest_submit(w->ing, d_pcm, fmt, w->bps, ch, is.data(), (uint32_t)n, w->slot * n, 0u, stream, &w->d_staging)) {
        const int code = device_gpu_error(rc);
        if (!is_refusal(rc)) return fail_gpu(code);
        for (size_t i = 0; i < n; i++) chunks[i].status = code;   // (nothing ran: this call's error, the writer stays usable)
        return code;
    }
    std::vector<uint32_t> altered(n, 0);
    if (int rc = flacgpu_ingest_finish(w->ing, altered.data(), nullptr)) return fail_gpu(device_gpu_error(rc));

    // ---- one frame per stream that brought samples
    std::vector<size_t> who;
    std::vector<TailFrame> frames;
    for (size_t i = 0; i < n; i++) {
        chunks[i].altered = altered[i];
        if (!jobs[i].samples) continue;
        who.push_back(i);
        frames.push_back(TailFrame{w->d_staging + i * w->slot, (uint32_t)jobs[i].samples, w->number[i]});
    }
    const int rc = encode_tail_blocks(
        w->g, w->bps, ch, w->device, w->sample_rate, frames, true, false, false,
        [&](const PooledContext &c, size_t t0, size_t count, const std::vector<uint64_t> &off) {
            for (size_t k = 0; k < count; k++) {
                const size_t i = who[t0 + k];
                flacenc_session_chunk &q = chunks[i];
                const uint64_t size = off[k + 1] - off[k];
                if (!q.out || size > q.out_cap) {   // (as when the host writer's sink fails: the number stays)
                    q.status = FLACENC_ERR_IO;
                    continue;
                }
                std::memcpy(q.out, c.out + off[k], (size_t)size);
                q.out_len = (size_t)size;
                // (flacenc_stream_writer_write: the frame is written, the count cannot go on)
                if (w->number[i] >= kMaxFrameNumber) q.status = FLACENC_ERR_EXCESSIVE_FRAME_NUMBER;
                else w->number[i]++;
            }
            return (int)FLACGPU_OK;
        });
    if (rc) return fail_gpu(rc);   // (encode_tail_blocks has set the text; the checks above leave it no argument to refuse)
    return 0;   // (a stream's own failure is in its chunk's status)
} catch (const std::bad_alloc &) {
    return refuse(FLACENC_ERR_UNSUPPORTED, "out of memory");
}

void flacenc_device_stream_writer_close(flacenc_device_stream_writer *w) {
    if (!w) return;
    flacgpu_ingest_destroy(w->ing);
    delete w;
}

}  // extern "C"
