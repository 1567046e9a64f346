// host_internal.h -- what the host driver's translation units share besides the public C ABI (stream_writer.cpp defines them).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "flacenc_gpu.h"
#include "flacenc_stream.h"

// Not part of the public C ABI (include/flacenc_stream.h does not declare it): stream_header_len() below behind a C name, for
// tests/test_stream_header_unknown_total.py, which binds it by name.  has_total = 0: total_pcm_frames is ignored.
extern "C" int flacenc_stream_header_len(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                         uint32_t channels, int has_total, uint64_t total_pcm_frames, size_t *len);

namespace flacenc_host {

double now_ms();
int options_error(const flacenc_options &o);                                   // Options' own ranges (encode.rs:1418-1455)
flacgpu_options gpu_options(const flacenc_options &o, uint32_t block_size);   // EncoderOptions (encode.rs:1701-1709)
// interleaved int32 samples -> update_md5's byte string: little-endian samples of `width` bytes (encode.rs:1292-1318)
void pack_le(const int32_t *s, size_t count, unsigned width, uint8_t *d);
// the checks of FlacSampleWriter::new / Encoder::new for a stream whose total is known (encode.rs:487-531, 1882-1917) and
// the number of bytes in front of its first frame (fixed at `new`: the SEEKTABLE placeholder has its final size).
// has_total = false: `new` with None -- total_pcm_frames is ignored, there is no placeholder SEEKTABLE, and the size holds
// at finalize too, since a seek table then comes out of the PADDING block (encode.rs:1909-1939, 2029-2076)
int stream_header_len(const flacenc_options &o, uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels,
                      uint64_t total_pcm_frames, size_t *len, bool has_total = true);
// FlacStreamWriter::write's two subset checks, in its order (encode.rs:1127-1137): a sample rate the frame header cannot
// code (FLACENC_ERR_NON_SUBSET_SAMPLE_RATE; from 2^20 on FLACENC_ERR_INVALID_SAMPLE_RATE), then bits per sample other than
// 8, 12, 16, 20, 24 or 32 (FLACENC_ERR_NON_SUBSET_BITS_PER_SAMPLE)
int subset_frame_error(uint32_t sample_rate, uint32_t bits_per_sample);
// `helpers` parked threads of the process-wide pool run fn() side by side with the caller; returns when all are done
void run_parallel(unsigned helpers, const std::function<void()> &fn);
// what flacenc_last_error() answers on this thread
void set_last_error(const std::string &text);
// CPUs this process may really use: the cgroup's CPU quota when there is one (coalesce.cpp), else the hardware threads
unsigned usable_cpus();
// idle analysis lanes of the per-stream writers (flacenc_release_pools)
void release_lane_pool();
// idle ingest handles of flacenc_encode_many_device (device_batch.cpp; flacenc_release_pools)
void release_device_batch_pool();

// ---- coalesce.cpp's batch plan and context pool, for the other front end that batches segments of many streams
// (device_batch.cpp) ----
struct PlanSeg {
    uint32_t stream;   // index into `whole`
    uint64_t first;    // first block of the segment in its stream
    uint32_t n;        // blocks
};
// the batches of streams of whole[k] whole blocks of one shape (samples_per_block = block size x channels): plan_batches
// under the frames-per-batch rule of flacenc_encode_many_coalesced (*batch_cap: what a batch's context must hold)
std::vector<std::vector<PlanSeg>> plan_stream_batches(const std::vector<uint64_t> &whole, uint32_t batch_frames,
                                                      size_t samples_per_block, uint32_t *batch_cap);
// an analysis context for `frames` frames with its pinned buffers, from the coalescing front end's pool of idle ones
struct PooledContext {
    flacgpu_ctx *ctx;
    uint8_t *in, *out;   // pinned; out holds flacgpu_packed_cap(ctx) bytes
    size_t in_cap, out_cap;
};
int pooled_context_take(const flacgpu_options &g, uint32_t bps, uint32_t channels, uint32_t frames, int device, PooledContext *out);
void pooled_context_give(const flacgpu_options &g, uint32_t bps, uint32_t channels, uint32_t frames, int device, const PooledContext &c);

}  // namespace flacenc_host
