// host_internal.h -- what the host driver's translation units share besides the public C ABI.  Each group says which unit
// defines it; the container rules of a stream (options_error, subset_frame_error, stream_header_len, ...) are stream_ledger.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "flacenc_gpu.h"
#include "flacenc_stream.h"
#include "stream_ledger.h"

// Not part of the public C ABI (include/flacenc_stream.h does not declare it): stream_header_len() (stream_ledger.h) behind a C name, for
// tests/test_stream_header_unknown_total.py, which binds it by name.  has_total = 0: total_pcm_frames is ignored.
extern "C" int flacenc_stream_header_len(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                         uint32_t channels, int has_total, uint64_t total_pcm_frames, size_t *len);

namespace flacenc_host {

// ---- stream_writer.cpp ----
double now_ms();
flacgpu_options gpu_options(const flacenc_options &o, uint32_t block_size);   // EncoderOptions (encode.rs:1701-1709)
// interleaved int32 samples -> update_md5's byte string: little-endian samples of `width` bytes (encode.rs:1292-1318)
void pack_le(const int32_t *s, size_t count, unsigned width, uint8_t *d);
// `helpers` parked threads of the process-wide pool run fn() side by side with the caller; returns when all are done
void run_parallel(unsigned helpers, const std::function<void()> &fn);
// what flacenc_last_error() answers on this thread
void set_last_error(const std::string &text);
// idle analysis lanes of the per-stream writers (flacenc_release_pools)
void release_lane_pool();
// CPUs this process may really use: the cgroup's CPU quota when there is one (cpu_quota.cpp), else the hardware threads
unsigned usable_cpus();
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
