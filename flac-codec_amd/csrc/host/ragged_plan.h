// ragged_plan.h -- a RAGGED batch (flacgpu_encode_ragged_device: every frame has a length of its own): the checks and the
// layout of the window pool, as one pure function.  Plain C++ (no HIP, no context, no getenv): flacgpu_ragged_plan exports
// it, flacgpu_encode_ragged_device runs it first, tools/ragged_plan_check.cpp walks it under a sanitizer.
#ifndef FLACENC_HOST_RAGGED_PLAN_H
#define FLACENC_HOST_RAGGED_PLAN_H
#include <stdint.h>

#include <string>
#include <vector>

#include "../kernels/shape.h"   // MAXP

namespace flacenc_ragged {

constexpr uint32_t kWindowPad = 64;   // zero doubles behind every window of the pool (the kernels' tiles may read them)

// 0, or the negative FLACGPU_ERR_* value with *err set
constexpr int kOk = 0, kInvalidArg = -1, kUnsupported = -2;

// samples[n_frames]: the frames' lengths.  block_size / max_partition_order: the context's options.
// Out (any may be nullptr): window_of[n_frames] -- the index of frame f's window among the distinct lengths;
// distinct[<= n_frames] -- the distinct lengths in first-appearance order, *n_distinct of them; *pool_doubles -- the pool's
// size, sum(n + kWindowPad) over them (window d starts at the sum over the windows in front of it).
// Nothing is written unless the batch is accepted.
inline int plan(uint32_t block_size, uint32_t max_partition_order, const uint32_t *samples, uint32_t n_frames, uint32_t *window_of,
                uint32_t *distinct, uint32_t *n_distinct, uint64_t *pool_doubles, std::string *err) {
    auto fail = [&](int rc, const std::string &text) {
        if (err) *err = text;
        return rc;
    };
    if (!samples || n_frames == 0) return fail(kInvalidArg, "ragged batch: no frames");
    if (block_size < 16 || block_size > 65535 || max_partition_order > 15) return fail(kInvalidArg, "ragged batch: invalid options");
    for (uint32_t f = 0; f < n_frames; f++) {
        const uint32_t n = samples[f];
        if (n == 0) return fail(kInvalidArg, "ragged batch: frame " + std::to_string(f) + " has no samples");
        if (n > block_size)
            return fail(kInvalidArg, "ragged batch: frame " + std::to_string(f) + " has " + std::to_string(n) +
                                         " samples, more than the block size " + std::to_string(block_size));
    }
    // the reference collects partitions into ArrayVec<_, 64> and panics beyond (encode.rs:3880)
    for (uint32_t f = 0; f < n_frames; f++) {
        const uint32_t tz = (uint32_t)__builtin_ctz(samples[f]);
        if ((tz < max_partition_order ? tz : max_partition_order) > (uint32_t)MAXP)
            return fail(kUnsupported, "ragged batch: frame " + std::to_string(f) + " (" + std::to_string(samples[f]) +
                                          " samples): effective partition order > " + std::to_string((int)MAXP) +
                                          ": the reference panics (MAX_PARTITIONS = 64)");
    }
    // distinct lengths in first-appearance order: slot[n] = index + 1 (block_size <= 65535)
    std::vector<uint32_t> seen((size_t)block_size + 1, 0u);   // (a search of `distinct` would be quadratic)
    uint32_t nd = 0;
    uint64_t pool = 0;
    for (uint32_t f = 0; f < n_frames; f++) {
        const uint32_t n = samples[f];
        if (!seen[n]) {
            seen[n] = ++nd;
            if (distinct) distinct[nd - 1] = n;
            pool += (uint64_t)n + kWindowPad;
        }
        if (window_of) window_of[f] = seen[n] - 1;
    }
    if (n_distinct) *n_distinct = nd;
    if (pool_doubles) *pool_doubles = pool;
    return kOk;
}

}  // namespace flacenc_ragged
#endif
