// device_blocks.h -- what the two device front ends share (device_batch.cpp: flacenc_encode_many_device[_out];
// device_session.cpp: flacenc_device_session_*): the loop that sends planned batches of whole-block segments, all lying in
// device memory, through two pooled contexts in rotation.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "host_internal.h"

namespace flacenc_host {

inline int device_gpu_error(int rc) {
    set_last_error(std::string("gpu: ") + flacgpu_last_error());
    return rc == FLACGPU_ERR_UNSUPPORTED ? FLACENC_ERR_UNSUPPORTED : FLACENC_ERR_GPU;
}

// The batches of plan_stream_batches, two contexts of `ctx_frames` frames in rotation: batch b + 1 is submitted before
// batch b is retired, so one batch's kernels run while the other's frames (or their sizes) cross the link.
//   pcm_of(seg)      the device address of the segment's first sample (interleaved int32)
//   number_of(seg)   the frame number of its first block
//   retire(slot, batch, off)   batch b is complete in `slot` (frames_to_host: its frames lie in slot.out; else only the
//                    offsets were fetched): off[f] .. off[f + 1] is frame f of the batch, segments in order; returns a
//                    FLACGPU code
// Returns 0 or the FLACENC code of the first GPU failure (the text in flacenc_last_error); nothing of the call is in
// flight when it returns.
template <class PcmOf, class NumberOf, class Retire>
int encode_whole_blocks(const flacgpu_options &g, uint32_t bps, uint32_t ch, int device, uint32_t sample_rate,
                        const std::vector<std::vector<PlanSeg>> &batches, uint32_t ctx_frames, bool frames_to_host,
                        PcmOf pcm_of, NumberOf number_of, Retire retire) {
    int whole_rc = 0;
    if (batches.empty()) return 0;
    PooledContext slot[2] = {};
    const size_t n_slots = std::min<size_t>(2, batches.size());
    size_t have = 0;
    for (; have < n_slots; have++)
        if (int rc = pooled_context_take(g, bps, ch, ctx_frames, device, &slot[have])) {
            whole_rc = device_gpu_error(rc);
            break;
        }
    const auto submit = [&](size_t b) {
        std::vector<flacgpu_segment> gs(batches[b].size());
        for (size_t k = 0; k < gs.size(); k++) {
            const PlanSeg &p = batches[b][k];
            gs[k].pcm = pcm_of(p);
            gs[k].n_frames = p.n;
            gs[k].reserved = 0;
            gs[k].first_frame_number = number_of(p);
        }
        return flacgpu_encode_segments_device(slot[b % 2].ctx, gs.data(), (uint32_t)gs.size(), sample_rate, nullptr);
    };
    std::vector<uint64_t> off;
    int rc = whole_rc ? FLACGPU_ERR_HIP : submit(0);
    for (size_t b = 0; b < batches.size() && !rc; b++) {
        if (b + 1 < batches.size()) rc = submit(b + 1);   // its kernels run while batch b's frames are fetched
        if (rc) break;
        const PooledContext &s = slot[b % 2];
        uint32_t frames = 0;
        for (const PlanSeg &p : batches[b]) frames += p.n;
        off.assign((size_t)frames + 1, 0);
        uint64_t total = 0;
        // host output: the frames cross the link; device output: only their sizes do
        rc = frames_to_host ? flacgpu_fetch_frames(s.ctx, s.out, s.out_cap, off.data(), &total)
                            : flacgpu_frame_offsets(s.ctx, off.data(), &total);
        if (rc) break;
        rc = retire(s, batches[b], off);
    }
    if (rc && !whole_rc) whole_rc = device_gpu_error(rc);
    for (size_t k = 0; k < have; k++) {
        (void)flacgpu_wait(slot[k].ctx);   // (a batch submitted before a failure: nothing of this call may be in flight)
        pooled_context_give(g, bps, ch, ctx_frames, device, slot[k]);
    }
    return whole_rc;
}

}  // namespace flacenc_host
