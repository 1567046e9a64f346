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

// ---- the streams' SHORT LAST BLOCKS (device_batch.cpp, DESIGN.md 4c "Short last blocks as one batch") ----
struct TailFrame {
    const int32_t *pcm;   // device address of the block's first sample (interleaved int32)
    uint32_t samples;     // per channel, 1 .. block_size - 1 (the device stream writer's frames: up to block_size)
    uint64_t number;      // the frame number: the stream's whole blocks
};
// FLACGPU_NO_RAGGED (read_knobs(), read once per process): the tails one by one, a one-frame flacgpu_encode_device call each
// on two one-frame contexts in rotation -- the loop every call ran before ragged batches; kept for A/B and as the tests'
// reference
bool tails_one_by_one();
// flacenc_device_tail_stats: the calling thread's last front-end call
void tail_stats_reset();
void tail_stats_add(uint64_t frames, uint64_t batches);
// frames a tail context holds: a power of two (calls with about as many tails then find the same pooled context), the
// smallest one >= 16 that holds the tails, but never above what a whole-block batch's context may hold (16 Mi samples, 64 ..
// 8192 frames): more tails than that are several batches
inline uint32_t tail_ctx_frames(size_t n_tails, size_t samples_per_block) {
    const uint64_t cap = std::min<uint64_t>(8192, std::max<uint64_t>(64, (16u << 20) / std::max<size_t>(samples_per_block, 1)));
    uint32_t f = 16;
    while (f < n_tails && 2ull * f <= cap) f *= 2;
    return f;
}

// The tails as RAGGED batches (flacgpu_encode_ragged_device) of up to a pooled context's frames, two contexts in rotation
// when one batch does not hold them all: batch b + 1 is submitted before batch b is retired, as for the whole blocks.
//   one_by_one       the caller's choice of the one-frame loop instead (a one-frame flacgpu_encode_device call per tail on
//                    two one-frame contexts in rotation); FLACGPU_NO_RAGGED=1 forces it for every caller
//   count_stats      the batches count into flacenc_device_tail_stats (the one-shot calls and a session's finalize); a
//                    caller whose frames are no stream's short last block (device_stream_writer.cpp) leaves the stats alone
//   retire(slot, t0, count, off)   tails [t0, t0 + count) are complete in `slot` (frames_to_host: their frames lie in
//                    slot.out; else only the offsets were fetched): off[k] .. off[k + 1] is tail t0 + k; returns a FLACGPU
//                    code
// Returns 0 or the FLACENC code of the first GPU failure (the text in flacenc_last_error); nothing of the call is in flight
// when it returns.
template <class Retire>
int encode_tail_blocks(const flacgpu_options &g, uint32_t bps, uint32_t ch, int device, uint32_t sample_rate,
                       const std::vector<TailFrame> &tails, bool frames_to_host, bool one_by_one, bool count_stats,
                       Retire retire) {
    if (tails.empty()) return 0;
    const bool single = one_by_one || tails_one_by_one();
    const uint32_t ctx_frames = single ? 1u : tail_ctx_frames(tails.size(), (size_t)g.block_size * ch);
    const size_t n_batches = (tails.size() + ctx_frames - 1) / ctx_frames;
    PooledContext slot[2] = {};
    const size_t n_slots = std::min<size_t>(2, n_batches);
    size_t have = 0;
    int rc = 0;
    for (; have < n_slots && !rc; have++) rc = pooled_context_take(g, bps, ch, ctx_frames, device, &slot[have]);
    if (rc) have--;
    std::vector<flacgpu_ragged_frame> rf;
    const auto count_of = [&](size_t b) { return std::min<size_t>(ctx_frames, tails.size() - b * ctx_frames); };
    const auto submit = [&](size_t b) {
        const size_t t0 = b * ctx_frames;
        if (single)
            return flacgpu_encode_device(slot[b % 2].ctx, tails[t0].pcm, FLACGPU_LAYOUT_INTERLEAVED, 1, tails[t0].samples,
                                         tails[t0].number, sample_rate, nullptr);
        rf.assign(count_of(b), flacgpu_ragged_frame{});
        for (size_t k = 0; k < rf.size(); k++) rf[k] = flacgpu_ragged_frame{tails[t0 + k].pcm, tails[t0 + k].samples, 0u, tails[t0 + k].number};
        return flacgpu_encode_ragged_device(slot[b % 2].ctx, rf.data(), (uint32_t)rf.size(), sample_rate, nullptr);
    };
    std::vector<uint64_t> off;
    if (!rc) rc = submit(0);
    for (size_t b = 0; b < n_batches && !rc; b++) {
        if (b + 1 < n_batches) rc = submit(b + 1);
        if (rc) break;
        const PooledContext &s = slot[b % 2];
        off.assign(count_of(b) + 1, 0);
        uint64_t total = 0;
        rc = frames_to_host ? flacgpu_fetch_frames(s.ctx, s.out, s.out_cap, off.data(), &total)
                            : flacgpu_frame_offsets(s.ctx, off.data(), &total);
        if (rc) break;
        if (count_stats) tail_stats_add(count_of(b), 1);
        rc = retire(s, b * ctx_frames, count_of(b), off);
    }
    const int tail_rc = rc ? device_gpu_error(rc) : 0;
    for (size_t k = 0; k < have; k++) {
        (void)flacgpu_wait(slot[k].ctx);
        pooled_context_give(g, bps, ch, ctx_frames, device, slot[k]);
    }
    return tail_rc;
}

}  // namespace flacenc_host
