// plan_check.h -- what the frame assembly kernels assume of a plan and never test, checked on the host.
//
// The packers (k_frame64, k_sub64, k_emit + k_pack + k_crc) are written for the decisions the analysis makes: field values in
// range, partitions that tile the block, a frame no longer than the LDS image its launch gets (kernels/shape.h
// frame_fb_words: a bound on what the ENCODER can decide).  flacgpu_pack_plans takes a caller's decisions instead, and a
// plan outside those assumptions would make a kernel index past its plan arrays or write past its image.  check_plans()
// looks at the plan arrays while they are still on the host and names the first field a kernel could not hold; nothing is
// copied or launched for such a batch.  Whether the residuals are consistent with the PCM stays the caller's contract.
// Plain C++: no HIP, no context; the shape comes in as plan_route() takes it (tests/test_plan_check_host.py walks it on
// the CPU through flacenc_check_plans_row).
#ifndef FLACENC_HOST_PLAN_CHECK_H
#define FLACENC_HOST_PLAN_CHECK_H
#include <stdint.h>

#include "batch_route.h"
#include "flacenc_gpu.h"

namespace flacenc_route {

struct PlanFault {
    bool bad = false;
    uint32_t frame = 0, subframe = 0;   // subframe == channels: a field of the frame's own record
    const char *field = "";
};

// The first offending (frame, subframe, field) of a batch of n_frames plans (the last frame of last_len samples) whose
// frames [0, r.fast_pack) go to a wave assembly kernel and the rest to the generic packer, or none.  out_cap: bytes of
// the buffer the frames are assembled into.
PlanFault check_plans(const RouteContext &c, const Route &r, uint32_t n_frames, uint32_t last_len, uint64_t out_cap,
                      const flacgpu_frame_plan *plans, const flacgpu_subframe_plan *subs);

}  // namespace flacenc_route
#endif
