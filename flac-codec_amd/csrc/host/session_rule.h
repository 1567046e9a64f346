// session_rule.h -- the rule of a decoder session (DESIGN.md 4b "Decoder sessions"): raw frame streams fed chunk by
// chunk, as plain host code.  Plain C++: no HIP call, no global state; every byte read is bounded by the length given.
// flacgpu_session_host_* (session_rule.cpp) is this rule over host chunks; the device session (decode_many.hip) finds
// the links on the device and shares the counts below.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "flac_stream.h"
#include "flacenc_gpu.h"

namespace flacenc {
constexpr uint32_t kSessionHead = 16;              // a position is judged once this many bytes follow it
constexpr uint32_t kSessionMinW = 16, kSessionMaxW = 1u << 22;   // the bounds of max_frame_bytes

// One stream's cumulative counts.  A gap is a maximal run of bytes in no kept frame over the whole byte string: a run
// that goes on from the feed before is not counted again.
struct SessionCount {
    uint64_t skipped = 0;
    uint32_t frames = 0, gaps = 0;
    bool in_gap = false;   // the last decided byte lies in no kept frame
    void skip(uint64_t n) {
        if (!n) return;
        skipped += n;
        if (!in_gap) gaps++;
        in_gap = true;
    }
    void keep() {
        frames++;
        in_gap = false;
    }
};

// One feed of one stream: d[0, L) is the held tail followed by the new chunk, `base` the offset of d[0] from the
// stream's first byte.  The frames decided now are appended to `out` (stream `stream`, out_offset from *elements on,
// which is moved on); `count` is updated for every byte in front of the hold position, which is returned: d[h, L) is
// held.  final: the stream is flushed, h == L.
size_t session_decide(const uint8_t *d, size_t L, bool final, uint32_t W, uint64_t base, uint32_t stream,
                      SessionCount &count, std::vector<flacgpu_frame_record> &out, uint64_t *elements);
}  // namespace flacenc
