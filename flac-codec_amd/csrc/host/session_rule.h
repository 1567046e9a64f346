// session_rule.h -- the rule of a decoder session (DESIGN.md 4b "Decoder sessions"): raw frame streams fed chunk by
// chunk, as plain host code.  Plain C++: no HIP call, no global state; every byte read is bounded by the length given.
// flacgpu_session_host_* (session_rule.cpp) is this rule over host chunks; the device session (decode_many.hip) finds
// the links on the device and runs the same walk with the same counts (raw_walk.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "flac_stream.h"
#include "flacenc_gpu.h"
#include "raw_walk.h"

namespace flacenc {
constexpr uint32_t kSessionMinW = 16, kSessionMaxW = 1u << 22;   // the bounds of max_frame_bytes

// One feed of one stream: d[0, L) is the held tail followed by the new chunk, `base` the offset of d[0] from the
// stream's first byte.  The frames decided now are appended to `out` (stream `stream`, out_offset from *elements on,
// which is moved on); `count` is updated for every byte in front of the hold position, which is returned: d[h, L) is
// held.  final: the stream is flushed, h == L.
size_t session_decide(const uint8_t *d, size_t L, bool final, uint32_t W, uint64_t base, uint32_t stream,
                      SessionCount &count, std::vector<flacgpu_frame_record> &out, uint64_t *elements);

// The same for a stream of a container session in its frame phase (DESIGN.md 4b "Container sessions": the regular end
// rule with STREAMINFO's `info` and `min_frame`, bounded by W): d[0] is the cursor.  Returns the walk: d[cursor, L) is
// held, or (lost) dropped.  A record's sample rate and sample size are STREAMINFO's where its header defers to it.
RegularWalk container_decide(const uint8_t *d, size_t L, bool final, uint32_t W, const flacgpu_stream_info &info,
                             uint32_t min_frame, uint64_t base, uint32_t stream, std::vector<flacgpu_frame_record> &out,
                             uint64_t *elements);
}  // namespace flacenc
