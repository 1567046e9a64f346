// container_rule.h -- one stream of a container session (DESIGN.md 4b "Container sessions"): metadata, then frames in a
// chain (regular_walk, raw_walk.h), or refused, or lost for good -- stated once for the host session
// (container_host_step, session_rule.cpp), which the CPU tests hold against a Python model, and the device session
// (container_step, decode_many.hip).  Each caller handles its own bytes and runs its own walk; the phases, the counts
// and the summary are these.  Header only, plain C++: no HIP call, no global state.
#pragma once
#include "../kernels/meta_feed_rule.h"
#include "raw_walk.h"

namespace flacenc {
enum : uint32_t { CS_META = 0, CS_FRAMES = 1, CS_LOST = 2, CS_REFUSED = 3 };

struct ContainerStream {
    MetaFeed meta{};             // the metadata walk so far (CS_META)
    uint32_t phase = CS_META;
    uint64_t fed = 0;            // bytes fed to this stream
    flacgpu_stream_info info{};  // metadata_of_record's: STREAMINFO from CS_FRAMES on, what a refused stream reports
    uint32_t min_frame = 0;
    uint64_t frames = 0, samples = 0, skipped = 0;   // cumulative: frames decided, their samples per channel, bytes dropped
};

// A feed of `fed_now` bytes begins (finish: none, the input ends); `meta` is the metadata walk behind those bytes.  The
// metadata phase ends when the walk is through or refused, or with the input.  True: the stream entered its frame phase
// now, and *frames_at is the frame region's offset from the stream's first byte.  A lost stream's new bytes are
// skipped; a refused stream has skipped all it was fed.
static inline bool container_begin(ContainerStream &k, const MetaFeed &meta, uint64_t fed_now, bool finish,
                                   uint64_t *frames_at) {
    bool entered = false;
    k.fed += fed_now;
    if (k.phase == CS_META) {
        k.meta = meta;
        if (meta.phase == MF_DONE || meta.phase == MF_REFUSED || finish) {
            MetaRecord rec;
            meta_feed_record(meta, meta.phase == MF_DONE ? meta.taken : k.fed, rec);
            size_t at = 0;
            entered = !metadata_of_record(rec, &k.info, &k.min_frame, &at);
            k.phase = entered ? CS_FRAMES : CS_REFUSED;
            if (entered) *frames_at = at;
        }
    } else if (k.phase == CS_LOST) {
        k.skipped += fed_now;
    }
    if (k.phase == CS_REFUSED) k.skipped = k.fed;
    return entered;
}

// The feed's walk `w` over the stream's segment, which ends at `end`, kept `frames` frames of `samples` samples per
// channel.  Returns how many bytes are held, from w.cursor on: none of a lost stream, whose bytes from the cursor on
// are skipped (the first it skips: until then every byte was metadata, a kept frame's, or held).
static inline uint64_t container_end(ContainerStream &k, const RegularWalk &w, uint64_t end, uint64_t frames,
                                     uint64_t samples) {
    k.frames += frames;
    k.samples += samples;
    if (!w.lost) return end - w.cursor;
    k.phase = CS_LOST;
    k.skipped += end - w.cursor;
    return 0;
}

// The stream's summary behind a feed whose frames begin at `first_frame` of the feed's table
static inline flacgpu_raw_stream container_summary(const ContainerStream &k, size_t first_frame) {
    flacgpu_raw_stream sum{};
    sum.first_frame = first_frame;
    sum.frames = (uint32_t)k.frames;
    sum.skipped_bytes = k.skipped;
    sum.gaps = k.skipped ? 1 : 0;
    sum.uniform = k.phase == CS_FRAMES || k.phase == CS_LOST;
    return sum;
}
}  // namespace flacenc
