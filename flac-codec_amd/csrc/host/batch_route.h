// batch_route.h -- which kernels a batch of the encoder runs, decided ONCE, by a pure function.
//
// flacenc_gpu.hip asks plan_route() when a batch arrives and every later stage (analysis, host re-decision, frame assembly,
// range cutting, the segment entries) reads the answer.  A new path is added HERE: a value of Route::Input or a field of
// Route, its conditions in plan_route(), and a row in tests/test_route_table.py's properties.  No HIP, no context, no
// pointers, no getenv: tests/test_route_table.py walks it on the CPU.
#ifndef FLACENC_HOST_BATCH_ROUTE_H
#define FLACENC_HOST_BATCH_ROUTE_H
#include <stdint.h>

#include "../kernels/shape.h"

namespace flacenc_route {

// fixed when the context is created or tuned
struct RouteContext {
    uint32_t channels = 0, bps = 0, block_size = 0, max_lpc_order = 0, max_partition_order = 0;
    bool exhaustive = false;
    uint32_t stereo4 = 0, ncand = 0;   // the four L/R/M/S candidates of a stereo stream below 32 bits; candidate slots per frame
    bool has_hand = false;             // the context owns Params::hand_meta's flags
    bool has_edges = false;            // ... and k_sub64's edge records
    Knobs knobs;
    int lag_split = 4;                 // FLACGPU_TUNE_LAG_SPLIT
    bool two_ranges = false;           // FLACGPU_TUNE_TWO_RANGES
    uint32_t chunk_samples = 64u << 20;   // FLACGPU_TUNE_CHUNK_MSAMPLES (0: never cut)
    bool chunk_auto = true;               // nobody set the tuning: only stereo batches are cut
    bool timing = false;               // per-kernel timing: everything on one stream, nothing cut
};
// RouteContext::chunk_samples of a FLACGPU_TUNE_CHUNK_MSAMPLES value
inline uint32_t chunk_samples_of(int msamples) { return msamples <= 0 ? 0u : (uint32_t)(msamples < 2047 ? msamples : 2047) << 20; }
// what flacgpu_create derives from the stream's shape and the knobs (the tunings at their defaults)
RouteContext route_context(uint32_t channels, uint32_t bps, uint32_t block_size, uint32_t max_lpc_order,
                           uint32_t max_partition_order, bool exhaustive, const Knobs &knobs);

// per call
struct RouteBatch {
    uint32_t n_frames = 0, last_len = 0;
    int layout = 0;                  // FLACGPU_LAYOUT_INTERLEAVED (0) / FLACGPU_LAYOUT_PLANAR (1)
    bool aligned16 = false;          // the PCM (every segment's) starts on a 16-byte boundary
    uint32_t packed_bytes = 0;       // != 0: stream-width little-endian samples in the context's input buffer
    bool segments_in_place_wanted = false;   // a batch of device segments that would rather not be gathered
    bool whole_call = false;         // flacgpu_encode_device: analysis and assembly in one call, so the batch may be cut
    bool ragged = false;             // every frame has a length of its own (flacgpu_encode_ragged_device; last_len: the last frame's)
};

struct Route {
    enum Input {
        K0_COPY,           // k_deinterleave* writes the planar rows
        K0_PACKED,         // k_deinterleave_packed widens them on the way
        PLANAR_IN_PLACE,   // the caller's planar rows are Params::planar
        DIRECT_STEREO,     // Params::inter: interleaved stereo read in place by every stage
        SPLIT,             // Params::split_src: k_autocorr4's producers write the rows (one channel: nothing to write)
        SPLIT_XPOSE        // ... and nobody does: the candidate and subframe kernels read the interleaved batch too
    } input = K0_COPY;
    bool hand = false;               // Params::hand_meta set
    uint32_t fast_analysis = 0;      // frames [0, n) on k_cand64*, the rest on the generic kernels
    uint32_t fast_pack = 0;          // frames [0, n) on k_frame64 / k_sub64, the rest on k_emit + k_pack + k_crc
    bool k4_in_autocorr = false;     // what dispatch_autocorr returns for the whole blocks (no k_lpc_u launch for them)
    uint32_t range_frames = 0;       // flacgpu_encode_device cuts the batch into ranges of this many frames (0: no)
    bool two_ranges = false;         // the two-stream branch of flacgpu_encode_device
    bool host_out_possible = false;  // every frame assembled by stores only: the frames may go straight to pinned host memory
    bool segments_in_place = false;  // the wish of RouteBatch was granted (otherwise the segments are gathered first)

    bool in_place() const { return input == DIRECT_STEREO || input == SPLIT || input == SPLIT_XPOSE; }
};

Route plan_route(const RouteContext &c, const RouteBatch &b);

}  // namespace flacenc_route
#endif
