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
// words of the LDS image a wave assembly launch of this context gets (plan_route sizes by it, pack_impl launches with it):
// whatever the channel choice, or the smaller image of the exhaustive stereo choice
inline uint32_t frame_image_words(const RouteContext &c) {
    const uint32_t any = frame_fb_words(c.channels, c.bps, c.block_size);
    const uint32_t ex = frame_fb_words_exhaustive_stereo(c.bps, c.block_size);
    return (c.stereo4 && c.exhaustive && ex < any) ? ex : any;
}
// the context and the batch of one row of the test hooks (flacenc_plan_route_row's in[18])
void route_row(const int32_t *in, RouteContext &c, RouteBatch &b);

// ---- which autocorrelation kernel ONE launch runs (autocorr.hip switches on the answer and on nothing else; a test that
// names an instantiation asks the same function through flacenc_plan_autocorr_row).  The inputs are what the launchers read
// from Params, the knobs and their arguments.
struct AcLaunch {
    uint32_t ncand = 0, stereo4 = 0, channels = 0, bps = 0, max_lpc_order = 0;
    uint32_t n = 0, block_size = 0;     // the launch's frame length; the context's block size
    bool inter = false;                 // Params::inter set (Route::DIRECT_STEREO)
    bool split_src = false;             // Params::split_src set (Route::SPLIT / SPLIT_XPOSE)
    uint32_t ac_split = 4;              // Params::ac_split (FLACGPU_TUNE_LAG_SPLIT)
    uint32_t nframes = 0;               // frames in the launch
    bool whole_batch = false;           // the launch covers the batch: frame0 == 0 && nframes == Params::n_frames
    bool mfma = false;                  // Knobs::experiment_mfma_ac
    uint32_t fma_t0 = 0, fma_t1 = 0;    // Params::fma_t0 / fma_t1 (fused_tile_range)
    bool ragged = false;                // launch_autocorr_ragged: every frame its own length
};
struct AcKernel {
    enum Family { AC4, AC4_DEEP, AC2, RAGGED, MFMA } family = AC2;
    uint32_t size = 0;                  // AC4: NL (5, 9, 13, 17); AC2 / RAGGED: H (4 .. 36); AC4_DEEP: 33; MFMA: 17
    uint32_t ns = 4;                    // lag-group waves per 64 candidates (MFMA: one wave per candidate, 0)
    enum Producer { PLANAR, DIRECT, SPLIT, SPLIT4, SPLIT8 } producer = PLANAR;
    bool stereo = false;                // the STEREO template argument of k_autocorr4 / _deep
    bool fused_k4 = false;              // K4 in the kernel's tail: what dispatch_autocorr returns
    bool fused_tiles = false;           // tiles [fma_t0, fma_t1) take one v_fma_f64 per term in this launch
};
AcKernel plan_autocorr(const AcLaunch &a);
// Params::fma_t0 / fma_t1 of a context: the 32-sample tiles of a FULL block whose every product has both factors under window
// values of exactly 1.0 ([flat_lo, flat_hi): the flat run of the block's window); t0 >= t1: none
void fused_tile_range(uint32_t bps, uint32_t stereo4, uint32_t max_lpc_order, uint32_t flat_lo, uint32_t flat_hi, bool no_ac_fma,
                      uint32_t *t0, uint32_t *t1);

}  // namespace flacenc_route
#endif
