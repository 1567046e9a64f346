// shape.h -- the constants and size formulas that both the kernels and the plain C++ host code (host/batch_route.cpp,
// built without HIP) decide by.  Included by kernels/types.h; compiles with and without hipcc.
#ifndef FLACGPU_KERNEL_SHAPE_H
#define FLACGPU_KERNEL_SHAPE_H
#include <stdint.h>

#ifdef __HIPCC__
#define FLACGPU_HD __host__ __device__
#else
#define FLACGPU_HD
#endif

constexpr int MAXP = 6;          // max effective partition order (64 partitions, encode.rs:3756)
constexpr uint32_t FN = 4096;    // the block length of every preset but `fast`

// largest block the generic kernels keep whole in LDS (k_fixed / k_fir: two arrays of it); larger
// blocks (up to 65535, encode.rs:1418-1423) use per-workgroup arrays in HBM instead
constexpr uint32_t LDS_BLOCK_LIMIT = 16384;

// words of LDS a whole frame of 4096-sample subframes may need (VERBATIM everywhere + header +
// CRC-16 + one guard word for the funnel shifts); multiple of 4 words
FLACGPU_HD constexpr uint32_t frame_fb_words(uint32_t channels, uint32_t bps, uint32_t n = FN) {
    return (((16u + 2u) * 8u + channels * (n * (bps + 1u) + 64u) + 31u) / 32u + 2u + 3u) & ~3u;
}

// Stereo frames whose channel assignment is chosen EXHAUSTIVELY (first minimum of the candidate pairs' bit counts,
// encode.rs:2747-2786): the chosen pair is never larger than L + R, and a chosen subframe never larger than its
// VERBATIM form, so the frame body is bounded by two bps-bit VERBATIM subframes -- not by the bps + 1 bits of a side
// channel.  For 24-bit stereo that is 24.6 KB instead of 25.6 KB of LDS per k_frame64 workgroup: six workgroups per
// CU instead of five.  (The fast channel choice picks its pair before any bit count exists: frame_fb_words.)
FLACGPU_HD constexpr uint32_t frame_fb_words_exhaustive_stereo(uint32_t bps, uint32_t n = FN) {
    return (((16u + 2u) * 8u + 2u * (n * bps + 64u) + 31u) / 32u + 2u + 3u) & ~3u;
}

// k_autocorr4 / k_autocorr4_deep (kernels/autocorr.inc): how far ahead of its conversion a 32-sample tile of input is
// requested, in tiles, and the ONE rule of which tile a request reads and which of the AC4_FETCH_DEPTH rotating
// staging register sets receives it.  The producers' schedule: before the tile loop they request tile 0, convert it and
// request tiles 1 .. DEPTH; in tile t they convert tile t + 1 out of its set and then request tile
// ac4_fetch_next(t) = t + 1 + DEPTH into the set that conversion has just freed -- the same set, because the set of a
// tile is its index modulo DEPTH.  A request past the frame's end reads the LAST tile again (the clamp keeps every
// address inside the frame; what such a request brings is converted into a buffer nobody reads, or not at all).
// DEPTH 1 is the schedule this kernel had before the second set (profiles/ac4_fetch_depth.json).
#ifndef AC4_FETCH_DEPTH
#define AC4_FETCH_DEPTH 2
#endif
struct Ac4FetchSlot {
    uint32_t tile;   // the tile whose samples the request reads: t, clamped to the frame
    uint32_t set;    // the staging set its loads go to and its conversion reads
};
FLACGPU_HD constexpr Ac4FetchSlot ac4_fetch_slot(uint32_t t, uint32_t ntiles, uint32_t depth = AC4_FETCH_DEPTH) {
    return Ac4FetchSlot{t < ntiles ? t : ntiles - 1u, t % depth};
}
FLACGPU_HD constexpr uint32_t ac4_fetch_next(uint32_t t, uint32_t depth = AC4_FETCH_DEPTH) { return t + 1u + depth; }

// block lengths the wave kernels are instantiated for: 64 lanes x SPL samples
#define FLACGPU_WAVE_SIZES(X) X(4096, 64) X(2304, 36) X(2048, 32) X(1152, 18) X(1024, 16)
inline bool wave_block_size(uint32_t B) {
    switch (B) {
#define X(n, spl) case n:
        FLACGPU_WAVE_SIZES(X)
#undef X
        return true;
    default: return false;
    }
}

// Every FLACGPU_* environment knob, resolved ONCE per context (flacgpu_create; flacenc_gpu.hip read_knobs) -- the
// dispatch path never calls getenv.  The A/B selectors keep an older or generic kernel reachable for measurements
// and parity tests; the TEST knobs (tie_band, tie_perturb, experiment_mfma_ac, fir_suspect_bits) are honoured only
// when FLACGPU_TEST_KNOBS=1 is set as well.  Every one of them is exercised by a test, a tool or a bench leg
// ("Environment selectors"; tests/test_knob_inventory.py keeps that list honest).
struct Knobs {
    bool no_direct = false, no_w64 = false, no_fused_pack = false, no_frame64 = false,
         early_download = false,   // the frames' D2H copy queued before the sizes are known (FLACGPU_EARLY_DOWNLOAD)
         no_hand = false,          // A/B: Params::hand_meta off (FLACGPU_NO_HAND)
         no_direct_short = false,  // A/B: 1024 / 1152 / 2048 / 2304-sample blocks through K0 + k_cand64 (FLACGPU_NO_DIRECT_SHORT)
         no_ac_fma = false,        // A/B: every autocorrelation term a multiply and an add (FLACGPU_NO_AC_FMA)
         no_xpose = false,         // A/B: 4 / 8 interleaved channels split into planar rows by k_autocorr4 instead of read in place (FLACGPU_NO_XPOSE)
         no_cand_pair = false,     // A/B: four waves per frame also for the fast channel choice without LPC (FLACGPU_NO_CAND_PAIR)
         no_ragged = false;        // A/B: the device front ends' short last blocks one one-frame call each, not as ragged batches (FLACGPU_NO_RAGGED)
    bool force_fir_check = false;       // A/B + TEST: every candidate takes the exact ResidualOverflow test first (FLACGPU_FIR_CHECK)
    uint32_t cand_grid = 0;             // resident workgroups of the persistent candidate kernels, 0: default
    bool experiment_mfma_ac = false;    // TEST: the re-associating MFMA autocorrelation (not bit-exact)
    bool has_tie_band = false, has_tie_perturb = false;
    double tie_band = 0.0, tie_perturb = 0.0;   // TEST
    uint32_t fir_suspect_bits = 0;      // TEST: Params::fir_suspect_bits, 0: default (30)
    int defer_fixed = -1;               // FLACGPU_DEFER_FIXED: 0 / 1 / 2 / 3 (Params::defer_fixed); -1: default (1)
    int defer_margin16 = -1;            // FLACGPU_DEFER_MARGIN16: Params::defer_margin16; -1: default
};
#endif
