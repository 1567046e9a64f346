// batch_route.cpp -- plan_route(): see batch_route.h.  Plain C++ (no HIP headers).
#include "batch_route.h"

#include <stddef.h>

namespace flacenc_route {

RouteContext route_context(uint32_t channels, uint32_t bps, uint32_t block_size, uint32_t max_lpc_order,
                           uint32_t max_partition_order, bool exhaustive, const Knobs &knobs) {
    RouteContext c;
    c.channels = channels;
    c.bps = bps;
    c.block_size = block_size;
    c.max_lpc_order = max_lpc_order;
    c.max_partition_order = max_partition_order;
    c.exhaustive = exhaustive;
    c.stereo4 = (channels == 2 && bps < 32) ? 1u : 0u;  // side needs bps+1 <= 32 (encode.rs:2715)
    c.ncand = c.stereo4 ? 4u : channels;
    // the residual handed from k_cand64p to k_frame64: stereo contexts of 4096-sample blocks with LPC
    c.has_hand = c.stereo4 && block_size == FN && max_lpc_order > 0 && !knobs.no_hand;
    c.has_edges = channels >= 5;   // k_sub64 assembles the frames of 5..8 channels
    c.knobs = knobs;
    return c;
}

namespace {
constexpr int kInterleaved = 0, kPlanar = 1;   // FLACGPU_LAYOUT_*
constexpr size_t kFrameLdsBytes = 150 * 1024;  // what a frame kernel's workgroup may ask of the CU's 160 KiB
bool fits_lds(uint32_t fb_words) { return (size_t)fb_words * sizeof(int32_t) <= kFrameLdsBytes; }
}  // namespace

Route plan_route(const RouteContext &c, const RouteBatch &b) {
    Route r;
    // a ragged batch: every frame on the generic kernels (analysis and assembly), its samples gathered into the context's
    // input buffer and split by K0 -- nothing read in place, nothing cut, no host output
    if (b.ragged) return r;
    const Knobs &kn = c.knobs;
    const uint32_t B = c.block_size, C_ = c.channels, n_frames = b.n_frames;
    const bool whole_blocks = b.last_len == B;
    const uint32_t full = whole_blocks ? n_frames : n_frames - 1;
    const bool narrow = c.bps + (c.stereo4 ? 1u : 0u) <= 25u;   // candidates of <= 25 bits: the wave kernels' FIR
    const bool po_ok = c.max_partition_order <= (uint32_t)MAXP;
    const uint32_t fbw_any = frame_fb_words(C_, c.bps, B);      // a frame's LDS image whatever the channel choice

    // ---- the candidate stage: the wave-per-candidate kernel (FIXED + LPC analysis of a candidate in one wave, after the
    // LPC parameters are known) for whole blocks of 64 x {16, 18, 32, 36, 64} samples, LPC order <= 16 (4096: <= 32);
    // anything else (other block sizes, a short last frame, wider candidates) the generic LDS kernels
    const bool w64 = narrow && wave_block_size(B) && (c.max_lpc_order <= 16 || B == FN) && po_ok && !kn.no_w64;
    r.fast_analysis = w64 ? full : 0;

    // ---- frame assembly: frames of a wave block length are assembled whole in LDS by k_frame64 / k_sub64 (residuals
    // recomputed from the PCM, CRC-16 from LDS, one write of the finished bytes) -- orders 17..32 and 5..8 channels for
    // 4096-sample blocks only (and not both); any other frame goes through k_emit (residual rows) -> k_pack (one workgroup
    // per subframe, zero-filled output, atomic OR at shared words) -> k_crc
    const uint32_t fbw = frame_image_words(c);   // (the exhaustive stereo choice gets the smaller image)
    const bool f64w = narrow && wave_block_size(B) && (c.max_lpc_order <= 16 || (B == FN && C_ <= 4)) && (C_ <= 4 || B == FN) &&
                      po_ok && fits_lds(fbw) && !kn.no_fused_pack && !kn.no_frame64;
    r.fast_pack = f64w ? full : 0;
    // host output: k_frame64 only ever stores (dwords inside a frame, bytes at its ends), so it can write over PCIe into
    // pinned memory; the generic packer builds its frames with atomic ORs and cannot
    r.host_out_possible = r.fast_pack != 0 && r.fast_pack == n_frames;
    const bool all_fast = whole_blocks && w64 && f64w;   // every frame on the wave kernels, analysis and assembly

    // ---- the input.  The in-place kernels fetch 16-byte pieces (vector loads, LDS-DMA): a batch that does not start on a
    // 16-byte boundary (a view into a larger device buffer) takes a copying K0 path, whose loads are dwords.  They read whole
    // blocks of int32 samples with the 4-way lag split, and none of the knobs that select an older kernel is set.
    const bool in_place_ok = !b.packed_bytes && b.aligned16 && whole_blocks && po_ok && c.lag_split != 2 &&
                             !(kn.no_direct || kn.no_w64 || kn.experiment_mfma_ac);
    // DIRECT: interleaved stereo with the four L/R/M/S candidates of <= 24-bit samples, read in place by the
    // autocorrelation, candidate and frame kernels -- 4096-sample blocks; 1024 / 1152 / 2048 / 2304 with LPC order <= 16
    // (the persistent candidate kernel stages the interleaved frame once per frame in LDS; the non-persistent one read it
    // once per candidate wave and lost to the split pass, 0.114 -> 0.172 ms at 1152 samples).  Every stage must be on its
    // wave kernel: the generic ones read Params::planar.
    const bool direct = in_place_ok && b.layout == kInterleaved && c.stereo4 && C_ == 2 && c.bps <= 24 &&
                        (B == FN || (wave_block_size(B) && c.max_lpc_order <= 16 && !kn.no_direct_short)) &&
                        !kn.no_fused_pack && !kn.no_frame64 && fits_lds(fbw_any);
    // planar rows (one channel: interleaved and planar are the same bytes) are Params::planar as they lie
    const bool planar_rows = !b.packed_bytes && b.aligned16 && (b.layout == kPlanar || C_ == 1) && (B % 4 == 0) && whole_blocks &&
                             !kn.no_direct;
    // SPLIT: independent channels, interleaved, 4096-sample blocks with LPC of order <= 16: k_autocorr4's producers split the
    // batch into the planar rows while they read it -- the K0 pass (8 B per sample at the HBM roofline) disappears.  Needs
    // every frame on the wave-per-candidate kernel (no generic-path frame reads the rows before the autocorrelation has
    // written them).  (One channel: the input is its own planar row -- nothing to split, but the ORs still come out of
    // the autocorrelation instead of a k_orbits pass over the batch.)
    const bool split = in_place_ok && !c.stereo4 && c.ncand == C_ && c.max_lpc_order >= 1 && c.max_lpc_order <= 16 && B == FN &&
                       c.bps <= 25u && (C_ == 1 ? planar_rows : b.layout == kInterleaved);
    // XPOSE: 3, 4, 6 or 8 channels: the candidate and subframe kernels read the interleaved batch in place as well
    // (load_lane_xpose: a workgroup fetches a whole frame -- or half of a 6- or 8-channel one -- together) -- the planar
    // rows, half of the autocorrelation kernel's HBM traffic, are not written at all, so every frame must be assembled by
    // k_frame64 (3, 4 channels) / k_sub64 (6, 8: it needs its edge records) too.  (Whole frames of 5 or 6 channels in one
    // workgroup: measured -- five or six 152-register waves do not pack onto the four SIMDs, the candidate and subframe
    // kernels lose more (0.09 -> 0.13-0.15, 0.15 -> 0.25-0.27 ms per 67 M samples) than the autocorrelation gains (0.21 ->
    // 0.14); 5 and 7 channels keep the rows.  >= 8-bit samples: the transposing buffer lies in the LDS image areas of the
    // frame kernels, sized by the sample width.)
    const bool xpose = split && all_fast && !kn.no_xpose && c.bps >= 8 &&
                       (C_ == 3 || C_ == 4 || ((C_ == 8 || C_ == 6) && c.has_edges));
    r.input = direct ? Route::DIRECT_STEREO
              : split ? (xpose ? Route::SPLIT_XPOSE : Route::SPLIT)
              : b.packed_bytes ? Route::K0_PACKED
              : planar_rows ? Route::PLANAR_IN_PLACE
                            : Route::K0_COPY;
    // the winners' LPC residuals handed from k_cand64p to k_frame64 (Params::hand_meta): 4096-sample direct stereo frames
    // with LPC -- the candidate kernel's instantiations that keep the frame's image through the turn
    r.hand = direct && B == FN && c.max_lpc_order > 0 && c.has_hand;
    // segments stay where they are when every stage finds its frames through the table (Params::inter_tab); one channel's
    // rows are Params::planar, which has no table
    r.segments_in_place = b.segments_in_place_wanted && r.in_place() && C_ >= 2;
    // K4 in the tail of the autocorrelation kernel: its in-place instantiations for up to 16 lags (plan_autocorr's
    // fused_k4 below; the deep kernel of orders 17..32 leaves K4 to k_lpc_u)
    r.k4_in_autocorr = r.in_place() && c.max_lpc_order >= 1 && c.max_lpc_order <= 16;

    // ---- flacgpu_encode_device (int32 samples: no entry point hands it a stream-width upload)
    if (!b.whole_call || b.packed_bytes || c.timing) return r;
    // FLACGPU_TUNE_TWO_RANGES: a batch whose every frame takes the wave kernels is cut in two, and the halves run the whole
    // chain -- K0 (or the caller's planar rows), the planar autocorrelation with k_lpc_u behind it, k_cand64, k_frame64 --
    // on two streams
    if (c.two_ranges && n_frames >= 256 && all_fast && fits_lds(fbw_any) && (b.layout == kInterleaved || b.layout == kPlanar)) {
        r.two_ranges = true;
        // (planar rows are read in place unless the caller asked for a copy: FLACGPU_TUNE_COPY_INPUT / FLACGPU_NO_DIRECT)
        r.input = (b.layout == kPlanar && planar_rows) ? Route::PLANAR_IN_PLACE : Route::K0_COPY;
        r.hand = r.k4_in_autocorr = r.segments_in_place = false;
        return r;
    }
    // A batch of more samples than the chip's last-level cache likes (256 MiB of Infinity Cache: the candidate and frame
    // kernels re-read what the autocorrelation just streamed) is run range by range -- the whole kernel chain for ~64 Mi
    // samples at a time, each range's frame offsets continuing from the one before (k_layout): a stereo batch of 16384
    // frames (134 M samples) runs 9 % faster as two ranges of 8192 (profiles/r04_chunk_ab.json; 8-channel batches of 8192
    // frames as four ranges: no difference, so independent channels are cut only when the tuning asks).  Only batches of
    // 4096-sample blocks whose every frame runs the in-place wave kernels with K4 inside the autocorrelation kernel are
    // cut, and stereo only with the exhaustive channel choice (the fast one sums the whole batch first).
    if (c.chunk_samples && B == FN && C_ >= 2 && r.in_place() && all_fast && r.k4_in_autocorr &&
        (c.stereo4 ? c.exhaustive : !c.chunk_auto)) {
        const uint32_t chunk = (uint32_t)(c.chunk_samples / ((uint64_t)B * C_)) & ~63u;   // whole candidate groups of the autocorrelation
        if (chunk >= 256 && n_frames >= chunk + chunk / 2) r.range_frames = chunk;        // (else nothing to cut, or ranges too small to fill the chip)
    }
    return r;
}

void fused_tile_range(uint32_t bps, uint32_t stereo4, uint32_t max_lpc_order, uint32_t flat_lo, uint32_t flat_hi, bool no_ac_fma,
                      uint32_t *t0, uint32_t *t1) {
    *t0 = *t1 = 0;
    // integer samples below 2^26 (candidates of <= 25 bits + the side channel's extra bit) have exact f64 products
    if (!no_ac_fma && bps + (stereo4 ? 1u : 0u) <= 26u && flat_hi > flat_lo) {
        // (the margin is the most lags a launch can carry -- its lag count is the order + 1 rounded up to four --, not the order)
        const uint32_t maxlag = max_lpc_order <= 16 ? 16u : 32u;
        *t0 = (flat_lo + maxlag + 31u) / 32u;      // first 32-sample tile whose every partner sample is flat too
        *t1 = flat_hi / 32u;                        // tiles t < t1 end inside the flat run
    }
}

AcKernel plan_autocorr(const AcLaunch &a) {
    AcKernel k;
    const uint32_t H = ((a.max_lpc_order + 1) + 3u) & ~3u;   // the generic kernels' lag count: order + 1 rounded up to four
    if (a.ragged) {
        k.family = AcKernel::RAGGED;
        k.size = H <= 36 ? H : 36;
        return k;
    }
    // EXPERIMENT switch (bench.py --experiment mfma_autocorr): the re-associating f64-MFMA kernel in place of the exact one, to
    // measure what a whole step costs with the autocorrelation off the VALU pipe.  NOT bit-exact; never set in production.
    if (a.mfma && a.max_lpc_order >= 1 && a.max_lpc_order <= 16 && a.whole_batch && a.n == a.block_size) {
        k.family = AcKernel::MFMA;
        k.size = 17;
        k.ns = 0;
        return k;
    }
    // k_autocorr4 / _deep: frame length a multiple of 32 (orders 17..32: two blocks of history, a multiple of 64), and either
    // stereo L/R/M/S candidates of <= 24-bit samples (mid/side formed with one v_mad_i32_i24) or independent channels of any width
    const bool stereo = a.stereo4 && a.ncand == 4 && a.channels == 2 && a.bps <= 24;
    const bool indep = !a.stereo4 && a.ncand == a.channels;
    const bool deep = a.max_lpc_order > 16;
    if (a.n < 32 || a.n % 32 != 0 || (!stereo && !indep) || (deep && a.n % 64 != 0)) {
        k.family = AcKernel::AC2;
        k.size = H <= 36 ? H : 36;
        return k;
    }
    // a short last frame has a window of its own: no fused tiles
    k.fused_tiles = a.n == a.block_size && a.fma_t0 < a.fma_t1;
    k.stereo = stereo;
    if (deep) {
        // (K4 in the tail of the deep kernel, as in k_autocorr4: measured and removed -- 228 instead of 153 VGPRs leave no room
        // for another kernel's wave beside two of these, and the four-context step of config 5 goes 0.566 -> 0.588 ms,
        // profiles/r04_autocorr_lpc_fuse.json)
        k.family = AcKernel::AC4_DEEP;
        k.size = 33;
        k.producer = (stereo && a.inter) ? AcKernel::DIRECT : AcKernel::PLANAR;
        return k;
    }
    k.family = AcKernel::AC4;
    const uint32_t nl = a.max_lpc_order + 1;
    k.size = nl <= 5 ? 5 : nl <= 9 ? 9 : nl <= 13 ? 13 : 17;
    const uint32_t groups = (a.nframes * a.ncand + 63) / 64;
    // 4 waves per 64 candidates (lags split 4 ways) by default: the f64 stream needs two waves per SIMD to issue at full rate and
    // 8192 frames are only 512 candidate groups (0.23 ms against 0.31 ms split 2 ways).  When other contexts keep the SIMDs busy
    // anyway, the 2-way split wins: the int -> f64 x window conversion is replicated 2x instead of 4x (71 M instead of 92 M
    // instructions).
    if (stereo && a.inter) {   // interleaved input read in place (the route selects this only with the 4-way split)
        // small batches (<= 1024 frames: at most 64 workgroups for 256 CUs) are a latency problem -- the serial walk over a
        // frame's samples -- and take the eight-wave split of the lags, whose walk is shorter (512 frames: 0.0555 -> 0.0441 ms
        // per batch in the four-context loop, profiles/r04_batch_sweep.json); large batches are a throughput problem and keep
        // four waves (the eight-wave kernel reads the tile twice as often)
        k.producer = AcKernel::DIRECT;
        k.ns = (groups <= 64 && k.size == 13) ? 8 : 4;
        k.fused_k4 = true;
    } else if (!stereo && a.split_src) {   // interleaved independent channels: the producers split them on the way (no K0 pass)
        k.producer = a.channels == 8 ? AcKernel::SPLIT8 : a.channels == 4 ? AcKernel::SPLIT4 : AcKernel::SPLIT;
        k.fused_k4 = true;
    } else {
        k.ns = a.ac_split == 2 ? 2 : 4;
    }
    return k;
}

}  // namespace flacenc_route

// Test hook (tests/test_autocorr_edge_matrix_oracle.py; not in the public header, needs no device): the kernel of one
// autocorrelation launch.  in[17]: ncand, stereo4, channels, bps, max LPC order, n, block size, inter set, split_src set,
// ac_split, frames in the launch, the launch covers the batch, experiment_mfma_ac, the window's flat run [flat_lo, flat_hi),
// no_ac_fma, ragged.  out[9]: AcKernel's fields in their order, then fma_t0 and fma_t1 as fused_tile_range gives them.
extern "C" void flacenc_plan_autocorr_row(const int32_t *in, uint32_t *out) {
    using namespace flacenc_route;
    AcLaunch a;
    a.ncand = (uint32_t)in[0];
    a.stereo4 = (uint32_t)in[1];
    a.channels = (uint32_t)in[2];
    a.bps = (uint32_t)in[3];
    a.max_lpc_order = (uint32_t)in[4];
    a.n = (uint32_t)in[5];
    a.block_size = (uint32_t)in[6];
    a.inter = in[7] != 0;
    a.split_src = in[8] != 0;
    a.ac_split = (uint32_t)in[9];
    a.nframes = (uint32_t)in[10];
    a.whole_batch = in[11] != 0;
    a.mfma = in[12] != 0;
    fused_tile_range(a.bps, a.stereo4, a.max_lpc_order, (uint32_t)in[13], (uint32_t)in[14], in[15] != 0, &a.fma_t0, &a.fma_t1);
    a.ragged = in[16] != 0;
    const AcKernel k = plan_autocorr(a);
    out[0] = (uint32_t)k.family;
    out[1] = k.size;
    out[2] = k.ns;
    out[3] = (uint32_t)k.producer;
    out[4] = k.stereo;
    out[5] = k.fused_k4;
    out[6] = k.fused_tiles;
    out[7] = a.fma_t0;
    out[8] = a.fma_t1;
}

// Test hook (tests/test_route_table.py, tools/route_table_check.cpp; not in the public header, needs no device): the route of
// one row of the test's matrix.  in[18]: channels, bps, block size, max LPC order, max partition order, exhaustive, layout,
// aligned16, last_len, n_frames, packed bytes, lag split, timing, segments-in-place wanted, knobs (bit 0 no_direct, 1 no_w64,
// 2 no_fused_pack, 3 no_frame64, 4 no_direct_short, 5 no_xpose, 6 no_hand, 7 experiment_mfma_ac), FLACGPU_TUNE_CHUNK_MSAMPLES
// (-1: never set), two_ranges, whole call.  out[9]: Route's fields in their order.
namespace flacenc_route {
void route_row(const int32_t *in, RouteContext &c, RouteBatch &b) {
    Knobs kn;
    const uint32_t bits = (uint32_t)in[14];
    kn.no_direct = bits & 1u;
    kn.no_w64 = bits & 2u;
    kn.no_fused_pack = bits & 4u;
    kn.no_frame64 = bits & 8u;
    kn.no_direct_short = bits & 16u;
    kn.no_xpose = bits & 32u;
    kn.no_hand = bits & 64u;
    kn.experiment_mfma_ac = bits & 128u;
    c = route_context((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], in[5] != 0, kn);
    c.lag_split = in[11];
    c.timing = in[12] != 0;
    if (in[15] >= 0) {
        c.chunk_samples = chunk_samples_of(in[15]);
        c.chunk_auto = false;
    }
    c.two_ranges = in[16] != 0;
    b.layout = in[6];
    b.aligned16 = in[7] != 0;
    b.last_len = (uint32_t)in[8];
    b.n_frames = (uint32_t)in[9];
    b.packed_bytes = (uint32_t)in[10];
    b.segments_in_place_wanted = in[13] != 0;
    b.whole_call = in[17] != 0;
}
}  // namespace flacenc_route
extern "C" void flacenc_plan_route_row(const int32_t *in, uint32_t *out) {
    using namespace flacenc_route;
    RouteContext c;
    RouteBatch b;
    route_row(in, c, b);
    const Route r = plan_route(c, b);
    out[0] = (uint32_t)r.input;
    out[1] = r.hand;
    out[2] = r.fast_analysis;
    out[3] = r.fast_pack;
    out[4] = r.k4_in_autocorr;
    out[5] = r.range_frames;
    out[6] = r.two_ranges;
    out[7] = r.host_out_possible;
    out[8] = r.segments_in_place;
}
