/*
 * flacenc_gpu.h -- C ABI of the MI355X-native FLAC encode hot path.
 *
 * This is the drop-in boundary.  The reference
 * (tuffy/flac-codec 1.3.2) is 100 % safe Rust with no FFI, so the boundary is
 * the narrowest internal call that separates per-frame ANALYSIS from stream
 * bookkeeping: the analysis half of `encode_frame`
 * (/root/reference/src/encode.rs:2259-2406) -- i.e. correlate_channels[_exhaustive]
 * (:2463-2847), encode_subframe (:2849-2980), encode_fixed_subframe (:3020-3088),
 * LpcParameters::best / encode_residuals (:3145-3332), write_residuals' partition
 * search (:3747-3962) -- for a BATCH of frames instead of one.  In the reference
 * the result of that half is up to 8 `BitRecorder`s per frame; here it is a
 * decision record per subframe plus the residual signal, or (flacgpu_pack_*) the
 * finished frame bytes.
 *
 * A Rust maintainer binds these with `extern "C"` inside `Encoder::encode`
 * (encode.rs:1997-2022); see INTEGRATION.md for the stub.
 *
 * Plain pointers and sizes only.  All functions return 0 on success or a
 * negative FLACGPU_ERR_*.  A context is NOT thread-safe (one per stream or per
 * GPU shard of a stream), exactly like the reference's `&mut Encoder`.
 * Internal analysis failures of the reference (InsufficientLpcSamples,
 * NoBestLpcOrder, ZeroLpCoefficients, LpNegativeShiftError, ResidualOverflow)
 * are never surfaced: as in encode.rs:2929-2968 they only steer the
 * FIXED / VERBATIM fallback.
 */
#ifndef FLACENC_GPU_H
#define FLACENC_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLACGPU_MAX_CHANNELS 8
#define FLACGPU_MAX_LPC_ORDER 32
#define FLACGPU_MAX_PARTITIONS 64
#define FLACGPU_MAX_BLOCK_SIZE 65535 /* every block size the reference accepts (encode.rs:1418-1423); blocks
                                        above 16384 take kernels that keep their arrays in HBM, not LDS */

enum {
    FLACGPU_OK = 0,
    FLACGPU_ERR_INVALID_ARG = -1,
    FLACGPU_ERR_UNSUPPORTED = -2, /* legal for the reference but not for this build (or the
                                     reference itself would panic, e.g. > 64 partitions,
                                     encode.rs:3756/3880) */
    FLACGPU_ERR_HIP = -3,         /* HIP runtime failure; flacgpu_last_error() has the text */
    FLACGPU_ERR_NO_DEVICE = -4,
    FLACGPU_ERR_BUFFER_TOO_SMALL = -5,
    FLACGPU_ERR_BUSY = -6,        /* flacgpu_pipeline_submit: every slot holds a batch, retire one first */
    FLACGPU_ERR_NO_RCCL = -7      /* flacgpu_rccl_allgather_counters: librccl could not be loaded (no fallback) */
};

/* encode.rs:1713-1720 `Window` */
enum { FLACGPU_WINDOW_RECTANGLE = 0, FLACGPU_WINDOW_HANN = 1, FLACGPU_WINDOW_TUKEY = 2 };

/* Mirror of `EncoderOptions` (encode.rs:1701-1709) + Options::block_size (:1366).
 * use_rice2 is derived exactly like encode.rs:1965 (stream bits_per_sample > 16). */
typedef struct {
    uint32_t block_size;          /* 16..=65535 */
    uint32_t max_partition_order; /* 0..=15 (effective order is capped at 6, see above) */
    uint32_t max_lpc_order;       /* 0 = None, else 1..=32 */
    uint8_t mid_side;
    uint8_t exhaustive_channel_correlation;
    uint8_t window_kind;          /* FLACGPU_WINDOW_* */
    uint8_t reserved;
    float window_param;           /* Tukey p */
} flacgpu_options;

/* subframe types (stream.rs:1452-1460) */
enum { FLACGPU_SUB_CONSTANT = 0, FLACGPU_SUB_VERBATIM = 1, FLACGPU_SUB_FIXED = 2, FLACGPU_SUB_LPC = 3 };

/* channel assignment as coded in the frame header (stream.rs:996-1010) */
enum {
    FLACGPU_ASSIGN_INDEPENDENT = 0,
    FLACGPU_ASSIGN_LEFT_SIDE = 8,
    FLACGPU_ASSIGN_SIDE_RIGHT = 9,
    FLACGPU_ASSIGN_MID_SIDE = 10
};

/* candidate a subframe was computed from */
enum { FLACGPU_SRC_MID = 8, FLACGPU_SRC_SIDE = 9 }; /* 0..7 = input channel */

/* Decision record of one subframe: everything `BitRecorder::playback`
 * (encode.rs:2332-2333) needs except the residual values themselves. */
typedef struct {
    uint8_t type;            /* FLACGPU_SUB_* */
    uint8_t wasted;          /* wasted bits per sample (encode.rs:2878-2898) */
    uint8_t bps;             /* effective bits per sample of this subframe */
    uint8_t order;           /* FIXED 0..4 / LPC 1..32 */
    uint8_t precision;       /* LPC coefficient precision (encode.rs:3305-3315) */
    uint8_t shift;           /* LPC shift (encode.rs:3360) */
    uint8_t coding_method;   /* 0 = RICE (4-bit), 1 = RICE2 (5-bit) (encode.rs:3929-3942) */
    uint8_t partition_order; /* as written: ilog2(n_partitions) (encode.rs:3902) */
    uint8_t source;          /* 0..7 input channel, FLACGPU_SRC_MID, FLACGPU_SRC_SIDE */
    uint8_t reserved[3];
    uint32_t n_partitions;   /* partitions actually emitted */
    uint32_t part_len;       /* residual chunk length; the first chunk is short (encode.rs:3876-3879) */
    uint32_t bits;           /* exact subframe length in bits == BitRecorder::written() */
    int32_t coeffs[FLACGPU_MAX_LPC_ORDER];
    uint8_t rice[FLACGPU_MAX_PARTITIONS];        /* Rice parameter; 0xFF = escaped / constant */
    uint8_t escape_bits[FLACGPU_MAX_PARTITIONS]; /* escape size, 0 = all-zero partition */
} flacgpu_subframe_plan;

typedef struct {
    uint8_t assignment; /* FLACGPU_ASSIGN_* */
    uint8_t channels;
    uint16_t block_size; /* samples per channel in this frame */
    uint32_t body_bits;  /* sum of the subframes' bits (frame = header + ceil(body/8) + 2) */
} flacgpu_frame_plan;

/* diagnostic counters of the last analyze call */
typedef struct {
    uint32_t frames;
    uint32_t lpc_failed;        /* candidates whose LPC path errored (fell back to FIXED) */
    uint32_t order_ties;        /* candidates whose two best LPC-order estimates were within
                                   1e-9 relative: inside that band the device's log() is not
                                   trusted to pick like the host libm the reference uses; they are
                                   re-decided on the host (see order_ties_resolved) */
    uint32_t log2_edge;         /* quantise calls where max|c| sat in the libm-sensitive band
                                   just below a power of two (handled by the host table) */
    uint32_t order_ties_resolved; /* of order_ties: candidates whose LPC parameters were recomputed on
                                   the host with its libm (encode.rs:3656-3702) before the results
                                   were handed out; every fetch / verify entry point does this */
    uint32_t fir_recheck;       /* candidates whose LPC residual, computed WITHOUT the per-sample overflow test of
                                   encode.rs:3190-3197, was too large to rule an overflow out (a lane's sum of
                                   folded residuals >= 2^30: garbage predictions only) */
    uint32_t fir_rechecked;     /* of fir_recheck: re-analysed with the exact test before the results were handed
                                   out (the same entry points as order_ties_resolved) */
    /* CUMULATIVE since the context was created (direct stereo input with LPC): candidates whose FIXED partition search and
     * exact bit count were put off behind the LPC half because the LPC size estimate undercut a lower bound of the
     * FIXED size -- fixed_decided: the exact LPC size then lay below the bound, encode.rs:2929-2934 was decided for LPC
     * without them; fixed_refetched: it did not, the samples were fetched again and counted.  Same bytes either way.
     * Both saturate at 2^32 - 1 (diagnostics of long-lived contexts, not arithmetic). */
    uint32_t fixed_decided;
    uint32_t fixed_refetched;
} flacgpu_stats;

typedef struct flacgpu_ctx flacgpu_ctx;

/* PCM layouts accepted by analyze */
enum {
    FLACGPU_LAYOUT_INTERLEAVED = 0, /* [pcm_frame][channel]  (FlacSampleWriter::write, encode.rs:558) */
    FLACGPU_LAYOUT_PLANAR = 1       /* [flac_frame][channel][block_size] (Frame, audio.rs:190-199) */
};

/* Create a context for one stream shape.  Replaces `EncodingCaches`
 * (encode.rs:1810-1851): all scratch lives in HBM, sized for `max_frames`
 * FLAC frames per call (at most 2 097 152: eight frame-layout chunks of 256 x 1024 frames).
 * device < 0 selects the current HIP device. */
int flacgpu_create(const flacgpu_options *opts, uint32_t bits_per_sample, uint32_t channels,
                   int device, uint32_t max_frames, flacgpu_ctx **out);
void flacgpu_destroy(flacgpu_ctx *ctx);
const char *flacgpu_last_error(void);

/* Analyse `n_frames` FLAC frames (all `block_size` long except the last, which is
 * `last_frame_len` samples per channel, 1..=block_size).
 *   pcm        host pointer, layout as given; samples must fit bits_per_sample
 *   plans      out, [n_frames]
 *   subframes  out, [n_frames * channels], subframe c of frame f at f*channels + c
 *   residuals  out, [n_frames][channels][block_size] int32: for FIXED/LPC subframes the
 *              `order` warm-up samples followed by the n-order residuals; for VERBATIM
 *              the n samples; for CONSTANT the sample at [0] (all after wasted-bit removal)
 * Synchronous, like the reference's encode_frame. */
int flacgpu_analyze(flacgpu_ctx *ctx, const int32_t *pcm, int layout, uint32_t n_frames,
                    uint32_t last_frame_len, flacgpu_frame_plan *plans,
                    flacgpu_subframe_plan *subframes, int32_t *residuals);

/* Same, PCM already resident in device memory (d_pcm is a device pointer).  Results stay
 * on the device until flacgpu_fetch().  Asynchronous with respect to the host.
 * `stream` is a hipStream_t.  NULL selects the context's own non-blocking stream, ordered AFTER
 * everything the caller has already submitted to the legacy default stream (so a d_pcm produced
 * there is safe to hand over); the results are then ordered on the context's stream, which every
 * flacgpu_fetch* / flacgpu_get_stats / flacgpu_wait call synchronises.  A caller that chains further
 * device work on the results passes its own stream instead.
 * Every entry point makes the context's device current for the duration of the call and restores
 * the caller's device afterwards.
 * Lifetime of d_pcm: interleaved stereo PCM of whole blocks of 1024, 1152, 2048, 2304 or 4096 samples (<= 24 bits), interleaved
 * 3-, 4-, 6- and 8-channel PCM of whole 4096-sample blocks (LPC order 1..16), one-channel PCM and planar PCM are read IN PLACE by the
 * analysis and frame kernels -- the
 * context keeps no copy (no K0 split pass; this is what the reference's `write(&[i32])` hands over,
 * encode.rs:558).  The buffer must therefore stay valid and unchanged until the batch's results have
 * been fetched (flacgpu_fetch* / flacgpu_verify_device / flacgpu_pack_device included) or the next
 * batch is submitted to this context.  flacgpu_set_tuning(ctx, FLACGPU_TUNE_COPY_INPUT, 1) (or FLACGPU_NO_DIRECT=1
 * in the environment) restores the copy and with it the old rule: free once the submitted work has run. */
int flacgpu_analyze_device(flacgpu_ctx *ctx, const int32_t *d_pcm, int layout, uint32_t n_frames,
                           uint32_t last_frame_len, void *stream);
/* Copy the results of the last flacgpu_analyze_device to host buffers (any may be NULL). */
int flacgpu_fetch(flacgpu_ctx *ctx, flacgpu_frame_plan *plans, flacgpu_subframe_plan *subframes,
                  int32_t *residuals);
int flacgpu_get_stats(flacgpu_ctx *ctx, flacgpu_stats *out);
/* Diagnostic (bench, tests): of the last batch's subframes, how many the candidate kernel handed to the frame kernel together
 * with their residual -- 4096-sample stereo frames read in place, LPC on: the wave that wins a subframe with an LPC candidate
 * stores the folded residual it still holds, and the frame kernel neither fetches the channels nor runs the FIR again
 * (encode.rs:3174-3203 is evaluated once per winning subframe instead of twice).  *enabled = 0 where the batch's shape has no
 * hand-over, FLACGPU_NO_HAND=1 is set, or the residual rows were fetched in between.  Synchronises the context. */
int flacgpu_handed_subframes(flacgpu_ctx *ctx, uint32_t *handed, uint32_t *subframes, int *enabled);

/* Device pointers of the last analysis (for callers that chain further device work):
 * which: 0 frame plans, 1 subframe plans, 2 residuals, 3 planar pcm, 4 packed frame bytes,
 * 5 frame byte offsets (uint64[n_frames + 1]), 6 the autocorrelation of every candidate (double[n_frames * candidates][36]:
 * lags 0 .. max_lpc_order of the windowed samples, encode.rs:3403-3413 -- bit for bit the reference's sums),
 * 7 the LPC parameters of every candidate ([n_frames * candidates] records of 136 bytes: int32 status -- 0 ok, else the
 * reference's error: 1 InsufficientLpcSamples (or no candidate / all zero), 2 NoBestLpcOrder, 3 ZeroLpCoefficients,
 * 4 LpNegativeShiftError --, uint8 order, precision, shift, size hint, int32 qlp[32]; the fields behind a non-zero status
 * are stale), handed out after what flacgpu_resolve re-decides (synchronous). */
void *flacgpu_device_buffer(flacgpu_ctx *ctx, int which);
/* The plans (0, 1) and the frame bytes / offsets (4, 5) an asynchronous call leaves in HBM are FINAL only after a resolving
 * entry point has run: flacgpu_fetch, flacgpu_fetch_frames, flacgpu_frames_ready, flacgpu_verify_device -- or this one, for
 * callers that consume the device buffers directly.  It waits for the context's stream, re-decides on the host the few
 * candidates whose LPC order estimate lies inside the libm-sensitive band (encode.rs:3656-3702) and re-runs the candidate
 * stage with the exact ResidualOverflow test (encode.rs:3189-3201) when the unchecked FIR could not rule an overflow out
 * (flacgpu_stats::fir_recheck != 0), then re-assembles the frames.  Nothing to do (the usual case): one stream sync and a
 * 16-byte read.  Synchronous. */
int flacgpu_resolve(flacgpu_ctx *ctx);

/* ---- device-side frame assembly ---------------------------------
 * Replaces, for the frames of the last flacgpu_analyze_device call, the host half of
 * encode_frame (encode.rs:2284-2294 header, :2332-2333 playback, :2408-2409 align + CRC-16)
 * and write_partitions / Partition::to_writer (encode.rs:3834-3907): frame header + CRC-8,
 * subframe headers, warm-up, LPC parameters, Rice/escaped residual codes (bit offsets by
 * prefix scan), byte alignment, CRC-16 -- producing the exact bytes `Encoder::encode` would
 * hand to its writer.  Frame f carries frame number first_frame_number + f.
 * Asynchronous; results stay in HBM until flacgpu_fetch_frames. */
int flacgpu_pack_device(flacgpu_ctx *ctx, uint64_t first_frame_number, uint32_t sample_rate,
                        void *stream);
/* flacgpu_analyze_device + flacgpu_pack_device of one batch in one asynchronous call: the device
 * half of `Encoder::encode` for every frame of the batch (encode.rs:2274-2440).
 * Overlap comes in two forms.  (1) Several contexts on several streams (double / triple buffering
 * of consecutive batches, what bench.py does): the HBM-, latency- and VALU-bound kernels of
 * different batches overlap; measured 0.86 -> 0.70 ms per 8192-frame batch with three contexts.
 * (2) FLACGPU_TUNE_TWO_RANGES: a single batch whose frames all take the 4096-sample wave kernels is
 * cut into two frame ranges whose kernel chains run on two HIP streams inside the context (worth
 * ~4 % for a lone batch, counter-productive together with (1), so off by default).
 * Either way the bytes, plans and counters are those of the two separate calls, and work submitted
 * to `stream` afterwards sees all of it. */
enum {
    FLACGPU_TUNE_TWO_RANGES = 1, /* 0 (default) / 1 */
    /* waves the autocorrelation lags of a 64-candidate group are split over: 4 (default; best for
     * a context that has the GPU to itself) or 2 (fewer instructions; best when several contexts
     * keep the SIMDs busy).  Results are identical. */
    FLACGPU_TUNE_LAG_SPLIT = 2,
    /* 1: flacgpu_frames_ready / flacgpu_fetch_frames_async / flacgpu_wait sleep between looks at their
     * event (50-200 us) instead of spinning in hipEventSynchronize.  For processes with more waiting threads
     * than CPUs (many concurrent writers): a spinning waiter burns the CPU time the others -- and the MD5
     * engines -- need.  0 (default) spins (lowest latency). */
    FLACGPU_TUNE_BLOCKING_WAIT = 3,
    /* 1: the context copies (splits) every batch of flacgpu_analyze_device / flacgpu_encode_device into its own
     * planar buffer at submission, as before r02: d_pcm may be refilled as soon as the submitted work has run,
     * whatever is fetched later (an LPC order tie re-decided at fetch time, flacgpu_verify_device, residual rows
     * all work from the copy).  0 (default): direct input, the lifetime rule at flacgpu_analyze_device applies.
     * For streaming callers that recycle one input buffer without waiting for their fetch. */
    FLACGPU_TUNE_COPY_INPUT = 4,
    /* flacgpu_encode_device runs a batch of in-place wave-kernel frames (interleaved whole 4096-sample blocks, LPC order
     * 1..16, exhaustive channel choice) range by range once it holds more than 1.5 x this many Mi samples: the whole kernel
     * chain for `value` Mi samples at a time.  Default: 64, stereo batches only (16384-frame batches: + 9 %; 8-channel batches
     * measured no gain and are cut only once this tuning has been set).  0: never cut.  The bytes, plans and counters are
     * those of the uncut batch. */
    FLACGPU_TUNE_CHUNK_MSAMPLES = 5
};
int flacgpu_set_tuning(flacgpu_ctx *ctx, int key, int value);
int flacgpu_encode_device(flacgpu_ctx *ctx, const int32_t *d_pcm, int layout, uint32_t n_frames,
                          uint32_t last_frame_len, uint64_t first_frame_number,
                          uint32_t sample_rate, void *stream);
/* Copies the packed frames of the last flacgpu_pack_device to the host.  offsets (may be NULL)
 * receives n_frames + 1 byte offsets into `out`; *total (may be NULL) the byte count.  When
 * `out` is NULL or cap is too small only offsets/total are filled and
 * FLACGPU_ERR_BUFFER_TOO_SMALL is returned. */
int flacgpu_fetch_frames(flacgpu_ctx *ctx, uint8_t *out, size_t cap, uint64_t *offsets,
                         uint64_t *total);
/* ---- frames that stay on the device (DESIGN.md 4c "Device-resident output") ----
 * flacgpu_frame_offsets: flacgpu_fetch_frames without the frame bytes.  Waits for the context's stream, re-decides what
 * flacgpu_resolve re-decides, and downloads the n_frames + 1 byte offsets of the packed frames (offsets, may be NULL;
 * *total, may be NULL, = offsets[n_frames]).  Synchronous.
 * flacgpu_place_frames: copies runs of the packed frame bytes to places in device memory, on the context's own stream
 * (k_place_runs: csrc/kernels/place_rule.h).  Run i takes the n bytes at byte `src` of the packed buffer
 * (flacgpu_device_buffer 4) to the device address `dst`; src, dst and n have any alignment, n may be 0.  Exactly the bytes
 * [dst, dst + n) are written; runs of one call must not overlap in their destinations.  Asynchronous: stream order
 * makes the copy finish before the context's next batch overwrites the packed buffer, and flacgpu_wait waits for it.
 * FLACGPU_ERR_INVALID_ARG (nothing is launched) when nothing is packed, the frames were assembled into a host buffer,
 * or a run reaches past the packed bytes.  The run table travels through buffers the context keeps between calls. */
typedef struct {
    uint64_t src;   /* flacgpu_place_frames: byte offset into the packed buffer; flacgpu_place_runs_host: an address */
    uint64_t dst;   /* an address */
    uint64_t n;     /* bytes */
} flacgpu_place_run;
int flacgpu_frame_offsets(flacgpu_ctx *ctx, uint64_t *offsets, uint64_t *total);
int flacgpu_place_frames(flacgpu_ctx *ctx, const flacgpu_place_run *runs, uint32_t n_runs);
/* The copy rule of k_place_runs run over HOST memory, one destination group after another in the kernel's lane order: a
 * test hook (no device is touched).  src and dst are host addresses.  flacgpu_place_workgroup: the kernel's lanes per
 * workgroup. */
int flacgpu_place_runs_host(const flacgpu_place_run *runs, uint32_t n_runs);
uint32_t flacgpu_place_workgroup(void);
/* analyze + pack + fetch in one synchronous call on host PCM: the whole of the reference's
 * `Encoder::encode` loop for a batch of blocks, minus stream bookkeeping. */
int flacgpu_encode_frames(flacgpu_ctx *ctx, const int32_t *pcm, int layout, uint32_t n_frames,
                          uint32_t last_frame_len, uint64_t first_frame_number,
                          uint32_t sample_rate, uint8_t *out, size_t cap, uint64_t *offsets,
                          uint64_t *total);

/* Device-side frame assembly of CALLER-SUPPLIED decisions (the device counterpart of
 * flacenc_pack_frames, include/flacenc_stream.h): `pcm` (host, interleaved, as for flacgpu_analyze)
 * is split into rows, `plans` [n_frames] / `subframes` [n_frames * channels] replace what an analysis
 * would have decided, and the packers produce the frame bytes (flacgpu_fetch_frames).  The decisions
 * must be consistent with the PCM (residuals are recomputed from it): that stays the caller's contract.
 * What the kernels assume of a plan and never test is checked on the host before anything is copied or
 * launched: channels and block_size equal to the context's (the last frame: last_frame_len), type, source,
 * bps + wasted equal to the stream's width (one more for a side source), order <= 4 (FIXED) or 1 .. the
 * context's max_lpc_order (LPC) and no larger than part_len, precision 1..15 with coefficients that fit it,
 * shift 0..15, coding_method 0 / 1 with rice[i] <= 14 / 30 or 0xFF and escape_bits[i] <= 31, partition_order
 * <= min(max_partition_order, 6), n_partitions == 1 << partition_order, part_len << partition_order equal to
 * the frame's length, body_bits equal to the sum of the subframes' bits, and a frame (a header of at most 16
 * bytes + ceil(body_bits / 8) + 2) no longer than the image its assembly kernel is launched with -- a plan
 * coded longer than its VERBATIM form (a Rice parameter far off) can be.  Such a plan is refused with
 * FLACGPU_ERR_INVALID_ARG, flacgpu_last_error naming the first offending frame, subframe and field. */
int flacgpu_pack_plans(flacgpu_ctx *ctx, const int32_t *pcm, uint32_t n_frames, uint32_t last_frame_len,
                       const flacgpu_frame_plan *plans, const flacgpu_subframe_plan *subframes,
                       uint64_t first_frame_number, uint32_t sample_rate);

/* ---- asynchronous host path: stream-width upload, sizes ahead of the bytes ---------------------
 * What a streaming front end (FlacSampleWriter / FlacByteWriter, encode.rs:359, 558) needs to keep
 * several batches in flight: PCM enters as the little-endian `bytes_per_sample = ceil(bps / 8)`-byte
 * samples that FlacByteWriter::write receives and update_md5 hashes (encode.rs:1292-1318,
 * byteorder.rs:60-72) -- 2 or 3 bytes per sample across PCIe instead of 4, widened by K0 on the
 * device --, ideally from pinned memory (flacgpu_host_alloc), so that the copy is asynchronous.
 *   flacgpu_encode_packed_async  H2D + analysis + frame assembly, all queued; returns at once
 *   flacgpu_frames_ready         waits for the frame SIZES only (they leave the device right after
 *                                k_layout, while the bytes are still being assembled); *offsets
 *                                (n_frames + 1 entries) stays valid until the context's next batch
 *   flacgpu_fetch_frames_async   queues the copy of exactly those bytes to `out`
 *   flacgpu_wait                 waits for that copy (or, without one, for the context's stream)
 * One batch per context at a time; several contexts overlap (H2D of one, kernels of another, D2H of
 * a third run concurrently on their own streams). */
void *flacgpu_host_alloc(size_t bytes); /* pinned host memory (hipHostMalloc), NULL on failure */
void flacgpu_host_free(void *p);
int flacgpu_current_device(void);       /* the caller's current HIP device, -1 without one */
/* Diagnostic: GB/s the host link of `device` (-1: current) carries, both directions summed, moving `bytes` each way with
 * up_mode / down_mode = 0 (idle), 1 (copy engine: hipMemcpyAsync on its own stream) or 2 (a kernel loading from /
 * storing to pinned host memory) at the same time.  The asynchronous host path uploads by copy engine and lets k_frame64
 * store the frames into pinned memory: (1, 2) is its ceiling. */
int flacgpu_link_probe(int device, size_t bytes, int up_mode, int down_mode, double *sum_gbs);
/* 1 when flacgpu_encode_packed_async takes this sample width for the context's stream shape (a block
 * must be a whole number of 16-byte groups); otherwise widen to int32 and pass bytes_per_sample 4 */
int flacgpu_packed_input_supported(const flacgpu_ctx *ctx, uint32_t bytes_per_sample);
/* the same question before a context exists (it depends on the block size, the channel count and the width only) */
int flacgpu_packed_input_shape_supported(uint32_t block_size, uint32_t channels, uint32_t bytes_per_sample);
int flacgpu_encode_packed_async(flacgpu_ctx *ctx, const uint8_t *pcm_le, uint32_t bytes_per_sample,
                                uint32_t n_frames, uint32_t last_frame_len, uint64_t first_frame_number,
                                uint32_t sample_rate);
int flacgpu_frames_ready(flacgpu_ctx *ctx, const uint64_t **offsets, uint64_t *total);
/* As flacgpu_encode_packed_async, with the frames assembled STRAIGHT INTO `out_host` (pinned memory from
 * flacgpu_host_alloc, at least flacgpu_packed_cap(ctx) bytes, 4-byte aligned): k_frame64 only stores -- dwords
 * inside a frame, bytes at its ends -- so it writes over PCIe while it works and no download follows.  Taken
 * when every frame of the batch is assembled by k_frame64 (whole blocks of a wave block length); otherwise
 * the frames stay in device memory as usual.  flacgpu_fetch_frames_async(out_host) then has nothing to copy;
 * flacgpu_wait returns when the frames are in `out_host`. */
int flacgpu_encode_packed_async_host(flacgpu_ctx *ctx, const uint8_t *pcm_le, uint32_t bytes_per_sample,
                                     uint32_t n_frames, uint32_t last_frame_len, uint64_t first_frame_number,
                                     uint32_t sample_rate, uint8_t *out_host, size_t out_cap);
size_t flacgpu_packed_cap(const flacgpu_ctx *ctx);   /* bytes a batch of max_frames frames can need */
int flacgpu_fetch_frames_async(flacgpu_ctx *ctx, uint8_t *out, size_t cap);
int flacgpu_wait(flacgpu_ctx *ctx);

/* ---- the pipelined batch loop: host PCM in, finished frames in host memory out, both link directions busy ----------
 * Replaces the per-block loop of `Encoder::encode` as FlacSampleWriter::write drives it (encode.rs:558-585) for callers
 * that bring whole batches of blocks and do their own stream bookkeeping: `depth` encoder contexts take consecutive
 * batches in rotation, each on its own HIP stream, so the upload of batch n, the kernels of batch n - 1 and the frames of
 * batch n - 2 (stored by k_frame64 straight into the slot's pinned buffer) are in flight together.
 *   submit   queues H2D + analysis + frame assembly of one batch and returns at once; FLACGPU_ERR_BUSY when all `depth`
 *            slots hold a batch.  `pcm`: interleaved samples in PINNED host memory (flacgpu_host_alloc), int32 when
 *            bytes_per_sample == 4, else the little-endian ceil(bps / 8)-byte samples of flacgpu_encode_packed_async;
 *            it must stay valid until that batch has been retired.
 *   retire   waits for the OLDEST batch in flight and hands out its frames: `*frames` (pinned memory owned by the
 *            pipeline), `*offsets` (n_frames + 1 byte offsets) and `*total` stay valid until the next submit, which
 *            reuses that slot.  Frames are byte-identical to flacgpu_encode_frames on the same batch.
 * Batches are independent (frame numbers come from the caller), so the output order is the submit order.
 * examples/c_abi_pipeline.c is the whole recipe; bench.py's end_to_end.pipelined_pcie measures it. */
typedef struct flacgpu_pipeline flacgpu_pipeline;
int flacgpu_pipeline_create(const flacgpu_options *opts, uint32_t bits_per_sample, uint32_t channels, int device,
                            uint32_t max_frames, uint32_t depth, flacgpu_pipeline **out);
void flacgpu_pipeline_destroy(flacgpu_pipeline *p);
int flacgpu_pipeline_submit(flacgpu_pipeline *p, const void *pcm, uint32_t bytes_per_sample, uint32_t n_frames,
                            uint32_t last_frame_len, uint64_t first_frame_number, uint32_t sample_rate);
int flacgpu_pipeline_retire(flacgpu_pipeline *p, const uint8_t **frames, const uint64_t **offsets, uint32_t *n_frames,
                            uint64_t *total);
uint32_t flacgpu_pipeline_in_flight(const flacgpu_pipeline *p);
uint32_t flacgpu_pipeline_depth(const flacgpu_pipeline *p);

/* ---- a batch made of SEGMENTS: frames of SEVERAL streams in one analysis batch ------------------------------------------
 * The reference encodes every file with an `Encoder` of its own, block by block (encode.rs:487-627 once per file); a batch of
 * a few hundred frames leaves most of the GPU idle and still pays the kernels' launches and their serial walk over a block
 * (256 frames of 24-bit stereo run at 0.3 of the per-sample rate of 8192).  Here runs of WHOLE blocks of several streams of
 * the context's shape (bits per sample, channels, options) form one batch: segment s contributes n_frames frames numbered
 * first_frame_number, first_frame_number + 1, ...; the frames come out concatenated in segment order (offsets: one entry per
 * frame of the batch plus the end).  A stream's short last block is not a segment: it goes through flacgpu_encode_frames, or,
 * with the short last blocks of many streams at once, through flacgpu_encode_ragged_device (below).
 *   flacgpu_encode_segments_device  PCM resident in device memory, asynchronous like flacgpu_encode_device (results through
 *                                   flacgpu_fetch_frames / flacgpu_device_buffer).  Every shape flacgpu_analyze_device reads in
 *                                   place -- interleaved stereo of 4096-, 2304-, 2048-, 1152- or 1024-sample blocks (<= 24
 *                                   bits), 2..8 interleaved independent channels of 4096-sample blocks (LPC order 1..16) --
 *                                   is read IN PLACE through a per-frame address table when every segment starts on a
 *                                   16-byte boundary (the buffers must stay valid until the results were fetched); other
 *                                   shapes (one channel, other block sizes, 32-bit samples) are gathered into the
 *                                   context's input buffer first.
 *   flacgpu_encode_segments         host PCM (int32): every segment is uploaded to its place in the context's input buffer --
 *                                   the gather costs nothing beyond the upload; synchronous, frames to `out`. */
typedef struct {
    const int32_t *pcm;            /* interleaved samples of n_frames whole blocks */
    uint32_t n_frames;
    uint32_t reserved;
    uint64_t first_frame_number;   /* of the segment's first frame (the frame number counts the stream's blocks) */
} flacgpu_segment;
int flacgpu_encode_segments_device(flacgpu_ctx *ctx, const flacgpu_segment *segments, uint32_t n_segments,
                                   uint32_t sample_rate, void *stream);
int flacgpu_encode_segments(flacgpu_ctx *ctx, const flacgpu_segment *segments, uint32_t n_segments, uint32_t sample_rate,
                            uint8_t *out, size_t cap, uint64_t *offsets, uint64_t *total);
/* ---- a RAGGED batch: frames of ANY length 1 .. block_size, of any streams of the context's shape, as one batch ------------
 * What the short last blocks of many streams need: one call for all of them instead of one one-frame call each.
 *   flacgpu_encode_ragged_device  asynchronous like flacgpu_encode_segments_device; results through flacgpu_fetch_frames,
 *       flacgpu_frame_offsets / flacgpu_place_frames and flacgpu_verify_device, one offset per frame plus the end.  Frame
 *       f's bytes are exactly what flacgpu_encode_device(ctx1, frames[f].pcm, FLACGPU_LAYOUT_INTERLEAVED, 1,
 *       frames[f].samples, frames[f].frame_number, sample_rate, ...) produces on a one-frame context with the same options,
 *       whatever the other frames of the batch are and whatever order they come in.  The samples are copied into the
 *       context's input buffer by the call's first kernel: the caller's buffers must stay valid until that has run (any
 *       fetch entry waits for it), not longer.  Every frame runs the generic kernels, a whole block included.
 *       Refused before anything is launched, the context's last batch left as it was: n_frames == 0 or more than the
 *       context's max_frames, a frame without PCM, samples == 0 or > block_size (FLACGPU_ERR_INVALID_ARG); a frame whose
 *       effective partition order min(ctz(samples), max_partition_order) exceeds 6 (FLACGPU_ERR_UNSUPPORTED, the rule of a
 *       short last frame everywhere; flacgpu_last_error names the first such frame).
 *   flacgpu_ragged_plan           the same checks and the layout of the call's window pool, on the host alone (no device, no
 *       context): one window per DISTINCT length in first-appearance order, each followed by 64 zero doubles.  Any out
 *       pointer may be NULL; window_of[n_frames] gets every frame's index among the distinct lengths, distinct[] (room for
 *       n_frames) the lengths, *pool_doubles = sum(n + 64) over them.  Nothing is written for a refused batch. */
typedef struct {
    const int32_t *pcm;      /* device memory: `samples` interleaved sample groups of the context's channel count; any 4-byte alignment */
    uint32_t samples;        /* per channel, 1 .. block_size */
    uint32_t reserved;       /* 0 */
    uint64_t frame_number;   /* the number coded into this frame's header */
} flacgpu_ragged_frame;
int flacgpu_encode_ragged_device(flacgpu_ctx *ctx, const flacgpu_ragged_frame *frames, uint32_t n_frames,
                                 uint32_t sample_rate, void *stream);
int flacgpu_ragged_plan(const flacgpu_options *opts, const uint32_t *samples, uint32_t n_frames,
                        uint32_t *window_of, uint32_t *distinct, uint32_t *n_distinct, uint64_t *pool_doubles);
/* how often the context has uploaded its ragged window pool so far: a batch whose every length has a window in the pool
 * the context keeps uploads none (for tests of that reuse) */
uint64_t flacgpu_ragged_pool_uploads(const flacgpu_ctx *ctx);

/* The asynchronous, stream-width form (r06): what a front end that coalesces many streams needs to keep the link busy.  The
 * segments' whole blocks lie BACK TO BACK in `pcm_le` (pinned memory; int32 when bytes_per_sample == 4, else the little-endian
 * ceil(bps / 8)-byte samples of flacgpu_encode_packed_async -- the byte string update_md5 hashes, encode.rs:1292-1318) in
 * segment order; flacgpu_segment::pcm is ignored.  Upload, analysis and frame assembly are queued and the call returns;
 * k_frame64 stores the frames straight into `out_host` (pinned, >= flacgpu_packed_cap(ctx) bytes) when every frame takes it.
 * Results as for flacgpu_encode_packed_async_host: flacgpu_frames_ready (one offset per frame of the batch plus the end),
 * flacgpu_fetch_frames_async, flacgpu_wait.  `pcm_le` must stay valid until the batch has been waited for. */
int flacgpu_encode_segments_packed_async_host(flacgpu_ctx *ctx, const uint8_t *pcm_le, uint32_t bytes_per_sample,
                                              const flacgpu_segment *segments, uint32_t n_segments, uint32_t sample_rate,
                                              uint8_t *out_host, size_t out_cap);

/* ---- several GPUs ------------------------------------------------------------------------------------
 * A FLAC frame depends on its own samples, the options and its frame number only (encode.rs:2284-2294), so a stream shards
 * by CONTIGUOUS FRAME RANGES with no data-path exchange.  What crosses shards is bookkeeping -- the reference's single
 * process keeps it in `Encoder` (encode.rs:1997-2022): the seek points' byte offsets, a prefix sum of frame sizes
 * (:1999-2003), STREAMINFO's min / max frame size (:2414-2436) and the totals.  One record of four integers per shard
 * carries all of it. */
typedef struct {
    uint64_t frames;     /* frames of the shard */
    uint64_t bytes;      /* their bytes */
    uint64_t min_frame;  /* smallest / largest frame of the shard; 0 for a shard without frames, which takes no part in */
    uint64_t max_frame;  /* the merged min / max */
} flacgpu_shard_counters;
/* Stream-level bookkeeping from the per-shard records, in shard order: totals, min / max frame size and (optional, n
 * entries) the byte offset of every shard's first frame behind the stream's first frame (exclusive prefix sum). */
int flacgpu_merge_counters(const flacgpu_shard_counters *shards, uint32_t n, flacgpu_shard_counters *merged,
                           uint64_t *shard_byte_offsets);
/* The contiguous frame range [lo, hi) of shard `shard` of `shards`: [k F / G, (k + 1) F / G). */
void flacgpu_shard_range(uint64_t total_frames, uint32_t shards, uint32_t shard, uint64_t *lo, uint64_t *hi);
int flacgpu_device_count(void);   /* visible HIP devices */
/* The host side of a device: the NUMA node its PCI function hangs off (-1: unknown) and the CPUs local to it as sysfs spells
 * them ("0-63,128-191"; empty: unknown) -- where the host threads that feed the device belong. */
int flacgpu_device_numa_info(int device, int *numa_node, char *cpulist, size_t cap);

/* ONE PROCESS, SEVERAL DEVICES.  `devices` lists HIP ordinals, one shard each (NULL / 0: every visible device; an ordinal
 * may be listed more than once -- each listing is a shard with contexts of its own).  Every shard owns up to `depth`
 * encoder contexts sized for `max_frames` frames per batch.
 *   flacgpu_multi_encode         a run of blocks of ONE stream in host memory (int32, or the little-endian ceil(bps/8)-byte
 *                                samples of flacgpu_encode_packed_async; pinned memory keeps the uploads asynchronous): cut into
 *                                batches of <= max_frames frames that are DEALT to the shards in turn (batch j to shard j mod
 *                                shards), each shard keeping `depth` of its batches in flight on a parked host thread of its own
 *                                that is bound to the CPUs of its GPU's NUMA node; every frame carries the number the stream
 *                                gives it.  The frames come back concatenated in stream order in `out` -- each retired batch is
 *                                copied ONCE, from its pinned slot to its final place (a batch's place is the sum of the sizes of
 *                                the batches before it, published as they retire) --, `offsets` (n_frames + 1 entries),
 *                                `per_shard` (flacgpu_multi_shards entries: what each shard encoded) and `merged` as
 *                                flacgpu_merge_counters leaves them.  Any out pointer may be NULL (FLACGPU_ERR_BUFFER_TOO_SMALL
 *                                with *total set when `out` is too small).  Byte-identical to one context's
 *                                flacgpu_encode_frames over the same blocks.  Synchronous.
 *   flacgpu_multi_encode_device  PCM resident in shard `shard`'s device memory: flacgpu_encode_device on the shard's next
 *                                context in rotation, asynchronous; flacgpu_multi_wait drains every context of every shard;
 *                                flacgpu_multi_counters reads the records of every shard's LAST batch (and merges them);
 *                                flacgpu_multi_last_context hands that batch's context out (fetch / verify). */
/* A flacgpu_multi belongs to one calling thread at a time (like a flacgpu_ctx); flacgpu_multi_encode runs its shards on
 * threads of its own for the duration of the call. */
typedef struct flacgpu_multi flacgpu_multi;
int flacgpu_multi_create(const flacgpu_options *opts, uint32_t bits_per_sample, uint32_t channels, const int *devices,
                         uint32_t n_devices, uint32_t max_frames, uint32_t depth, flacgpu_multi **out);
void flacgpu_multi_destroy(flacgpu_multi *m);
uint32_t flacgpu_multi_shards(const flacgpu_multi *m);
/* Cumulative over the object's flacgpu_multi_encode calls: bytes handed out in `out`, bytes the host copied to put them there
 * (the same number: one copy per output byte), and how many of the shards' threads were bound to their GPU's local CPUs. */
int flacgpu_multi_host_copy_stats(const flacgpu_multi *m, uint64_t *bytes_out, uint64_t *bytes_copied, uint32_t *threads_near_gpu);
int flacgpu_multi_device_of(const flacgpu_multi *m, uint32_t shard);
int flacgpu_multi_encode(flacgpu_multi *m, const void *pcm, uint32_t bytes_per_sample, uint64_t n_frames,
                         uint32_t last_frame_len, uint64_t first_frame_number, uint32_t sample_rate, uint8_t *out,
                         size_t cap, uint64_t *offsets, uint64_t *total, flacgpu_shard_counters *per_shard,
                         flacgpu_shard_counters *merged);
int flacgpu_multi_encode_device(flacgpu_multi *m, uint32_t shard, const int32_t *d_pcm, int layout, uint32_t n_frames,
                                uint32_t last_frame_len, uint64_t first_frame_number, uint32_t sample_rate);
int flacgpu_multi_wait(flacgpu_multi *m);
int flacgpu_multi_counters(flacgpu_multi *m, flacgpu_shard_counters *per_shard, flacgpu_shard_counters *merged);
flacgpu_ctx *flacgpu_multi_last_context(flacgpu_multi *m, uint32_t shard);

/* ONE PROCESS PER GPU (torchrun / MPI): the same record all-gathered over the caller's RCCL communicator (an
 * `ncclComm_t`; `stream` a hipStream_t or NULL) -- the path's only collective, 32 bytes per rank.  `all` receives
 * *n_ranks records in rank order (cap_ranks entries provided).  librccl is loaded on first use; when it cannot be,
 * the call fails with FLACGPU_ERR_NO_RCCL -- there is no fallback.  Synchronous. */
int flacgpu_rccl_available(void);
int flacgpu_rccl_allgather_counters(void *nccl_comm, void *stream, const flacgpu_shard_counters *mine,
                                    flacgpu_shard_counters *all, uint32_t cap_ranks, uint32_t *n_ranks, uint32_t *my_rank);

/* ---- device-side decode + verify of the frames packed last ----------
 * The reference's frame decoder (decode.rs:1388-1436 read_frame, 1494-1633 read_subframes,
 * 1635-1752 read_subframe / predict, 1800-1856 read_residuals) run on the GPU, one lane per
 * subframe, over the bytes produced by flacgpu_pack_device, plus a CRC-16 check of every frame.
 * A lane starts where the encoder's plan says its subframe starts; the plan is proven, not
 * trusted: subframe 0 must start where the frame header ends, every subframe must end exactly
 * where the next one starts and the last one at the padding before the CRC-16 (otherwise the
 * frame counts as bad_structure) -- i.e. the frame parses front to back as a sequential decoder
 * would parse it.
 * When the analysed PCM is still in the context (host-input or interleaved device input), the
 * decoded samples are compared with it -- the round trip every encoder test of the reference
 * performs (tests/format.rs), without leaving HBM. */
typedef struct {
    uint32_t frames;
    uint32_t bad_structure;      /* header / CRC-8 / subframe structure errors */
    uint32_t bad_crc16;
    uint32_t frames_pcm_differs; /* only meaningful when compared_pcm != 0 */
    uint32_t samples_differ;
    uint32_t compared_pcm;
} flacgpu_verify_result;
int flacgpu_verify_device(flacgpu_ctx *ctx, uint32_t sample_rate, uint64_t first_frame_number,
                          flacgpu_verify_result *result, float *kernel_ms);
/* decoded PCM of the last flacgpu_verify_device, interleaved, to host memory
 * ((n_frames-1)*block_size + last_frame_len) * channels samples */
int flacgpu_fetch_decoded(flacgpu_ctx *ctx, int32_t *interleaved);

/* ---- stand-alone decoder: any FLAC stream, not only this encoder's output ---------------------
 * The reference's `verify` / frame reader (decode.rs:1282, 1388-1436 read_frame, 1494-1856) for a
 * whole stream held in host memory: the host parses the metadata and finds the frame boundaries
 * (next valid header preceded by the CRC-16 of everything since the frame's start), the GPU decodes
 * the frames in parallel (one lane per frame walks its subframes front to back), re-checks every
 * CRC-16 and undoes the stereo decorrelation; the MD5 of the decoded PCM is compared with
 * STREAMINFO's.  `out` (may be NULL: verify only) receives the interleaved samples. */
typedef struct {
    uint32_t sample_rate, channels, bits_per_sample, min_block, max_block;
    uint32_t frames;            /* frames found by the scan */
    uint32_t bad_frames;        /* frames that did not parse (+1 when the scan lost synchronisation) */
    uint32_t bad_crc16;
    uint64_t total_samples;     /* STREAMINFO: samples per channel, 0 = unknown */
    uint64_t decoded_samples;   /* samples per channel in the frames found */
    uint8_t md5[16];            /* STREAMINFO */
    uint8_t decoded_md5[16];    /* of the decoded PCM */
    uint32_t md5_status;        /* 1: equal, 0: different, 2: STREAMINFO holds no MD5 (all zero) */
    uint32_t reserved;
} flacgpu_stream_info;
int flacgpu_decode_stream(const uint8_t *data, size_t len, int device, int32_t *out, size_t out_cap_samples,
                          flacgpu_stream_info *info);
/* The host half of flacgpu_decode_stream alone: the metadata parse and the frame scan, the very code that call starts
 * with.  Makes no HIP call and needs no device.  Returns what flacgpu_decode_stream returns for the metadata; fills
 * `info` as it stands after the scan (STREAMINFO fields, frames, decoded_samples, bad_frames = 1 when the scan lost
 * synchronisation; the CRC-16 and MD5 fields stay 0) and *n_frames = info->frames.  frame_off / frame_n (either may be
 * NULL: the count alone) receive every frame's first byte in `data` and its block size; with one given and
 * cap < *n_frames the call writes neither and returns FLACGPU_ERR_BUFFER_TOO_SMALL. */
int flacgpu_scan_stream_host(const uint8_t *data, size_t len, flacgpu_stream_info *info, uint64_t *frame_off,
                             uint32_t *frame_n, size_t cap, uint32_t *n_frames);

/* ---- batch decoder: many FLAC streams in one call, into host or device memory -------------------------------------
 * The same result as flacgpu_decode_stream for every stream (rc, every field of `info`, the samples), for any bytes,
 * with frame discovery, decoding, the CRC-16 check and the MD5 on the device.  One exception: a stream without frames
 * is hashed as the empty input (md5_status 1 when STREAMINFO holds the MD5 of nothing, 2 when it holds zeros), where
 * flacgpu_decode_stream returns before hashing (md5_status 0).  The samples of a frame that does not decode are
 * undefined in both.  A handle keeps its device buffers and pinned staging between calls; it is not thread-safe.
 *   scan    parses the metadata on the host, uploads every stream's frames in one copy and finds the frames on the
 *           device; fills rc, info (all but bad_crc16 and the MD5 fields, and bad_frames only for the scan), out_offset,
 *           and *total_samples = the int32 count `out` must hold.  The inputs may be freed after return.
 *   decode  decodes the scanned batch into `out`: device memory of the decoder's device with FLACGPU_DECODE_OUT_DEVICE,
 *           else host memory.  Every stream's record is written in full.  Synchronous.  A whole-call failure (HIP
 *           error, out of memory, FLACGPU_ERR_BUFFER_TOO_SMALL) writes nothing past out_cap_samples. */
#define FLACGPU_DECODE_OUT_DEVICE 1u
#define FLACGPU_DECODE_NO_MD5 2u   /* md5_status 3: not checked */
typedef struct flacgpu_decoder flacgpu_decoder;
typedef struct {
    int32_t rc;                 /* what flacgpu_decode_stream returns for this stream alone */
    uint32_t reserved;
    uint64_t out_offset;        /* first int32 of this stream in `out` (interleaved samples) */
    flacgpu_stream_info info;
} flacgpu_decoded_stream;
int flacgpu_decoder_create(int device, flacgpu_decoder **out);
void flacgpu_decoder_destroy(flacgpu_decoder *d);
int flacgpu_decoder_scan(flacgpu_decoder *d, const uint8_t *const *data, const size_t *len, uint32_t n_streams,
                         flacgpu_decoded_stream *streams, uint64_t *total_samples);
int flacgpu_decoder_decode(flacgpu_decoder *d, int32_t *out, size_t out_cap_samples, uint32_t flags,
                           flacgpu_decoded_stream *streams);

/* ---- batch decoder: other sample formats and layouts -----------------------------------------------------------------
 * decode_as decodes the scanned batch as flacgpu_decoder_decode does (flags, host or device `out`, the records), in
 * the element type and layout of `fmt`, converted on the sample's one way from the decoder's scratch to `out`:
 *   I32  the sample.
 *   I16  sample << (16 - bps).  Needs bps <= 16 in every stream with rc == 0; else the whole call returns
 *        FLACGPU_ERR_UNSUPPORTED, flacgpu_last_error names the first such stream, and nothing is written.
 *   S24  (sample << (24 - bps)) & 0xFFFFFF as 3 bytes, little-endian, two's complement, no padding between elements:
 *        element e starts at byte 3 * e (WAV's left-justified 24-bit container).  Needs bps <= 24 in every stream with
 *        rc == 0; refused like I16 otherwise.  `out` needs no alignment.
 *   F32  (float)sample (round to nearest even) * 2^-(bps - 1): exact for bps <= 25, correctly rounded above.
 *   FLAT    streams back to back, each [samples][channels]; stream i starts at element out_offset (of the scan).
 *   PADDED  [n_streams][channels_padded][samples_padded], planar: stream i starts at element
 *           i * channels_padded * samples_padded, channel c at c * samples_padded behind that.  Elements with
 *           c >= channels or t >= decoded_samples, and every element of a stream with rc != 0 or without frames, are
 *           zero.  channels_padded and samples_padded must cover every stream with rc == 0 (FLACGPU_ERR_INVALID_ARG
 *           otherwise); 0 is valid only when no stream has samples.
 * After FLACGPU_OK all out_bytes (plan_output) are defined, whatever `out` held before; the samples of a frame that
 * does not decode are undefined, inside that frame's own samples of its own stream's rows.  A refused call
 * (INVALID_ARG, UNSUPPORTED, BUFFER_TOO_SMALL when out_cap_bytes < out_bytes) writes nothing.  For host output the
 * decoder stages and downloads out_bytes, not 4 bytes per sample.  A scan may be decoded any number of times, in any
 * formats, in either order with flacgpu_decoder_decode.
 * The MD5 is taken over interleaved int32: with a format other than I32 / FLAT, verification costs 4 * total_samples
 * bytes of device memory (a decoder-owned copy the same kernel pass writes); FLACGPU_DECODE_NO_MD5 neither writes nor
 * allocates it.
 * plan_output is a pure host function (no device, no handle): validates `fmt` against scanned records and returns
 * the bytes `out` must hold. */
#define FLACGPU_SAMPLE_I32 0u
#define FLACGPU_SAMPLE_I16 1u
#define FLACGPU_SAMPLE_F32 2u
#define FLACGPU_SAMPLE_S24 24u    /* packed 3-byte little-endian elements (the value is 24, not 3) */
#define FLACGPU_LAYOUT_FLAT   0u  /* streams back to back, each [samples][channels]: flacgpu_decoder_decode's layout */
#define FLACGPU_LAYOUT_PADDED 1u  /* [n_streams][channels_padded][samples_padded], planar, zero-filled */
typedef struct {
    uint32_t dtype, layout;
    uint32_t channels_padded;   /* PADDED only, else 0 */
    uint32_t reserved;          /* 0 */
    uint64_t samples_padded;    /* PADDED only, else 0 */
} flacgpu_out_format;
int flacgpu_decoder_plan_output(const flacgpu_out_format *fmt, const flacgpu_decoded_stream *streams,
                                uint32_t n_streams, uint64_t *out_bytes);
int flacgpu_decoder_decode_as(flacgpu_decoder *d, void *out, size_t out_cap_bytes, const flacgpu_out_format *fmt,
                              uint32_t flags, flacgpu_decoded_stream *streams);

/* ---- batch decoder: sample windows of a scanned batch (random crops) ---------------------------------------------
 * decode_windows decodes only the frames that each window touches and writes only the windows:
 * [n_windows][channels_padded][samples_padded], planar, in fmt->dtype with decode_as's conversions.  fmt->layout must be
 * FLACGPU_LAYOUT_PADDED, samples_padded must cover the longest window and channels_padded every stream with rc == 0
 * that a window names.  Element [w][c][t] is sample start + t of channel c for c < channels and t < samples (of the
 * window's result); every other element is zero, and so is the whole block of a window on a stream with rc != 0.  After
 * FLACGPU_OK all out_bytes (plan_windows) are defined, whatever `out` held before.  `out` is host or device memory as
 * for decode_as; `flags` are its flags.
 * The frames come from the scan's own frame table, which is exact for any stream (variable block sizes included); a
 * SEEKTABLE is not read.  Windows may overlap, come in any order, and name a stream several times or not at all; a
 * frame that two windows touch is decoded once per window.  The samples of a frame that does not decode are undefined,
 * inside that frame's share of that window only.  No MD5 is computed (a window has none; FLACGPU_DECODE_NO_MD5 changes
 * nothing); the CRC-16 of every decoded frame is checked and counted per window.  Device scratch is sized by the
 * selected frames, not by the batch.
 * A refused call writes nothing: no scanned batch, stream >= n_streams, reserved != 0, start + length overflowing, a
 * layout other than PADDED or padding too small (FLACGPU_ERR_INVALID_ARG), out_cap_bytes < out_bytes
 * (FLACGPU_ERR_BUFFER_TOO_SMALL), I16 with a named rc == 0 stream of more than 16 bits or S24 with one of more than 24
 * (FLACGPU_ERR_UNSUPPORTED, flacgpu_last_error names the stream of the first such window).  A stream that no window names takes no part in these
 * checks.  n_windows == 0 is valid and writes nothing.  decode, decode_as and decode_windows may follow one another in
 * any order on one scan.
 * plan_windows is a pure host function (no device, no handle): the checks above on scanned records, and the bytes `out`
 * must hold.  flacgpu_window_frames is the frame selection alone on a list of block sizes: frames [*first, *first +
 * *count) hold samples [start, start + length) clipped to the stream, *skip samples of frame *first lie in front of
 * `start`; an empty window or one past the end gives *count = 0 (*first = 0, *skip = 0). */
typedef struct {
    uint32_t stream;    /* index into the scanned batch */
    uint32_t reserved;  /* 0 */
    uint64_t start;     /* first sample per channel */
    uint64_t length;    /* samples per channel; 0 is valid */
} flacgpu_window;
typedef struct {
    int32_t  rc;         /* the stream's scan rc; a window on an rc != 0 stream is all zero */
    uint32_t frames;     /* frames decoded for this window */
    uint32_t bad_frames; /* of those, frames that did not parse */
    uint32_t bad_crc16;  /* of those */
    uint64_t samples;    /* valid samples per channel: clamp(decoded_samples - start, 0, length) */
} flacgpu_window_result;
int flacgpu_decoder_plan_windows(const flacgpu_out_format *fmt, const flacgpu_decoded_stream *streams,
                                 uint32_t n_streams, const flacgpu_window *w, uint32_t n_windows, uint64_t *out_bytes);
int flacgpu_decoder_decode_windows(flacgpu_decoder *d, void *out, size_t out_cap_bytes, const flacgpu_out_format *fmt,
                                   uint32_t flags, const flacgpu_window *w, uint32_t n_windows,
                                   flacgpu_window_result *results);
int flacgpu_window_frames(const uint32_t *frame_n, uint32_t n_frames, uint64_t start, uint64_t length, uint32_t *first,
                          uint32_t *count, uint64_t *skip);

/* ---- batch decoder: raw frame streams (bare frames, no fLaC marker, no STREAMINFO) ----------------------------------
 * What FlacStreamWriter / flacenc_stream_writer emits, and what a byte range cut out of the middle of a .flac file is:
 * frames whose "subset" headers carry their own sample rate, channels and sample size, which may change from frame to
 * frame.  The scan needs no metadata, skips to the first whole frame and resynchronises after damage (DESIGN.md 4b
 * "Raw frame streams" states the rule): a position is a candidate when a frame header with a CRC-8 parses there and
 * neither its sample-rate code nor its sample-size code is 0; a candidate's frame ends at the first later candidate
 * at least header + 2 + channels bytes on that the frame's CRC-16 precedes, or with the input when its last two bytes
 * are that CRC-16; a candidate without an end is passed over.  Bytes in no kept frame are skipped_bytes, each maximal
 * run of them one gap.  A frame is recognised by the header behind it: damage to a frame's header also costs the frame
 * in front of it.  A whole frame that is no candidate (its header leaves the rate or the sample size to a STREAMINFO)
 * is never a record of its own, and it does not break the CRC-16 of what precedes it: the record of the frame in front
 * runs on to the next candidate, so its `bytes` spans both frames, and decode_frames gives it status bit 0.
 *   scan_frames_host  the rule on the host alone, one input, no device needed.  `frames` may be NULL (the count alone);
 *                     with cap < *n_frames nothing is written and FLACGPU_ERR_BUFFER_TOO_SMALL returned.  len == 0 is
 *                     valid (data may be NULL then): 0 frames.  stream and first_frame are 0.
 *   scan_frames       the same frames for every input of a batch, found on the device; replaces the handle's scanned
 *                     batch as scan does.  records are ordered by stream, then position; out_offset is the running sum
 *                     of block_size * channels over the batch's kept frames, *total_elements its end.  raw[i] (may be
 *                     NULL) summarises stream i.  streams[i] is filled so that decode, decode_as, plan_output,
 *                     plan_windows and decode_windows work exactly as after scan: a UNIFORM stream (frames > 0, all of
 *                     one sample rate, channel count and sample size) has rc FLACGPU_OK, info from its first frame (min /
 *                     max block over its frames), total_samples 0 and md5 all zero (an MD5 pass reports md5_status 2 with
 *                     decoded_md5 filled), bad_frames 0; a stream whose frames differ has rc FLACGPU_ERR_UNSUPPORTED,
 *                     one without a kept frame FLACGPU_ERR_INVALID_ARG, and both are absent from those calls (zero rows,
 *                     no samples).  out_offset and *total_samples lay out the uniform streams alone.
 *   frame_records     the records of the last scan_frames (cap >= *total_frames, else FLACGPU_ERR_BUFFER_TOO_SMALL).
 *   decode_frames     decodes EVERY kept frame of the batch, uniform stream or not: frame f is [block_size][channels]
 *                     interleaved int32 at out_offset, in host memory or (FLACGPU_DECODE_OUT_DEVICE, the only flag)
 *                     device memory.  records (cap entries, >= total_frames) receives the scan's records with status
 *                     filled: bit 0 the frame did not parse, bit 1 its CRC-16 is wrong; the samples of such a frame are
 *                     undefined.  A refused call (no raw scan, buffers too small, unknown flag) writes nothing.
 * decode, decode_as, decode_windows and decode_frames may follow one another in any order on one scan_frames.
 *
 * scan_frames_host_ex / scan_frames_ex take `flags`: 0 makes them the two functions above (which call them with 0), an
 * unknown flag gives FLACGPU_ERR_INVALID_ARG and nothing is written.  FLACGPU_SCAN_SPECULATIVE changes one step of the
 * rule: a candidate s that has no end by the two tests above is not passed over at once but gets its OWN EXTENT, found
 * from its own bits (DESIGN.md 4b "A frame's own extent"; csrc/kernels/frame_extent.h):
 *   window     W = min(len - s, 2^22) bytes; bit positions count from s, and a read that would pass bit 8 W means no
 *              extent.  4 MiB holds any frame of 8 channels x 65535 samples x 32 bits coded VERBATIM; a frame larger
 *              than that is not found by its own bits.
 *   subframes  from bit 8 * header_bytes(s), with n, the assignment, channels and bps of s's own header; per coded
 *              channel sbps = bps (+ 1 for the side channel: assignment 8 channel 1, 9 channel 0, 10 channel 1): a pad
 *              bit that must be 0, 6 bits of type, a wasted flag; if set, wasted = the zeros before the next 1 bit, + 1,
 *              and wasted >= sbps fails; eb = sbps - wasted.
 *   bodies     type 0: eb bits; type 1: n * eb bits; types 8-12: order = type - 8, types 32-63: order = type - 31, every
 *              other type fails; order > n fails; order * eb bits of warm-up; LPC only: 4 bits precision - 1 (precision
 *              16 fails), 5 bits of signed shift (negative fails), order * precision bits.
 *   residual   2 bits method (> 1 fails), 4 bits po; plen = n >> po, failing when plen < order or (plen << po) != n; per
 *              partition a parameter of 4 (method 0) or 5 (method 1) bits; all ones is an escape: 5 bits w, then
 *              count * w bits; otherwise count Rice codes (zeros, a 1, parameter bits); count = plen, less order in the
 *              first partition.
 *   frame end  the bits up to the next byte boundary must be 0, then 16 bits follow: e = s + pos / 8, and [s, e) is the
 *              extent if its CRC-16, stored CRC included, is 0.
 * These are the tests under which decode_frames accepts a frame, with the end unknown: a frame kept this way never gets
 * status bit 0.  It is a kept frame [s, e) like any other, the cursor moves to e, and its record has
 * FLACGPU_FRAME_SPECULATIVE in `reserved`.  A candidate that has an end by the two tests keeps that end (the whole
 * non-subset frame swallowed by the frame in front stays as described), and everything else -- candidates, minimum
 * distance, the walk, skipped_bytes, gaps, uniform -- stands.  Damage to a frame's header then costs that frame alone,
 * and the last whole frame of a byte range is kept when less than a header of the next one follows. */
#define FLACGPU_SCAN_SPECULATIVE 1u  /* scan flag: end a frame that no header ends by its own bits */
#define FLACGPU_FRAME_SPECULATIVE 1u /* flacgpu_frame_record.reserved bit 0: the frame was ended by its own bits */
typedef struct {            /* 64 bytes */
    uint64_t byte_offset;   /* first byte of the frame in its stream's input */
    uint64_t number;        /* coded frame number (blocking 0) or sample number (blocking 1) */
    uint64_t out_offset;    /* first element of the frame in decode_frames' output */
    uint32_t stream, bytes; /* input index; header .. CRC-16 inclusive */
    uint32_t block_size, sample_rate;
    uint32_t channels, bits_per_sample;
    uint32_t assignment, blocking;
    uint32_t status, reserved; /* 0 after the scan; after decode_frames bit 0: did not parse, bit 1: CRC-16 wrong;
                                * reserved: 0, or FLACGPU_FRAME_SPECULATIVE under FLACGPU_SCAN_SPECULATIVE */
} flacgpu_frame_record;
typedef struct {            /* 32 bytes */
    uint64_t first_frame;   /* index of the stream's first record */
    uint64_t skipped_bytes;
    uint32_t frames, gaps;
    uint32_t uniform;       /* 1: frames > 0 and all share sample_rate, channels, bits_per_sample */
    uint32_t reserved;
} flacgpu_raw_stream;
int flacgpu_scan_frames_host(const uint8_t *data, size_t len, flacgpu_frame_record *frames, size_t cap,
                             uint32_t *n_frames, flacgpu_raw_stream *summary);
int flacgpu_decoder_scan_frames(flacgpu_decoder *d, const uint8_t *const *data, const size_t *len, uint32_t n_streams,
                                flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                                uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples);
int flacgpu_scan_frames_host_ex(const uint8_t *data, size_t len, uint32_t flags, flacgpu_frame_record *frames, size_t cap,
                                uint32_t *n_frames, flacgpu_raw_stream *summary);
int flacgpu_decoder_scan_frames_ex(flacgpu_decoder *d, const uint8_t *const *data, const size_t *len, uint32_t n_streams,
                                   uint32_t flags, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                                   uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples);
int flacgpu_decoder_frame_records(flacgpu_decoder *d, flacgpu_frame_record *records, size_t cap);
int flacgpu_decoder_decode_frames(flacgpu_decoder *d, int32_t *out, size_t out_cap_elements, uint32_t flags,
                                  flacgpu_frame_record *records, size_t cap);

/* ---- batch decoder: frame analysis -----------------------------------------------------------------------------------
 * What every frame of a scanned batch is made of: the reference's FrameIterator / Frame / Subframe / Residuals /
 * ResidualPartition (stream.rs:1621-3079) for a whole batch in one call, as the records the encoder states its own
 * decisions in.  One lane per frame walks the frame's bits (csrc/kernels/frame_analysis.h, the same function on the host
 * and on the device) under the tests of decode_frames: status bit 0 is decode_frames' bit 0, bit 1 its bit 1.  No sample
 * is reconstructed.
 *   frames      one flacgpu_frame_analysis per frame of the scan, in the scan's order (after scan_frames: the order of
 *               the records).  `plan` is a flacgpu_frame_plan as flacgpu_analyze writes it: `assignment` is
 *               FLACGPU_ASSIGN_*, that is 0 for independent channels and the coded 8, 9, 10 otherwise, so that the plan
 *               goes into flacgpu_pack_plans as it is; the value as CODED in the header (0..10, independent channels
 *               code channels - 1) stands in `assignment_code`.  plan.block_size is block_size & 0xFFFF, body_bits the
 *               sum of the subframes' bits.
 *   subframes   the frame's subframe c at first_subframe + c, a flacgpu_subframe_plan with the meaning the encoder
 *               gives each field: type, wasted, bps (the coded width less the wasted bits; the side channel's width is
 *               the stream's + 1), order, precision / shift / coeffs[0..order) (LPC only; 0 otherwise, FIXED included),
 *               coding_method, partition_order as coded, n_partitions = 1 << partition_order, part_len = n >>
 *               partition_order, bits (exact), rice[p] (0xFF: escaped), escape_bits[p] (0: the all-zero partition),
 *               source (independent: c; 8: 0, SIDE; 9: SIDE, 1; 10: MID, SIDE).  Every entry a subframe does not use is
 *               0.  reserved[0] holds two flags:
 *                 FLACGPU_AN_WIDE          the subframe is wider than 32 bits (the 33-bit side channel of 32-bit stereo,
 *                                          SubframeWidth::Wide): its int32 row holds the low 32 bits of every value
 *                 FLACGPU_AN_PARTS_CLIPPED more than FLACGPU_MAX_PARTITIONS partitions (a foreign stream may have 2^15):
 *                                          rice[] / escape_bits[] hold the first 64; partition_order, n_partitions,
 *                                          part_len and bits stay true
 *   rows        optional, int32: channel c of a frame at row_offset + c * roundup4(block_size) (the layout of the
 *               decoder's own scratch), the row flacgpu_analyze documents: FIXED / LPC the `order` warm-up samples, then
 *               the n - order residuals as coded; VERBATIM the n samples; CONSTANT the value at [0]; all after
 *               wasted-bit removal.  Elements [n, roundup4(n)) and the rest of a CONSTANT row are unspecified.
 * A frame with status bit 0 has unspecified subframe records and rows; nothing outside its own records and rows is
 * written, whatever its bits say.
 *   analyze_frame_host   the rule on the host alone, for one frame [frame, frame + len) (len: header .. CRC-16, as a scan
 *                        gives it); no device needed.  streaminfo_bps: the sample size of a header that leaves it to the
 *                        STREAMINFO (0: none known, such a frame gets status bit 0).  subframes: 8 records.  rows64 (may
 *                        be NULL: records only) receives channel c at c * roundup4(block_size) as int64, so that a wide
 *                        subframe is exact; rows64_cap < channels * roundup4(block_size) writes nothing and returns
 *                        FLACGPU_ERR_BUFFER_TOO_SMALL.  row_offset and first_subframe are 0.
 *   plan_analysis        the sizes for the handle's scanned batch: frames, subframe records, row elements.
 *   analyze              fills the three outputs, in host memory or (FLACGPU_DECODE_OUT_DEVICE, the only flag) device
 *                        memory; rows == NULL selects the records-only pass, which stores no sample.  Works after scan,
 *                        scan_frames(_ex), the two device scans and a session's feed (that feed's frames), and may
 *                        alternate with every decode call on one scan, in any order.  A refused call (no scanned batch,
 *                        a cap too small: FLACGPU_ERR_BUFFER_TOO_SMALL, an unknown flag) writes nothing; a batch without
 *                        frames succeeds with zero counts. */
#define FLACGPU_AN_WIDE 1u
#define FLACGPU_AN_PARTS_CLIPPED 2u
typedef struct {              /* 40 bytes */
    uint64_t row_offset;      /* first int32 of the frame's rows */
    uint64_t first_subframe;  /* index of the frame's subframe 0 */
    uint32_t block_size, header_bytes;
    uint32_t status;          /* bit 0: did not parse, bit 1: CRC-16 wrong */
    uint32_t assignment_code; /* the channel assignment as coded, 0..10 */
    flacgpu_frame_plan plan;
} flacgpu_frame_analysis;
int flacgpu_analyze_frame_host(const uint8_t *frame, size_t len, uint32_t streaminfo_bps, flacgpu_frame_analysis *analysis,
                               flacgpu_subframe_plan *subframes, int64_t *rows64, size_t rows64_cap);
int flacgpu_decoder_plan_analysis(flacgpu_decoder *d, uint64_t *n_frames, uint64_t *n_subframes, uint64_t *row_elements);
int flacgpu_decoder_analyze(flacgpu_decoder *d, uint32_t flags, flacgpu_frame_analysis *frames, size_t frames_cap,
                            flacgpu_subframe_plan *subframes, size_t subframes_cap, int32_t *rows, size_t rows_cap);

/* ---- batch decoder: streams that already lie in device memory -------------------------------------------------------
 * The scans' second front door, for compressed bytes that are born or delivered in device memory: the frames
 * flacgpu_encode_device leaves there (flacgpu_device_buffer 4 and 5), a shard broadcast into every rank's GPU, a shard
 * tensor loaded onto the device.  The bytes never travel to the host: a kernel gathers them into the decoder's own
 * buffer, and only small tables come down (a regular stream's STREAMINFO, the headers of a raw stream's candidates).
 *   scan_device         = flacgpu_decoder_scan for the same bytes in host memory: every field of every streams[i] and
 *                         *total_samples.
 *   scan_frames_device  = flacgpu_decoder_scan_frames_ex for the same bytes and flags: streams, raw, the totals and every
 *                         flacgpu_frame_record.
 * The handle is then in the state the host call leaves it in, and every later call on it (decode, decode_as,
 * decode_windows, decode_frames, plan_timeline, decode_timeline) writes the same bytes and records.  The 16 GiB limit,
 * a NULL pointer or a zero length per stream, and the stream without a frame region behave as there.
 * d_data and len are HOST arrays of n_streams entries.  d_data[i] is a device pointer on the decoder's device, of any
 * alignment: views into one shard buffer are the expected use.  An entry that is NULL or has len[i] == 0 is never
 * dereferenced or looked at.  `stream` is a hipStream_t: the first read of the sources is ordered after the work queued
 * on it so far (NULL: the legacy default stream, as for flacenc_encode_many_device).  The calls are synchronous and the
 * decoder keeps its own copy: the sources may be reused or freed on return.  A handle that only sees device scans
 * allocates no pinned staging.
 * Refused with FLACGPU_ERR_INVALID_ARG before anything is launched, flacgpu_last_error naming the stream where there is
 * one: d == NULL, a missing array, an unknown flag, or an entry with bytes that hipPointerGetAttributes does not report
 * as device memory of the decoder's device (pinned host memory and managed memory are not device memory) or that
 * reaches past the end of its allocation.  A refused call leaves the handle without a scanned batch, as a failed host
 * scan does.
 *   slot_bytes      downloads the decoder's slot buffer as the last scan left it, whichever door it came through: every
 *                   stream's frame region at a 64-byte boundary, zeros up to the next one, 64 bytes of look-ahead.
 *                   *bytes is its size (0: the batch has no frame region) also when cap is short
 *                   (FLACGPU_ERR_BUFFER_TOO_SMALL, nothing written).  For tests: the two doors must build the same bytes.
 *   meta_walk_host  the metadata walk scan_device runs on the device (csrc/kernels/meta_walk.h), compiled for the host: the
 *                   return value, `info` (the STREAMINFO fields; everything else 0) and *frames_at (the first byte behind
 *                   the metadata, 0 when refused) that flacgpu_scan_stream_host gives for the metadata of the same bytes;
 *                   *min_frame is STREAMINFO's minimum frame size.  Makes no HIP call and needs no device. */
int flacgpu_decoder_scan_device(flacgpu_decoder *d, const uint8_t *const *d_data, const size_t *len, uint32_t n_streams,
                                void *stream, flacgpu_decoded_stream *streams, uint64_t *total_samples);
int flacgpu_decoder_scan_frames_device(flacgpu_decoder *d, const uint8_t *const *d_data, const size_t *len,
                                       uint32_t n_streams, uint32_t flags, void *stream, flacgpu_decoded_stream *streams,
                                       flacgpu_raw_stream *raw, uint64_t *total_frames, uint64_t *total_elements,
                                       uint64_t *total_samples);
int flacgpu_decoder_slot_bytes(flacgpu_decoder *d, uint8_t *out, size_t cap, uint64_t *bytes);
int flacgpu_meta_walk_host(const uint8_t *data, size_t len, flacgpu_stream_info *info, uint32_t *min_frame,
                           uint64_t *frames_at);

/* ---- batch decoder: sessions that take raw frame streams chunk by chunk ----------------------------------------------
 * The receiving end of flacenc_device_stream_writer, of sockets that deliver frame streams in arbitrary pieces, of a file
 * read piece by piece: n_streams RAW FRAME STREAMS (the rule above, flags 0, never FLACGPU_SCAN_SPECULATIVE), each fed in
 * chunks cut anywhere.  DESIGN.md 4b "Decoder sessions" states the rule; in short, with W = max_frame_bytes
 * (16 <= W <= 2^22) and D the concatenation of a stream's chunks so far:
 *   flush     a feed may mark a stream flushed: "what I have fed ends on a frame boundary; decide everything now, as at
 *             the end of an input".  Flushes cut D into segments; finish flushes every stream.  Within a segment the
 *             result is the raw rule applied to the segment's bytes alone, with one clause added: an end e of candidate s
 *             must have e - s <= W (a following candidate and the segment's end alike).  No frame spans a flush.
 *   online    with L bytes of the open segment fed, position q is judged once 16 bytes follow it (q <= L - 16).  A
 *             candidate's link is decided once a judged candidate ends it, or L - 16 >= s + W (it has no end: passed
 *             over).  The walk stops at the first undecided candidate c at or behind the cursor; the bytes from
 *             h = max(cursor, min(c, L - 15)) on are HELD (never more than W + 15) and are judged again, in front of the
 *             next chunk; everything before h is decided and never revisited.  So the frames are a function of the bytes
 *             and the flush positions, not of where the chunks were cut; without a flush a frame comes out one frame late
 *             (the header behind it must have arrived).
 * A session owns a decoder of its own (session_decoder): a scan call on it is refused with FLACGPU_ERR_INVALID_ARG, and
 * every decode call (decode_frames, frame_records, decode, decode_as, decode_windows, plan_timeline, decode_timeline,
 * slot_bytes) works on it, over THIS FEED's frames: a feed leaves the handle in the state scan_frames leaves it in for
 * a batch made of exactly the frames decided in the feed.  The held bytes stay in device memory: a kernel puts them in
 * front of the next chunk, in the second of two batch buffers that take turns.
 *   feed         data / len / flush are host arrays of n_streams entries; data[i] is HOST memory.  len[i] == 0 or a NULL
 *                data[i] means no bytes for stream i in this feed, any number of feeds in a row; flush may be NULL (no
 *                stream is flushed).  streams, raw and the three totals as scan_frames fills them, with these
 *                differences: flacgpu_frame_record.byte_offset counts from the stream's first byte since open;
 *                raw[i].frames, skipped_bytes and gaps are CUMULATIVE since open (a run of skipped bytes that goes on
 *                from an earlier feed, or across a flush, is one gap, counted when it opens; the held bytes are not
 *                counted yet), first_frame is the index of the stream's first record of this feed, and uniform and
 *                streams[i] describe this feed's frames alone (no frame decided in this feed: rc FLACGPU_ERR_INVALID_ARG
 *                and zero rows).  out_offset lays out this feed's frames.
 *   feed_device  the same with d_data[i] a device pointer of any alignment on the session's device, checked and ordered
 *                behind `stream` as scan_frames_device does.  Both doors run the same kernel and build the same slots.
 *   finish       flushes every stream, without new bytes; afterwards raw[i] is the whole stream's summary.  Every later
 *                feed or finish is refused.
 *   pending      held_bytes[i] (n_streams entries, may be NULL): the bytes of stream i not decided yet; *fed_bytes (may
 *                be NULL): all bytes fed to the session so far.
 * A refused call (FLACGPU_ERR_INVALID_ARG: a NULL handle or array, max_frame_bytes out of range, flags != 0, a feed after
 * finish, a device pointer that is not device memory of the session's device) writes nothing and leaves the session as
 * it was, its decoder included: the frames of the last feed can still be decoded.  So does a feed whose slots (held
 * bytes + chunks) exceed the scans' 16 GiB limit, and one that cannot allocate its layout (FLACGPU_ERR_UNSUPPORTED).
 * After a failure further on -- a HIP error, memory running out during the scan or the walk, more than 2^31 - 1 frames
 * in one feed -- the session refuses every further call.
 *   session_decoder     the handle belongs to the session and goes with session_close; flacgpu_decoder_destroy does
 *                       nothing for it.
 *   last_feed_timing    where the host's time went in the last successful feed or finish (milliseconds, wall clock):
 *                       stage_ms the argument checks and the chunks' copy into the pinned staging with the upload queued;
 *                       to_first_sync_ms from the scan's start to the end of its first synchronisation (the candidate
 *                       count: slots built and scanned on the device); to_second_sync_ms from there to the end of the
 *                       second (the candidates, links and headers downloaded); scan_rest_ms the rest of the scan call;
 *                       walk_ms the host walk with its records; table_upload_ms the frame table's upload, which ends
 *                       with a third synchronisation.  Always taken (six clock reads a feed); no switch.
 *   session_host_*      the same rule as plain host code, no device needed: the counterpart the device session is tested
 *                       against.  records (cap entries) receives this feed's records, *total_frames their count; with
 *                       cap too small FLACGPU_ERR_BUFFER_TOO_SMALL is returned, only *total_frames is written and the
 *                       session stays as it was.  raw as above; held_bytes (may be NULL) as pending gives it.
 *   session_slots_host  the per-group rule of the kernel that builds the slots (csrc/kernels/session_slots_rule.h) run
 *                       over host memory: slot i = srcs[i]'s tail, then its chunk, at a 64-byte boundary (a slot with no byte
 *                       is left out), zeros up to the next one, 64 bytes of look-ahead, as slot_bytes shows them.
 *                       *bytes is the size also when cap is short (FLACGPU_ERR_BUFFER_TOO_SMALL, nothing written). */
typedef struct flacgpu_decoder_session flacgpu_decoder_session;
typedef struct flacgpu_session_host flacgpu_session_host;
typedef struct {            /* 48 bytes */
    double stage_ms, to_first_sync_ms, to_second_sync_ms, scan_rest_ms, walk_ms, table_upload_ms;
} flacgpu_session_timing;
typedef struct {
    const uint8_t *tail;    /* the held bytes, any alignment */
    uint64_t tail_len;
    const uint8_t *chunk;   /* the new bytes, any alignment */
    uint64_t chunk_len;
} flacgpu_session_slot_src;
int flacgpu_decoder_session_open(int device, uint32_t n_streams, uint32_t max_frame_bytes, uint32_t flags,
                                 flacgpu_decoder_session **out);
int flacgpu_decoder_session_feed(flacgpu_decoder_session *s, const uint8_t *const *data, const size_t *len,
                                 const uint8_t *flush, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                                 uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples);
int flacgpu_decoder_session_feed_device(flacgpu_decoder_session *s, const uint8_t *const *d_data, const size_t *len,
                                        const uint8_t *flush, void *stream, flacgpu_decoded_stream *streams,
                                        flacgpu_raw_stream *raw, uint64_t *total_frames, uint64_t *total_elements,
                                        uint64_t *total_samples);
int flacgpu_decoder_session_finish(flacgpu_decoder_session *s, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                                   uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples);
int flacgpu_decoder_session_pending(flacgpu_decoder_session *s, uint64_t *held_bytes, uint64_t *fed_bytes);
int flacgpu_decoder_session_last_feed_timing(flacgpu_decoder_session *s, flacgpu_session_timing *out);
flacgpu_decoder *flacgpu_decoder_session_decoder(flacgpu_decoder_session *s);
void flacgpu_decoder_session_close(flacgpu_decoder_session *s);
int flacgpu_session_host_open(uint32_t n_streams, uint32_t max_frame_bytes, flacgpu_session_host **out);
int flacgpu_session_host_feed(flacgpu_session_host *s, const uint8_t *const *data, const size_t *len, const uint8_t *flush,
                              flacgpu_frame_record *records, size_t cap, flacgpu_raw_stream *raw, uint64_t *held_bytes,
                              uint64_t *total_frames);
int flacgpu_session_host_finish(flacgpu_session_host *s, flacgpu_frame_record *records, size_t cap, flacgpu_raw_stream *raw,
                                uint64_t *total_frames);
void flacgpu_session_host_close(flacgpu_session_host *s);
int flacgpu_session_slots_host(const flacgpu_session_slot_src *srcs, uint32_t n_slots, uint8_t *out, size_t cap,
                               uint64_t *bytes);

/* ---- batch decoder: container sessions -- whole .flac files chunk by chunk, MD5 across feeds ---------------------------
 * A second kind of session, chosen by its entry point: n_streams REGULAR .flac streams (fLaC marker, metadata chain,
 * frames), each fed in chunks cut anywhere -- inside the marker, a block header, STREAMINFO or a frame.  DESIGN.md 4b
 * "Container sessions" states the rule; in short, per stream:
 *   metadata  walked across feeds by the resumable form of the metadata walk (csrc/kernels/meta_feed_rule.h); nothing of
 *             the chain is buffered but the STREAMINFO block.  A wrong marker or an unusable STREAMINFO refuses the stream
 *             for good: its rc is the one-shot call's, its later bytes are counted and ignored, the other streams go on.
 *   frames    from the first byte behind the metadata the frame at the cursor s ends at the FIRST judged
 *             q >= s + max(header_bytes + 2 + channels, min_frame) where a header parses (the regular candidate test:
 *             headers that leave rate or sample size to STREAMINFO included) with s's blocking bit, CRC(s, q) == 0 and
 *             q - s <= W; at finish also at the input's end L when its last two bytes are the frame's CRC-16 and
 *             L - s <= W.  q is judged once 16 bytes follow it; s is decided once such a q exists or L - 16 >= s + W.
 *             A cursor that is no candidate, or a frame without an end, LOSES the stream: bad_frames 1, nothing from s on
 *             is kept, every later byte is dropped and counted as skipped.  There is no resynchronisation.
 *   no flush  `flush` must be NULL or all zero (FLACGPU_ERR_INVALID_ARG otherwise, nothing changes); finish alone ends
 *             the input.
 * With W no smaller than the longest frame the one-shot scan links, the frames, the samples and the final record are those
 * of flacgpu_decoder_scan + flacgpu_decoder_decode on the concatenation, however the chunks were cut.
 * After a feed the session's decoder is in the state flacgpu_decoder_scan leaves it in, for a batch whose stream i is
 * "this STREAMINFO plus the frames decided in this feed": decode, decode_as and decode_windows work on it; decode_frames,
 * frame_records, plan_timeline and decode_timeline are refused as after scan.  streams[i]: rc 0, `info` from STREAMINFO
 * with this feed's frames / decoded_samples, md5_status 3; a stream without a frame in this feed is a zero row with rc
 * FLACGPU_ERR_INVALID_ARG.  raw[i] (may be NULL): cumulative frames and skipped_bytes (bytes dropped after lost
 * synchronisation, or all bytes of a refused stream), gaps 0 or 1, uniform 1 once STREAMINFO is accepted.
 * total_frames / total_elements count this feed's frames and their samples x channels.
 * MD5: the session owns one resumable MD5 chain per stream.  The FIRST decode or decode_as after a feed without
 * FLACGPU_DECODE_NO_MD5 appends that feed's samples to the chains (on the decoder's stream, behind the kernel that wrote
 * them) and adds the call's bad_frames / bad_crc16 to the session's counts; later decodes of the same feed append nothing.
 * A feed that decided frames for a stream and was never hashed breaks that stream's chain: its final md5_status is 3.
 *   verdict   once, after finish and the decode that follows it: pads the chains and fills, per stream, the record the
 *             one-shot decode gives (rc, STREAMINFO fields, cumulative frames, decoded_samples, bad_frames, bad_crc16,
 *             decoded_md5, md5_status: 1 equal, 0 different, 2 STREAMINFO all zero, 3 chain broken).  Before finish, or
 *             twice: FLACGPU_ERR_INVALID_ARG, nothing written.  On a raw session: FLACGPU_ERR_INVALID_ARG.
 *   session_host_open_container  the rule as plain host code; feed / finish / close are session_host_*'s.  Records carry
 *             byte_offset from the stream's first byte, and STREAMINFO's rate and sample size where the header defers.
 *             raw[i].uniform && raw[i].gaps says the stream lost synchronisation.
 *   meta_feed_*_host  the resumable metadata walk over host memory on a caller-owned state of 104 bytes: init; feed
 *             (*consumed: the bytes of the chunk that belong to the metadata -- all of them until the block with the last
 *             flag ends, 0 afterwards); result: what flacgpu_meta_walk_host gives for the total_bytes fed so far seen as
 *             one input. */
typedef struct {
    uint64_t words[13];
} flacgpu_meta_feed;
int flacgpu_decoder_session_open_container(int device, uint32_t n_streams, uint32_t max_frame_bytes,
                                           flacgpu_decoder_session **out);
int flacgpu_decoder_session_verdict(flacgpu_decoder_session *s, flacgpu_decoded_stream *out);
int flacgpu_session_host_open_container(uint32_t n_streams, uint32_t max_frame_bytes, flacgpu_session_host **out);
void flacgpu_meta_feed_init_host(flacgpu_meta_feed *state);
int flacgpu_meta_feed_host(flacgpu_meta_feed *state, const uint8_t *chunk, size_t len, size_t *consumed);
int flacgpu_meta_feed_result_host(const flacgpu_meta_feed *state, uint64_t total_bytes, flacgpu_stream_info *info,
                                  uint32_t *min_frame, uint64_t *frames_at);

/* ---- batch decoder: raw frame streams on a timeline, lost frames zero-filled -----------------------------------------
 * The kept frames of every stream of a raw scan, each put where its coded number says it belongs; what no frame covers
 * is zero, and so is a frame that does not decode.  The rule (DESIGN.md 4b "Timeline"), for the records r_0 .. r_{m-1}
 * of one stream in scan order:
 *   status    rc of the stream: m == 0 FLACGPU_ERR_INVALID_ARG; records that differ in sample rate, channels or sample
 *             size, or in `blocking`, FLACGPU_ERR_UNSUPPORTED; blocking 0 with m >= 2 and B = r_0.block_size: some r_k,
 *             k < m - 1, with block_size != B, or r_{m-1}.block_size > B, FLACGPU_ERR_UNSUPPORTED (a stream whose frame
 *             numbers count frames, not time: FlacStreamWriter called with different lengths).  A refused stream is all
 *             zero in the output and the mask and does not fail the call; flacgpu_last_error names the first such
 *             stream and its reason after a call that returns FLACGPU_OK.
 *   position  p_k = number_k (blocking 1) or number_k * B (blocking 0; B = r_0.block_size), in 64 bits.
 *   walk      r_0 is PLACED, origin = p_0, end = p_0 + n_0.  For k = 1 ..: p_k < end: the frame is DROPPED (a duplicate,
 *             a re-ordered frame, a wrapped number) and not decoded; else it is PLACED at row position at_k = p_k -
 *             origin, and end = p_k + n_k.  first_sample = origin, timeline_samples = end - origin; gaps is the number
 *             of maximal runs of row positions in [0, timeline_samples) that no placed frame covers, gap_samples their
 *             sum.
 *   conceal   a placed frame whose decode_frames status would not be 0 is CONCEALED: its n_k samples are zero in every
 *             channel.  The device decides this from its own per-frame counts; the host learns it afterwards.
 *   output    FLACGPU_LAYOUT_PADDED alone: [n_streams][channels_padded][samples_padded] in fmt->dtype with decode_as's
 *             conversions.  Element [i][c][t] is the sample at at_k <= t < at_k + n_k of a placed, unconcealed frame for
 *             c < channels; every other element is zero.  mask (may be NULL): uint8 [n_streams][samples_padded], 1
 *             exactly where channel 0 holds a decoded sample.  After FLACGPU_OK every byte of out_bytes and mask_bytes
 *             is defined, whatever the buffers held before.  No MD5 is computed.
 *   timeline_host   the rule for one stream's records on the host alone (no device, no handle).  frames_out (may be
 *                   NULL; cap >= n_records, else FLACGPU_ERR_BUFFER_TOO_SMALL and nothing written) gets one entry per
 *                   record: at, flags PLACED or DROPPED, status 0 (all zero for a refused stream).  The stream's status
 *                   is result->rc; the call itself fails only for NULL arguments.
 *   plan_timeline   the checks and the sizes for the handle's last raw scan; launches nothing.  results (n_streams of
 *                   the scan) is filled first, also when the call is then refused, so that the caller sizes the tensor
 *                   from timeline_samples.  Refused: no raw scan, unknown dtype, reserved != 0, a layout other than
 *                   PADDED, samples_padded below the longest timeline_samples or channels_padded below the most channels
 *                   of an rc == 0 stream (FLACGPU_ERR_INVALID_ARG); I16 with an rc == 0 stream of more than 16 bits, S24
 *                   with one of more than 24 (FLACGPU_ERR_UNSUPPORTED, flacgpu_last_error names the stream).
 *                   *mask_bytes (may be NULL) = n_streams * samples_padded.
 *   decode_timeline plan_timeline's checks, then the decode.  flags: FLACGPU_DECODE_OUT_DEVICE alone; mask lives where
 *                   out lives.  frames (may be NULL; frames_cap >= the scan's total_frames) gets one entry per record of
 *                   the batch: timeline_host's, with FLACGPU_TL_CONCEALED and the decode_frames status of a placed
 *                   frame.  A refused call (the above, out_cap_bytes / mask_cap_bytes / frames_cap too small:
 *                   FLACGPU_ERR_BUFFER_TOO_SMALL, a misaligned out) writes nothing.  Device scratch is sized by the
 *                   placed frames.  It may follow or precede decode, decode_as, decode_windows and decode_frames on one
 *                   scan, in any order.
 * Gaps and concealed frames are zeroed on the device by runs of at most FLACGPU_TIMELINE_PIECE_BYTES bytes, one
 * workgroup each (flacgpu_timeline_piece_bytes returns the constant the library was built with). */
#define FLACGPU_TL_PLACED    1u
#define FLACGPU_TL_DROPPED   2u
#define FLACGPU_TL_CONCEALED 4u  /* with PLACED, after a decode */
#define FLACGPU_TIMELINE_PIECE_BYTES 12288u
typedef struct {            /* 16 bytes */
    uint64_t at;            /* row position of a placed frame's first sample; 0 otherwise */
    uint32_t flags;         /* FLACGPU_TL_*; 0 for every frame of a refused stream */
    uint32_t status;        /* decode_timeline, placed frames: decode_frames' status bits; else 0 */
} flacgpu_timeline_frame;
typedef struct {            /* 56 bytes */
    int32_t  rc;            /* the stream's status */
    uint32_t placed, dropped, concealed, gaps;
    uint32_t reserved;
    uint64_t first_sample;  /* origin: the position of row element 0 */
    uint64_t timeline_samples, gap_samples, concealed_samples;
} flacgpu_timeline_result;
int flacgpu_timeline_host(const flacgpu_frame_record *records, size_t n_records, flacgpu_timeline_frame *frames_out,
                          size_t cap, flacgpu_timeline_result *result);
uint32_t flacgpu_timeline_piece_bytes(void);
int flacgpu_decoder_plan_timeline(flacgpu_decoder *d, const flacgpu_out_format *fmt, flacgpu_timeline_result *results,
                                  uint64_t *out_bytes, uint64_t *mask_bytes);
int flacgpu_decoder_decode_timeline(flacgpu_decoder *d, void *out, size_t out_cap_bytes, uint8_t *mask,
                                    size_t mask_cap_bytes, const flacgpu_out_format *fmt, uint32_t flags,
                                    flacgpu_timeline_result *results, flacgpu_timeline_frame *frames, size_t frames_cap);

/* ---- the encoder's ingest pass: a device tensor -> interleaved int32 the encoder reads in place ----------------------
 * The device half of flacenc_encode_many_device (include/flacenc_stream.h), the mirror image of
 * flacgpu_decoder_decode_as: a batch of streams of one shape held in device memory as int32, int16, packed 24-bit or float32, planar and
 * padded or interleaved and flat (flacgpu_out_format describes the INPUT here), is converted and written as interleaved
 * int32 into a staging buffer the handle owns -- stream i at int32 element staging_offset (a multiple of 4: a 16-byte
 * boundary, from which flacgpu_encode_segments_device reads segments in place).  Conversion (csrc/kernels/ingest_rule.h,
 * the inverse of decode_as's): I32 clamped to bps bits; I16 x >> (16 - bps), bps <= 16; S24 (3-byte little-endian elements,
 * element e at byte 3 * e, d_pcm at any byte) sign_extend24(x) >> (24 - bps), bps <= 24; F32 x * 2^(bps - 1) rounded to
 * nearest even and clamped, NaN -> 0.  Padding (rows c >= channels, elements t >= samples, gaps between flat streams) is
 * never read.  This version always ingests; reading an aligned FLAT I32 batch in place is a follow-up.
 *   submit  runs the pass on a stream of the handle's, ordered after `stream` (a hipStream_t; NULL: the legacy default
 *           stream), and returns when the staging buffer is complete: d_pcm may be reused, *d_staging (valid until the next
 *           submit) may be read from any stream.  With FLACGPU_INGEST_MD5 the MD5 of every stream's samples as
 *           ceil(bps / 8)-byte little-endian values (k_md5_many, one lane per stream: about 15 MB/s per stream, fine for
 *           many clips and poor for one long stream) is queued behind it and runs beside whatever the caller does next.
 *   finish  waits for it; altered[i] (may be NULL) = elements of stream i that were clamped, NaN or (I16, S24) lost non-zero
 *           low bits; md5 (may be NULL; [n_streams][16]) is written only when the MD5 was asked for.
 * The arguments are the ones flacenc_device_batch_plan validates; submit repeats the checks its kernel's bounds rest on. */
#define FLACGPU_INGEST_MD5 1u
typedef struct flacgpu_ingest flacgpu_ingest;
typedef struct {
    uint64_t in_offset;        /* FLAT: first element of the stream in d_pcm; PADDED: ignored (stream i is block i) */
    uint64_t samples;          /* per channel */
    uint64_t staging_offset;   /* first int32 of the stream in the staging buffer, a multiple of 4 */
} flacgpu_ingest_stream;
int flacgpu_ingest_create(int device, flacgpu_ingest **out);
void flacgpu_ingest_destroy(flacgpu_ingest *g);
int flacgpu_ingest_device(const flacgpu_ingest *g);
int flacgpu_ingest_submit(flacgpu_ingest *g, const void *d_pcm, const flacgpu_out_format *fmt, uint32_t bits_per_sample,
                          uint32_t channels, const flacgpu_ingest_stream *streams, uint32_t n_streams,
                          uint64_t staging_elements, uint32_t flags, void *stream, int32_t **d_staging);
int flacgpu_ingest_finish(flacgpu_ingest *g, uint32_t *altered, uint8_t *md5);
/* Small host-built pieces (the streams' headers) to their places in device memory, for flacenc_encode_many_device_out:
 *   scratch  *pinned = a pinned host buffer of the handle's that holds at least `bytes` bytes (valid until the next
 *            scratch call), for the caller to fill;
 *   place    uploads its first `bytes` bytes in ONE copy into device scratch the handle keeps, then ONE k_place_runs launch
 *            copies run i's n bytes from byte `src` of that scratch to the device address `dst` (exactly [dst, dst + n) is
 *            written), on the handle's stream; returns when the copies are complete.  FLACGPU_ERR_INVALID_ARG when a
 *            run reaches past `bytes`. */
int flacgpu_ingest_scratch(flacgpu_ingest *g, size_t bytes, uint8_t **pinned);
int flacgpu_ingest_place(flacgpu_ingest *g, size_t bytes, const flacgpu_place_run *runs, uint32_t n_runs);
/* Device-to-device runs for flacenc_device_session_write (the carried samples of every stream to the staging buffer's
 * other half): ONE k_place_runs launch over `runs`, whose src and dst are both device ADDRESSES (exactly [dst, dst + n) is
 * written, [src, src + n) read; no run's source may overlap any run's destination), on the handle's stream; returns when
 * the copies are complete.  The caller orders it behind whatever still reads the destinations. */
int flacgpu_ingest_move(flacgpu_ingest *g, const flacgpu_place_run *runs, uint32_t n_runs);
/* The handle's stream (a hipStream_t), for work that must run in order with the handle's own. */
void *flacgpu_ingest_stream_of(flacgpu_ingest *g);

/* ---- resumable MD5 chains: a stream's MD5 taken piece by piece, on the device ------------------------------------------
 * k_md5_many starts every chain from the initial state and pads at the end of its call; these chains keep {h[4], the
 * 64-bit byte length, up to 63 buffered message bytes} per chain in device memory between calls, so that a stream can be
 * hashed in as many pieces as it arrives in (flacenc_device_session_write).  The rule -- how a piece's samples and the
 * buffered bytes become 64-byte blocks, what stays buffered, the padding -- is csrc/kernels/md5_feed_rule.h, one set of
 * functions for both sides; the kernel (csrc/kernels/md5_chain.inc, one wave per piece) loads a window of
 * flacgpu_md5_stage_bytes() message bytes with coalesced 16-byte loads, parks its blocks in LDS, and one lane consumes them.
 *   create   n_chains chains at the initial state, on `device` (< 0: the current one).
 *   update   piece p appends `count` int32 samples, from element `off` of d_samples, to chain `chain`; every sample gives
 *            its low `width` bytes, little-endian (what k_md5_many reads).  Asynchronous on `stream` (a hipStream_t; NULL:
 *            the legacy default stream); every call on one handle must use one stream, or streams the caller has ordered.
 *            At most one piece per chain and call (a chain is serial).  A duplicate chain, a chain >= n_chains, reserved
 *            != 0, a count above 2^58 or a width outside 1..4: FLACGPU_ERR_INVALID_ARG, nothing launched, no state
 *            changed.  count == 0 changes nothing.  No byte of d_samples outside a piece's [off, off + count) is read.
 *   final    pads every chain, downloads the digests (md5_out: [n_chains][16]) and leaves every chain at the initial
 *            state; ordered after every update so far; synchronous.  A chain never fed: the MD5 of the empty message.
 * flacgpu_md5_init_host / feed_host / final_host run the same rule over host memory on a caller-owned state; they touch
 * no device.  final_host leaves the state initial again. */
typedef struct flacgpu_md5_chains flacgpu_md5_chains;
typedef struct {
    uint32_t chain, reserved;
    uint64_t off, count;
} flacgpu_md5_piece;
typedef struct {
    uint32_t h[4];
    uint64_t len;
    uint8_t buf[64];
} flacgpu_md5_state;
int flacgpu_md5_chains_create(int device, uint32_t n_chains, flacgpu_md5_chains **out);
void flacgpu_md5_chains_destroy(flacgpu_md5_chains *c);
int flacgpu_md5_chains_update(flacgpu_md5_chains *c, const int32_t *d_samples, const flacgpu_md5_piece *pieces,
                              uint32_t n_pieces, uint32_t width, void *stream);
int flacgpu_md5_chains_final(flacgpu_md5_chains *c, uint8_t *md5_out);
uint32_t flacgpu_md5_stage_bytes(void);
void flacgpu_md5_init_host(flacgpu_md5_state *state);
int flacgpu_md5_feed_host(flacgpu_md5_state *state, const int32_t *samples, uint64_t count, uint32_t width);
int flacgpu_md5_final_host(flacgpu_md5_state *state, uint8_t md5[16]);

/* EXPERIMENT, not on the product path: recomputes the autocorrelation of the last analysed
 * batch on the f64 matrix cores (v_mfma_f64_16x16x4_f64, block-Gram form), times that kernel,
 * reruns Levinson/quantisation on it and reports how many candidates' quantised LPC parameters
 * (order, shift, coefficients) differ from the exact-summation-order path, and the largest
 * relative error of an autocorrelation lag.  The context's exact results are restored.
 * Requires full blocks and 1 <= max_lpc_order <= 16. */
int flacgpu_experiment_mfma_autocorr(flacgpu_ctx *ctx, float *kernel_ms, uint32_t *compared,
                                     uint32_t *params_differ, double *max_rel_err);

/* Duration in milliseconds of each kernel of the last analyze call, measured with HIP events
 * on the launch stream (names via flacgpu_kernel_name).  Requires flacgpu_set_timing(ctx, 1). */
#define FLACGPU_N_KERNELS 12
int flacgpu_set_timing(flacgpu_ctx *ctx, int enable);
int flacgpu_get_kernel_ms(flacgpu_ctx *ctx, float ms[FLACGPU_N_KERNELS]);
const char *flacgpu_kernel_name(int index);

/* Identity of this build: the first 16 hex digits of the SHA-256 over the library's sources (every file under
 * csrc/ but build/, in sorted path order: csrc/Makefile `BUILD_ID`).  Counter collections under profiles/ carry the
 * id of the library they were taken with; bench.py prints `counters_stale` when it differs from the running one. */
const char *flacgpu_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
