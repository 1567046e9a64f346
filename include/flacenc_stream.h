/*
 * flacenc_stream.h -- C ABI of the host-side stream writers.
 *
 * Mirrors the public encode surface of the reference (tuffy/flac-codec 1.3.2):
 *   encode::Options                    /root/reference/src/encode.rs:1361-1672
 *   FlacSampleWriter::{new,write,finalize}           encode.rs:487, 558, 624
 *   FlacByteWriter::{new,write(io::Write),finalize}  encode.rs:143, 359, 258
 *   FlacChannelWriter::{new,write,finalize}          encode.rs:769, 832, 939
 *   FlacStreamWriter::{new,write}                    encode.rs:1094, 1142
 * Same argument meaning and the same error conditions (the FLACENC_ERR_* values
 * name the reference's `Error` / `OptionsError` variants, src/lib.rs:59-193,
 * encode.rs:1676-1698).  The per-frame analysis is done by the gfx950 kernels
 * behind include/flacenc_gpu.h; this layer does what stays on the host in the
 * reference's design: block buffering, MD5, frame headers, Rice bit-packing,
 * CRC-8/16, seek points and the metadata rewrite at finalize
 * (Encoder::new / encode / finalize_inner, encode.rs:1882-2110).
 *
 * Frames are analysed in batches (`batch_frames`), so a `write` may emit its
 * frames later than the reference would (at the latest at finalize); the bytes
 * are identical.
 */
#ifndef FLACENC_STREAM_H
#define FLACENC_STREAM_H

#include <stddef.h>
#include <stdint.h>

#include "flacenc_gpu.h" /* flacgpu_out_format, FLACGPU_SAMPLE_*, FLACGPU_LAYOUT_* (flacenc_encode_many_device) */

#ifdef __cplusplus
extern "C" {
#endif

enum {
    FLACENC_OK = 0,
    /* OptionsError, encode.rs:1676-1698 */
    FLACENC_ERR_INVALID_BLOCK_SIZE = -101,
    FLACENC_ERR_INVALID_LPC_ORDER = -102,
    FLACENC_ERR_INVALID_MAX_PARTITIONS = -103,
    FLACENC_ERR_EXCESSIVE_PADDING = -104,
    /* Error, src/lib.rs:59-193 */
    FLACENC_ERR_INVALID_BITS_PER_SAMPLE = -110,        /* encode.rs:495 */
    FLACENC_ERR_INVALID_SAMPLE_RATE = -111,            /* encode.rs:1902 */
    FLACENC_ERR_EXCESSIVE_CHANNELS = -112,             /* encode.rs:1908 */
    FLACENC_ERR_SAMPLES_NOT_DIVISIBLE_BY_CHANNELS = -113, /* encode.rs:517 */
    FLACENC_ERR_INVALID_TOTAL_SAMPLES = -114,          /* encode.rs:518 */
    FLACENC_ERR_INVALID_TOTAL_BYTES = -115,            /* encode.rs:177 */
    FLACENC_ERR_EXCESSIVE_TOTAL_SAMPLES = -116,        /* encode.rs:1913, 2010, 2094 */
    FLACENC_ERR_SAMPLE_COUNT_MISMATCH = -117,          /* encode.rs:2083 */
    FLACENC_ERR_NO_SAMPLES = -118,                     /* encode.rs:2090 */
    FLACENC_ERR_EXCESSIVE_FRAME_NUMBER = -119,         /* stream.rs:1235 */
    FLACENC_ERR_CHANNEL_COUNT_MISMATCH = -120,         /* encode.rs:858 */
    FLACENC_ERR_CHANNEL_LENGTH_MISMATCH = -121,        /* encode.rs:854 */
    FLACENC_ERR_NON_SUBSET_SAMPLE_RATE = -122,         /* encode.rs:1181 */
    FLACENC_ERR_NON_SUBSET_BITS_PER_SAMPLE = -123,     /* encode.rs:1151, 1187 */
    FLACENC_ERR_IO = -130,
    /* not reference errors */
    FLACENC_ERR_INVALID_ARG = -140,
    FLACENC_ERR_FINALIZED = -141,
    FLACENC_ERR_GPU = -150,          /* flacgpu_* failed; flacenc_last_error() has the text */
    FLACENC_ERR_UNSUPPORTED = -151   /* legal upstream, not in this build (see flacenc_gpu.h) */
};

enum { FLACENC_SEEKTABLE_NONE = 0, FLACENC_SEEKTABLE_SECONDS = 1, FLACENC_SEEKTABLE_FRAMES = 2 };

/* encode::Options (encode.rs:1363-1374).  Metadata beyond STREAMINFO / SEEKTABLE /
 * PADDING / VORBIS_COMMENT is out of scope. */
typedef struct {
    uint32_t block_size;          /* Options::block_size, >= 16 (encode.rs:1418) */
    uint32_t max_partition_order; /* 0..=15 (encode.rs:1447) */
    uint32_t max_lpc_order;       /* 0 = None, 1..=32 (encode.rs:1430) */
    uint8_t mid_side;             /* encode.rs:1460 */
    uint8_t exhaustive_channel_correlation; /* !fast_channel_correlation (encode.rs:1472) */
    uint8_t window_kind;          /* 0 Rectangle, 1 Hann, 2 Tukey (encode.rs:1713) */
    uint8_t reserved0;
    float window_param;
    int64_t padding;              /* PADDING bytes; 0 removes the block (encode.rs:1486-1508) */
    int32_t seektable_mode;       /* FLACENC_SEEKTABLE_* (encode.rs:1568-1590) */
    uint32_t seektable_value;     /* seconds (u8) or frames */
    /* execution knobs (no reference equivalent) */
    uint32_t batch_frames;        /* FLAC frames analysed per GPU call; 0 = default (256: small enough that a stream's first batch reaches the MD5 thread and the GPU within ~2 ms) */
    int32_t device;               /* HIP device ordinal, -1 = current */
    uint32_t pack_threads;        /* host bit-pack threads; 0 = default */
    uint32_t host_pack;           /* 0: frames are assembled on the GPU (k_layout/k_pack/k_crc);
                                     1: Rice bit-packing + CRC stay on the host, as in the
                                     north-star split (same bytes either way) */
    /* VORBIS_COMMENT (Options::tag / Options::comment, encode.rs:1513-1528).  n_comment_fields
     * == 0 and vendor_string == NULL: no block.  Fields are "NAME=value" strings; a NULL
     * vendor_string with fields present means VorbisComment::default()'s "flac-codec 1.3.2"
     * (metadata/mod.rs:2225-2232).  The pointers are only read during *_writer_new. */
    const char *vendor_string;
    const char *const *comment_fields;
    uint32_t n_comment_fields;
    uint32_t pipeline_depth;      /* batches in flight per writer (device-side frame assembly): each on
                                     a context, HIP stream and pinned staging buffers of its own, so
                                     that upload, kernels, download and the MD5 of neighbouring
                                     batches overlap; 0 = default (2), at most 4 */
    uint32_t shared_md5;          /* 1: the stream's MD5 chain runs on the shared multi-stream engines
                                     (host/md5_mb.h: up to 16 streams per engine thread, one per AVX-512
                                     lane) instead of on a worker thread of its own -- for callers that
                                     encode many streams side by side; flacenc_encode_many sets it */
} flacenc_options;

void flacenc_options_default(flacenc_options *o); /* Options::default(), encode.rs:1376-1408 */
void flacenc_options_fast(flacenc_options *o);    /* Options::fast(),    encode.rs:1635-1644 */
void flacenc_options_best(flacenc_options *o);    /* Options::best(),    encode.rs:1649-1657 */
/* validation of the setters (returns the OptionsError the reference's builder would) */
int flacenc_options_validate(const flacenc_options *o);

/* Output sink = the reference's `W: Write + Seek`.  `seek` is only used by finalize
 * (rewind to the stream start to rewrite the metadata, encode.rs:2104-2106).
 * Return 0 on success. */
typedef int (*flacenc_write_fn)(void *user, const uint8_t *data, size_t len);
typedef int (*flacenc_seek_fn)(void *user, uint64_t absolute_offset);
typedef struct {
    flacenc_write_fn write;
    flacenc_seek_fn seek;
    void *user;
    uint64_t start; /* writer.stream_position() at creation (encode.rs:1941) */
} flacenc_sink;

typedef struct flacenc_writer flacenc_writer;

/* FlacSampleWriter::new (encode.rs:487).  has_total = 0 is `None`; total_samples counts
 * ALL channels like the reference (must divide by channels).  sink == NULL collects the
 * stream in memory (see flacenc_writer_data). */
int flacenc_sample_writer_new(const flacenc_options *opts, uint32_t sample_rate,
                              uint32_t bits_per_sample, uint32_t channels, int has_total,
                              uint64_t total_samples, const flacenc_sink *sink,
                              flacenc_writer **out);
/* FlacByteWriter::new (encode.rs:143); total_bytes like the reference. */
int flacenc_byte_writer_new(const flacenc_options *opts, uint32_t sample_rate,
                            uint32_t bits_per_sample, uint32_t channels, int has_total,
                            uint64_t total_bytes, int big_endian, const flacenc_sink *sink,
                            flacenc_writer **out);
/* FlacChannelWriter::new (encode.rs:769); total_samples is per channel. */
int flacenc_channel_writer_new(const flacenc_options *opts, uint32_t sample_rate,
                               uint32_t bits_per_sample, uint32_t channels, int has_total,
                               uint64_t total_samples, const flacenc_sink *sink,
                               flacenc_writer **out);

/* FlacSampleWriter::write (encode.rs:558): interleaved samples, any count. */
int flacenc_write_samples(flacenc_writer *w, const int32_t *samples, size_t count);
/* FlacByteWriter's io::Write::write (encode.rs:359): PCM bytes, any count. */
int flacenc_write_bytes(flacenc_writer *w, const uint8_t *bytes, size_t count);
/* FlacChannelWriter::write (encode.rs:832): n_channels arrays of `len` samples. */
int flacenc_write_channels(flacenc_writer *w, const int32_t *const *channels, uint32_t n_channels,
                           size_t len);
/* finalize (encode.rs:624 / 258 / 939): flush the last partial block, update SEEKTABLE,
 * STREAMINFO (sizes, total samples, MD5) and rewrite the metadata.  Idempotent. */
int flacenc_finalize(flacenc_writer *w);
/* Drop (encode.rs:399, 2113): finalizes, swallowing errors, then frees. */
void flacenc_writer_free(flacenc_writer *w);

/* memory sink access (sink == NULL at creation) */
const uint8_t *flacenc_writer_data(flacenc_writer *w, size_t *len);

/* Batch front end: many independent streams encoded concurrently by `threads` host workers (0 =
 * default), each one FlacSampleWriter::new(total known) / write / finalize (encode.rs:487, 558, 624)
 * with the .flac bytes written to the job's own buffer (FLACENC_ERR_IO in `status` when it is too
 * small; flacenc_worst_case_bytes() is always enough: every frame VERBATIM at bps + 1 bits with its headers, one seek
 * point per frame, the metadata blocks).  The workers share the
 * GPU through the pooled analysis lanes; every stream's MD5 chain runs on a thread of its own.
 * Returns 0 or the first job's error. */
/* Upper bound of the .flac size of a stream of `pcm_frames` samples per channel under `opts`. */
size_t flacenc_worst_case_bytes(const flacenc_options *opts, uint32_t bits_per_sample, uint32_t channels,
                                uint64_t pcm_frames);
typedef struct {
    const int32_t *samples;   /* interleaved, the whole stream */
    size_t count;             /* samples over all channels */
    uint32_t sample_rate, bits_per_sample, channels;
    uint32_t reserved;
    uint8_t *out;             /* caller-owned output buffer */
    size_t out_cap;
    size_t out_len;           /* out: bytes of the finished stream */
    int32_t status;           /* out: FLACENC_OK or the error of this stream */
    int32_t reserved1;
    /* out, diagnostics: wall time of this stream from its first phase to its last, and inside it the staging
     * (sample packing), the GPU calls incl. waiting for results, and the MD5 thread's busy time */
    double elapsed_ms, pack_ms, gpu_ms, md5_ms, start_ms;
} flacenc_job;
/* `threads` workers (0: half the hardware threads) share the streams' three phases -- first blocks, remaining samples,
 * finish --, at most 64 streams open at a time: the thread count need not match the stream count (a few threads per
 * usable CPU are enough), every stream's MD5 chain starts at once.  Returns the first failing stream's status. */
int flacenc_encode_many(const flacenc_options *opts, flacenc_job *jobs, size_t n_jobs, uint32_t threads);
/* The same over several GPUs of one process: stream i is encoded whole on devices[i mod n_devices] (streams are independent:
 * one `Encoder` per file in the reference, encode.rs:1882-1980 -- the natural shard; nothing crosses devices).  devices ==
 * NULL with n_devices == FLACENC_ALL_DEVICES: every visible device; NULL / 0: opts->device as flacenc_encode_many.  An
 * ordinal may be listed more than once.  Output is byte-identical to flacenc_encode_many's. */
/* The same with the streams of one shape (sample rate, bits per sample, channels) SHARING analysis batches: runs of whole
 * blocks of several streams form one batch (every frame with its own stream's frame number), and the batches travel through
 * a ring of pinned staging buffers -- samples packed to the stream's width on the way in (2 or 3 bytes across PCIe; the packed
 * bytes are what the MD5 lanes hash), upload of batch i + 1, kernels of batch i and the frames of batch i - 1 in flight
 * together, frames copied once from the pinned ring to `out`.  A library of short files runs at the per-sample rate of large
 * batches (a 256-frame batch of 24-bit stereo on its own: 0.3 of it), long streams at the link's.  A stream's short last
 * block is encoded by a one-frame call, its metadata is rebuilt from the frame sizes (flacenc_stream_header).  Output
 * byte-identical to flacenc_encode_many's, stream by stream (csrc/host/coalesce.cpp; measured: DESIGN.md section 6). */
int flacenc_encode_many_coalesced(const flacenc_options *opts, flacenc_job *jobs, size_t n_jobs, uint32_t threads);
/* Frees what the front ends keep between calls: idle analysis contexts and their pinned staging buffers (the writers' lane
 * pool, the coalescing ring).  Contexts in use are not touched. */
void flacenc_release_pools(void);
#define FLACENC_ALL_DEVICES 0xFFFFFFFFu
int flacenc_encode_many_devices(const flacenc_options *opts, flacenc_job *jobs, size_t n_jobs, uint32_t threads,
                                const int *devices, uint32_t n_devices);

/* ---- a batch of streams RESIDENT IN DEVICE MEMORY -> finished .flac files, without a host copy of the samples --------
 * The mirror image of flacgpu_decoder_decode_as (include/flacenc_gpu.h): `d_pcm` is a device tensor of int32, int16,
 * packed 24-bit (FLACGPU_SAMPLE_S24: 3 bytes per element, little-endian, element e at byte 3 * e, no alignment) or float32
 * elements holding n_jobs streams of one shape (sample rate, bits per sample, channels), laid out as `fmt` says
 * (FLACGPU_SAMPLE_* / FLACGPU_LAYOUT_* as in the decoder; the format describes the INPUT here):
 *   PADDED  [n_jobs][channels_padded][samples_padded], planar; of stream i only the first `channels` rows and the first
 *           jobs[i].samples elements of each are read -- padding may hold anything;
 *   FLAT    stream i is [samples][channels] interleaved from element jobs[i].in_offset; the streams must not overlap,
 *           what lies between them is never read.
 * Conversion to bits_per_sample-bit samples (csrc/kernels/ingest_rule.h, the exact inverse of decode_as's; testable on
 * the host through flacenc_ingest_sample): I32 the value clamped to [-2^(bps-1), 2^(bps-1) - 1]; I16 x >> (16 - bps),
 * bps <= 16 only; S24 sign_extend24(x) >> (24 - bps), bps <= 24 only; F32 x * 2^(bps-1) rounded to nearest even, clamped, NaN -> 0.  jobs[i].altered counts the elements of
 * stream i that were clamped, were NaN or (I16, S24) had non-zero bits below the ones kept.
 * What happens: one ingest pass writes interleaved int32 into a staging buffer of the library's (staging_bytes = 4 x the
 * sum over the streams of samples x channels rounded up to 4; this version always ingests -- reading an aligned FLAT I32
 * batch in place is a follow-up); the MD5 of every stream is taken on the device (k_md5_many: one lane per stream, about
 * 15 MB/s per stream -- fine for many clips, poor for one long stream; FLACENC_DEVICE_NO_MD5 is the way round it in this
 * call, and the sessions below hash with the staged resumable chain of flacgpu_md5_chains_*); runs of whole blocks of several streams go through
 * flacgpu_encode_segments_device in batches planned as flacenc_encode_many_coalesced plans them, on two pooled contexts in
 * rotation (one batch's kernels run while the other's frames travel to pinned memory); a stream's short last block is a
 * one-frame flacgpu_encode_device call on the staging buffer; everything in front of the first frame is
 * flacenc_stream_header's; every output byte is copied once, from pinned memory to jobs[i].out.
 * Output byte-identical to flacenc_encode_many's on the converted samples, stream by stream; a stream without samples
 * gets FLACENC_ERR_INVALID_ARG in its status, as there; an `out` too small FLACENC_ERR_IO in that job's status, the other
 * streams unaffected.  Synchronous: `d_pcm` may be reused when the call returns.  The ingest is ordered after `stream` (a
 * hipStream_t; NULL: the legacy default stream, the rule of flacgpu_analyze_device).  opts->device < 0: the current device;
 * d_pcm must live on that device.
 * plan is pure host code (no device): it validates the call -- FLACENC_ERR_INVALID_ARG for channels_padded < channels, a
 * stream longer than samples_padded, FLAT streams that overlap, channels outside 1..8, bits_per_sample outside 1..32, an
 * unknown type or layout, reserved != 0, padded fields under FLAT; FLACENC_ERR_UNSUPPORTED for I16 with more than 16
 * bits or S24 with more than 24 -- and returns the elements d_pcm must hold (S24: 3-byte elements) and the staging bytes.  encode runs the same checks first: a refused
 * call launches nothing and writes nothing (no job field, no output byte).  Returns 0 or the first failing job's status. */
typedef flacgpu_out_format flacenc_tensor_format;   /* the decoder's format record under a direction-neutral name */
typedef struct {
    uint64_t in_offset;      /* FLAT: first element of the stream; PADDED: ignored */
    uint64_t samples;        /* per channel */
    uint8_t *out;            /* caller-owned host buffer for the finished .flac */
    size_t out_cap, out_len;
    int32_t status;          /* FLACENC_OK or this stream's error */
    uint32_t altered;
    uint8_t md5[16];         /* what went into STREAMINFO */
} flacenc_device_job;
#define FLACENC_DEVICE_NO_MD5 1u   /* STREAMINFO MD5 all zero ("unknown"); no hash kernel, no digest download */
int flacenc_device_batch_plan(const flacenc_options *opts, const flacenc_tensor_format *fmt, uint32_t bits_per_sample,
                              uint32_t channels, const flacenc_device_job *jobs, size_t n_jobs, size_t *in_elements,
                              size_t *staging_bytes);
int flacenc_encode_many_device(const flacenc_options *opts, const void *d_pcm, const flacenc_tensor_format *fmt,
                               uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels, flacenc_device_job *jobs,
                               size_t n_jobs, uint32_t flags, void *stream);
/* ---- ... and the finished .flac files left in DEVICE memory too (DESIGN.md 4c "Device-resident output") ----
 * flacenc_encode_many_device with a back door: stream i's file goes to bytes [out_offset, out_offset + out_cap) of `d_out`,
 * its SLOT, in device memory (on the tensor's device); only frame sizes, digests and the streams' headers cross the link.
 * The slots may start at any byte, come in any order and leave gaps; two slots that hold bytes (out_cap > 0) must not overlap.
 * A stream with status == 0 occupies [out_offset, out_offset + out_len) with exactly the bytes flacenc_encode_many_device
 * writes for the same tensor, options and flags; status, altered and md5 are that call's too (a stream without samples:
 * FLACENC_ERR_INVALID_ARG; a slot smaller than the header, or one the frames overflow: FLACENC_ERR_IO in that job's status,
 * the other streams unaffected).  A failed stream's slot holds undefined bytes.  No byte of d_out outside the slots is ever
 * written, and no byte of a slot behind out_len for a stream that succeeded: the frames are placed by k_place_runs
 * (csrc/kernels/place_rule.h: 16-byte stores for whole aligned groups, byte stores at a run's edges), batch by batch beside
 * the next batch's analysis, and the headers -- built on the host once the digests are there -- go up in one copy and to
 * their places in one launch of the same kernel.  Synchronous: the files are complete when the call returns, and d_pcm may
 * be reused; the work is ordered after `stream` as in flacenc_encode_many_device.
 * plan is pure host code: flacenc_device_batch_plan's checks, and FLACENC_ERR_INVALID_ARG for a slot that reaches past
 * d_out_bytes, out_offset + out_cap overflowing, or two slots with out_cap > 0 that overlap.  encode runs the same checks
 * first: a refused call launches nothing and writes nothing. */
typedef struct {
    uint64_t in_offset, samples;   /* as flacenc_device_job */
    uint64_t out_offset, out_cap;  /* the stream's slot: bytes [out_offset, out_offset + out_cap) of d_out */
    uint64_t out_len;              /* out */
    int32_t status;
    uint32_t altered;
    uint8_t md5[16];
} flacenc_device_out_job;
int flacenc_device_out_plan(const flacenc_options *opts, const flacenc_tensor_format *fmt, uint32_t bits_per_sample,
                            uint32_t channels, const flacenc_device_out_job *jobs, size_t n_jobs, size_t d_out_bytes,
                            size_t *in_elements, size_t *staging_bytes);
int flacenc_encode_many_device_out(const flacenc_options *opts, const void *d_pcm, const flacenc_tensor_format *fmt,
                                   uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels,
                                   flacenc_device_out_job *jobs, size_t n_jobs, void *d_out, size_t d_out_bytes, uint32_t flags,
                                   void *stream);
/* ---- ... and the same batch taken CHUNK BY CHUNK: sessions (DESIGN.md 4c "Sessions") ---------------------------------------
 * flacenc_encode_many_device needs every stream whole; a session takes n_streams streams of one shape in as many writes as
 * the samples come into being in, as FlacSampleWriter::write / finalize do for one stream on the host (encode.rs:487, 558,
 * 624).  The contract: for every stream that succeeds,
 *     header || frames of write 1 || ... || frames of write k || tail
 * is byte for byte the file flacenc_encode_many_device writes for the concatenated samples with the same options and
 * flags, and md5 and altered are that call's too.
 *   plan      pure host code: refuses what flacenc_device_batch_plan refuses for the shape (options, channels, bits per
 *             sample, stream count), max_chunk == 0 and unknown flags; *device_bytes = what the session holds in device
 *             memory for its whole life: a staging buffer of two halves, in each of which stream i owns room for
 *             block_size - 1 carried samples and a chunk of max_chunk (both rounded up to 16 bytes), and 128 bytes of MD5
 *             chain state and tables per stream.  (The analysis contexts are the pooled ones of the one-shot calls.)
 *   open      totals[i] = stream i's length per channel, declared now: everything in front of the first frame then has
 *             its final size (flacenc_stream_header builds it at finalize), as for FlacSampleWriter::new with a known
 *             total.  totals[i] == 0 (FLACENC_ERR_INVALID_ARG) or a total / option the reference's `new` refuses makes
 *             stream i dead from the start; the session opens for the others.  flags: FLACENC_DEVICE_NO_MD5.
 *   header_len  bytes in front of stream i's first frame (0 for a stream dead at open).
 *   write     chunks[i] = the next `samples` samples per channel of stream i (0: none this time) in `d_pcm`, which `fmt`
 *             describes exactly as for flacenc_encode_many_device with jobs[i] = {in_offset, samples}; type and layout may
 *             differ from write to write.  The chunks are ingested, the MD5 chains fed (flacgpu_md5_chains_update, beside
 *             the analysis), every block that the carried samples and the chunk complete is encoded, and those frames go,
 *             in order, to chunks[i].out (host memory; out_len = their size, 0 when no block was completed; altered = this
 *             chunk's count).  Synchronous: d_pcm may be reused on return.  Refused as a whole with
 *             FLACENC_ERR_INVALID_ARG -- nothing launched, no chunk field written, the session unchanged -- for a chunk
 *             longer than max_chunk, a chunk that would pass its stream's total, or anything flacenc_device_batch_plan
 *             refuses for this tensor.  An `out` too small for this write's frames: FLACENC_ERR_IO in that chunk's status,
 *             and the stream is dead: its later chunks are ignored and get the same status; the others are unaffected.
 *             Returns 0 when the call ran -- every stream's own outcome is in its chunk's status -- or the refusal.
 *   finalize  every stream's short last block (one-frame path) to finals[i].tail, everything in front of the first frame
 *             to finals[i].header; altered = the sum over all writes.  A stream that has not received its total:
 *             FLACENC_ERR_SAMPLE_COUNT_MISMATCH (encode.rs:2083), nothing written for it.  header_cap or tail_cap too
 *             small: FLACENC_ERR_IO.  Returns 0 or the first failing stream's status.  A second finalize, and a write
 *             after finalize: FLACENC_ERR_FINALIZED.
 *   close     frees everything; legal at any time, also on NULL.
 *   open_ex   open with `total_known`, one entry per stream, for streams whose length is NOT known when they start (a
 *             generative model's steps, a capture loop).  total_known == NULL is open, exactly.  total_known[i] == 0:
 *             stream i has no declared total and totals[i] is ignored (totals may be NULL when no stream has one); known
 *             and unknown streams mix freely.  Such a stream is FlacSampleWriter::new(.., None) (encode.rs:1909-1939):
 *             header_len is the size without a placeholder SEEKTABLE, and stays that at finalize, where the seek table is
 *             carved out of the PADDING block when it fits (encode.rs:2029-2076); write has no "passes the declared total"
 *             refusal; finalize gives FLACENC_ERR_NO_SAMPLES (encode.rs:2090) for a stream that never received a sample,
 *             nothing written for it, FLACENC_ERR_EXCESSIVE_TOTAL_SAMPLES at 2^36 samples or more, and otherwise builds
 *             the header with total = the samples received (flacenc_stream_header_unknown_total).  Frames, tail, md5
 *             and altered are a known-total stream's.  The contract: header || frames of every write || tail is byte for
 *             byte the file of flacenc_sample_writer_new(.., has_total = 0, ..) fed the same samples.
 *             FLACENC_ERR_SAMPLE_COUNT_MISMATCH remains a known-total stream's error.
 * A GPU error in any call is sticky: every later write and finalize returns it.  A session is not thread-safe; several
 * sessions, and one-shot calls beside them, do not disturb one another, nor does flacenc_release_pools(). */
typedef struct flacenc_device_session flacenc_device_session;
typedef struct {
    uint64_t in_offset;      /* FLAT: first element of the chunk in d_pcm; PADDED: ignored */
    uint64_t samples;        /* per channel, <= max_chunk; 0: nothing for this stream */
    uint8_t *out;            /* caller-owned host buffer for the frames this write completes */
    size_t out_cap, out_len;
    int32_t status;
    uint32_t altered;
} flacenc_session_chunk;
typedef struct {
    uint8_t *header;         /* caller-owned host buffers */
    size_t header_cap, header_len;
    uint8_t *tail;
    size_t tail_cap, tail_len;
    int32_t status;
    uint32_t altered;
    uint8_t md5[16];
} flacenc_session_final;
int flacenc_device_session_plan(const flacenc_options *opts, uint32_t bits_per_sample, uint32_t channels, size_t n_streams,
                                uint64_t max_chunk, uint32_t flags, size_t *device_bytes);
int flacenc_device_session_open(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                uint32_t channels, const uint64_t *totals, size_t n_streams, uint64_t max_chunk,
                                uint32_t flags, flacenc_device_session **session);
int flacenc_device_session_open_ex(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                   uint32_t channels, const uint64_t *totals, const uint8_t *total_known, size_t n_streams,
                                   uint64_t max_chunk, uint32_t flags, flacenc_device_session **session);
size_t flacenc_device_session_header_len(const flacenc_device_session *session, size_t i);
int flacenc_device_session_write(flacenc_device_session *session, const void *d_pcm, const flacenc_tensor_format *fmt,
                                 flacenc_session_chunk *chunks, void *stream);
int flacenc_device_session_finalize(flacenc_device_session *session, flacenc_session_final *finals);
void flacenc_device_session_close(flacenc_device_session *session);
/* The short last blocks of the calling thread's last flacenc_encode_many_device[_out] or flacenc_device_session_finalize
 * call (zero when that call was refused or had none): how many were encoded, and in how many batches.  The one-shot calls
 * send them through flacgpu_encode_ragged_device as ragged batches of up to a pooled context's frames (one batch for up to
 * 4096 mono clips); a session's finalize, and every call with FLACGPU_NO_RAGGED=1 in the environment, runs one one-frame
 * flacgpu_encode_device call each (tail_batches == tail_frames) -- the bytes are the same.  Either may be NULL. */
void flacenc_device_tail_stats(uint64_t *tail_frames, uint64_t *tail_batches);
/* ---- a device stream writer: ONE RAW FRAME per stream per call (DESIGN.md 4c "Device stream writer") -------------------------
 * FlacStreamWriter::write (encode.rs:1094-1274; flacenc_stream_writer_write below is the host form) for n_streams streams of
 * one shape whose samples lie in device memory: header-less subset frames, the input of flacgpu_decoder's raw frame streams.
 * No metadata and no MD5.
 *   plan      pure host code.  Refuses, in FlacStreamWriter's order and with its codes: invalid options (the OptionsError;
 *             opts->block_size is validated but otherwise ignored, as in FlacStreamWriter::new), bits per sample outside
 *             1..32 (FLACENC_ERR_NON_SUBSET_BITS_PER_SAMPLE), channels outside 1..8 (FLACENC_ERR_EXCESSIVE_CHANNELS),
 *             max_block outside 1..65535 (FLACENC_ERR_INVALID_BLOCK_SIZE), a sample rate no subset frame header codes
 *             (FLACENC_ERR_NON_SUBSET_SAMPLE_RATE; from 2^20 on FLACENC_ERR_INVALID_SAMPLE_RATE), bits per sample other
 *             than 8, 12, 16, 20, 24, 32 (FLACENC_ERR_NON_SUBSET_BITS_PER_SAMPLE); then what flacenc_device_batch_plan
 *             refuses for the shape (the stream count).  *device_bytes = the writer's staging buffer: per stream
 *             max_block * channels int32 elements rounded up to 16 bytes.  (The analysis contexts are the pooled ones, of
 *             block size max(16, max_block): a max_block of 1..15 is served by contexts of 16, as in the host writer.)
 *   open      the same checks; first_numbers[i] = stream i's first frame number (NULL: all 0; above 2^36 - 1:
 *             FLACENC_ERR_EXCESSIVE_FRAME_NUMBER).  The staging buffer is allocated here, at its final size: a buffer the
 *             device cannot hold is open's error (FLACENC_ERR_GPU), not a later write's.
 *   write     chunks[i].samples in 0..max_block samples per channel of stream i in `d_pcm`, described by `fmt`, in_offset
 *             and samples exactly as for flacenc_device_session_write.  Every stream with samples > 0 gets exactly ONE frame
 *             of that many samples, numbered with the stream's count, in chunks[i].out (out_len = its size; altered = the
 *             chunk's count), and its count advances by one; a stream with 0 samples gets nothing and its count stays.  The
 *             frame is byte for byte flacenc_stream_writer_write's for the same samples, options and frame number.  All
 *             frames of a call, whatever their lengths, are one ragged batch (flacgpu_encode_ragged_device; several when a
 *             pooled context does not hold them all); FLACGPU_NO_RAGGED=1 takes one one-frame call each, the same bytes.
 *             Synchronous: d_pcm may be reused on return.  Refused as a whole -- nothing launched, no chunk field written,
 *             no count advanced: a chunk longer than max_block and anything flacenc_device_batch_plan refuses for the tensor
 *             (FLACENC_ERR_INVALID_ARG / _UNSUPPORTED), a frame whose effective partition order min(ctz(samples),
 *             max_partition_order) exceeds 6 (FLACENC_ERR_UNSUPPORTED; flacenc_last_error names the stream).  Errors of
 *             one stream, in its chunk's status: an `out` too small FLACENC_ERR_IO -- the count is NOT advanced, as when
 *             the host writer's sink fails, and the stream stays usable: the same chunk written again with room gives the
 *             frame with the same number; a stream whose count stands at 2^36 - 1 gets its frame and
 *             FLACENC_ERR_EXCESSIVE_FRAME_NUMBER, the count staying, as in flacenc_stream_writer_write.  Returns 0 when the
 *             call ran, or the refusal.  A failure of the device is sticky: every later write returns it.  (Arguments a
 *             flacgpu_* call refuses -- none is left once the checks above have passed -- are that call's error alone.)
 *   frame_number  stream i's next frame number (0 for an i out of range).
 *   close     frees everything; legal on NULL.
 * flacenc_device_tail_stats is not touched by a writer's calls.  A writer is not thread-safe; several writers, sessions
 * and one-shot calls beside one another do not disturb one another. */
typedef struct flacenc_device_stream_writer flacenc_device_stream_writer;
int flacenc_device_stream_writer_plan(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                      uint32_t channels, size_t n_streams, uint32_t max_block, size_t *device_bytes);
int flacenc_device_stream_writer_open(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                      uint32_t channels, size_t n_streams, uint32_t max_block, const uint64_t *first_numbers,
                                      flacenc_device_stream_writer **writer);
int flacenc_device_stream_writer_write(flacenc_device_stream_writer *writer, const void *d_pcm,
                                       const flacenc_tensor_format *fmt, flacenc_session_chunk *chunks, void *stream);
uint64_t flacenc_device_stream_writer_frame_number(const flacenc_device_stream_writer *writer, size_t i);
void flacenc_device_stream_writer_close(flacenc_device_stream_writer *writer);
/* The conversion rule on the host, one element: raw_bits holds the element's bits (I16: in the low half; S24: in the low 24 bits, bits
 * 24-31 are ignored).  *altered
 * (may be NULL) = 1 when the element was changed beyond rounding.  A combination plan refuses (unknown type, bps outside
 * 1..32, I16 with bps > 16, S24 with bps > 24) gives 0 and *altered = 1. */
int32_t flacenc_ingest_sample(uint32_t sample_type, uint32_t raw_bits, uint32_t bits_per_sample, int *altered);

/* FlacStreamWriter (encode.rs:1050-1290): header-less subset frames, parameters per call. */
typedef struct flacenc_stream_writer flacenc_stream_writer;
int flacenc_stream_writer_new(const flacenc_options *opts, const flacenc_sink *sink,
                              flacenc_stream_writer **out);
int flacenc_stream_writer_write(flacenc_stream_writer *w, uint32_t sample_rate, uint32_t channels,
                                uint32_t bits_per_sample, const int32_t *samples, size_t count);
const uint8_t *flacenc_stream_writer_data(flacenc_stream_writer *w, size_t *len);
void flacenc_stream_writer_free(flacenc_stream_writer *w);

/* statistics of a writer (after finalize) */
typedef struct {
    uint64_t frames, samples_per_channel, bytes_written;
    uint32_t min_frame_size, max_frame_size;
    uint8_t md5[16];
    double gpu_ms, pack_ms, md5_ms; /* accumulated host-side wall time per stage */
} flacenc_stats;
int flacenc_writer_stats(flacenc_writer *w, flacenc_stats *out);

/* Host bit-packing of one analysed batch (what Encoder::encode does after the analysis:
 * frame header + CRC-8, subframes, Rice residuals, CRC-16; encode.rs:2284-2409, 3834-3863).
 * Inputs are the outputs of flacgpu_analyze / flacgpu_fetch.  Frame f gets frame number
 * first_frame_number + f and lands at out[offsets[f] .. offsets[f+1]); offsets has
 * n_frames + 1 entries.  Returns 0, or FLACENC_ERR_INVALID_ARG when `cap` is too small
 * (offsets[n_frames] then holds the required size). */
int flacenc_pack_frames(uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels,
                        uint64_t first_frame_number, uint32_t n_frames, uint32_t row_stride,
                        const void *frame_plans, const void *subframe_plans,
                        const int32_t *residual_rows, uint32_t threads, uint8_t *out, size_t cap,
                        uint64_t *offsets);

/* Everything in front of the first frame (fLaC + STREAMINFO + SEEKTABLE + VORBIS_COMMENT + PADDING)
 * exactly as a writer that had emitted frames of these sizes leaves it at finalize: for the owner of a
 * stream whose contiguous frame ranges were encoded on several GPUs (encode.rs:1999-2003
 * seek points, 2414-2436 min/max frame size, 2024-2110 finalize).  `md5`: of the whole PCM, computed by
 * the owner.  *len receives the size; FLACENC_ERR_INVALID_ARG when `cap` is too small. */
int flacenc_stream_header(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                          uint32_t channels, uint64_t total_pcm_frames, const uint8_t md5[16], uint64_t n_frames,
                          const uint32_t *frame_sizes, uint32_t last_frame_len, uint8_t *out, size_t cap,
                          size_t *len);
/* The same for a writer created WITHOUT a total (flacenc_sample_writer_new(.., has_total = 0, ..); FlacSampleWriter::new
 * with None, encode.rs:1909-1939): no placeholder SEEKTABLE; the seek points go into the PADDING block when it has room
 * for them (behind it, the padding shrunk by their size; encode.rs:2029-2076), else there are none; STREAMINFO's total is
 * the frames' own, (n_frames - 1) * block_size + last_frame_len (FLACENC_ERR_EXCESSIVE_TOTAL_SAMPLES from 2^36 on).  The
 * size does not depend on the frames.  Pure host code. */
int flacenc_stream_header_unknown_total(const flacenc_options *opts, uint32_t sample_rate, uint32_t bits_per_sample,
                                        uint32_t channels, const uint8_t md5[16], uint64_t n_frames,
                                        const uint32_t *frame_sizes, uint32_t last_frame_len, uint8_t *out, size_t cap,
                                        size_t *len);

/* The 34-byte STREAMINFO body exactly as the writers serialise it (metadata/mod.rs:1599-1630). */
int flacenc_streaminfo_bytes(uint32_t min_block, uint32_t max_block, uint32_t min_frame, uint32_t max_frame,
                             uint32_t sample_rate, uint32_t channels, uint32_t bits_per_sample,
                             uint64_t total_samples, const uint8_t md5[16], uint8_t out[34]);

/* Test hooks of the multi-stream MD5 engine (host/md5_mb.cpp): digests of `streams` chains fed through the
 * pool in `runs` runs of assorted lengths against the scalar implementation (returns the mismatches), and
 * whether this host runs the 16-lane AVX-512 step. */
int flacenc_md5_selftest(uint32_t streams, uint32_t runs, uint32_t seed);
int flacenc_md5_simd_available(void);
/* Diagnostic: GB/s of `lanes` (1..48) independent MD5 chains advanced in lockstep by one thread over kib_per_lane KiB each;
 * divided by the lane count it is the speed of ONE chain -- the per-stream bound of every front end (a stream's MD5 is one
 * serial chain, encode.rs:571, 1292-1318). */
double flacenc_md5_probe(uint32_t lanes, uint32_t kib_per_lane);
/* Test hook of flacenc_encode_many_coalesced's batch planning (host/coalesce.cpp, tests/test_coalesce_plan.py): streams of
 * whole[k] whole blocks of one shape (samples_per_block = block size x channels), batch_frames as in flacenc_options (0: the
 * default) -> segment i is blocks [seg_first[i], seg_first[i] + seg_n[i]) of stream seg_stream[i] in batch seg_batch[i].
 * Returns the number of segments (the arrays hold up to `cap`); *batch_cap: the frames a batch may hold. */
size_t flacenc_coalesce_plan(const uint64_t *whole, size_t n_streams, uint32_t batch_frames, uint32_t samples_per_block, uint32_t *seg_stream,
                             uint64_t *seg_first, uint32_t *seg_n, uint32_t *seg_batch, size_t cap, uint32_t *batch_cap);

const char *flacenc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
