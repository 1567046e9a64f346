// stream_ledger.h -- the container state of ONE stream: what the reference's Encoder::new / encode / finalize_inner
// (encode.rs:1882-2110) keep besides the frames themselves -- STREAMINFO, the metadata layout, the seek points, the counters --
// and the bytes in front of the first frame that follow from them.  No analysis, no I/O, no GPU: the per-stream writers
// (stream_writer.cpp) own one beside their transport, the header functions (flacenc_stream_header*) use one by itself.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "flacenc_stream.h"

namespace flacenc_host {

constexpr uint64_t kMaxSamples = 68719476736ull;         // Encoder::MAX_SAMPLES, encode.rs:1880
constexpr uint32_t kMaxFrameSize = (1u << 24) - 1;       // Streaminfo::MAX_FRAME_SIZE
constexpr size_t kMaxSeekPoints = (1u << 24) / 18;       // SeekTable::MAX_POINTS
constexpr uint64_t kMaxFrameNumber = (1ull << 36) - 1;   // FrameNumber::MAX_FRAME_NUMBER

struct SeekPoint {
    uint64_t sample_offset, byte_offset;
    uint16_t frame_samples;
    bool defined;
};

// SeekTableInterval::filter, encode.rs:1338-1358
std::vector<SeekPoint> filter_points(const flacenc_options &o, uint32_t sample_rate, const std::vector<SeekPoint> &in);

// ---- metadata serialisation (metadata/mod.rs:257-266, 904-960, 1740-1760, 1826-1831,
//      2010-2036, 2118-2139) ----------------------------------------------------------
struct StreamInfo {
    uint32_t min_block = 0, max_block = 0, min_frame = 0, max_frame = 0;
    uint32_t sample_rate = 0, channels = 0, bps = 0;
    uint64_t total_samples = 0;  // 0 = None
    uint8_t md5[16] = {0};
};

struct MetaLayout {
    bool vorbis = false;              // a VORBIS_COMMENT block is present (sorts first)
    std::vector<uint8_t> vorbis_body;
    bool seektable = false;           // a SEEKTABLE block is present
    bool seektable_after_padding = false;  // inserted at finalize => pushed last
    std::vector<SeekPoint> points;
    bool padding = false;
    uint32_t padding_size = 0;
};

void put_be(std::vector<uint8_t> &v, uint64_t x, int bytes);
void put_block_header(std::vector<uint8_t> &v, bool last, uint8_t type, uint32_t size);
std::vector<uint8_t> build_metadata(const StreamInfo &si, const MetaLayout &m);

int options_error(const flacenc_options &o);   // Options' own ranges (encode.rs:1418-1455)
// FlacStreamWriter::write's two subset checks, in its order (encode.rs:1127-1137): a sample rate the frame header cannot
// code (FLACENC_ERR_NON_SUBSET_SAMPLE_RATE; from 2^20 on FLACENC_ERR_INVALID_SAMPLE_RATE), then bits per sample other than
// 8, 12, 16, 20, 24 or 32 (FLACENC_ERR_NON_SUBSET_BITS_PER_SAMPLE)
int subset_frame_error(uint32_t sample_rate, uint32_t bits_per_sample);
// the checks of FlacSampleWriter::new / Encoder::new for a stream whose total is known (encode.rs:487-531, 1882-1917) and
// the number of bytes in front of its first frame (fixed at `new`: the SEEKTABLE placeholder has its final size).
// has_total = false: `new` with None -- total_pcm_frames is ignored, there is no placeholder SEEKTABLE, and the size holds
// at finalize too, since a seek table then comes out of the PADDING block (encode.rs:1909-1939, 2029-2076)
int stream_header_len(const flacenc_options &o, uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels,
                      uint64_t total_pcm_frames, size_t *len, bool has_total = true);
// Encoder::finalize_inner's verdict on the sample count (encode.rs:2079-2097): a declared total must have been met; without
// one the count must fit 36 bits and be non-zero.  0, or the reference's error in the reference's order.
int totals_verdict(bool known, uint64_t total, uint64_t written);

struct StreamLedger {
    flacenc_options o{};   // the rules below read block_size and the seek table mode; no pointer into caller memory is kept
    StreamInfo si;
    MetaLayout meta;
    size_t metadata_len = 0;
    uint64_t frame_number = 0, samples_written = 0, byte_count = 0;  // Counter::count
    std::vector<SeekPoint> seekpoints;
    const char *why = nullptr;   // what flacenc_last_error() should say about close()'s refusal, when it has words for it

    // Encoder::new, encode.rs:1882-1980: the checks in the reference's order, the metadata layout, and into `header` the
    // bytes that stand in front of the first frame until close() replaces them
    int open(const flacenc_options &opts, uint32_t rate, uint32_t bps, uint32_t channels, bool has_total,
             uint64_t total_pcm_frames, std::vector<uint8_t> &header);

    // ExcessiveTotalSamples is raised BEFORE the offending frame is encoded (encode.rs:2006-2011): of a run of n_frames
    // blocks, the last one last_len long, offered when `already` samples have been taken, the first `usable` may be encoded;
    // `deferred` is the error to return once they have been (and overrun() has run).  `error`: the run is refused outright.
    struct Admit {
        uint32_t usable;
        int deferred, error;
    };
    Admit admit(uint64_t already, uint32_t n_frames, uint32_t last_len) const {
        Admit a{n_frames, 0, 0};
        if (si.total_samples) {
            uint64_t w = already;
            for (uint32_t f = 0; f < n_frames; f++) {
                w += (f + 1 == n_frames) ? last_len : o.block_size;
                if (w > si.total_samples) {
                    a.usable = f;
                    a.deferred = FLACENC_ERR_EXCESSIVE_TOTAL_SAMPLES;
                    break;
                }
            }
        }
        if (a.usable && frame_number + a.usable - 1 > kMaxFrameNumber) a.error = FLACENC_ERR_EXCESSIVE_FRAME_NUMBER;
        return a;
    }

    // Encoder::encode's bookkeeping (encode.rs:1999-2003) and encode_frame's tail (:2414-2436) for a run of n_frames
    // encoded blocks, the last one last_len samples long, frame k size_of(k) bytes: a seek point each, the sample count,
    // STREAMINFO's frame sizes, the byte count.  Runs accumulate: the frames of a stream may come in any cuts.
    template <class SizeOf>
    void frames(uint64_t n_frames, uint32_t last_len, SizeOf size_of) {
        for (uint64_t k = 0; k < n_frames; k++) {
            const uint32_t n = (k + 1 == n_frames) ? last_len : o.block_size;
            seekpoints.push_back({samples_written, byte_count, static_cast<uint16_t>(n), true});
            samples_written += n;
            const uint32_t size = size_of(k);
            if (size != 0 && size < kMaxFrameSize) {
                si.min_frame = si.min_frame ? std::min(si.min_frame, size) : size;
                si.max_frame = std::max(si.max_frame, size);
            }
            byte_count += size;
        }
    }

    // the tail of a run that admit() cut short: the reference pushes the seek point and bumps samples_written before failing
    void overrun(uint32_t n_frames, uint32_t usable, uint32_t last_len) {
        seekpoints.push_back({samples_written, byte_count, static_cast<uint16_t>(o.block_size), true});
        samples_written += (usable + 1 == n_frames) ? last_len : o.block_size;
    }

    // Encoder::finalize_inner, encode.rs:2024-2110: the SEEKTABLE filled in (or carved out of PADDING), the verdict on the
    // sample count, the stream's MD5, and into `header` the final bytes in front of the first frame -- as many as open() gave
    int close(const uint8_t md5[16], std::vector<uint8_t> &header);
};

}  // namespace flacenc_host
