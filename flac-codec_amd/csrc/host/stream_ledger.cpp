// stream_ledger.cpp -- the container rules of one stream (stream_ledger.h): Encoder::new's checks and metadata layout,
// finalize_inner's seek table, totals and header (encode.rs:1882-1980, 2024-2110), the metadata blocks' bytes
// (metadata/mod.rs), and the C entry point that exposes STREAMINFO's.  Pure host code: it links without the rest of the driver.
#include "stream_ledger.h"

#include <cstring>
#include <string>

namespace flacenc_host {

// SeekTableInterval::filter, encode.rs:1338-1358
std::vector<SeekPoint> filter_points(const flacenc_options &o, uint32_t sample_rate,
                                     const std::vector<SeekPoint> &in) {
    std::vector<SeekPoint> out;
    if (o.seektable_mode == FLACENC_SEEKTABLE_SECONDS) {
        const uint64_t nth = static_cast<uint32_t>((o.seektable_value & 0xFFu) * sample_rate);
        uint64_t offset = 0;
        for (const auto &p : in)
            if (offset >= p.sample_offset && offset < p.sample_offset + p.frame_samples) {
                offset += nth;
                out.push_back(p);
            }
    } else if (o.seektable_mode == FLACENC_SEEKTABLE_FRAMES) {
        const size_t step = o.seektable_value ? o.seektable_value : 1;
        for (size_t i = 0; i < in.size(); i += step) out.push_back(in[i]);
    }
    return out;
}

void put_be(std::vector<uint8_t> &v, uint64_t x, int bytes) {
    for (int i = bytes - 1; i >= 0; i--) v.push_back(static_cast<uint8_t>(x >> (8 * i)));
}
void put_block_header(std::vector<uint8_t> &v, bool last, uint8_t type, uint32_t size) {
    v.push_back(static_cast<uint8_t>((last ? 0x80 : 0) | type));
    put_be(v, size, 3);
}

std::vector<uint8_t> build_metadata(const StreamInfo &si, const MetaLayout &m) {
    std::vector<uint8_t> v;
    v.insert(v.end(), {'f', 'L', 'a', 'C'});
    int remaining = (m.seektable ? 1 : 0) + (m.padding ? 1 : 0) + (m.vorbis ? 1 : 0);
    put_block_header(v, remaining == 0, 0, 34);
    put_be(v, si.min_block, 2);
    put_be(v, si.max_block, 2);
    put_be(v, si.min_frame, 3);
    put_be(v, si.max_frame, 3);
    // 20 bits rate | 3 bits channels-1 | 5 bits bps-1 | 36 bits total samples
    uint64_t packed = (static_cast<uint64_t>(si.sample_rate) << 44) |
                      (static_cast<uint64_t>(si.channels - 1) << 41) |
                      (static_cast<uint64_t>(si.bps - 1) << 36) | (si.total_samples & 0xFFFFFFFFFull);
    put_be(v, packed, 8);
    v.insert(v.end(), si.md5, si.md5 + 16);
    auto emit_seektable = [&]() {
        remaining--;
        put_block_header(v, remaining == 0, 3, static_cast<uint32_t>(m.points.size() * 18));
        for (const auto &p : m.points) {
            if (p.defined) {
                put_be(v, p.sample_offset, 8);
                put_be(v, p.byte_offset, 8);
                put_be(v, p.frame_samples, 2);
            } else {  // SeekPoint::Placeholder
                put_be(v, ~0ull, 8);
                put_be(v, 0, 8);
                put_be(v, 0, 2);
            }
        }
    };
    auto emit_padding = [&]() {
        remaining--;
        put_block_header(v, remaining == 0, 1, m.padding_size);
        v.insert(v.end(), m.padding_size, 0);
    };
    if (m.vorbis) {  // VorbisComment::to_writer, metadata/mod.rs:2512-2536
        remaining--;
        put_block_header(v, remaining == 0, 4, static_cast<uint32_t>(m.vorbis_body.size()));
        v.insert(v.end(), m.vorbis_body.begin(), m.vorbis_body.end());
    }
    // block order after Encoder::new's sort (encode.rs:1944-1951): VORBIS_COMMENT < SEEKTABLE < PADDING;
    // a SEEKTABLE created at finalize is pushed behind PADDING (metadata/mod.rs:4425-4441)
    if (m.seektable && !m.seektable_after_padding) emit_seektable();
    if (m.padding) emit_padding();
    if (m.seektable && m.seektable_after_padding) emit_seektable();
    return v;
}

int options_error(const flacenc_options &o) {
    if (o.block_size < 16 || o.block_size > 65535) return FLACENC_ERR_INVALID_BLOCK_SIZE;
    if (o.max_lpc_order > 32) return FLACENC_ERR_INVALID_LPC_ORDER;
    if (o.max_partition_order > 15) return FLACENC_ERR_INVALID_MAX_PARTITIONS;
    if (o.padding < 0 || o.padding >= (1 << 24)) return FLACENC_ERR_EXCESSIVE_PADDING;
    return 0;
}

int subset_frame_error(uint32_t rate, uint32_t bps) {
    {  // SampleRate::try_from + "Streaminfo => NonSubsetSampleRate"
        bool named = false;
        for (uint32_t r : {88200u, 176400u, 192000u, 8000u, 16000u, 22050u, 24000u, 32000u, 44100u, 48000u, 96000u})
            named |= (r == rate);
        bool coded = named || (rate % 1000 == 0 && rate / 1000 < 255) ||
                     (rate % 10 == 0 && rate / 10 < 65535) || rate < 65535;
        if (!coded) return rate < (1u << 20) ? FLACENC_ERR_NON_SUBSET_SAMPLE_RATE : FLACENC_ERR_INVALID_SAMPLE_RATE;
    }
    if (!(bps == 8 || bps == 12 || bps == 16 || bps == 20 || bps == 24 || bps == 32))
        return FLACENC_ERR_NON_SUBSET_BITS_PER_SAMPLE;
    return 0;
}

int totals_verdict(bool known, uint64_t total, uint64_t written) {
    if (known) return total != written ? FLACENC_ERR_SAMPLE_COUNT_MISMATCH : 0;
    if (written >= kMaxSamples) return FLACENC_ERR_EXCESSIVE_TOTAL_SAMPLES;
    if (written == 0) return FLACENC_ERR_NO_SAMPLES;
    return 0;
}

int StreamLedger::open(const flacenc_options &opts, uint32_t rate, uint32_t bps, uint32_t channels, bool has_total,
                       uint64_t total_pcm_frames, std::vector<uint8_t> &header) {
    o = opts;
    if (int e = options_error(o)) return e;
    if (rate >= 1048576u) return FLACENC_ERR_INVALID_SAMPLE_RATE;
    if (channels < 1 || channels > 8) return FLACENC_ERR_EXCESSIVE_CHANNELS;
    if (has_total && total_pcm_frames >= kMaxSamples) return FLACENC_ERR_EXCESSIVE_TOTAL_SAMPLES;
    si.min_block = si.max_block = o.block_size;
    si.sample_rate = rate;
    si.channels = channels;
    si.bps = bps;
    si.total_samples = has_total ? total_pcm_frames : 0;
    meta.padding = o.padding > 0;
    meta.padding_size = static_cast<uint32_t>(o.padding);
    if (o.n_comment_fields || o.vendor_string) {
        auto put_le32 = [&](uint32_t x) {
            for (int i = 0; i < 4; i++) meta.vorbis_body.push_back(static_cast<uint8_t>(x >> (8 * i)));
        };
        const std::string vendor = o.vendor_string ? o.vendor_string : "flac-codec 1.3.2";
        put_le32(static_cast<uint32_t>(vendor.size()));
        meta.vorbis_body.insert(meta.vorbis_body.end(), vendor.begin(), vendor.end());
        put_le32(o.n_comment_fields);
        for (uint32_t i = 0; i < o.n_comment_fields; i++) {
            const std::string f = o.comment_fields[i];
            put_le32(static_cast<uint32_t>(f.size()));
            meta.vorbis_body.insert(meta.vorbis_body.end(), f.begin(), f.end());
        }
        meta.vorbis = true;
    }
    // the ledger keeps no pointers into caller memory
    o.vendor_string = nullptr;
    o.comment_fields = nullptr;
    if (has_total && o.seektable_mode != FLACENC_SEEKTABLE_NONE) {
        // placeholder SEEKTABLE, encode.rs:1920-1939 + EncoderSeekPoint::placeholders :2131
        std::vector<SeekPoint> all;
        for (uint64_t off = 0; off < total_pcm_frames; off += o.block_size) {
            uint64_t rem = total_pcm_frames - off;
            uint16_t fs = static_cast<uint16_t>(rem > 65535 ? o.block_size
                                                             : std::min<uint64_t>(rem, o.block_size));
            all.push_back({off, 0, fs, false});
        }
        meta.points = filter_points(o, rate, all);
        if (meta.points.size() > kMaxSeekPoints) meta.points.resize(kMaxSeekPoints);
        for (auto &p : meta.points) p.defined = false;
        meta.seektable = true;
    }
    header = build_metadata(si, meta);
    metadata_len = header.size();
    return 0;
}

int StreamLedger::close(const uint8_t md5[16], std::vector<uint8_t> &header) {
    // SEEKTABLE, encode.rs:2029-2076
    if (o.seektable_mode != FLACENC_SEEKTABLE_NONE) {
        std::vector<SeekPoint> enc = filter_points(o, si.sample_rate, seekpoints);
        if (meta.seektable) {
            const size_t n = meta.points.size();
            for (size_t i = 0; i < n; i++) {
                if (i < enc.size()) meta.points[i] = enc[i];
                else meta.points[i] = SeekPoint{0, 0, 0, false};
            }
        } else if (meta.padding) {
            if (enc.size() > kMaxSeekPoints) {
                why = "more seek points than a SEEKTABLE holds (the reference panics)";
                return FLACENC_ERR_UNSUPPORTED;
            }
            const uint64_t st_total = static_cast<uint64_t>(enc.size()) * 18 + 4;
            if (enc.size() * 18 < (1u << 24) && meta.padding_size >= st_total) {
                meta.padding_size -= static_cast<uint32_t>(st_total);
                meta.points = enc;
                meta.seektable = true;
                meta.seektable_after_padding = true;
            }
        }
    }
    // total samples, encode.rs:2079-2097
    if (int e = totals_verdict(si.total_samples != 0, si.total_samples, samples_written)) return e;
    si.total_samples = samples_written;
    std::memcpy(si.md5, md5, 16);
    header = build_metadata(si, meta);
    if (header.size() != metadata_len) {
        why = "internal: metadata size changed at finalize";
        return FLACENC_ERR_IO;
    }
    return 0;
}

int stream_header_len(const flacenc_options &o, uint32_t sample_rate, uint32_t bits_per_sample, uint32_t channels,
                      uint64_t total_pcm_frames, size_t *len, bool has_total) {
    StreamLedger l;
    std::vector<uint8_t> header;
    const int rc = l.open(o, sample_rate, bits_per_sample, channels, has_total, total_pcm_frames, header);
    if (!rc && len) *len = l.metadata_len;
    return rc;
}

}  // namespace flacenc_host

// The 34 bytes of a STREAMINFO block body (metadata/mod.rs:1599-1630, 1740-1760) as the writers
// serialise them: exposed so that the layout can be checked against the reference's literal bytes.
extern "C" int flacenc_streaminfo_bytes(uint32_t min_block, uint32_t max_block, uint32_t min_frame, uint32_t max_frame,
                                        uint32_t sample_rate, uint32_t channels, uint32_t bits_per_sample,
                                        uint64_t total_samples, const uint8_t md5[16], uint8_t out[34]) {
    if (!md5 || !out) return FLACENC_ERR_INVALID_ARG;
    flacenc_host::StreamInfo si;
    si.min_block = min_block;
    si.max_block = max_block;
    si.min_frame = min_frame;
    si.max_frame = max_frame;
    si.sample_rate = sample_rate;
    si.channels = channels;
    si.bps = bits_per_sample;
    si.total_samples = total_samples;
    std::memcpy(si.md5, md5, 16);
    flacenc_host::MetaLayout m;
    const std::vector<uint8_t> v = flacenc_host::build_metadata(si, m);   // "fLaC" + header (4) + body (34)
    if (v.size() != 42) return FLACENC_ERR_IO;
    std::memcpy(out, v.data() + 8, 34);
    return 0;
}
