#include "flac_stream.h"

#include <algorithm>
#include <cstring>

#include "../kernels/frame_extent.h"
#include "checksums.h"
#include "raw_walk.h"

namespace flacenc {
namespace {
// frame_extent's bit source over data[0, len): MSB first, the bytes behind `len` read as 0
struct ByteBits {
    const uint8_t *d;
    size_t len;
    uint64_t p = 0;
    uint32_t byte(size_t i) const { return i < len ? d[i] : 0u; }
    uint32_t pos() const { return (uint32_t)p; }
    void seek(uint32_t bit) { p = bit; }
    uint32_t get(uint32_t n) {   // 1 <= n <= 32: five bytes hold the 7 odd bits in front and the n
        const size_t b = (size_t)(p >> 3);
        uint64_t v = 0;
        for (size_t i = 0; i < 5; i++) v = v << 8 | byte(b + i);
        v = (v >> (40 - (uint32_t)(p & 7) - n)) & (((uint64_t)1 << n) - 1);
        p += n;
        return (uint32_t)v;
    }
    uint32_t zeros(uint32_t limit) {
        uint32_t q = 0;
        for (;;) {
            const uint32_t odd = (uint32_t)(p & 7);
            const uint32_t cur = (byte((size_t)(p >> 3)) << odd) & 0xFFu;
            if (cur) {
                const uint32_t z = (uint32_t)__builtin_clz(cur) - 24u;
                p += z + 1;
                return q + z;
            }
            q += 8 - odd;
            p += 8 - odd;
            if (p > limit) return q;   // no 1 bit inside the window
        }
    }
    void rice(uint32_t k, uint32_t limit) {
        zeros(limit);
        p += k;
    }
};
}  // namespace

void streaminfo_fields(const uint8_t *b, flacgpu_stream_info *info, uint32_t *min_frame) {
    info->min_block = b[0] << 8 | b[1];   // metadata/mod.rs:1599-1630
    info->max_block = b[2] << 8 | b[3];
    *min_frame = b[4] << 16 | b[5] << 8 | b[6];
    info->sample_rate = (uint32_t)b[10] << 12 | (uint32_t)b[11] << 4 | b[12] >> 4;
    info->channels = ((b[12] >> 1) & 7) + 1;
    info->bits_per_sample = (((uint32_t)b[12] & 1) << 4 | b[13] >> 4) + 1;
    info->total_samples = ((uint64_t)(b[13] & 15) << 32) | (uint64_t)b[14] << 24 | (uint64_t)b[15] << 16 |
                          (uint64_t)b[16] << 8 | b[17];
    memcpy(info->md5, b + 18, 16);
}

const char *metadata_of_record(const MetaRecord &rec, flacgpu_stream_info *info, uint32_t *min_frame, size_t *frames_at) {
    memset(info, 0, sizeof *info);
    *min_frame = 0;
    if (!(rec.status & META_MARKER)) return "not a FLAC stream (no fLaC marker)";
    if (rec.status & META_HAVE_SI) streaminfo_fields(rec.si, info, min_frame);
    if (!(rec.status & META_COMPLETE)) return "";
    if (!(rec.status & META_HAVE_SI) || info->channels > 8 || info->bits_per_sample > 32 || info->max_block < 1)
        return "no usable STREAMINFO block";
    *frames_at = (size_t)rec.frames_at;
    return nullptr;
}

// the metadata blocks (metadata/mod.rs:257-266) are walked by kernels/meta_walk.h, which the device shares
const char *parse_metadata(const uint8_t *data, size_t len, flacgpu_stream_info *info, uint32_t *min_frame,
                           size_t *frames_at) {
    MetaRecord rec;
    meta_walk(data, len, rec);
    return metadata_of_record(rec, info, min_frame, frames_at);
}

bool host_parse_header(const uint8_t *d, size_t avail, HostFrameHead &h) {
    if (avail < 6 || d[0] != 0xFF || (d[1] & 0xFE) != 0xF8) return false;
    h.blocking = d[1] & 1;
    const uint32_t bcode = d[2] >> 4, rcode = d[2] & 15;
    h.acode = d[3] >> 4;
    h.bps_code = (d[3] >> 1) & 7;
    if ((d[3] & 1) || h.acode > 10 || bcode == 0 || rcode == 15 || h.bps_code == 3) return false;
    size_t k = 4;
    {   // UTF-8 like number
        const uint8_t b0 = d[k];
        uint32_t ones = 0;
        while (ones < 8 && (b0 & (0x80 >> ones))) ones++;
        if (ones == 1 || ones > 7) return false;
        const uint32_t extra = ones ? ones - 1 : 0;
        if (k + 1 + extra > avail) return false;
        for (uint32_t i = 1; i <= extra; i++)
            if ((d[k + i] & 0xC0) != 0x80) return false;
        k += 1 + extra;
    }
    switch (bcode) {
    case 1: h.n = 192; break;
    case 2: h.n = 576; break;
    case 3: h.n = 1152; break;
    case 4: h.n = 2304; break;
    case 5: h.n = 4608; break;
    case 6:
        if (k + 1 > avail) return false;
        h.n = d[k] + 1u;
        k += 1;
        break;
    case 7:
        if (k + 2 > avail) return false;
        h.n = ((uint32_t)d[k] << 8 | d[k + 1]) + 1u;
        k += 2;
        break;
    default: h.n = 256u << (bcode - 8); break;
    }
    if (rcode == 12) k += 1;
    else if (rcode == 13 || rcode == 14) k += 2;
    if (k + 1 > avail) return false;
    if (crc8(d, k) != d[k]) return false;
    h.header_bytes = (uint32_t)k + 1;
    return true;
}

bool host_parse_frame_info(const uint8_t *d, size_t avail, HostFrameInfo &h) {
    if (!host_parse_header(d, avail, h)) return false;
    host_frame_fields(d, h);
    return true;
}

void host_frame_fields(const uint8_t *d, HostFrameInfo &h) {
    static const uint32_t kRate[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    static const uint32_t kBits[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    h.rcode = d[2] & 15;
    h.channels = h.acode < 8 ? h.acode + 1 : 2;
    h.bits_per_sample = kBits[h.bps_code];
    // the coded number (stream.rs:1244-1262): the bits of the first byte behind its leading ones, then 6 per byte
    uint32_t ones = 0;
    while (d[4] & (0x80 >> ones)) ones++;
    h.number = ones ? d[4] & (0x7Fu >> ones) : d[4];
    for (uint32_t i = 1; i < ones; i++) h.number = h.number << 6 | (d[4 + i] & 0x3F);
    // the rate's own bytes are the last of the header in front of the CRC-8
    const uint8_t *tail = d + h.header_bytes - 1;
    if (h.rcode < 12) h.sample_rate = kRate[h.rcode];
    else if (h.rcode == 12) h.sample_rate = tail[-1] * 1000u;
    else h.sample_rate = ((uint32_t)tail[-2] << 8 | tail[-1]) * (h.rcode == 14 ? 10u : 1u);
}

void summarise_raw_frames(const flacgpu_frame_record *frames, size_t n, size_t len, flacgpu_raw_stream &summary) {
    summary.frames = (uint32_t)n;
    summary.uniform = raw_frames_uniform(frames, n);
    summary.skipped_bytes = 0;
    summary.gaps = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const flacgpu_frame_record &f = frames[i];
        if (f.byte_offset > at) {
            summary.skipped_bytes += f.byte_offset - at;
            summary.gaps++;
        }
        at = f.byte_offset + f.bytes;
    }
    if (len > at) {
        summary.skipped_bytes += len - at;
        summary.gaps++;
    }
}

size_t raw_frame_extent(const uint8_t *data, size_t len, const HostFrameInfo &h) {
    const uint16_t *const T = crc16_table();
    ByteBits bits{data, len};
    const size_t e = frame_extent(bits, h.header_bytes, h.n, h.acode, h.bits_per_sample,
                                  std::min<uint64_t>(len, kFrameExtentWindow));
    if (!e) return 0;
    uint16_t crc = 0;
    for (size_t i = 0; i < e; i++) crc = crc16_step(T, crc, data[i]);   // e <= the window <= len
    return crc == 0 ? e : 0;
}

void scan_raw_frames(const uint8_t *data, size_t len, uint32_t flags, std::vector<flacgpu_frame_record> &frames,
                     flacgpu_raw_stream &summary) {
    std::vector<size_t> cand;
    std::vector<HostFrameInfo> head;
    raw_candidates(data, len, len, cand, head);
    frames.clear();
    uint64_t out = 0;
    raw_walk(
        cand.data(), 0, cand.size(), 0, len,
        [&](size_t i, uint64_t s) {   // a later candidate or the input's end; else (speculative) the frame's own extent
            if (const size_t end = raw_end_by_crc(data, len, cand, i, head[i], SIZE_MAX, true)) return RawEnd{end, false};
            if (flags & FLACGPU_SCAN_SPECULATIVE)
                if (const size_t e = raw_frame_extent(data + s, len - s, head[i])) return RawEnd{s + e, true};
            return RawEnd{};   // no end: passed over, the walk goes on behind it
        },
        [&](size_t i, uint64_t s, uint64_t end, bool own) {
            const flacgpu_frame_record f = raw_frame_record(head[i], 0, s, end - s, out, own);
            frames.push_back(f);
            out += (uint64_t)head[i].n * head[i].channels;
        });
    summary = flacgpu_raw_stream{};
    summarise_raw_frames(frames.data(), frames.size(), len, summary);
}

const char *timeline_of_records(const flacgpu_frame_record *records, size_t n, flacgpu_timeline_frame *frames_out,
                                flacgpu_timeline_result &result) {
    result = flacgpu_timeline_result{};
    for (size_t k = 0; frames_out && k < n; k++) frames_out[k] = flacgpu_timeline_frame{};
    const auto refuse = [&](int rc, const char *why) {
        result.rc = rc;
        return why;
    };
    if (!n) return refuse(FLACGPU_ERR_INVALID_ARG, "no whole frame");
    const flacgpu_frame_record &r0 = records[0];
    if (!raw_frames_uniform(records, n))
        return refuse(FLACGPU_ERR_UNSUPPORTED, "frames differ in sample rate, channels or sample size");
    for (size_t k = 1; k < n; k++)
        if (records[k].blocking != r0.blocking)
            return refuse(FLACGPU_ERR_UNSUPPORTED, "frames differ in blocking strategy");
    const uint64_t B = r0.block_size;
    if (!r0.blocking) {
        for (size_t k = 0; k + 1 < n; k++)
            if (records[k].block_size != B)
                return refuse(FLACGPU_ERR_UNSUPPORTED,
                              "fixed blocking, but a frame before the last has another block size than the first");
        if (records[n - 1].block_size > B)
            return refuse(FLACGPU_ERR_UNSUPPORTED, "fixed blocking, but the last frame is larger than the block size");
    }
    // numbers reach 2^36 and block sizes 2^16: no product or sum of a scanned record leaves 64 bits
    const auto position = [&](const flacgpu_frame_record &r) { return r0.blocking ? r.number : r.number * B; };
    const uint64_t origin = position(r0);
    uint64_t end = origin;
    for (size_t k = 0; k < n; k++) {
        const uint64_t p = position(records[k]);
        const bool placed = k == 0 || p >= end;
        if (placed) {
            if (p > end) {
                result.gaps++;
                result.gap_samples += p - end;
            }
            end = p + records[k].block_size;
            result.placed++;
        } else {
            result.dropped++;
        }
        if (frames_out) {
            frames_out[k].at = placed ? p - origin : 0;
            frames_out[k].flags = placed ? FLACGPU_TL_PLACED : FLACGPU_TL_DROPPED;
        }
    }
    result.first_sample = origin;
    result.timeline_samples = end - origin;
    return nullptr;
}

void scan_frames(const uint8_t *data, size_t len, size_t pos, uint32_t min_frame, flacgpu_stream_info *info, FrameScan &scan) {
    const uint16_t *const T = crc16_table();   // taken once: the inner loop is one table step per byte
    size_t p = pos;
    while (p < len) {
        HostFrameHead h;
        if (!host_parse_header(data + p, len - p, h)) {
            info->bad_frames++;
            break;   // lost synchronisation: what follows is not decoded
        }
        uint16_t crc = 0, d1 = 0, d2 = 0;   // the CRC-16 of [p, q), of [p, q - 1), of [p, q - 2)
        size_t q = p, end = 0;
        const size_t min_end = p + std::max<size_t>(h.header_bytes + 2 + info->channels, min_frame);
        for (; q < len; q++) {
            // candidate: a header starts at q and bytes [q-2, q) are the CRC-16 of [p, q-2)
            if (q >= min_end && q >= p + 2 && data[q] == 0xFF && (data[q + (q + 1 < len ? 1 : 0)] & 0xFE) == 0xF8 &&
                (uint16_t)(data[q - 2] << 8 | data[q - 1]) == d2) {
                HostFrameHead hn;
                if (host_parse_header(data + q, len - q, hn) && hn.blocking == h.blocking) {
                    end = q;
                    break;
                }
            }
            d2 = d1;
            d1 = crc;
            crc = crc16_step(T, crc, data[q]);
        }
        if (!end) {   // the last frame ends with the stream
            if (q == len && len >= p + 2 && (uint16_t)(data[len - 2] << 8 | data[len - 1]) == d2) end = len;
            else {
                info->bad_frames++;
                break;
            }
        }
        scan.off.push_back(p);
        scan.n.push_back(h.n);
        info->decoded_samples += h.n;
        p = end;
    }
    scan.off.push_back(p);
    info->frames = (uint32_t)scan.n.size();
}

void finish_stream(const int32_t *planar, size_t ldb, const std::vector<uint32_t> &frame_n, int32_t *out,
                   flacgpu_stream_info *info) {
    const size_t F = frame_n.size(), C = info->channels;
    Md5 md5;
    const unsigned width = (info->bits_per_sample + 7) / 8;
    std::vector<uint8_t> le(*std::max_element(frame_n.begin(), frame_n.end()) * C * width);
    size_t o = 0;
    for (size_t f = 0; f < F; f++) {
        const size_t n = frame_n[f];
        size_t k = 0;
        for (size_t i = 0; i < n; i++)
            for (size_t ch = 0; ch < C; ch++) {
                const int32_t v = planar[(f * C + ch) * ldb + i];
                if (out) out[o++] = v;
                for (unsigned w = 0; w < width; w++) le[k++] = (uint8_t)((uint32_t)v >> (8 * w));
            }
        md5.update(le.data(), k);
    }
    const uint8_t zero[16] = {0};
    md5.digest(info->decoded_md5);
    info->md5_status = memcmp(info->md5, zero, 16) == 0 ? 2 : (memcmp(info->md5, info->decoded_md5, 16) == 0 ? 1 : 0);
}
}  // namespace flacenc
