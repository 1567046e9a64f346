// meta_walk.h -- the walk over a FLAC stream's metadata chain, as flacenc::parse_metadata (host/flac_stream.cpp) walks it:
// the fLaC marker and len >= 42, then block after block a 4-byte header (last flag + type, 24-bit length) and the jump
// over the block; the last STREAMINFO (type 0, length 34) wins; truncation ends the walk anywhere.  One function for the
// host (parse_metadata, flacgpu_meta_walk_host) and the device (k_meta_walk, decode_many.hip: streams that already lie in
// device memory), so that the rule is tested without a GPU.  It reads bytes of [data, data + len) alone, one at a time,
// and nothing when data is null.  What the STREAMINFO bytes mean (flacgpu_stream_info, the minimum frame size, the
// usability test) is the host's business: flacenc::metadata_of_record.
#ifndef FLACGPU_META_WALK_H
#define FLACGPU_META_WALK_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLACGPU_MW __host__ __device__ inline
#else
#define FLACGPU_MW inline
#endif

constexpr uint32_t kStreamInfoBytes = 34;
constexpr uint32_t META_MARKER = 1u;     // data != null, len >= 42 and the fLaC marker: the chain was walked
constexpr uint32_t META_COMPLETE = 2u;   // the walk reached the block with the last flag, whole: frames_at is valid
constexpr uint32_t META_HAVE_SI = 4u;    // a STREAMINFO block was seen whole: si holds the last one

struct MetaRecord {                  // 56 bytes
    uint32_t status;                 // META_* bits
    uint32_t reserved;
    uint64_t frames_at;              // first byte behind the metadata (META_COMPLETE), else 0
    uint8_t si[kStreamInfoBytes];    // the last STREAMINFO's bytes (META_HAVE_SI), else zeros
    uint8_t pad[6];
};
static_assert(sizeof(MetaRecord) == 56, "MetaRecord is a table row shared by the device and the host");

FLACGPU_MW void meta_walk(const uint8_t *data, uint64_t len, MetaRecord &r) {
    r.status = r.reserved = 0;
    r.frames_at = 0;
    for (uint32_t i = 0; i < kStreamInfoBytes; i++) r.si[i] = 0;
    for (uint32_t i = 0; i < 6; i++) r.pad[i] = 0;
    if (!data || len < 42 || data[0] != 'f' || data[1] != 'L' || data[2] != 'a' || data[3] != 'C') return;
    r.status = META_MARKER;
    uint64_t pos = 4;   // <= len throughout, so no sum below leaves 64 bits
    for (;;) {
        if (pos + 4 > len) return;   // truncated in a block header
        const uint32_t head = data[pos];
        const uint64_t blen = (uint64_t)data[pos + 1] << 16 | (uint64_t)data[pos + 2] << 8 | data[pos + 3];
        pos += 4;
        if (pos + blen > len) return;   // truncated in a block
        if ((head & 0x7Fu) == 0 && blen == kStreamInfoBytes) {
            for (uint32_t i = 0; i < kStreamInfoBytes; i++) r.si[i] = data[pos + i];
            r.status |= META_HAVE_SI;
        }
        pos += blen;
        if (head & 0x80u) break;
    }
    r.status |= META_COMPLETE;
    r.frames_at = pos;
}
#endif
