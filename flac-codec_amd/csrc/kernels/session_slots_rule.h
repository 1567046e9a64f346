// session_slots_rule.h -- the per-group rule of k_session_slots (kernels/session.inc; DESIGN.md 4b "Decoder sessions"): one
// 16-byte group of a decoder session's slot, which is the stream's held tail followed by its new chunk.  One set of
// functions for the device (k_session_slots) and the host (flacgpu_session_slots_host, decode_many.hip, one "lane" after
// another over host memory), so that the rule is tested without a GPU.  For .hip translation units (kernels/byte_shift.h).
//   * Slot byte k is tail[k] for k < tail_len and chunk[k - tail_len] behind that; the bytes from tail_len + chunk_len
//     on are zero.  Both sources have any alignment.
//   * A group's bytes of one source are taken from the aligned 16-byte source group that holds the first of them and,
//     only when they reach into it, the aligned group behind it (k_gather_slots' rule: a loaded group holds at least one
//     byte that is wanted, so it cannot leave that byte's page), combined by shift_group.
//   * The group that holds the junction takes its low bytes from the tail and the rest from the chunk: the chunk's bytes
//     are shifted so that they land behind the tail's, and the two results are merged by byte masks.  A source group
//     that holds none of the wanted bytes is not loaded.
#ifndef FLACGPU_SESSION_SLOTS_RULE_H
#define FLACGPU_SESSION_SLOTS_RULE_H
#include <stdint.h>
#include <string.h>

#include "byte_shift.h"

struct SessionSrc {         // one slot's two sources, as addresses of the memory the rule runs over
    uint64_t tail, tail_len;     // the held bytes (in the session's other batch buffer); tail_len may be 0
    uint64_t chunk, chunk_len;   // this feed's bytes; chunk_len may be 0
};

// the aligned 16-byte group at `grp`, which holds at least one byte of [first, end).  The device loads the group; the
// host pass copies the group's bytes of [first, end) alone, so that a sanitizer run of the host rule checks the reads.
__host__ __device__ inline uint4 session_load(uint64_t grp, uint64_t first, uint64_t end) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)first;
    (void)end;
    return *reinterpret_cast<const uint4 *>(grp);
#else
    uint8_t b[16] = {0};
    const uint64_t lo = grp > first ? grp : first, hi = grp + 16 < end ? grp + 16 : end;
    memcpy(b + (lo - grp), reinterpret_cast<const void *>(lo), (size_t)(hi - lo));
    uint4 v;
    memcpy(&v, b, 16);
    return v;
#endif
}

// 16 bytes of which byte j is the source byte p + j wherever p + j lies in [first, end); the other bytes are undefined.
// [first, end) is not empty and lies inside [p, p + 16).
__host__ __device__ inline uint4 session_take(uint64_t p, uint64_t first, uint64_t end) {
    const uint32_t a = (uint32_t)(p & 15u);
    const uint64_t g = p - a;
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = make_uint4(0u, 0u, 0u, 0u);
    if (first < g + 16) lo = session_load(g, first, end);        // holds `first`
    if (end > g + 16) hi = session_load(g + 16, first, end);     // holds the wanted byte g + 16, or `first`
    return shift_group(lo, hi, a);
}

// bytes [lo, hi) of the group, 0 <= lo <= hi <= 16, the others cleared
__host__ __device__ inline uint4 session_keep(uint4 v, int64_t lo, int64_t hi) {
    v.x = keep_bytes(v.x, hi) ^ keep_bytes(v.x, lo);
    v.y = keep_bytes(v.y, hi - 4) ^ keep_bytes(v.y, lo - 4);
    v.z = keep_bytes(v.z, hi - 8) ^ keep_bytes(v.z, lo - 8);
    v.w = keep_bytes(v.w, hi - 12) ^ keep_bytes(v.w, lo - 12);
    return v;
}

// the group at slot offset rel (a multiple of 16) of the slot made of `s`
__host__ __device__ inline uint4 session_group(const SessionSrc &s, uint64_t rel) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (rel >= s.tail_len + s.chunk_len) return v;   // the zero tail: nothing is loaded
    int64_t have = 0;   // bytes of the group the tail fills
    if (rel < s.tail_len) {
        have = s.tail_len - rel >= 16 ? 16 : (int64_t)(s.tail_len - rel);
        const uint64_t p = s.tail + rel;
        v = session_keep(session_take(p, p, p + have), 0, have);
        if (have == 16 || !s.chunk_len) return v;
    }
    // the chunk's bytes of the group: from chunk byte `off` on, landing at byte `have`
    const uint64_t off = have ? 0 : rel - s.tail_len;
    const int64_t room = 16 - have;
    const int64_t n = s.chunk_len - off >= (uint64_t)room ? room : (int64_t)(s.chunk_len - off);
    const uint64_t first = s.chunk + off;
    const uint4 c = session_keep(session_take(first - have, first, first + n), have, have + n);
    v.x |= c.x;
    v.y |= c.y;
    v.z |= c.z;
    v.w |= c.w;
    return v;
}
#endif
