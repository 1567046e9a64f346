// place_rule.h -- the copy rule of k_place_runs (kernels/place.inc; DESIGN.md 4c "Device-resident output"): a table of byte
// runs {src, dst, n} of any alignment, copied one 16-byte-aligned DESTINATION group per lane.  One set of functions for the
// device (k_place_runs) and the host (flacgpu_place_runs_host, place.hip, one "lane" after another over host memory), so
// that the rule is tested without a GPU.  For .hip translation units (kernels/byte_shift.h).
//   * A run of n > 0 bytes touches the groups floor(dst / 16) .. floor((dst + n - 1) / 16): place_groups of them.  The
//     lanes are numbered run after run (PlaceRun::group0 is the prefix sum); a lane finds its run by binary search
//     (place_run_of, the shape of slot_of_block in kernels/frame_scan.inc).  A group that two adjacent runs share has one
//     lane for each of them, and each lane writes only its own run's bytes.
//   * The group's bytes of the run are [lo, hi) = [max(group, dst), min(group + 16, dst + n)), never empty.  They come
//     from the aligned source group that holds the source byte of lo and, only when the hi - lo bytes reach into it, the
//     aligned source group behind it: both hold at least one byte of [src, src + n) (k_gather_slots' rule: such a group
//     cannot leave the page of that byte), combined by shift_group.
//   * hi - lo == 16: one 16-byte store.  Anything less -- the run's head in front of the first boundary, its tail behind
//     the last, a run that starts and ends inside one group -- is written with BYTE stores, one per byte of [lo, hi), and
//     never by load, merge and 16-byte store: the group's other bytes belong to someone else (the header in front, the
//     next frame, another stream's slot), and another lane or launch may be writing them at this moment.
//   * No byte outside [dst, dst + n) is written.
#ifndef FLACGPU_PLACE_RULE_H
#define FLACGPU_PLACE_RULE_H
#include <stdint.h>
#include <string.h>

#include "byte_shift.h"

struct PlaceRun {
    uint64_t src, dst, n;   // addresses (of the memory the rule runs over) and the byte count; n may be 0
    uint64_t group0;        // the run's first lane: the groups of the runs in front of it
};

// destination groups a run touches
__host__ __device__ inline uint64_t place_groups(uint64_t dst, uint64_t n) {
    return n ? ((dst + n - 1) >> 4) - (dst >> 4) + 1 : 0;
}

// the run of lane g (< the table's group count): the last one with group0 <= g.  Empty runs share their group0 with the
// run behind them (or equal the total at the table's end), so an empty run is never the answer.
__host__ __device__ inline uint32_t place_run_of(const PlaceRun *runs, uint32_t n, uint64_t g) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (runs[mid].group0 <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the aligned 16-byte group at `grp`, which holds at least one byte of [src, src_end).  The device loads the group; the
// host pass copies the group's bytes of [src, src_end) alone (the others are never looked at by place_group), so that a
// sanitizer run of the host rule checks the reads as well.
__host__ __device__ inline uint4 place_load(uint64_t grp, uint64_t src, uint64_t src_end) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)src;
    (void)src_end;
    return *reinterpret_cast<const uint4 *>(grp);
#else
    uint8_t b[16] = {0};
    const uint64_t lo = grp > src ? grp : src, hi = grp + 16 < src_end ? grp + 16 : src_end;
    memcpy(b + (lo - grp), reinterpret_cast<const void *>(lo), (size_t)(hi - lo));
    uint4 v;
    memcpy(&v, b, 16);
    return v;
#endif
}

// group k (< place_groups(r.dst, r.n)) of run r
__host__ __device__ inline void place_group(const PlaceRun &r, uint64_t k) {
    const uint64_t group = (r.dst & ~(uint64_t)15) + 16 * k, end = r.dst + r.n;
    const uint64_t lo = group > r.dst ? group : r.dst, hi = group + 16 < end ? group + 16 : end;
    const uint32_t count = (uint32_t)(hi - lo);     // 1 .. 16 bytes of the run in this group
    const uint64_t sp = r.src + (lo - r.dst);       // the source byte of lo
    const uint32_t a = (uint32_t)(sp & 15u);
    const uint4 g0 = place_load(sp - a, r.src, r.src + r.n);   // holds sp, a byte of the run
    uint4 g1 = make_uint4(0u, 0u, 0u, 0u);
    if (a + count > 16u) g1 = place_load(sp - a + 16, r.src, r.src + r.n);   // holds sp + 16 - a, a byte of the run
    const uint4 v = shift_group(g0, g1, a);         // byte j of v: the source byte sp + j
    if (count == 16u) {
        *reinterpret_cast<uint4 *>(group) = v;
        return;
    }
    uint8_t *d = reinterpret_cast<uint8_t *>(lo);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t j = 0; j < 15u; j++)   // (unrolled: w is indexed by constants alone, nothing goes to scratch)
        if (j < count) d[j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
}

// The table of `n` runs with its prefix of groups; returns the group count = the lanes of a launch.
// src_base / dst_base are added to every run's src / dst.
template <class Run>
inline uint64_t place_table(const Run *runs, uint32_t n, uint64_t src_base, uint64_t dst_base, PlaceRun *out) {
    uint64_t groups = 0;
    for (uint32_t i = 0; i < n; i++) {
        out[i] = PlaceRun{src_base + runs[i].src, dst_base + runs[i].dst, runs[i].n, groups};
        groups += place_groups(out[i].dst, out[i].n);
    }
    return groups;
}
#endif
