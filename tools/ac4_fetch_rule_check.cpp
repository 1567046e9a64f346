// The input schedule of k_autocorr4 / k_autocorr4_deep, walked on the host with the rule the kernels use
// (ac4_fetch_slot, ac4_fetch_next: kernels/shape.h): prints every request and every conversion in program order.
//   g++ -std=c++17 -I flac-codec_amd/csrc -o ac4_fetch_rule_check tools/ac4_fetch_rule_check.cpp
//   ac4_fetch_rule_check <ntiles> [depth]      (depth defaults to the library's AC4_FETCH_DEPTH)
// "R <index> <tile> <set>": tile index requested, the tile the request reads (clamped), the staging set it fills
// "C <index> <set>": the conversion of tile <index> (into tile buffer index & 1) reads staging set <set>
// tests/test_ac4_fetch_rule.py holds the trace to the schedule's contract.
#include <stdio.h>
#include <stdlib.h>

#include "kernels/shape.h"

static_assert(ac4_fetch_slot(5, 4, 2).tile == 3 && ac4_fetch_slot(5, 4, 2).set == 1, "usable in constant expressions");

static void request(uint32_t t, uint32_t ntiles, uint32_t depth) {
    const Ac4FetchSlot s = ac4_fetch_slot(t, ntiles, depth);
    printf("R %u %u %u\n", t, s.tile, s.set);
}
static void convert(uint32_t t, uint32_t depth) { printf("C %u %u\n", t, ac4_fetch_slot(t, ~0u, depth).set); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const uint32_t ntiles = (uint32_t)strtoul(argv[1], nullptr, 10);
    const uint32_t depth = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 10) : (uint32_t)AC4_FETCH_DEPTH;
    if (!ntiles || !depth) return 2;
    printf("D %u\n", depth);
    // before the tile loop (ac4_wave, ac4_wave_deep)
    request(0, ntiles, depth);
    convert(0, depth);
    for (uint32_t k = 1; k <= depth; k++) request(k, ntiles, depth);
    // tile t: tile t + 1 converted, then tile ac4_fetch_next(t) requested
    for (uint32_t t = 0; t < ntiles; t++) {
        convert(t + 1, depth);
        request(ac4_fetch_next(t, depth), ntiles, depth);
    }
    return 0;
}
