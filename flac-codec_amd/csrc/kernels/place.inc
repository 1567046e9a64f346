// place.inc -- k_place_runs: a table of byte runs copied inside device memory, the device encoder's back door (DESIGN.md
// 4c "Device-resident output"): frames from a context's packed buffer, and headers from the ingest handle's scratch, to
// their places in the caller's files.  Included inside place.hip's anonymous namespace, after kernels/place_rule.h.
// No LDS, no atomics, no scratch.

// Lane per destination 16-byte group of a run (place_rule.h): consecutive lanes of a run store consecutive groups, one
// uint4 each; a run's partial first and last groups are written byte by byte.  n_groups: the table's place_table() total.
__global__ void __launch_bounds__(WG) k_place_runs(const PlaceRun *__restrict__ runs, uint32_t n_runs, uint64_t n_groups) {
    const uint64_t g = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (g >= n_groups) return;
    const PlaceRun r = runs[place_run_of(runs, n_runs, g)];
    place_group(r, g - r.group0);
}
