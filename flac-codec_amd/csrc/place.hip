// place.hip -- k_place_runs (kernels/place.inc), its launcher for the translation units that own run tables
// (flacenc_gpu.hip: flacgpu_place_frames; ingest.hip: flacgpu_ingest_place), and the same rule over host memory
// (flacgpu_place_runs_host).
// One of the translation units of libflacenc_amd.so (gfx950 only).
#include "kernels/types.h"
#include "kernels/place_rule.h"

#include <new>
#include <vector>

namespace {
#include "kernels/place.inc"
}  // namespace

namespace flacgpu_k {
int launch_place_runs(const PlaceRun *d_runs, uint32_t n_runs, uint64_t n_groups, hipStream_t st) {
    if (!n_groups) return FLACGPU_OK;
    const uint64_t blocks = (n_groups + WG - 1) / WG;
    if (blocks > 0x7FFFFFFFull) {
        g_last_error = "k_place_runs: more than 2^31 - 1 workgroups";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(k_place_runs, dim3((uint32_t)blocks), dim3(WG), 0, st, d_runs, n_runs, n_groups);
    HIP_TRY(hipGetLastError());
    return FLACGPU_OK;
}
}  // namespace flacgpu_k

uint32_t flacgpu_place_workgroup(void) { return WG; }

int flacgpu_place_runs_host(const flacgpu_place_run *runs, uint32_t n_runs) {
    if (!runs && n_runs) {
        g_last_error = "flacgpu_place_runs_host: no run table";
        return FLACGPU_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; i < n_runs; i++)
        if (runs[i].n && (runs[i].src + runs[i].n < runs[i].src || runs[i].dst + runs[i].n < runs[i].dst)) {
            g_last_error = "flacgpu_place_runs_host: a run wraps round the address space";
            return FLACGPU_ERR_INVALID_ARG;
        }
    std::vector<PlaceRun> tab(n_runs);
    const uint64_t groups = place_table(runs, n_runs, 0, 0, tab.data());
    for (uint64_t g = 0; g < groups; g++) {   // one "lane" after another, as k_place_runs numbers them
        const PlaceRun &r = tab[place_run_of(tab.data(), n_runs, g)];
        place_group(r, g - r.group0);
    }
    return FLACGPU_OK;
}
