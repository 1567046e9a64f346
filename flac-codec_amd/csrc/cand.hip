// cand.hip -- K2+K5 wave kernel k_cand64: FIXED + LPC + Rice search + choice of one candidate per wave.
// One of the translation units of libflacenc_amd.so (gfx950 only; built with -ffp-contract=off, see
// Makefile); the kernels are reached through the launchers declared in kernels/types.h.
#include "kernels/types.h"

#include <stdlib.h>

namespace {
#include "kernels/common.inc"
#include "kernels/wave_cand.inc"
}  // namespace

namespace flacgpu_k {
bool launch_cand64(const Params &p, const Knobs &kn, uint32_t B, uint32_t blocks, hipStream_t st) {
    if (p.inter) {   // interleaved stereo input read in place: persistent kernels only (cand_direct.hip)
        return launch_cand64_direct(p, kn, B, blocks, st);
    }
    // (the callers pass a wave block length, and orders 17..32 with 4096-sample blocks only: analyze_impl's `w64`)
    if (B == FN && p.max_lpc_order > 16) {
        const uint32_t cap = kn.cand_grid ? kn.cand_grid : 512u;
        const uint32_t grid = blocks < cap ? blocks : cap;
        const bool stereo = p.stereo4 && p.ncand == 4;
        if (stereo) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64p<64, 32, true>), dim3(grid), dim3(WG), 0, st, p);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64p<64, 32, false>), dim3(grid), dim3(WG), 0, st, p);
        return stereo;
    }
    // persistent variant with LDS prefetch: the L/R/M/S candidates of 4096-sample blocks, order <= 16; three workgroups
    // per CU (165 VGPRs, 32 KB of LDS)
    const bool stereo_cands = p.stereo4 && p.ncand == 4;
    if (B == FN && p.max_lpc_order <= 16 && stereo_cands) {
        const uint32_t cap = kn.cand_grid ? kn.cand_grid : 768u;
        const uint32_t grid = blocks < cap ? blocks : cap;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64p<64, 16, true>), dim3(grid), dim3(WG), 0, st, p);
        return true;
    }
    // independent channels (mono, 3..8 channels, wide stereo) are not persistent: that kernel's four 16 KB rows per workgroup
    // allowed two workgroups per CU; k_cand64<64, 16, false> (152 VGPRs, no LDS) runs three waves per SIMD and is faster
    // (config 4: 0.50 -> 0.33 ms per batch)
    if (B == FN && !p.stereo4) {   // the instantiation without mid / side
        if (p.xpose) {   // 3, 4 / 8 channels read in place from the interleaved batch (load_lane_xpose): CW waves per workgroup
            const uint32_t cands = p.fcount * p.ncand;
            if (p.channels == 3 || p.channels == 6) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64<64, 16, false, 3>), dim3(cands / 3), dim3(192), 0, st, p);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64<64, 16, false, 4>), dim3(cands / 4), dim3(WG), 0, st, p);
        }
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64<64, 16, false>), dim3(blocks), dim3(WG), 0, st, p);
        return false;
    }
    // the shorter wave block lengths (4096 went one of the ways above: a context with stereo4 has ncand == 4, create_impl)
    switch (B) {
    case 2304: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64<36, 16>), dim3(blocks), dim3(WG), 0, st, p); break;
    case 2048: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64<32, 16>), dim3(blocks), dim3(WG), 0, st, p); break;
    case 1152: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64<18, 16>), dim3(blocks), dim3(WG), 0, st, p); break;
    case 1024: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cand64<16, 16>), dim3(blocks), dim3(WG), 0, st, p); break;
    default: break;
    }
    return false;
}
}  // namespace flacgpu_k
