// autocorr.hip -- K3: window + exact autocorrelation (encode.rs:1785-1801, 3478-3501) and the MFMA experiment.
// One of the translation units of libflacenc_amd.so (gfx950 only; built with -ffp-contract=off, see
// Makefile); the kernels are reached through the launchers declared in kernels/types.h.
#include "kernels/types.h"
#include "batch_route.h"

#include <stdlib.h>

#include <type_traits>

namespace {
#include "kernels/common.inc"
#include "kernels/lpc.inc"        // lpc_candidate: the Levinson tail of the DIRECT k_autocorr4 instantiations
#include "kernels/autocorr.inc"

using flacenc_route::AcKernel;

// k_autocorr4<NL, ...> as plan_autocorr chose it
template <int NL>
void launch_autocorr4(const AcKernel &k, const Params &p, uint32_t frame0, uint32_t nframes, uint32_t n, const double *win,
                      hipStream_t st) {
    const uint32_t groups = (nframes * p.ncand + 63) / 64;
#define AC4_LAUNCH(NS, ...)                                                                                           \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_autocorr4<__VA_ARGS__>), dim3(groups), dim3(64 * NS), 0, st, p, frame0, nframes, n, win)
    switch (k.producer) {
    case AcKernel::DIRECT:
        if (k.ns == 8) AC4_LAUNCH(8, 13, 8, true, true, 0, true);   // (plan_autocorr: NL == 13 only)
        else AC4_LAUNCH(4, NL, 4, true, true, 0, true);
        break;
    case AcKernel::SPLIT8: AC4_LAUNCH(4, NL, 4, false, true, 8, true); break;
    case AcKernel::SPLIT4: AC4_LAUNCH(4, NL, 4, false, true, 4, true); break;
    case AcKernel::SPLIT: AC4_LAUNCH(4, NL, 4, false, true, 0, true); break;
    case AcKernel::PLANAR:
        if (k.stereo) {
            if (k.ns == 2) AC4_LAUNCH(2, NL, 2, true);
            else AC4_LAUNCH(4, NL, 4, true);
        } else {
            if (k.ns == 2) AC4_LAUNCH(2, NL, 2, false);
            else AC4_LAUNCH(4, NL, 4, false);
        }
        break;
    }
#undef AC4_LAUNCH
}

template <int H>
void launch_autocorr(const Params &p, uint32_t frame0, uint32_t nframes, uint32_t n,
                     const double *win, hipStream_t st) {
    const uint32_t lanes = nframes * p.ncand;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_autocorr2<H, 4>), dim3((lanes + 63) / 64), dim3(WG), 0, st, p,
                       frame0, nframes, n, win);
}
}  // namespace

namespace flacgpu_k {
// the kernel is plan_autocorr's choice (host/batch_route.cpp): the conditions live there, the instantiations here
bool dispatch_autocorr(const Params &p_in, const Knobs &kn, uint32_t frame0, uint32_t nframes, uint32_t n, const double *win,
                       hipStream_t st) {
    Params p = p_in;
    flacenc_route::AcLaunch a;
    a.ncand = p.ncand;
    a.stereo4 = p.stereo4;
    a.channels = p.channels;
    a.bps = p.bps;
    a.max_lpc_order = p.max_lpc_order;
    a.n = n;
    a.block_size = p.block_size;
    a.inter = p.inter != nullptr;
    a.split_src = p.split_src != nullptr;
    a.ac_split = p.ac_split;
    a.nframes = nframes;
    a.whole_batch = frame0 == 0 && nframes == p.n_frames;
    a.mfma = kn.experiment_mfma_ac;
    a.fma_t0 = p.fma_t0;
    a.fma_t1 = p.fma_t1;
    const AcKernel k = flacenc_route::plan_autocorr(a);
    if (!k.fused_tiles) p.fma_t0 = p.fma_t1 = 0;
    const uint32_t groups = (nframes * p.ncand + 63) / 64;
    switch (k.family) {
    case AcKernel::MFMA:
        hipLaunchKernelGGL(k_autocorr_mfma, dim3((nframes * p.ncand + 3) / 4), dim3(WG), 0, st, p, n, win, p.ac);
        break;
    case AcKernel::AC4_DEEP:
        if (k.producer == AcKernel::DIRECT)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_autocorr4_deep<true, true>), dim3(groups), dim3(256), 0, st, p, frame0, nframes, n, win);
        else if (k.stereo)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_autocorr4_deep<true>), dim3(groups), dim3(256), 0, st, p, frame0, nframes, n, win);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_autocorr4_deep<false>), dim3(groups), dim3(256), 0, st, p, frame0, nframes, n, win);
        break;
    case AcKernel::AC4:
        switch (k.size) {
        case 5: launch_autocorr4<5>(k, p, frame0, nframes, n, win, st); break;
        case 9: launch_autocorr4<9>(k, p, frame0, nframes, n, win, st); break;
        case 13: launch_autocorr4<13>(k, p, frame0, nframes, n, win, st); break;
        default: launch_autocorr4<17>(k, p, frame0, nframes, n, win, st); break;
        }
        break;
    default:   // AC2 (RAGGED: launch_autocorr_ragged)
        switch (k.size) {
        case 4: launch_autocorr<4>(p, frame0, nframes, n, win, st); break;
        case 8: launch_autocorr<8>(p, frame0, nframes, n, win, st); break;
        case 12: launch_autocorr<12>(p, frame0, nframes, n, win, st); break;
        case 16: launch_autocorr<16>(p, frame0, nframes, n, win, st); break;
        case 20: launch_autocorr<20>(p, frame0, nframes, n, win, st); break;
        case 24: launch_autocorr<24>(p, frame0, nframes, n, win, st); break;
        case 28: launch_autocorr<28>(p, frame0, nframes, n, win, st); break;
        case 32: launch_autocorr<32>(p, frame0, nframes, n, win, st); break;
        default: launch_autocorr<36>(p, frame0, nframes, n, win, st); break;
        }
        break;
    }
    return k.fused_k4;
}
void launch_autocorr_ragged(const Params &p, hipStream_t st) {
    flacenc_route::AcLaunch a;
    a.max_lpc_order = p.max_lpc_order;
    a.ragged = true;
    const uint32_t H = flacenc_route::plan_autocorr(a).size;
    const dim3 grid((p.n_frames * p.ncand + 63) / 64);
#define AC_RAGGED(h) case h: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_autocorr_ragged<h, 4>), grid, dim3(WG), 0, st, p); break;
    switch (H) {
        AC_RAGGED(4) AC_RAGGED(8) AC_RAGGED(12) AC_RAGGED(16) AC_RAGGED(20) AC_RAGGED(24) AC_RAGGED(28) AC_RAGGED(32)
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_autocorr_ragged<36, 4>), grid, dim3(WG), 0, st, p); break;
    }
#undef AC_RAGGED
}
void launch_autocorr_mfma(const Params &p, uint32_t blocks, uint32_t n, const double *win, double *ac,
                          hipStream_t st) {
    hipLaunchKernelGGL(k_autocorr_mfma, dim3(blocks), dim3(WG), 0, st, p, n, win, ac);
}
}  // namespace flacgpu_k

#if AC4_TIMELINE
// measurement builds only (tools/ac4_timeline.py): the tile records of the last k_autocorr4 launches, copied to the host
// (clear != 0: zeroed afterwards); returns the buffer's size in bytes, 0 on a HIP error
extern "C" size_t flacgpu_ac4_timeline(void *dst, size_t bytes, int clear) {
    const size_t all = sizeof(uint32_t) * AC4_TL_WAVES * AC4_TL_TILES * AC4_TL_WORDS;
    if (hipDeviceSynchronize() != hipSuccess) return 0;
    if (dst && hipMemcpyFromSymbol(dst, HIP_SYMBOL(ac4_tl), bytes < all ? bytes : all) != hipSuccess) return 0;
    if (clear) {
        void *sym = nullptr;
        if (hipGetSymbolAddress(&sym, HIP_SYMBOL(ac4_tl)) != hipSuccess || hipMemset(sym, 0, all) != hipSuccess) return 0;
        if (hipDeviceSynchronize() != hipSuccess) return 0;
    }
    return all;
}
#endif
