// decode.hip -- device-side frame decoder + verifier (decode.rs:1388-1856), one lane per subframe, and the
// stand-alone decoder of a whole stream built on it (flacgpu_decode_stream; its host-side parsing is host/flac_stream.cpp).
// One of the translation units of libflacenc_amd.so (gfx950 only; built with -ffp-contract=off, see
// Makefile); the kernels are reached through the launchers declared in kernels/types.h.
#include "kernels/types.h"
#include "flac_stream.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>

namespace {
#include "kernels/common.inc"
#include "kernels/decode.inc"
}  // namespace

namespace flacgpu_k {
// One lane per subframe.  Every lane reads and writes its own cache lines, so the limit is the
// CU's address path (lines per instruction x waves per CU), not the SIMD: measured on 4096 / 8192
// / 32768 stereo frames, 32-lane waves win over 64 (fewer lines per instruction) and over 16 or 8
// (fewer waves per CU): 1.17 / 1.44 / 2.93 ms.
void launch_decode(uint32_t mo, uint32_t units, const Params &pd, const PackParams &q, int32_t *decoded,
                   uint32_t *verify_counts, hipStream_t st) {
    const uint32_t lanes = 32;
    const dim3 grid((units + lanes - 1) / lanes), block(lanes);
    // FIXED needs 4; the ring is also the store batch
    if (mo <= 8) hipLaunchKernelGGL(k_decode<8>, grid, block, 0, st, pd, q, decoded, verify_counts);
    else if (mo <= 12) hipLaunchKernelGGL(k_decode<12>, grid, block, 0, st, pd, q, decoded, verify_counts);
    else if (mo <= 16) hipLaunchKernelGGL(k_decode<16>, grid, block, 0, st, pd, q, decoded, verify_counts);
    else hipLaunchKernelGGL(k_decode<32>, grid, block, 0, st, pd, q, decoded, verify_counts);
}
void launch_decode_finish(const Params &p, int32_t *decoded, const int32_t *expect, uint32_t *verify_counts,
                          hipStream_t st, const uint32_t *frame_n) {
    hipLaunchKernelGGL(k_decode_finish, dim3(p.n_frames), dim3(WG), 0, st, p, decoded, expect, verify_counts,
                       frame_n);
}
// stand-alone decode: one lane per frame, 32-lane waves (see launch_decode), any LPC order
void launch_decode_frames(const uint32_t *words, const uint64_t *frame_off, const uint32_t *frame_n,
                          uint64_t cap_bytes, uint32_t n_frames, uint32_t channels, uint32_t bps, uint32_t ldb,
                          int32_t *decoded, uint32_t *verify_counts, hipStream_t st) {
    DecodeParams dp{words, frame_off, frame_n, cap_bytes, n_frames, channels, bps, ldb};
    const uint32_t lanes = 32;
    hipLaunchKernelGGL(k_decode_frames<32>, dim3((n_frames + lanes - 1) / lanes), dim3(lanes), 0, st, dp, decoded,
                       verify_counts);
}
}  // namespace flacgpu_k

// ---- stand-alone decoder: any FLAC stream (fLaC marker, metadata, frames) --------------------
using namespace flacgpu_k;

// The host half: metadata and frame boundaries (host/flac_stream.cpp), `info` as the scan leaves it.
static int scan_stream(const uint8_t *data, size_t len, flacgpu_stream_info *info, flacenc::FrameScan &scan) {
    uint32_t min_frame = 0;
    size_t pos = 0;
    if (const char *why = flacenc::parse_metadata(data, len, info, &min_frame, &pos)) {
        if (*why) g_last_error = why;
        return FLACGPU_ERR_INVALID_ARG;
    }
    flacenc::scan_frames(data, len, pos, min_frame, info, scan);
    return FLACGPU_OK;
}

int flacgpu_scan_stream_host(const uint8_t *data, size_t len, flacgpu_stream_info *info, uint64_t *frame_off,
                             uint32_t *frame_n, size_t cap, uint32_t *n_frames) {
    if (!data || !info || !n_frames) return FLACGPU_ERR_INVALID_ARG;
    *n_frames = 0;
    flacenc::FrameScan scan;
    if (int rc = scan_stream(data, len, info, scan)) return rc;
    *n_frames = info->frames;
    if ((frame_off || frame_n) && cap < info->frames) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (frame_off) std::copy(scan.off.begin(), scan.off.end() - 1, frame_off);
    if (frame_n) std::copy(scan.n.begin(), scan.n.end(), frame_n);
    return FLACGPU_OK;
}

// The raw-frame rule (host/flac_stream.cpp scan_raw_frames) for one input, without a device.
int flacgpu_scan_frames_host(const uint8_t *data, size_t len, flacgpu_frame_record *frames, size_t cap,
                             uint32_t *n_frames, flacgpu_raw_stream *summary) {
    return flacgpu_scan_frames_host_ex(data, len, 0, frames, cap, n_frames, summary);
}

int flacgpu_scan_frames_host_ex(const uint8_t *data, size_t len, uint32_t flags, flacgpu_frame_record *frames, size_t cap,
                                uint32_t *n_frames, flacgpu_raw_stream *summary) {
    if ((!data && len) || !n_frames || !summary || (flags & ~FLACGPU_SCAN_SPECULATIVE)) return FLACGPU_ERR_INVALID_ARG;
    *n_frames = 0;
    std::vector<flacgpu_frame_record> found;
    flacgpu_raw_stream sum{};
    flacenc::scan_raw_frames(data, len, flags, found, sum);
    *n_frames = sum.frames;
    if (frames && cap < found.size()) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (frames) std::copy(found.begin(), found.end(), frames);
    *summary = sum;
    return FLACGPU_OK;
}

int flacgpu_timeline_host(const flacgpu_frame_record *records, size_t n_records, flacgpu_timeline_frame *frames_out,
                          size_t cap, flacgpu_timeline_result *result) {
    if ((!records && n_records) || !result) return FLACGPU_ERR_INVALID_ARG;
    if (frames_out && cap < n_records) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (const char *why = flacenc::timeline_of_records(records, n_records, frames_out, *result))
        g_last_error = std::string("flacgpu_timeline_host: ") + why;
    return FLACGPU_OK;
}

uint32_t flacgpu_timeline_piece_bytes(void) { return FLACGPU_TIMELINE_PIECE_BYTES; }

// Decodes a whole FLAC stream held in host memory: the host finds the frame boundaries (scan_stream), the GPU decodes the
// frames in parallel, one lane per frame, re-checks every CRC-16 and undoes the stereo decorrelation; the host compares
// the MD5 of the decoded PCM with STREAMINFO's (decode.rs:1282 `verify`, 1388-1436 read_frame, 1494-1856).
int flacgpu_decode_stream(const uint8_t *data, size_t len, int device, int32_t *out, size_t out_cap,
                          flacgpu_stream_info *info) {
    if (!data || !info) return FLACGPU_ERR_INVALID_ARG;
    flacenc::FrameScan scan;
    if (int rc = scan_stream(data, len, info, scan)) return rc;
    const size_t F = scan.n.size(), C = info->channels;
    if (F == 0) return FLACGPU_OK;
    if (out && out_cap < info->decoded_samples * C) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_last_error = "no HIP device";
        return FLACGPU_ERR_NO_DEVICE;
    }
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    DeviceGuard guard(device);
    const uint32_t maxn = *std::max_element(scan.n.begin(), scan.n.end());
    const size_t ldb = (maxn + 3u) & ~3u;
    // ---- device buffers (freed on every path by the guard object below)
    struct Bufs {
        void *bytes = nullptr, *off = nullptr, *fn = nullptr, *pcm = nullptr, *counts = nullptr;
        hipStream_t st = nullptr;
        ~Bufs() {
            (void)hipFree(bytes); (void)hipFree(off); (void)hipFree(fn); (void)hipFree(pcm); (void)hipFree(counts);
            if (st) (void)hipStreamDestroy(st);
        }
    } b;
    const size_t bytes_cap = (len + 64 + 3) & ~(size_t)3;
    HIP_TRY(hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&b.bytes, bytes_cap));
    HIP_TRY(hipMalloc(&b.off, sizeof(uint64_t) * (F + 1)));
    HIP_TRY(hipMalloc(&b.fn, sizeof(uint32_t) * F));
    HIP_TRY(hipMalloc(&b.pcm, sizeof(int32_t) * (F * C * ldb + 64)));
    HIP_TRY(hipMalloc(&b.counts, sizeof(uint32_t) * (4 + F)));
    HIP_TRY(hipMemsetAsync(b.bytes, 0, bytes_cap, b.st));
    HIP_TRY(hipMemcpyAsync(b.bytes, data, len, hipMemcpyHostToDevice, b.st));
    HIP_TRY(hipMemcpyAsync(b.off, scan.off.data(), sizeof(uint64_t) * (F + 1), hipMemcpyHostToDevice, b.st));
    HIP_TRY(hipMemcpyAsync(b.fn, scan.n.data(), sizeof(uint32_t) * F, hipMemcpyHostToDevice, b.st));
    HIP_TRY(hipMemsetAsync(b.counts, 0, sizeof(uint32_t) * (4 + F), b.st));
    launch_decode_frames((const uint32_t *)b.bytes, (const uint64_t *)b.off, (const uint32_t *)b.fn, bytes_cap,
                         (uint32_t)F, (uint32_t)C, info->bits_per_sample, (uint32_t)ldb, (int32_t *)b.pcm,
                         (uint32_t *)b.counts, b.st);
    Params pp{};
    pp.channels = (uint32_t)C;
    pp.bps = info->bits_per_sample;
    pp.block_size = maxn;
    pp.ldb = (uint32_t)ldb;
    pp.n_frames = (uint32_t)F;
    pp.last_len = scan.n[F - 1];
    pp.fcount = (uint32_t)F;
    PackParams q;
    q.first_frame_number = 0;
    q.sample_rate = info->sample_rate;
    q.out_words = (uint32_t *)b.bytes;
    q.frame_off = (uint64_t *)b.off;
    q.cap_bytes = bytes_cap;
    launch_crc(true, pp, q, (uint32_t)F, (uint32_t *)b.counts, b.st);
    launch_decode_finish(pp, (int32_t *)b.pcm, nullptr, (uint32_t *)b.counts, b.st, (const uint32_t *)b.fn);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> planar;
    try {   // sizes come from the (untrusted) stream's headers: an allocation failure is an error code, not an exception
        planar.resize(F * C * ldb);
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decode_stream: out of host memory for the decoded PCM";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    uint32_t counts[4];
    HIP_TRY(hipMemcpyAsync(planar.data(), b.pcm, sizeof(int32_t) * planar.size(), hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipMemcpyAsync(counts, b.counts, sizeof counts, hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipStreamSynchronize(b.st));
    info->bad_frames += counts[0];
    info->bad_crc16 = counts[1];
    flacenc::finish_stream(planar.data(), ldb, scan.n, out, info);
    return FLACGPU_OK;
}
