// md5_chain.hip -- resumable MD5 chains (include/flacenc_gpu.h "resumable MD5 chains"): per-chain state kept in device
// memory between calls, k_md5_chain / k_md5_chain_final (kernels/md5_chain.inc) and the same rule over host memory
// (kernels/md5_feed_rule.h).  The chains of flacenc_device_session_* (host/device_session.cpp).
// One of the translation units of libflacenc_amd.so (gfx950 only).
#include "kernels/types.h"
#include "kernels/md5_feed_rule.h"

#include <string.h>

#include <new>
#include <string>
#include <vector>

static_assert(sizeof(flacgpu_md5_state) == sizeof(Md5Chain) && offsetof(flacgpu_md5_state, len) == offsetof(Md5Chain, len) &&
                  offsetof(flacgpu_md5_state, buf) == offsetof(Md5Chain, buf),
              "flacgpu_md5_state is Md5Chain");

namespace {
#include "kernels/md5_chain.inc"
}  // namespace

struct flacgpu_md5_chains {
    int device = 0;
    uint32_t n = 0;
    hipStream_t st = nullptr;     // final's stream
    hipEvent_t fed = nullptr;     // behind the last update, on the caller's stream
    hipEvent_t table_up = nullptr;   // behind the last upload of the piece table
    bool table_pending = false;
    Md5Chain *state = nullptr;
    flacgpu_md5_piece *pieces_dev = nullptr, *pieces_host = nullptr;   // n entries each; the host's pinned
    uint32_t *digest_dev = nullptr, *digest_host = nullptr;            // [n][4]
};

int flacgpu_md5_chains_create(int device, uint32_t n_chains, flacgpu_md5_chains **out) {
    if (!out) return FLACGPU_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_last_error = "no HIP device";
        return FLACGPU_ERR_NO_DEVICE;
    }
    if (device >= ndev) {
        g_last_error = "no such HIP device";
        return FLACGPU_ERR_NO_DEVICE;
    }
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    flacgpu_md5_chains *c = new (std::nothrow) flacgpu_md5_chains();
    if (!c) return FLACGPU_ERR_UNSUPPORTED;
    c->device = device;
    c->n = n_chains;
    const size_t n = n_chains ? n_chains : 1;
    std::vector<Md5Chain> init(n);
    for (Md5Chain &m : init) {
        memset(&m, 0, sizeof m);
        md5_chain_init(m);
    }
    hipError_t e;
    {
        DeviceGuard guard(device);
        e = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fed, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->table_up, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->state), sizeof(Md5Chain) * n);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->pieces_dev), sizeof(flacgpu_md5_piece) * n);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->digest_dev), 16 * n);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&c->pieces_host), sizeof(flacgpu_md5_piece) * n, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&c->digest_host), 16 * n, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMemcpy(c->state, init.data(), sizeof(Md5Chain) * n, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        g_last_error = std::string("flacgpu_md5_chains_create: ") + hipGetErrorString(e);
        flacgpu_md5_chains_destroy(c);
        return FLACGPU_ERR_HIP;
    }
    *out = c;
    return FLACGPU_OK;
}

void flacgpu_md5_chains_destroy(flacgpu_md5_chains *c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->fed) (void)hipEventSynchronize(c->fed);   // (an event never recorded is complete)
    if (c->st) (void)hipStreamSynchronize(c->st);
    if (c->fed) (void)hipEventDestroy(c->fed);
    if (c->table_up) (void)hipEventDestroy(c->table_up);
    if (c->st) (void)hipStreamDestroy(c->st);
    (void)hipFree(c->state);
    (void)hipFree(c->pieces_dev);
    (void)hipFree(c->digest_dev);
    (void)hipHostFree(c->pieces_host);
    (void)hipHostFree(c->digest_host);
    delete c;
}

int flacgpu_md5_chains_update(flacgpu_md5_chains *c, const int32_t *d_samples, const flacgpu_md5_piece *pieces,
                              uint32_t n_pieces, uint32_t width, void *stream) {
    if (!c || (n_pieces && !pieces)) return FLACGPU_ERR_INVALID_ARG;
    if (width < 1 || width > 4) {
        g_last_error = "flacgpu_md5_chains_update: width outside 1..4";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (n_pieces > c->n) {
        g_last_error = "flacgpu_md5_chains_update: more pieces than chains: a chain is named twice";
        return FLACGPU_ERR_INVALID_ARG;
    }
    std::vector<bool> seen(c->n, false);
    bool any = false;
    for (uint32_t p = 0; p < n_pieces; p++) {
        const flacgpu_md5_piece &pc = pieces[p];
        if (pc.chain >= c->n || pc.reserved || pc.count > ((uint64_t)1 << 58) || seen[pc.chain]) {
            g_last_error = "flacgpu_md5_chains_update: piece " + std::to_string(p) +
                           " names no chain, names one twice, is longer than 2^58 samples or has reserved != 0";
            return FLACGPU_ERR_INVALID_ARG;
        }
        seen[pc.chain] = true;
        any |= pc.count != 0;
    }
    if (!any) return FLACGPU_OK;
    if (!d_samples) return FLACGPU_ERR_INVALID_ARG;
    DeviceGuard guard(c->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (c->table_pending) HIP_TRY(hipEventSynchronize(c->table_up));   // the pinned table is still on its way up
    c->table_pending = false;
    memcpy(c->pieces_host, pieces, sizeof(flacgpu_md5_piece) * (size_t)n_pieces);
    HIP_TRY(hipMemcpyAsync(c->pieces_dev, c->pieces_host, sizeof(flacgpu_md5_piece) * (size_t)n_pieces, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(c->table_up, st));
    c->table_pending = true;
    hipLaunchKernelGGL(k_md5_chain, dim3(n_pieces), dim3(64), 0, st, d_samples, c->pieces_dev, c->state, width);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->fed, st));
    return FLACGPU_OK;
}

int flacgpu_k::md5_chains_update_widths(flacgpu_md5_chains *c, const int32_t *d_samples, const flacgpu_md5_piece *pieces,
                                        const uint32_t *width, uint32_t n_pieces, hipStream_t st) {
    if (!c || !n_pieces) return FLACGPU_OK;
    if (n_pieces > c->n || !pieces || !width || !d_samples) return FLACGPU_ERR_INVALID_ARG;
    uint32_t first[6] = {0, 0, 0, 0, 0, 0};   // pieces of width w: [first[w], first[w + 1]) of the table
    for (uint32_t p = 0; p < n_pieces; p++) {
        if (width[p] < 1 || width[p] > 4 || pieces[p].chain >= c->n) return FLACGPU_ERR_INVALID_ARG;
        first[width[p] + 1]++;
    }
    for (uint32_t w = 1; w < 6; w++) first[w] += first[w - 1];
    DeviceGuard guard(c->device);
    if (c->table_pending) HIP_TRY(hipEventSynchronize(c->table_up));   // the pinned table is still on its way up
    c->table_pending = false;
    uint32_t at[5] = {0, first[1], first[2], first[3], first[4]};
    for (uint32_t p = 0; p < n_pieces; p++) c->pieces_host[at[width[p]]++] = pieces[p];
    HIP_TRY(hipMemcpyAsync(c->pieces_dev, c->pieces_host, sizeof(flacgpu_md5_piece) * (size_t)n_pieces, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(c->table_up, st));
    c->table_pending = true;
    for (uint32_t w = 1; w <= 4; w++) {
        const uint32_t count = first[w + 1] - first[w];
        if (count) hipLaunchKernelGGL(k_md5_chain, dim3(count), dim3(64), 0, st, d_samples, c->pieces_dev + first[w], c->state, w);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->fed, st));
    return FLACGPU_OK;
}

int flacgpu_md5_chains_final(flacgpu_md5_chains *c, uint8_t *md5_out) {
    if (!c || (c->n && !md5_out)) return FLACGPU_ERR_INVALID_ARG;
    if (!c->n) return FLACGPU_OK;
    DeviceGuard guard(c->device);
    HIP_TRY(hipStreamWaitEvent(c->st, c->fed, 0));
    hipLaunchKernelGGL(k_md5_chain_final, dim3((c->n + 63) / 64), dim3(64), 0, c->st, c->state, c->n, c->digest_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->digest_host, c->digest_dev, 16 * (size_t)c->n, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    memcpy(md5_out, c->digest_host, 16 * (size_t)c->n);
    return FLACGPU_OK;
}

uint32_t flacgpu_md5_stage_bytes(void) { return MD5_STAGE_BYTES; }

void flacgpu_md5_init_host(flacgpu_md5_state *state) {
    if (!state) return;
    Md5Chain c;
    memset(&c, 0, sizeof c);
    md5_chain_init(c);
    memcpy(state, &c, sizeof c);
}

int flacgpu_md5_feed_host(flacgpu_md5_state *state, const int32_t *samples, uint64_t count, uint32_t width) {
    if (!state || (count && !samples) || width < 1 || width > 4 || count > ((uint64_t)1 << 58)) {
        g_last_error = "flacgpu_md5_feed_host: no state, no samples, more than 2^58 of them, or a width outside 1..4";
        return FLACGPU_ERR_INVALID_ARG;
    }
    Md5Chain c;
    memcpy(&c, state, sizeof c);
    md5_feed_host(c, samples, count, width);
    memcpy(state, &c, sizeof c);
    return FLACGPU_OK;
}

int flacgpu_md5_final_host(flacgpu_md5_state *state, uint8_t md5[16]) {
    if (!state || !md5) return FLACGPU_ERR_INVALID_ARG;
    Md5Chain c;
    memcpy(&c, state, sizeof c);
    md5_final_host(c, md5);
    memcpy(state, &c, sizeof c);
    return FLACGPU_OK;
}
