// ingest.hip -- the device half of flacenc_encode_many_device (host/device_batch.cpp): the ingest pass that turns a
// caller's device tensor into interleaved int32 in a staging buffer of the library's (kernels/ingest.inc), and the MD5
// of every ingested stream (k_md5_many, reached through decode_many.hip's launcher).
// One of the translation units of libflacenc_amd.so (gfx950 only).
#include "kernels/types.h"
#include "kernels/ingest_rule.h"
#include "kernels/place_rule.h"
#include "kernels/sample_types.h"

#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {
#include "kernels/ingest.inc"

// a buffer that only grows: device memory, or pinned host memory
template <bool PINNED> struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;
    void release() { (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    int ensure(size_t bytes) {
        if (bytes <= cap) return FLACGPU_OK;
        release();
        if (PINNED) HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        else HIP_TRY(hipMalloc(&p, bytes));
        cap = bytes;
        return FLACGPU_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    ~GrowBuf() { release(); }
};

template <uint32_t DT>
void launch_ingest(bool padded, uint32_t tiles, hipStream_t st, const void *in, const IngestStream *streams, uint32_t n,
                   uint32_t channels, uint32_t bps, uint64_t samples_padded, int32_t *staging, uint32_t *altered) {
    const auto k = padded ? k_ingest<DT, true> : k_ingest<DT, false>;
    hipLaunchKernelGGL(k, dim3(tiles), dim3(WG), 0, st, static_cast<const uint8_t *>(in), streams, n, channels, bps,
                       samples_padded, staging, altered);
}
}  // namespace

struct flacgpu_ingest {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev = nullptr;
    GrowBuf<false> staging, streams, altered, jobs, digest;
    GrowBuf<true> table, results;   // pinned: the tables on their way up, altered counts and digests on their way down
    // flacgpu_ingest_place: the callers' pieces and the run table, pinned and on the device
    GrowBuf<true> piece_host, run_host;
    GrowBuf<false> piece_dev, run_dev;
    uint32_t n = 0;
    bool md5 = false, pending = false;
};

int flacgpu_ingest_create(int device, flacgpu_ingest **out) {
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
    flacgpu_ingest *g = new (std::nothrow) flacgpu_ingest();
    if (!g) return FLACGPU_ERR_UNSUPPORTED;
    g->device = device;
    hipError_t e;
    {
        DeviceGuard guard(device);
        e = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        g_last_error = std::string("flacgpu_ingest_create: ") + hipGetErrorString(e);
        flacgpu_ingest_destroy(g);
        return FLACGPU_ERR_HIP;
    }
    *out = g;
    return FLACGPU_OK;
}

void flacgpu_ingest_destroy(flacgpu_ingest *g) {
    if (!g) return;
    DeviceGuard guard(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    if (g->ev) (void)hipEventDestroy(g->ev);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;   // the buffers free themselves, on the handle's device
}

int flacgpu_ingest_device(const flacgpu_ingest *g) { return g ? g->device : -1; }

int flacgpu_ingest_submit(flacgpu_ingest *g, const void *d_pcm, const flacgpu_out_format *fmt, uint32_t bits_per_sample,
                          uint32_t channels, const flacgpu_ingest_stream *streams, uint32_t n_streams,
                          uint64_t staging_elements, uint32_t flags, void *stream, int32_t **d_staging) {
    if (!g || !fmt || !d_staging || (n_streams && !streams) || (flags & ~FLACGPU_INGEST_MD5)) return FLACGPU_ERR_INVALID_ARG;
    *d_staging = nullptr;
    const bool padded = fmt->layout == FLACGPU_LAYOUT_PADDED;
    const uint32_t widest = sample_type_max_bits(fmt->dtype);
    if (!sample_type_known(fmt->dtype) || fmt->layout > FLACGPU_LAYOUT_PADDED || channels < 1 ||
        channels > FLACGPU_MAX_CHANNELS || bits_per_sample < 1 || bits_per_sample > 32 ||
        (widest && bits_per_sample > widest) || (padded && fmt->channels_padded < channels) ||
        reinterpret_cast<uintptr_t>(d_pcm) % sample_type_align(fmt->dtype)) {
        g_last_error = "flacgpu_ingest_submit: a format, shape or alignment that flacenc_device_batch_plan refuses";
        return FLACGPU_ERR_INVALID_ARG;
    }
    DeviceGuard guard(g->device);
    if (g->pending) HIP_TRY(hipStreamSynchronize(g->st));   // an unfinished batch: its tables and results are still in use
    g->pending = false;
    g->n = n_streams;
    g->md5 = flags & FLACGPU_INGEST_MD5;
    // ---- the tile table; every stream must lie inside the staging buffer, on a 16-byte boundary
    const uint32_t ts = ingest_tile_samples(channels);
    const size_t table_bytes = sizeof(IngestStream) * (size_t)n_streams + sizeof(flacgpu_k::Md5JobRec) * (size_t)n_streams;
    if (int rc = g->table.ensure(std::max<size_t>(table_bytes, 64))) return rc;
    IngestStream *tab = g->table.as<IngestStream>();
    flacgpu_k::Md5JobRec *jobs = reinterpret_cast<flacgpu_k::Md5JobRec *>(tab + n_streams);
    uint64_t tiles = 0;
    for (uint32_t i = 0; i < n_streams; i++) {
        const flacgpu_ingest_stream &s = streams[i];
        uint64_t count = 0, end = 0;
        if (__builtin_mul_overflow(s.samples, (uint64_t)channels, &count) ||
            __builtin_add_overflow(s.staging_offset, count, &end) || end > staging_elements || (s.staging_offset & 3u) ||
            (padded && s.samples > fmt->samples_padded)) {
            g_last_error = "flacgpu_ingest_submit: stream " + std::to_string(i) + " does not fit its place";
            return FLACGPU_ERR_INVALID_ARG;
        }
        tab[i].in_off = padded ? (uint64_t)i * fmt->channels_padded * fmt->samples_padded : s.in_offset;
        tab[i].out_off = s.staging_offset;
        tab[i].samples = s.samples;
        tab[i].tile0 = tiles;
        tiles += (s.samples + ts - 1) / ts;
        jobs[i] = flacgpu_k::Md5JobRec{};
        jobs[i].off = s.staging_offset;
        jobs[i].count = count;
        jobs[i].width = (bits_per_sample + 7) / 8;
    }
    if (tiles > 0x7FFFFFFFull) {
        g_last_error = "flacgpu_ingest_submit: more than 2^31 - 1 tiles";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (tiles && !d_pcm) return FLACGPU_ERR_INVALID_ARG;
    if (int rc = g->staging.ensure(std::max<size_t>(4 * (size_t)staging_elements, 64))) return rc;
    *d_staging = g->staging.as<int32_t>();
    if (!n_streams) return FLACGPU_OK;
    if (int rc = g->streams.ensure(sizeof(IngestStream) * (size_t)n_streams)) return rc;
    if (int rc = g->altered.ensure(4 * (size_t)n_streams)) return rc;
    if (int rc = g->results.ensure(24 * (size_t)n_streams)) return rc;   // altered [n] | digests [n][5]
    if (g->md5) {
        if (int rc = g->jobs.ensure(sizeof(flacgpu_k::Md5JobRec) * (size_t)n_streams)) return rc;
        if (int rc = g->digest.ensure(20 * (size_t)n_streams)) return rc;
    }
    // ---- ordered after the caller's stream (NULL: the legacy default stream), on the handle's own
    HIP_TRY(hipEventRecord(g->ev, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamWaitEvent(g->st, g->ev, 0));
    g->pending = true;
    HIP_TRY(hipMemcpyAsync(g->streams.p, tab, sizeof(IngestStream) * (size_t)n_streams, hipMemcpyHostToDevice, g->st));
    HIP_TRY(hipMemsetAsync(g->altered.p, 0, 4 * (size_t)n_streams, g->st));
    if (tiles) {
        const IngestStream *ds = g->streams.as<const IngestStream>();
        int32_t *out = g->staging.as<int32_t>();
        uint32_t *alt = g->altered.as<uint32_t>();
        const uint32_t T = (uint32_t)tiles;
        if (fmt->dtype == FLACGPU_SAMPLE_I16)
            launch_ingest<INGEST_I16>(padded, T, g->st, d_pcm, ds, n_streams, channels, bits_per_sample, fmt->samples_padded, out, alt);
        else if (fmt->dtype == FLACGPU_SAMPLE_S24)
            launch_ingest<INGEST_S24>(padded, T, g->st, d_pcm, ds, n_streams, channels, bits_per_sample, fmt->samples_padded, out, alt);
        else if (fmt->dtype == FLACGPU_SAMPLE_F32)
            launch_ingest<INGEST_F32>(padded, T, g->st, d_pcm, ds, n_streams, channels, bits_per_sample, fmt->samples_padded, out, alt);
        else
            launch_ingest<INGEST_I32>(padded, T, g->st, d_pcm, ds, n_streams, channels, bits_per_sample, fmt->samples_padded, out, alt);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(g->results.p, g->altered.p, 4 * (size_t)n_streams, hipMemcpyDeviceToHost, g->st));
    // the staging buffer is complete (and d_pcm read) when this returns: the encoder's contexts read it from streams of
    // their own
    HIP_TRY(hipStreamSynchronize(g->st));
    if (g->md5) {   // the chains run beside the encoder's kernels; flacgpu_ingest_finish waits for them
        HIP_TRY(hipMemcpyAsync(g->jobs.p, jobs, sizeof(flacgpu_k::Md5JobRec) * (size_t)n_streams, hipMemcpyHostToDevice, g->st));
        flacgpu_k::launch_md5_many(g->staging.as<const int32_t>(), g->jobs.as<const flacgpu_k::Md5JobRec>(), n_streams,
                                   g->digest.as<uint32_t>(), g->st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(g->results.as<uint32_t>() + n_streams, g->digest.p, 20 * (size_t)n_streams,
                               hipMemcpyDeviceToHost, g->st));
    }
    return FLACGPU_OK;
}

int flacgpu_ingest_finish(flacgpu_ingest *g, uint32_t *altered, uint8_t *md5) {
    if (!g) return FLACGPU_ERR_INVALID_ARG;
    DeviceGuard guard(g->device);
    if (g->pending) HIP_TRY(hipStreamSynchronize(g->st));
    g->pending = false;
    const uint32_t *res = g->results.as<const uint32_t>();
    for (uint32_t i = 0; i < g->n; i++) {
        if (altered) altered[i] = res[i];
        if (md5 && g->md5) memcpy(md5 + 16 * (size_t)i, res + g->n + 5 * (size_t)i, 16);
    }
    return FLACGPU_OK;
}

int flacgpu_ingest_scratch(flacgpu_ingest *g, size_t bytes, uint8_t **pinned) {
    if (!g || !pinned) return FLACGPU_ERR_INVALID_ARG;
    DeviceGuard guard(g->device);
    if (int rc = g->piece_host.ensure(std::max<size_t>(bytes, 64))) return rc;
    *pinned = g->piece_host.as<uint8_t>();
    return FLACGPU_OK;
}

int flacgpu_ingest_place(flacgpu_ingest *g, size_t bytes, const flacgpu_place_run *runs, uint32_t n_runs) {
    if (!g || (n_runs && !runs) || bytes > g->piece_host.cap) return FLACGPU_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_runs; i++) {
        uint64_t end = 0, dend = 0;
        if (__builtin_add_overflow(runs[i].src, runs[i].n, &end) || end > bytes ||
            __builtin_add_overflow(runs[i].dst, runs[i].n, &dend) || (runs[i].n && !runs[i].dst)) {
            g_last_error = "flacgpu_ingest_place: run " + std::to_string(i) + " reaches past the uploaded bytes, or has no destination";
            return FLACGPU_ERR_INVALID_ARG;
        }
    }
    if (!n_runs) return FLACGPU_OK;
    DeviceGuard guard(g->device);
    // (a 16-byte group that holds a byte of the scratch must lie inside the allocation: hipMalloc's alignment, and 16 spare)
    if (int rc = g->piece_dev.ensure(std::max<size_t>(bytes + 16, 64))) return rc;
    if (int rc = g->run_host.ensure(sizeof(PlaceRun) * (size_t)n_runs)) return rc;
    if (int rc = g->run_dev.ensure(sizeof(PlaceRun) * (size_t)n_runs)) return rc;
    PlaceRun *tab = g->run_host.as<PlaceRun>();
    const uint64_t groups = place_table(runs, n_runs, reinterpret_cast<uintptr_t>(g->piece_dev.p), 0, tab);
    HIP_TRY(hipMemcpyAsync(g->piece_dev.p, g->piece_host.p, bytes, hipMemcpyHostToDevice, g->st));
    HIP_TRY(hipMemcpyAsync(g->run_dev.p, tab, sizeof(PlaceRun) * (size_t)n_runs, hipMemcpyHostToDevice, g->st));
    if (int rc = flacgpu_k::launch_place_runs(g->run_dev.as<const PlaceRun>(), n_runs, groups, g->st)) return rc;
    HIP_TRY(hipStreamSynchronize(g->st));
    return FLACGPU_OK;
}

int flacgpu_ingest_move(flacgpu_ingest *g, const flacgpu_place_run *runs, uint32_t n_runs) {
    if (!g || (n_runs && !runs)) return FLACGPU_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_runs; i++) {
        uint64_t end = 0;
        if (runs[i].n && (!runs[i].src || !runs[i].dst || __builtin_add_overflow(runs[i].src, runs[i].n, &end) ||
                          __builtin_add_overflow(runs[i].dst, runs[i].n, &end))) {
            g_last_error = "flacgpu_ingest_move: run " + std::to_string(i) + " has no source or destination, or wraps round";
            return FLACGPU_ERR_INVALID_ARG;
        }
    }
    if (!n_runs) return FLACGPU_OK;
    DeviceGuard guard(g->device);
    if (int rc = g->run_host.ensure(sizeof(PlaceRun) * (size_t)n_runs)) return rc;
    if (int rc = g->run_dev.ensure(sizeof(PlaceRun) * (size_t)n_runs)) return rc;
    PlaceRun *tab = g->run_host.as<PlaceRun>();
    const uint64_t groups = place_table(runs, n_runs, 0, 0, tab);
    HIP_TRY(hipMemcpyAsync(g->run_dev.p, tab, sizeof(PlaceRun) * (size_t)n_runs, hipMemcpyHostToDevice, g->st));
    if (int rc = flacgpu_k::launch_place_runs(g->run_dev.as<const PlaceRun>(), n_runs, groups, g->st)) return rc;
    HIP_TRY(hipStreamSynchronize(g->st));
    return FLACGPU_OK;
}

void *flacgpu_ingest_stream_of(flacgpu_ingest *g) { return g ? static_cast<void *>(g->st) : nullptr; }
