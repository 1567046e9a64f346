// ingest.inc -- the encoder's ingest pass (ingest.hip): a caller's device tensor -> what the encoder reads in place.
// Included inside ingest.hip's anonymous namespace, after ingest_rule.h.
//   K_i1 k_ingest<DT, PADDED>  workgroup per tile of one stream: int32 / int16 / packed 24-bit / float32 elements, planar
//                              rows of a padded
//                              [n_streams][channels_padded][samples_padded] batch or interleaved streams at element
//                              offsets of their own, converted by ingest_sample (ingest_rule.h) and written as
//                              interleaved int32 into the staging buffer -- every stream from a 16-byte boundary, the
//                              streams back to back in stream order (flacgpu_encode_segments_device reads segments in
//                              place only from such boundaries).
// A streaming pass: every input element is read once and every output element written once, so all there is to get
// right is that both sides move whole 16-byte groups per lane, consecutive lanes consecutive groups.  The two sides do
// not line up -- a padded row starts at any element (samples_padded need not be a multiple of 4), a flat stream at any
// in_offset, the output always on a 16-byte boundary, and a planar row is `channels` dwords apart in the output -- so a
// tile goes through LDS: rows are loaded with load_run (store_run's shape, kernels/decode_many.inc: single elements up
// to the first 16-byte boundary, 16 bytes per lane, single elements), converted in registers and stored planar into
// LDS; the interleaved tile is then read back from LDS and stored with 16 bytes per lane.  Only the first `channels`
// rows and the first `samples` elements of each are ever addressed: padding is never read.
// This version always ingests.  A FLAT int32 batch whose streams start on 16-byte boundaries and whose samples fit bps
// bits could be read in place by the encoder instead; skipping the pass for that case is a follow-up.

struct IngestStream {
    uint64_t in_off;    // first element of the stream in the caller's tensor (PADDED: of its channel 0 row)
    uint64_t out_off;   // first int32 of the stream in the staging buffer, a multiple of 4
    uint64_t samples;   // per channel
    uint64_t tile0;     // the stream's first tile in the grid (a stream without samples owns none)
};

constexpr uint32_t INGEST_TILE = 4096;       // elements of a tile over all channels
constexpr uint32_t INGEST_ROW_PAD = 4;       // dwords between the planar rows of a tile in LDS
constexpr uint32_t INGEST_LDS = INGEST_TILE + INGEST_ROW_PAD * FLACGPU_MAX_CHANNELS;
// samples per channel of a tile: a multiple of 4, so that every tile starts on a 16-byte boundary of the staging buffer
__host__ __device__ constexpr uint32_t ingest_tile_samples(uint32_t channels) { return (INGEST_TILE / channels) & ~3u; }

// (The tile loops are not unrolled: a tile is at most four trips per lane, and unrolled eight times the F32 and I32
// instances took 190-256 VGPRs -- one or two waves per SIMD; rolled they take under 50 and the LDS bounds the residency.)
// n elements of ES bytes from src (ES-aligned), put(e, bits) with the element's bits in the low end of a dword: single
// elements up to the first 16-byte boundary, then 16 bytes per lane, then single elements.  Reads [src, src + n * ES).
template <uint32_t ES, class Put>
__device__ __forceinline__ void load_run(const uint8_t *src, uint32_t n, uint32_t tid, uint32_t nthreads, Put put) {
    constexpr uint32_t V = 16 / ES;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u) / ES;
    const uint32_t head = min(n, (V - mis) % V);
    const uint32_t nv = (n - head) / V, tail_at = head + nv * V;
    if (tid < head) {
        if (ES == 2) put(tid, (uint32_t)reinterpret_cast<const uint16_t *>(src)[tid]);
        else put(tid, reinterpret_cast<const uint32_t *>(src)[tid]);
    }
    const uint4 *body = reinterpret_cast<const uint4 *>(src + (size_t)head * ES);
#pragma nounroll
    for (uint32_t v = tid; v < nv; v += nthreads) {
        const uint4 w = body[v];
        const uint32_t e = head + v * V;
        if (ES == 2) {
            put(e, w.x & 0xFFFFu); put(e + 1, w.x >> 16);
            put(e + 2, w.y & 0xFFFFu); put(e + 3, w.y >> 16);
            put(e + 4, w.z & 0xFFFFu); put(e + 5, w.z >> 16);
            put(e + 6, w.w & 0xFFFFu); put(e + 7, w.w >> 16);
        } else {
            put(e, w.x); put(e + 1, w.y); put(e + 2, w.z); put(e + 3, w.w);
        }
    }
    if (tid < n - tail_at) {
        const uint32_t e = tail_at + tid;
        if (ES == 2) put(e, (uint32_t)reinterpret_cast<const uint16_t *>(src)[e]);
        else put(e, reinterpret_cast<const uint32_t *>(src)[e]);
    }
}

// n packed 3-byte elements from src (any byte address), put(e, bits) with the element's 24 bits in the low end of a
// dword -- bits 24-31 hold whatever followed and ingest_sample ignores them.  store_run3's mirror (kernels/
// decode_many.inc): the run is the 3n bytes [src, src + 3n), read as single bytes up to the first 16-byte boundary, 16
// bytes per lane, single bytes.  An element belongs to the part its FIRST byte lies in:
//   head  elements e with 3e < head (at most 5), a lane each, three byte loads (the last may reach into the body);
//   body  the lane of the 16 bytes at run byte B takes the elements that start in [B, B + 16): the first at offset
//         o = (3 - B % 3) % 3, then every 3 bytes -- five of them, and a sixth at offset 15 when o == 0.  The last one
//         reaches up to 2 bytes past the group: into the next group's first dword (inside the run, as that whole group
//         is), or, behind the last group, into tail bytes, each loaded only if it lies inside the run.  The five dwords
//         are shifted down by o bytes once, so that every element is cut from constant positions (no indexed registers);
//   tail  elements that start at or behind the last group's end (at most 5), a lane each, three byte loads.
// An element that starts inside the run ends inside it, so no byte outside [src, src + 3n) is ever read.  Indices are
// 32-bit (3n <= 3 * INGEST_TILE).
template <class Put>
__device__ __forceinline__ void load_run3(const uint8_t *src, uint32_t n, uint32_t tid, uint32_t nthreads, Put put) {
    const uint32_t bytes = 3u * n;
    const uint32_t head = min(bytes, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u);
    const uint32_t nv = (bytes - head) / 16u, tail_at = head + nv * 16u;
    const uint32_t head_n = (head + 2u) / 3u, tail_e = (tail_at + 2u) / 3u;
    const auto bytewise = [&](uint32_t e) {
        const uint8_t *p = src + 3u * e;
        put(e, (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
    };
    if (tid < head_n) bytewise(tid);
    const uint32_t *body = reinterpret_cast<const uint32_t *>(src + head);
#pragma nounroll
    for (uint32_t v = tid; v < nv; v += nthreads) {
        const uint4 w = reinterpret_cast<const uint4 *>(body)[v];
        const uint32_t at = head + v * 16u;
        uint32_t next = 0;
        if (v + 1 < nv) {
            next = body[4u * v + 4u];
        } else {
            if (at + 16u < bytes) next = src[at + 16u];
            if (at + 17u < bytes) next |= (uint32_t)src[at + 17u] << 8;
        }
        const uint32_t e = (at + 2u) / 3u, sh = 8u * (3u * e - at);   // the first element that starts in the group
        const uint32_t s0 = (uint32_t)(((uint64_t)w.y << 32 | w.x) >> sh);
        const uint32_t s1 = (uint32_t)(((uint64_t)w.z << 32 | w.y) >> sh);
        const uint32_t s2 = (uint32_t)(((uint64_t)w.w << 32 | w.z) >> sh);
        const uint32_t s3 = (uint32_t)(((uint64_t)next << 32 | w.w) >> sh);
        put(e, s0);
        put(e + 1, s0 >> 24 | s1 << 8);
        put(e + 2, s1 >> 16 | s2 << 16);
        put(e + 3, s2 >> 8);
        put(e + 4, s3);
        if (sh == 0) put(e + 5, s3 >> 24 | next << 8);
    }
    if (tid < n - tail_e) bytewise(tail_e + tid);
}

// a run of n elements of ES bytes: load_run, or load_run3 for the packed 3-byte elements
template <uint32_t ES, class Put>
__device__ __forceinline__ void load_elems(const uint8_t *src, uint32_t n, uint32_t tid, uint32_t nthreads, Put put) {
    if constexpr (ES == 3) load_run3(src, n, tid, nthreads, put);
    else load_run<ES>(src, n, tid, nthreads, put);
}

// n dwords to dst (16-byte aligned: a tile's place in the staging buffer), dword e = get(e): 16 bytes per lane, then
// single dwords.  Writes [dst, dst + n).
template <class Get>
__device__ __forceinline__ void store_tile(int32_t *dst, uint32_t n, uint32_t tid, uint32_t nthreads, Get get) {
    const uint32_t nv = n / 4, tail_at = nv * 4;
    uint4 *body = reinterpret_cast<uint4 *>(dst);
#pragma nounroll
    for (uint32_t v = tid; v < nv; v += nthreads) {
        const uint32_t e = v * 4;
        body[v] = make_uint4(get(e), get(e + 1), get(e + 2), get(e + 3));
    }
    if (tid < n - tail_at) dst[tail_at + tid] = (int32_t)get(tail_at + tid);
}

// the interleaved tile out of its planar rows in LDS; C is a constant so that e / C and e % C are a multiply and a shift
template <uint32_t C>
__device__ __forceinline__ void store_interleaved(int32_t *dst, const uint32_t *rows, uint32_t ld, uint32_t n,
                                                  uint32_t tid) {
    store_tile(dst, n * C, tid, WG, [&](uint32_t e) { return rows[(e % C) * ld + e / C]; });
}

template <uint32_t DT, bool PADDED>
__global__ void __launch_bounds__(WG) k_ingest(const uint8_t *__restrict__ in, const IngestStream *__restrict__ streams,
                                               uint32_t n_streams, uint32_t channels, uint32_t bps,
                                               uint64_t samples_padded, int32_t *__restrict__ staging,
                                               uint32_t *__restrict__ altered) {
    constexpr uint32_t ES = DT == INGEST_I16 ? 2 : DT == INGEST_S24 ? 3 : 4;
    __shared__ __attribute__((aligned(16))) uint32_t lds[INGEST_LDS];
    // the stream of this tile: the last one whose first tile is not behind it (streams without tiles stand in front
    // of the one that owns their tile0, or at the very end)
    uint32_t lo = 0, hi = n_streams;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (streams[mid].tile0 <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const IngestStream st = streams[lo];
    const uint32_t ts = ingest_tile_samples(channels), ld = ts + INGEST_ROW_PAD;
    const uint64_t s0 = (blockIdx.x - st.tile0) * ts;
    if (s0 >= st.samples) return;   // (cannot happen: the grid is the sum of the streams' tiles)
    const uint32_t n = (uint32_t)min((uint64_t)ts, st.samples - s0);
    uint32_t changed = 0;
    const auto convert = [&](uint32_t raw) {
        int a;
        const int32_t v = ingest_sample(DT, raw, bps, &a);
        changed += (uint32_t)a;
        return (uint32_t)v;
    };
    if (PADDED) {
        for (uint32_t c = 0; c < channels; c++)
            load_elems<ES>(in + (st.in_off + (uint64_t)c * samples_padded + s0) * ES, n, threadIdx.x, WG,
                         [&](uint32_t i, uint32_t raw) { lds[c * ld + i] = convert(raw); });
    } else {
        load_elems<ES>(in + (st.in_off + s0 * channels) * ES, n * channels, threadIdx.x, WG,
                     [&](uint32_t e, uint32_t raw) { lds[e] = convert(raw); });
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) changed += __shfl_xor(changed, off, 64);
    if ((threadIdx.x & 63u) == 0 && changed) atomicAdd(&altered[lo], changed);
    __syncthreads();
    int32_t *dst = staging + st.out_off + s0 * channels;
    if (!PADDED || channels == 1) {
        store_tile(dst, n * channels, threadIdx.x, WG, [&](uint32_t e) { return lds[e]; });
        return;
    }
    switch (channels) {
    case 2: store_interleaved<2>(dst, lds, ld, n, threadIdx.x); break;
    case 3: store_interleaved<3>(dst, lds, ld, n, threadIdx.x); break;
    case 4: store_interleaved<4>(dst, lds, ld, n, threadIdx.x); break;
    case 5: store_interleaved<5>(dst, lds, ld, n, threadIdx.x); break;
    case 6: store_interleaved<6>(dst, lds, ld, n, threadIdx.x); break;
    case 7: store_interleaved<7>(dst, lds, ld, n, threadIdx.x); break;
    default: store_interleaved<8>(dst, lds, ld, n, threadIdx.x); break;
    }
}
