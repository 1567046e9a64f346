// md5_chain.inc -- the resumable MD5 chains' kernels (md5_chain.hip).  Included inside md5_chain.hip's anonymous namespace,
// after kernels/md5_feed_rule.h, which holds the whole rule: these kernels only decide which lane does what.
//   K_m1 k_md5_chain        wave per piece: the wave loads and stages, one lane consumes (the remedy DESIGN.md 4b named
//                           for k_md5_many, where one lane walks a stream with one dependent global load per sample)
//   K_m2 k_md5_chain_final  lane per chain: padding, digest, and the chain back to its initial state
//
// k_md5_chain takes the virtual string of md5_feed_rule.h window by window (MD5_STAGE_BYTES, 16 blocks):
//   load     the samples that own a byte of the window, in 16-byte groups aligned in MEMORY, group q0 + lane + 64 g to
//            lane `lane` (coalesced); a group that is not wholly inside the piece -- the first and the last one -- is read
//            element by element, the elements of the piece only (load_run's edges, kernels/ingest.inc).  The values stay
//            in registers (MD5_LANE_GROUPS x 4 per lane);
//   scatter  md5_feed_scatter puts every loaded sample's bytes into the window's half of the LDS (byte stores; window 0
//            begins with the chain's buffered bytes);
//   chain    lane 0 reads the window's whole blocks from LDS, 4 x 16 bytes a block, and runs md5_rule_block: no global
//            load on the dependent path.
// The order per trip is load(r + 1), chain(r), scatter(r + 1): the next window's global loads are in flight while the
// chain works, and they land in the LDS half the chain is not reading.  Lanes past a window's last group address nothing.
// No byte outside [off, off + count) of the samples is read.

constexpr uint32_t MD5_LANE_GROUPS = 5;   // 16-byte groups per lane and window
// a window's samples: at most STAGE / width + 2 (one split at either edge); their groups: a quarter, + 1 for the misalignment
static_assert((MD5_STAGE_BYTES + 2u + 3u) / 4u + 1u <= 64u * MD5_LANE_GROUPS, "a window's groups fit the lanes' registers");
static_assert(MD5_STAGE_BYTES % 64u == 0, "a window is whole blocks");

__global__ void __launch_bounds__(64) k_md5_chain(const int32_t *__restrict__ samples,
                                                  const flacgpu_md5_piece *__restrict__ pieces,
                                                  Md5Chain *__restrict__ chains, uint32_t width) {
    __shared__ uint4 win4[2][MD5_STAGE_BYTES / 16];
    const flacgpu_md5_piece pc = pieces[blockIdx.x];
    if (!pc.count) return;
    const uint32_t lane = threadIdx.x;
    Md5Chain *const c = chains + pc.chain;
    const int32_t *const src = samples + pc.off;
    const uint64_t count = pc.count, len0 = c->len;
    const uint32_t fill = md5_feed_fill(len0);
    const uint64_t T = fill + count * width;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u) >> 2;   // elements behind a 16-byte boundary
    uint32_t h[4] = {c->h[0], c->h[1], c->h[2], c->h[3]};
    uint32_t x[MD5_LANE_GROUPS][4];

    // group q (counted from the boundary in front of src) holds the piece's elements [4 q - mis, 4 q - mis + 4)
    const auto window_len = [&](uint64_t lo) { return (uint32_t)(T - lo < MD5_STAGE_BYTES ? T - lo : MD5_STAGE_BYTES); };
    const auto load = [&](uint64_t lo) {
        const uint64_t e0 = md5_feed_first(lo, fill, width), e1 = md5_feed_end(lo + window_len(lo), fill, width, count);
        const uint64_t q0 = (e0 + mis) >> 2, q1 = (e1 + mis + 3u) >> 2;
#pragma unroll
        for (uint32_t g = 0; g < MD5_LANE_GROUPS; g++) {
            const uint64_t q = q0 + lane + 64u * g;
            if (q >= q1) continue;
            const int64_t eb = (int64_t)(4u * q) - (int64_t)mis;
            if (eb >= 0 && (uint64_t)eb + 4u <= count) {
                const uint4 v = *reinterpret_cast<const uint4 *>(src + eb);
                x[g][0] = v.x; x[g][1] = v.y; x[g][2] = v.z; x[g][3] = v.w;
            } else {
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (eb + t >= 0 && (uint64_t)(eb + t) < count) x[g][t] = (uint32_t)src[eb + t];
            }
        }
    };
    const auto scatter = [&](uint64_t lo, uint8_t *win) {
        const uint32_t wl = window_len(lo);
        const uint64_t e0 = md5_feed_first(lo, fill, width), e1 = md5_feed_end(lo + wl, fill, width, count);
        const uint64_t q0 = (e0 + mis) >> 2, q1 = (e1 + mis + 3u) >> 2;
#pragma unroll
        for (uint32_t g = 0; g < MD5_LANE_GROUPS; g++) {
            const uint64_t q = q0 + lane + 64u * g;
            if (q >= q1) continue;
            const int64_t eb = (int64_t)(4u * q) - (int64_t)mis;
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (eb + t >= (int64_t)e0 && (uint64_t)(eb + t) < e1)
                    md5_feed_scatter(win, lo, wl, fill, width, (uint64_t)(eb + t), x[g][t]);
        }
    };

    uint8_t *const win0 = reinterpret_cast<uint8_t *>(win4[0]), *const win1 = reinterpret_cast<uint8_t *>(win4[1]);
    if (lane < fill) win0[lane] = c->buf[lane];
    load(0);
    scatter(0, win0);
    uint32_t half = 0, last_blocks = 0;
    for (uint64_t lo = 0; lo < T; lo += MD5_STAGE_BYTES, half ^= 1u) {
        const bool more = lo + MD5_STAGE_BYTES < T;
        if (more) load(lo + MD5_STAGE_BYTES);
        __syncthreads();   // (one wave: the scatter's LDS stores are ordered in front of the chain's loads)
        const uint32_t blocks = window_len(lo) / 64u;
        if (lane == 0) {
            const uint4 *w = win4[half];
#pragma nounroll
            for (uint32_t b = 0; b < blocks; b++) {
                const uint4 m0 = w[4u * b], m1 = w[4u * b + 1u], m2 = w[4u * b + 2u], m3 = w[4u * b + 3u];
                const uint32_t m[16] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w,
                                        m2.x, m2.y, m2.z, m2.w, m3.x, m3.y, m3.z, m3.w};
                md5_rule_block(h, m);
            }
        }
        if (more) scatter(lo + MD5_STAGE_BYTES, half ? win0 : win1);
        last_blocks = blocks;
    }
    // what the last window holds behind its whole blocks is the new buffer (half was flipped once more on the way out)
    __syncthreads();
    const uint8_t *const last = half ? win0 : win1;
    if (lane < (uint32_t)(T & 63u)) c->buf[lane] = last[64u * last_blocks + lane];
    if (lane == 0) {
        c->h[0] = h[0]; c->h[1] = h[1]; c->h[2] = h[2]; c->h[3] = h[3];
        c->len = len0 + count * width;
    }
}

__global__ void __launch_bounds__(64) k_md5_chain_final(Md5Chain *__restrict__ chains, uint32_t n_chains,
                                                        uint32_t *__restrict__ digest) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chains) return;
    Md5Chain *const c = chains + i;
    uint32_t h[4] = {c->h[0], c->h[1], c->h[2], c->h[3]}, bufw[16], d[4];
    const uint32_t *bw = reinterpret_cast<const uint32_t *>(c->buf);
#pragma unroll
    for (int k = 0; k < 16; k++) bufw[k] = bw[k];
    md5_chain_final(h, c->len, bufw, d);
#pragma unroll
    for (int k = 0; k < 4; k++) digest[4 * (size_t)i + k] = d[k];
    md5_chain_init(*c);
}
