// common.inc -- candidate sources, reductions, the generic (LDS) Rice partition search.
// Included inside the anonymous namespace of every kernel translation unit (after kernels/types.h).

__device__ __forceinline__ uint32_t frame_len(const Params &p, uint32_t frame) {
    if (p.frame_n) return p.frame_n[frame];   // a ragged batch (Params::frame_n)
    return (frame + 1 == p.n_frames) ? p.last_len : p.block_size;
}

// XCD-aware (frame, candidate) <- blockIdx mapping: consecutive blockIdx values are dealt
// round-robin over the 8 XCDs, so put the candidates of one frame 8 blocks apart: they
// then share an XCD L2 and the frame's L/R rows are fetched from HBM once.
__device__ __forceinline__ void map_block(uint32_t bid, uint32_t nc, uint32_t nframes,
                                          uint32_t &frame, uint32_t &cand) {
    uint32_t full = nframes / 8u;
    uint32_t per = 8u * nc;
    if (bid < full * per) {
        uint32_t g = bid / per, rem = bid - g * per;
        cand = rem / 8u;
        frame = g * 8u + (rem & 7u);
    } else {
        uint32_t rem = bid - full * per, tail = nframes - full * 8u;
        cand = rem / tail;
        frame = full * 8u + (rem - cand * tail);
    }
}

// candidate -> source rows.  mode 0: a;  1: (a+b)>>1 (mid);  2: a-b (side)
struct CandSrc {
    const int32_t *a, *b;
    int mode;
    uint32_t bps;
    uint8_t source;
};
__device__ __forceinline__ CandSrc cand_src(const Params &p, uint32_t frame, uint32_t cand) {
    CandSrc s;
    const int32_t *base = p.planar + (size_t)frame * p.channels * p.ldb;
    s.bps = p.bps;
    if (p.stereo4 && cand >= 2) {
        s.a = base;
        s.b = base + p.ldb;
        if (cand == 2) {
            s.mode = 1;
            s.source = FLACGPU_SRC_MID;
        } else {
            s.mode = 2;
            s.bps = p.bps + 1;
            s.source = FLACGPU_SRC_SIDE;
        }
    } else {
        s.a = base + (size_t)cand * p.ldb;
        s.b = s.a;
        s.mode = 0;
        s.source = (uint8_t)cand;
    }
    return s;
}
__device__ __forceinline__ int32_t combine(int mode, int32_t a, int32_t b) {
    // encode.rs:2721 `(l + r) >> 1`, :2734 `l - r` (i32, wrapping in release builds)
    if (mode == 1) return (int32_t)((uint32_t)a + (uint32_t)b) >> 1;
    if (mode == 2) return (int32_t)((uint32_t)a - (uint32_t)b);
    return a;
}

// the fast channel choice's verdict on a stereo candidate (encode.rs:2463-2674: only the chosen pair is analysed)
__device__ __forceinline__ bool active_in_assignment(uint32_t assign, uint32_t cand) {
    return cand == 0 ? (assign == FLACGPU_ASSIGN_INDEPENDENT || assign == FLACGPU_ASSIGN_LEFT_SIDE)
         : cand == 1 ? (assign == FLACGPU_ASSIGN_INDEPENDENT || assign == FLACGPU_ASSIGN_SIDE_RIGHT)
         : cand == 2 ? (assign == FLACGPU_ASSIGN_MID_SIDE) : (assign != FLACGPU_ASSIGN_INDEPENDENT);
}

// the fast channel choice itself: first minimum over the reference's candidate order (encode.rs:2506-2514 with
// mid-side, :2600-2607 without) of the sums of |l|, |r|, |mid|, |side| over the frame
__device__ __forceinline__ uint32_t fast_assignment(bool mid_side, uint64_t ls, uint64_t rs, uint64_t ms, uint64_t ss) {
    if (mid_side) {
        const uint64_t tot[4] = {ls + rs, ls + ss, ss + rs, ms + ss};
        int b = 0;
        for (int i = 1; i < 4; i++)
            if (tot[i] < tot[b]) b = i;
        return b == 0 ? FLACGPU_ASSIGN_INDEPENDENT : b == 1 ? FLACGPU_ASSIGN_LEFT_SIDE
             : b == 2 ? FLACGPU_ASSIGN_SIDE_RIGHT : FLACGPU_ASSIGN_MID_SIDE;
    }
    const uint64_t tot[3] = {ls + ss, ss + rs, ls + rs};   // LeftSide, SideRight, Independent
    int b = 0;
    for (int i = 1; i < 3; i++)
        if (tot[i] < tot[b]) b = i;
    return b == 0 ? FLACGPU_ASSIGN_LEFT_SIDE : b == 1 ? FLACGPU_ASSIGN_SIDE_RIGHT : FLACGPU_ASSIGN_INDEPENDENT;
}

// per (frame, candidate): activity, wasted bits, effective bps from the OR of the candidate's samples
// (encode.rs:2870-2898); `prev_active` matters only for the fast channel choice (k_stereo_stats sets it)
__device__ __forceinline__ CandInfo cand_info_from_or(const Params &p, uint32_t cand, uint32_t orv, bool prev_active) {
    CandInfo ci;
    if (p.exhaustive || !p.stereo4)
        // exhaustive: L, R always; S if bps+1 <= 32 (guaranteed by stereo4); M iff mid_side
        ci.active = !(p.stereo4 && cand == 2 && !p.mid_side);
    else
        ci.active = prev_active;
    const uint32_t cbps = p.bps + ((p.stereo4 && cand == 3) ? 1u : 0u);
    if (orv == 0) {  // all zero -> CONSTANT(0) at the candidate's bps, wasted 0
        ci.is_const = 1;
        ci.wasted = 0;
        ci.bps = (uint8_t)cbps;
    } else {
        const uint32_t w = (uint32_t)__builtin_ctz(orv);
        ci.is_const = 0;
        ci.wasted = (uint8_t)w;
        ci.bps = (uint8_t)(cbps - w);
    }
    return ci;
}

// ---------------------------------------------------------------------------------
// workgroup reductions (wave64 shuffles, then 4-way LDS combine)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_down(v, off, 64);
    return v;
}
// all threads get the result; `scratch` holds >= 4 u64
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t *scratch) {
    v = wave_sum_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}
__device__ __forceinline__ uint32_t block_or_u32(uint32_t v, uint64_t *scratch) {
    v = wave_or_u32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return (uint32_t)(scratch[0] | scratch[1] | scratch[2] | scratch[3]);
}

__device__ __forceinline__ uint32_t uabs(int32_t v) {
    return v < 0 ? 0u - (uint32_t)v : (uint32_t)v;  // i32::unsigned_abs
}
__device__ __forceinline__ uint32_t zigzag(int32_t s) {  // encode.rs:3845-3849
    return ((uint32_t)s << 1) ^ (uint32_t)(s >> 31);
}

// ---------------------------------------------------------------------------------
// Rice partition search (encode.rs:3865-3896 best_partitions + 3765-3831 Partition::new)
// and exact residual-block bit count (replaces BitRecorder::written(), SURVEY.md A.6).
// Cooperative over the workgroup.  `r` is indexed by SAMPLE POSITION: residual of sample i
// lives at r[i], valid for i in [order, n).  Partitions are the reference's
// `residuals.rchunks(n >> porder).rev()`, i.e. cuts at multiples of the partition length.
// The f64 `ceil(log2(sum / n))` of encode.rs:3778-3780 is replaced by its exact integer
// equivalent (smallest k with n * 2^k >= sum; valid because sum < 2^53).
// ---------------------------------------------------------------------------------
// residual arrays in LDS use a padded index (one extra dword per 16) so that lanes walking
// contiguous 16-element runs (stride 17 dwords) hit distinct banks
__device__ __forceinline__ uint32_t RIDX(uint32_t i) { return i + (i >> 4); }

struct RiceShared {
    unsigned long long leaf[NLEAF];
    unsigned long long pre[NLEAF + 1];   // exclusive prefix of the leaf sums
    uint32_t nd_cnt[NNODE + 1];
    uint8_t nd_kind[NNODE + 1], nd_rice[NNODE + 1], nd_esc[NNODE + 1];
    uint32_t lv_est[MAXP + 1], lv_count[MAXP + 1], lv_bad[MAXP + 1], lv_hi[MAXP + 1];
    uint64_t red[4];
};
enum { PK_STANDARD = 0, PK_ESCAPED = 1, PK_CONSTANT = 2 };

// Partition::new (encode.rs:3765-3831) for one partition of `cnt` residuals with sum of
// absolute values `sum`: Rice parameter / escape decision and the size ESTIMATE the reference
// ranks partition orders by.  The f64 `ceil(log2(sum / n))` of :3778-3780 is replaced by its
// exact integer equivalent (smallest k with n * 2^k >= sum; sum < 2^53).
struct PartEval {
    uint32_t est;
    uint8_t kind, rice, esc, bad;
};
// S = unsigned long long, or uint32_t when the caller knows sum < 2^31 (then cnt << k stays below
// 2^32 and the u32::try_from of the estimate cannot fail)
template <class S>
__device__ __forceinline__ PartEval partition_eval_t(uint32_t cnt, S sum, uint32_t rice_max) {
    constexpr bool WIDE = sizeof(S) == 8;
    PartEval r;
    r.est = 0;
    r.kind = PK_CONSTANT;
    r.rice = 0xFF;
    r.esc = 0;
    r.bad = 0;
    if (cnt > 0 && sum > 0) {
        uint32_t k = 0;
        bool standard = true;
        if (sum > (S)cnt) {
            uint32_t bs;
            if constexpr (WIDE) bs = 64u - (uint32_t)__clzll((long long)sum);
            else bs = 32u - (uint32_t)__builtin_clz(sum);
            const uint32_t bc = 32u - (uint32_t)__builtin_clz(cnt);
            // smallest k with cnt 2^k >= sum: sum >= 2^(bs-1) and cnt < 2^bc put it strictly above bs - bc - 1, and
            // sum < 2^bs, cnt >= 2^(bc-1) at most at bs - bc + 1: two conditional steps from the start value, no loop
            // (a divergent loop cost more in its control than in its body)
            k = bs > bc ? bs - bc - 1 : 0;
            k += (((S)cnt << k) < sum) ? 1u : 0u;
            k += (((S)cnt << k) < sum) ? 1u : 0u;
            if (k >= rice_max) {
                standard = false;
                const uint32_t e = (bs - 1) + 2u;  // ilog2(sum) + 2
                if (e > 31u) r.bad = 1;
                r.kind = PK_ESCAPED;
                r.esc = (uint8_t)e;
                r.est = e * cnt;
            }
        }
        if (standard) {
            const S t = k ? (sum >> (k - 1)) : (sum << 1);
            if constexpr (WIDE) {
                if (t > 0xFFFFFFFFull) r.bad = 1;  // u32::try_from fails -> candidate dropped
            }
            r.kind = PK_STANDARD;
            r.rice = (uint8_t)k;
            r.est = 4u + (1u + k) * cnt + (uint32_t)t - cnt / 2u;  // wrapping u32
        }
    }
    return r;
}
__device__ __forceinline__ PartEval partition_eval(uint32_t cnt, unsigned long long sum, uint32_t rice_max) {
    return partition_eval_t<unsigned long long>(cnt, sum, rice_max);
}

__device__ __forceinline__ uint32_t rice_levels(uint32_t n, const Params &p) {
    uint32_t tz = (uint32_t)__builtin_ctz(n);
    uint32_t P = tz < p.max_po ? tz : p.max_po;
    return P > MAXP ? MAXP : P;  // host rejects calls with P > 6; clamp defensively
}
__device__ __forceinline__ void rice_init(RiceShared &S) {
    const uint32_t tid = threadIdx.x;
    if (tid < NLEAF) S.leaf[tid] = 0ull;
    if (tid <= MAXP) {
        S.lv_est[tid] = 0;
        S.lv_count[tid] = 0;
        S.lv_bad[tid] = 0;
        S.lv_hi[tid] = 0;
    }
}

// Partition tree evaluation.  Precondition: S.leaf[] holds the sums of |residual| of the
// 2^P finest partitions and a barrier has been passed.  One lane per tree node runs
// Partition::new (encode.rs:3765-3831); the f64 `ceil(log2(sum / n))` of :3778-3780 is
// replaced by its exact integer equivalent (smallest k with n * 2^k >= sum; sum < 2^53).
// Ends with a barrier; afterwards rice_pick() gives every lane the chosen level.
__device__ __forceinline__ void rice_tree(RiceShared &S, uint32_t n, uint32_t order, uint32_t P,
                                          uint32_t rice_max) {
    const uint32_t tid = threadIdx.x;
    // heap numbering: node = 2^level + j.  Nodes 1..63 (levels 0..5) are lanes of wave 0, which
    // first builds the inclusive prefix of the leaf sums with shuffles (no barrier) and reads
    // partition sums as prefix differences; nodes 64..127 exist only for P == 6 and are the
    // leaves themselves (wave 1).
    if (tid < 128) {
        unsigned long long incl = 0;
        if (tid < 64) {
            incl = S.leaf[tid];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                unsigned long long t = __shfl_up(incl, off, 64);
                if (tid >= (uint32_t)off) incl += t;
            }
        }
        const uint32_t node = tid;
        const bool is_node = node >= 1 && node < (2u << P);
        const uint32_t lvl = is_node ? 31u - (uint32_t)__builtin_clz(node) : 0u;
        const uint32_t j = node - (1u << lvl);
        unsigned long long sum;
        if (tid < 64) {
            const uint32_t span = 1u << (P - (lvl <= P ? lvl : P));
            const uint32_t hi = (j + 1) * span - 1, lo = j * span;  // leaves [lo, hi]
            const unsigned long long top = __shfl(incl, (int)(hi & 63), 64);
            const unsigned long long bot = __shfl(incl, (int)((lo ? lo - 1 : 0) & 63), 64);
            sum = top - (lo ? bot : 0ull);
        } else {
            sum = S.leaf[node & 63];
        }
        if (is_node) {
            const uint32_t plen = n >> lvl;
            const uint32_t start = j * plen, end = start + plen;
            const uint32_t cnt = (end > order) ? end - (start > order ? start : order) : 0u;
            const PartEval pe = partition_eval(cnt, sum, rice_max);
            const uint8_t kind = pe.kind, rice = pe.rice, esc = pe.esc;
            const uint32_t est = pe.est, bad = pe.bad;
            S.nd_kind[node] = kind;
            S.nd_rice[node] = rice;
            S.nd_esc[node] = esc;
            S.nd_cnt[node] = cnt;
            if (cnt > 0) {  // chunks lying inside the warm-up are not partitions
                atomicAdd(&S.lv_est[lvl], est);
                atomicAdd(&S.lv_count[lvl], 1u);
                if (bad) atomicOr(&S.lv_bad[lvl], 1u);
                if (kind == PK_STANDARD && rice >= 15) atomicOr(&S.lv_hi[lvl], 1u);
            }
        }
    }
    __syncthreads();
}

struct RicePick {
    int bp;            // chosen partition level, -1 = 31-bit escaped fallback (encode.rs:3887)
    uint32_t count;    // partitions emitted
    uint32_t method;   // 0 RICE, 1 RICE2
    uint32_t first_j;  // chunks of level bp lying wholly inside the warm-up
};
// first minimum estimate among valid levels (encode.rs:3881 `!p.is_empty() &&
// p.len().is_power_of_two()`, :3885 min_by_key); try_reduce_rice (:3929-3942)
__device__ __forceinline__ RicePick rice_pick(const RiceShared &S, uint32_t P, uint32_t use_rice2) {
    RicePick r;
    r.bp = -1;
    uint32_t best_est = 0;
    for (uint32_t lvl = 0; lvl <= P; lvl++) {
        const uint32_t c = S.lv_count[lvl];
        const bool ok = !S.lv_bad[lvl] && c > 0 && (c & (c - 1)) == 0;
        if (ok && (r.bp < 0 || S.lv_est[lvl] < best_est)) {
            r.bp = (int)lvl;
            best_est = S.lv_est[lvl];
        }
    }
    r.count = r.bp >= 0 ? S.lv_count[r.bp] : 1u;
    r.method = (r.bp >= 0 && use_rice2 && S.lv_hi[r.bp]) ? 1u : 0u;
    r.first_j = r.bp >= 0 ? (1u << r.bp) - r.count : 0u;
    return r;
}
// header + fixed part of partition `tid` of the chosen level, and the plan's parameter arrays
__device__ __forceinline__ unsigned long long rice_partition_fixed_bits(const RiceShared &S,
                                                                        const RicePick &pk,
                                                                        SubPlan &plan) {
    const uint32_t tid = threadIdx.x, hb = pk.method ? 5u : 4u;
    if (tid >= pk.count) return 0;
    const uint32_t nd = (1u << pk.bp) + pk.first_j + tid;
    const uint32_t c = S.nd_cnt[nd];
    plan.rice[tid] = S.nd_rice[nd];
    plan.escape_bits[tid] = S.nd_esc[nd];
    if (S.nd_kind[nd] == PK_STANDARD) return hb + (1u + S.nd_rice[nd]) * c;
    if (S.nd_kind[nd] == PK_ESCAPED) return hb + 5u + (uint32_t)S.nd_esc[nd] * c;
    return hb + 5u;
}
__device__ __forceinline__ bool rice_finish(RiceShared &S, const RicePick &pk, uint32_t n,
                                            unsigned long long mine, SubPlan &plan,
                                            uint32_t &resid_bits) {
    const unsigned long long tot = block_sum_u64(mine, S.red);
    if (threadIdx.x == 0) {
        plan.part_len = pk.bp >= 0 ? n >> pk.bp : n;
        plan.coding_method = (uint8_t)pk.method;
        plan.n_partitions = pk.count;
        plan.partition_order = (uint8_t)(31u - (uint32_t)__builtin_clz(pk.count));
    }
    // coding method (2) + partition order (4) (encode.rs:3949, 3902) + partitions
    resid_bits = 6u + (uint32_t)(tot & 0xFFFFFFFFull);
    return (tot >> 52) == 0;
}

// Generic Rice search over a residual array in LDS (any block length).
// Returns false when the reference's write_residuals would fail: only possible for the
// 31-bit escaped fallback partition (encode.rs:3887-3895) when a residual does not fit 31
// bits (`write_signed_counted` errors, :3857) -- the subframe candidate is then an Err.
__device__ bool rice_search(const int32_t *r, uint32_t n, uint32_t order, const Params &p,
                            RiceShared &S, SubPlan &plan /* LDS */, uint32_t &resid_bits) {
    const uint32_t tid = threadIdx.x;
    const uint32_t P = rice_levels(n, p);
    const uint32_t leaf_len = n >> P;
    const uint32_t ept = (n + WG - 1) / WG;
    const uint32_t lo = tid * ept > order ? tid * ept : order;
    const uint32_t hi = (tid + 1) * ept < n ? (tid + 1) * ept : n;
    rice_init(S);
    __syncthreads();
    if (lo < hi) {  // this lane's contiguous run of residuals -> leaf sums
        uint32_t i = lo;
        uint32_t cur = i / leaf_len;
        uint32_t bound = (cur + 1) * leaf_len;
        unsigned long long acc = 0;
        for (; i < hi; i++) {
            if (i == bound) {
                atomicAdd(&S.leaf[cur], acc);
                acc = 0;
                cur++;
                bound += leaf_len;
            }
            acc += uabs(r[RIDX(i)]);
        }
        atomicAdd(&S.leaf[cur], acc);
    }
    __syncthreads();
    rice_tree(S, n, order, P, p.use_rice2 ? 31u : 15u);
    const RicePick pk = rice_pick(S, P, p.use_rice2);
    unsigned long long mine = 0;  // this lane's share of the residual block's bit count
    if (pk.bp >= 0) {
        mine += rice_partition_fixed_bits(S, pk, plan);
        if (lo < hi) {  // exact body bits: sum over standard partitions of (u >> k)
            const uint32_t plen = n >> pk.bp;
            uint32_t i = lo;
            uint32_t cur = i / plen;
            uint32_t bound = (cur + 1) * plen;
            uint32_t k = S.nd_rice[(1u << pk.bp) + cur];
            for (; i < hi; i++) {
                if (i == bound) {
                    cur++;
                    bound += plen;
                    k = S.nd_rice[(1u << pk.bp) + cur];
                }
                if (k != 0xFF) mine += zigzag(r[RIDX(i)]) >> k;
            }
        }
    } else {
        if (tid == 0) {
            plan.rice[0] = 0xFF;
            plan.escape_bits[0] = 31;  // encode.rs:3887-3895
            mine += 4u + 5u + 31u * (n - order);
        }
        for (uint32_t i = lo; i < hi; i++)
            if (r[RIDX(i)] < -(1 << 30) || r[RIDX(i)] >= (1 << 30)) mine |= 1ull << 52;  // > 31 bits
    }
    return rice_finish(S, pk, n, mine, plan, resid_bits);
}


__device__ __forceinline__ void plan_clear(SubPlan &plan) {
    uint32_t *w = reinterpret_cast<uint32_t *>(&plan);
    for (uint32_t i = threadIdx.x; i < sizeof(SubPlan) / 4; i += WG) w[i] = 0;
}
__device__ __forceinline__ void plan_store(SubPlan *dst, const SubPlan &src) {
    const uint32_t *s = reinterpret_cast<const uint32_t *>(&src);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    for (uint32_t i = threadIdx.x; i < sizeof(SubPlan) / 4; i += WG) d[i] = s[i];
}

// fixed / LPC / verbatim choice of encode_subframe (encode.rs:2929-2979), thread 0 only.
// returns 0: keep `best`, 1: VERBATIM
__device__ __forceinline__ void make_verbatim(SubPlan &plan, uint32_t n, uint32_t bps_eff,
                                              uint32_t wasted, uint8_t source) {
    plan.type = FLACGPU_SUB_VERBATIM;
    plan.wasted = (uint8_t)wasted;
    plan.bps = (uint8_t)bps_eff;
    plan.order = 0;
    plan.precision = 0;
    plan.shift = 0;
    plan.coding_method = 0;
    plan.partition_order = 0;
    plan.source = source;
    plan.n_partitions = 0;
    plan.part_len = 0;
    plan.bits = 8u + wasted + n * bps_eff;
}
