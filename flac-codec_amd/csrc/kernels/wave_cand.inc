// wave_cand.inc -- K2+K5 wave kernel: FIXED + LPC + Rice search of a candidate in one wave.
// Part of flacenc_gpu.hip (one translation unit; included inside its anonymous namespace).

// =================================================================================
// Wave-per-candidate kernel for blocks of exactly 4096 samples (candidates <= 25 bits, LPC
// order <= 16): ONE wave64 does the whole FIXED + LPC analysis of one candidate.  Lane l owns
// samples [64 l, 64 l + 64) in registers, which is exactly one finest Rice partition, so the
// partition tree needs no atomics; neighbours come through wave shuffles; there is NO workgroup
// barrier in the kernel (the 4 waves of a workgroup are the 4 candidates of a frame and share
// L1/L2).  Same decisions as the generic k_fixed + k_fir (same helpers).
// =================================================================================
#define FIR_TURN(spl) ((spl) % 8 == 0 ? 8 : 6)   // samples per turn of fir64_dyn (independent accumulator chains: 2 VGPRs each; 18 and 36 samples per lane: turns of 6)
struct WaveRice {
    uint32_t bits;      // residual block bits (method + order + partitions)
    bool ok;            // false: the 31-bit fallback partition cannot hold a residual
    int bp;             // chosen partition level, -1 = 31-bit escaped fallback
    uint32_t count, method;
    uint8_t price, pesc;  // parameters of partition `lane` (valid for lane < count)
};

// v + (v moved across lanes by one DPP control); lanes without a source lane add 0
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true);
}
// inclusive prefix sum over the 64 lanes (wrapping u32), six DPP adds and no LDS traffic:
// row_shr 1/2/4/8 scan each row of 16, row_bcast:15 / :31 carry the row totals forward
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v) {
    v = dpp_add<0x111>(v);
    v = dpp_add<0x112>(v);
    v = dpp_add<0x114>(v);
    v = dpp_add<0x118>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    return v;
}
// NV independent scans, step by step across all of them: a DPP add needs its source two
// instructions old, and the other chains fill those slots (a lone chain pays an s_nop per step)
template <int NV>
__device__ __forceinline__ void wave_scan_n(uint32_t (&v)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = dpp_add<0x111>(v[i]);
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = dpp_add<0x112>(v[i]);
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = dpp_add<0x114>(v[i]);
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = dpp_add<0x118>(v[i]);
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = dpp_add<0x142, 0xa>(v[i]);
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = dpp_add<0x143, 0xc>(v[i]);
}
__device__ __forceinline__ uint32_t wave_total_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_u32(v), 63);
}
// total of per-lane values < 2^48 (two u32 limbs)
__device__ __forceinline__ uint64_t wave_total_u48(uint64_t v) {
    const uint32_t lo = wave_total_u32((uint32_t)v & 0xFFFFFFu);
    const uint32_t hi = wave_total_u32((uint32_t)(v >> 24));
    return ((uint64_t)hi << 24) + lo;
}
// the previous lane's value, 0 on lane 0 (wave_shr:1)
__device__ __forceinline__ int32_t lane_prev(int32_t v) {
    int32_t r = __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true);
    // keep it a v_mov_b32_dpp: folded into a consumer (v_sub_u32_dpp ... wave_shr:1) the halo of
    // the FIXED differences came out wrong on gfx950 (tests/test_gpu_pack.py, FIXED-only cases)
    asm volatile("" : "+v"(r));
    return r;
}
__device__ __forceinline__ uint32_t sread(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// Residual source of the exact FIXED bit count.  resid(e) is called with e = 0..SPL-1 ascending after reset().
// FixedSrc<K>: residual of fixed order K generated on the fly from the samples (encode.rs:
// 3039-3060); nothing is stored, the second pass of the search simply regenerates it (K
// subtractions per sample) -- this keeps the kernel at 64 instead of 128 array registers.
template <int K, int SPL>
struct FixedSrc {
    int32_t (&x)[SPL];
    int32_t (&h)[4];  // the 4 samples before x[0]
    int32_t q0, q1, q2, q3;
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int k = 0; k < 4; k++) asm volatile("" : "+v"(h[k]));
        q0 = h[3];
        q1 = h[3] - h[2];
        q2 = q1 - (h[2] - h[1]);
        q3 = q2 - ((h[2] - h[1]) - (h[1] - h[0]));
    }
    __device__ __forceinline__ int32_t resid(int e) {
        // an opaque copy of the sample, made where it is used: otherwise the compiler shares this pass's
        // differences with the previous pass (and with the order statistics), i.e. keeps 64..256 of them live, or
        // hoists the residuals above the caller's branches.  (All 64 samples made opaque up front -- the r02 form
        // -- doubles the live samples for a moment: fatal at 128 VGPRs.)
        if constexpr (K == 0) {
            int32_t xe = x[e];
            asm volatile("" : "+v"(xe));
            return xe;
        }
        int32_t d1;
        asm volatile("v_sub_u32 %0, %1, %2" : "=v"(d1) : "v"(x[e]), "v"(q0));
        const int32_t d2 = d1 - q1, d3 = d2 - q2, d4 = d3 - q3;
        q0 = x[e]; q1 = d1; q2 = d2; q3 = d3;
        return K == 1 ? d1 : K == 2 ? d2 : K == 3 ? d3 : d4;
    }
};

// Rice search of one wave's residual (encode.rs:3862-3947), lane l = samples [SPL l, SPL l + SPL)
// of a block of 64 SPL samples (SPL >= 16: one finest partition of a partition-order-6 block).
// Warm-up entries (lane 0, e < order <= MAXORD) count as zero and every value is folded to
// t = r ^ (r >> 31) = zigzag(r) >> 1, so that
//   sum |r| = sum t + #negative,  zigzag(r) >> k = t >> (k - 1) for k >= 1,
//   sum zigzag(r) = 2 sum t + #negative.
// Level totals come from one DPP scan of the node estimates plus ballots; nothing touches LDS.
// folded value of sample e in the second and later passes
template <int SPL, int MAXORD, class Src>
__device__ __forceinline__ uint32_t rice_folded(Src &src, int e, uint32_t first) {
    int32_t r = src.resid(e);
    if (e < MAXORD) r = (uint32_t)e >= first ? r : 0;
    return (uint32_t)(r ^ (r >> 31));
}
// Result of the partition-tree evaluation of one wave (everything of the search that needs only the
// 64 leaf sums): the chosen level, the parameters of partition `lane` and this lane's share of the
// bit count that does not depend on the individual residuals.
struct RiceTree {
    WaveRice w;       // bp, count, method, price, pesc (bits / ok are filled in by the exact pass)
    uint32_t mine;    // headers + (1 + k) * count / escaped / constant partitions: exact
    uint32_t k;       // Rice parameter of the partition this lane's SPL samples fall in, 0xFF: none
};
// mysum = this lane's sum |r| over its SPL samples (warm-up entries excluded)
// (a lower bound of the exact count from the leaf sums alone, without this tree: wave_cand_fixed.inc, Params::defer_fixed)
template <int SPL>
__device__ __forceinline__ RiceTree wave_rice_tree(uint64_t mysum, uint32_t order, const Params &p) {
    uint32_t lane = threadIdx.x & 63;
    // (opaque: the node geometry below depends on the lane only, and a persistent kernel's frame loop would
    // otherwise carry a dozen hoisted registers of it through the whole analysis)
    asm volatile("" : "+v"(lane));
    constexpr uint32_t N = 64u * SPL;  // block length
    const uint32_t P = rice_levels(N, p);
    const uint32_t rice_max = p.use_rice2 ? 31u : 15u;
    const uint32_t first = lane == 0 ? order : 0u;
    // leaf node 64 + lane (level 6) and internal node `lane` (levels 0..5), heap numbering: the
    // internal nodes' sums are differences of the inclusive prefix of the leaf sums
    const uint32_t leaf_cnt = (uint32_t)SPL - first;
    const uint32_t node = lane;
    const uint32_t lvl = node ? 31u - (uint32_t)__builtin_clz(node) : 0u;
    const uint32_t j = node - (1u << lvl);
    const uint32_t span = 64u >> lvl;
    const uint32_t hi = (j + 1) * span - 1, lo = j * span;
    const uint32_t plen = N >> lvl;
    const uint32_t istart = j * plen, iend = istart + plen;
    const uint32_t icnt = (node && iend > order) ? iend - (istart > order ? istart : order) : 0u;
    PartEval le, ie;
    if (!__any((mysum >> 25) != 0)) {
        // every leaf sum < 2^25, so every partition sum < 2^31: 32-bit arithmetic, one scan
        const uint32_t incl = wave_scan_u32((uint32_t)mysum);
        le = partition_eval_t<uint32_t>(leaf_cnt, (uint32_t)mysum, rice_max);
        const uint32_t top = __shfl(incl, (int)(hi & 63), 64);
        const uint32_t bot = __shfl(incl, (int)((lo ? lo - 1 : 0) & 63), 64);
        const uint32_t isum = top - (lo ? bot : 0u);
        ie = partition_eval_t<uint32_t>(icnt, isum, rice_max);
    } else {  // two limbs
        uint32_t sc[2] = {(uint32_t)mysum & 0xFFFFFu, (uint32_t)(mysum >> 20)};
        wave_scan_n<2>(sc);
        const uint64_t incl = ((uint64_t)sc[1] << 20) + sc[0];
        le = partition_eval(leaf_cnt, mysum, rice_max);
        const uint64_t top = __shfl(incl, (int)(hi & 63), 64);
        const uint64_t bot = __shfl(incl, (int)((lo ? lo - 1 : 0) & 63), 64);
        const uint64_t isum = top - (lo ? bot : 0ull);
        ie = partition_eval(icnt, isum, rice_max);
    }
    // per-level aggregates: estimate sums from a scan over the node lanes, the rest from ballots
    uint32_t est2[2] = {icnt ? ie.est : 0u, leaf_cnt ? le.est : 0u};
    wave_scan_n<2>(est2);
    const uint32_t esc = est2[0];
    const uint64_t m_cnt = __ballot(icnt > 0);
    const uint64_t m_bad = __ballot(icnt > 0 && ie.bad);
    const uint64_t m_hi = __ballot(icnt > 0 && ie.kind == PK_STANDARD && ie.rice >= 15);
    RiceTree t;
    WaveRice &w = t.w;
    w.bp = -1;
    w.bits = 0;
    w.ok = true;
    uint32_t best_est = 0, best_cnt = 1, best_hi = 0;
#pragma unroll
    for (uint32_t l = 0; l <= 6; l++) {
        if (l > P) break;
        uint32_t est, c;
        bool bad, hi15;
        if (l < 6) {
            const uint64_t lm = ((1ull << (1u << l)) - 1ull) << (1u << l);  // lanes 2^l .. 2^(l+1)-1
            est = sread(esc, (2 << l) - 1) - sread(esc, (1 << l) - 1);
            c = (uint32_t)__popcll(m_cnt & lm);
            bad = (m_bad & lm) != 0;
            hi15 = (m_hi & lm) != 0;
        } else {
            est = sread(est2[1], 63);
            c = (uint32_t)__popcll(__ballot(leaf_cnt > 0));
            bad = __ballot(leaf_cnt > 0 && le.bad) != 0;
            hi15 = __ballot(leaf_cnt > 0 && le.kind == PK_STANDARD && le.rice >= 15) != 0;
        }
        // `!p.is_empty() && p.len().is_power_of_two()` (encode.rs:3881), first minimum (:3885)
        const bool ok = !bad && c > 0 && (c & (c - 1)) == 0;
        if (ok && (w.bp < 0 || est < best_est)) {
            w.bp = (int)l;
            best_est = est;
            best_cnt = c;
            best_hi = hi15 ? 1u : 0u;
        }
    }
    w.count = best_cnt;
    w.method = (w.bp >= 0 && p.use_rice2 && best_hi) ? 1u : 0u;  // try_reduce_rice, :3929-3942
    const uint32_t hb = w.method ? 5u : 4u;
    // packed evaluation records to pass between lanes: cnt | kind << 16 | rice << 18 | esc << 26
    const uint32_t lrec = leaf_cnt | ((uint32_t)le.kind << 16) | ((uint32_t)le.rice << 18) | ((uint32_t)le.esc << 26);
    const uint32_t irec = icnt | ((uint32_t)ie.kind << 16) | ((uint32_t)ie.rice << 18) | ((uint32_t)ie.esc << 26);
    t.mine = 0;  // bits, wrapping u32 like the reference's counter
    t.k = 0xFF;
    w.price = 0;
    w.pesc = 0;
    if (w.bp >= 0) {
        const uint32_t bp = (uint32_t)w.bp;
        const uint32_t first_j = (1u << bp) - w.count;
        // partition q = lane of the chosen level: its record lives on lane first_j + q (leaf
        // level) or on lane 2^bp + first_j + q (internal node)
        const uint32_t qsrc = bp == 6 ? first_j + lane : (1u << bp) + first_j + lane;
        const uint32_t qrec = __shfl(bp == 6 ? lrec : irec, (int)(qsrc & 63), 64);
        if (lane < w.count) {
            const uint32_t c = qrec & 0xFFFF, kind = (qrec >> 16) & 3, rice = (qrec >> 18) & 0xFF, esc2 = qrec >> 26;
            w.price = (uint8_t)rice;
            w.pesc = (uint8_t)esc2;
            if (kind == PK_STANDARD) t.mine += hb + (1u + rice) * c;
            else if (kind == PK_ESCAPED) t.mine += hb + 5u + esc2 * c;
            else t.mine += hb + 5u;
        }
        // Rice parameter of the partition this lane's 64 samples fall in
        const uint32_t msrc = (1u << bp) + (lane >> (6 - bp));
        const uint32_t mrec = bp == 6 ? lrec : (uint32_t)__shfl(irec, (int)(msrc & 63), 64);
        t.k = (mrec >> 18) & 0xFF;
    } else if (lane == 0) {
        w.price = 0xFF;
        w.pesc = 31;  // one escaped 31-bit partition, encode.rs:3887-3895
        t.mine += 4u + 5u + 31u * (N - order);
    }
    return t;
}
// exact bit count, stored source: a[] holds the folded residuals t = r ^ (r >> 31)
// SIGNS: ... with r's sign in bit 31 (wave_rice_fold): every negative residual adds 2^(31 - sh) to the lane's sum of quotients,
// taken off again in one step (the lane's count of negatives is `neg`; arithmetic mod 2^32)
template <int SPL, bool SIGNS = false>
__device__ __forceinline__ WaveRice wave_rice_exact_stored(const RiceTree &t, const int32_t (&a)[SPL],
                                                           uint64_t sum_t, uint32_t neg) {
    WaveRice w = t.w;
    uint32_t mine = t.mine;
    bool wide = false;
    if (w.bp >= 0) {
        const uint32_t k = t.k;
        const uint32_t sh = (k == 0 || k == 0xFF) ? 0u : k - 1u;
        uint32_t q = 0;
        if constexpr (SIGNS) q = 0u - (neg << (31u - sh));
#pragma unroll
        for (int e = 0; e < SPL; e++) {
            q += (uint32_t)a[e] >> sh;
            if ((e & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        mine += k == 0xFF ? 0u : k == 0 ? 2u * (uint32_t)sum_t + neg : q;
    } else {
        // t >= 2^30  <=>  r outside [-2^30, 2^30): write_signed_counted(31) fails (:3857)
#pragma unroll
        for (int e = 0; e < SPL; e++) wide |= ((uint32_t)a[e] & (SIGNS ? 0x7FFFFFFFu : 0xFFFFFFFFu)) >= (1u << 30);
    }
    w.bits = 6u + wave_total_u32(mine);  // method (2) + partition order (4), :3949, :3902
    w.ok = !__any(wide);
    return w;
}
// exact bit count, generated source: the residual is regenerated from the samples.  With
// t = r ^ (r >> 31): zigzag(r) >> k = t >> (k - 1) for k >= 1 (4 instructions per sample beside the
// K subtractions); a wave with a k = 0 partition takes the plain zigzag form.
template <int SPL, int MAXORD, class Src>
__device__ __forceinline__ WaveRice wave_rice_exact_gen(const RiceTree &t, Src src, uint32_t order) {
    const bool lane0 = (threadIdx.x & 63) == 0;
    WaveRice w = t.w;
    uint32_t mine = t.mine;
    bool wide = false;
    // (reset() inside each branch: it makes the samples opaque, so that the compiler does not hoist
    // the residuals above the branches and keep all of them alive)
    if (w.bp >= 0) {
        const uint32_t k = t.k;
        uint32_t q = 0;
        if (!__any(k == 0)) {
            const uint32_t sh = k == 0xFF ? 0u : k - 1u;
            src.reset();
#pragma unroll
            for (int e = 0; e < SPL; e++) {
                int32_t r = src.resid(e);
                if (e < MAXORD) r = (lane0 && (uint32_t)e < order) ? 0 : r;  // warm-up: no residual
                q += (uint32_t)(r ^ (r >> 31)) >> sh;
                if ((e & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            const uint32_t ks = k == 0xFF ? 0u : k;
            src.reset();
#pragma unroll
            for (int e = 0; e < SPL; e++) {
                int32_t r = src.resid(e);
                if (e < MAXORD) r = (lane0 && (uint32_t)e < order) ? 0 : r;
                q += zigzag(r) >> ks;
                if ((e & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
        mine += k == 0xFF ? 0u : q;
    } else {
        const uint32_t first = lane0 ? order : 0u;
        src.reset();
#pragma unroll
        for (int e = 0; e < SPL; e++) wide |= rice_folded<SPL, MAXORD>(src, e, first) >= (1u << 30);
    }
    w.bits = 6u + wave_total_u32(mine);
    w.ok = !__any(wide);
    return w;
}
// Params::defer_fixed, the TIGHT bound (wave_cand_fixed.inc): one pass over the regenerated FIXED residual of the lane's leaf for
// ysum = sum (t >> sh) and odd = the number of odd quotients among them, so that sum (t >> (sh + 1)) = (ysum - odd) / 2 is
// exact as well -- two neighbouring Rice parameters from one shift per sample.  The quotients' low bits are collected 32 to a
// register (v_alignbit_b32 shifts one in at the top) and counted twice per pass.  sh is per lane; warm-up entries count as zero.
template <int SPL, int MAXORD, class Src>
__device__ __forceinline__ void wave_leaf_quotients(Src src, uint32_t order, uint32_t sh, uint32_t &ysum, uint32_t &odd) {
    static_assert(SPL % 32 == 0, "the low bits are counted 32 at a time");
    const bool lane0 = (threadIdx.x & 63) == 0;
    uint32_t acc = 0, low = 0, cnt = 0;
    src.reset();
#pragma unroll
    for (int e = 0; e < SPL; e++) {
        int32_t r = src.resid(e);
        if (e < MAXORD) r = (lane0 && (uint32_t)e < order) ? 0 : r;  // warm-up: no residual
        // (the fold commutes with the arithmetic shift: r < 0 is ~t, and ~t >> sh = ~(t >> sh))
        const uint32_t y = (uint32_t)((r >> sh) ^ (r >> 31));
        acc += y;
        // (as an opaque instruction: the builtin is a funnel shift the optimiser sees through -- it rebuilds the 32 bits as
        // a tree of and / shift / or over all 64 quotients, which are then alive together)
        asm("v_alignbit_b32 %0, %1, %0, 1" : "+v"(low) : "v"(y));
        if ((e & 31) == 31) cnt += (uint32_t)__builtin_popcount(low);
        if ((e & 7) == 7) {
            // pin the partial sum: left alone, the quotients are kept (in scratch) and added up behind the pass
            asm volatile("" : "+v"(acc));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    ysum = acc;
    odd = cnt;
}
// first pass over a stored residual: fold in place, sum |r| of this lane (= sum_t + neg)
// SIGNS (Params::hand_meta): a[e] keeps r's sign in bit 31 beside t (t < 2^31; one merging instruction per sample) -- zigzag(r)
// is then a[e] rotated left by one, which is what k_frame64 makes of the words the winning wave hands over.  Samples go in
// pairs: the second one's t exists only inside the pair's sum
template <int SPL, int MAXORD, bool SIGNS = false>
__device__ __forceinline__ void wave_rice_fold(int32_t (&a)[SPL], uint32_t order, uint64_t &sum_t, uint32_t &neg) {
    const bool lane0 = (threadIdx.x & 63) == 0;
    sum_t = 0;
    // the sign masks (0 / -1) are what the fold needs anyway: they are ADDED up (one v_add3_u32 per pair) and the
    // count of negatives is the negated sum -- written as `neg -= s` the compiler forms a second value (r >>> 31)
    // per sample for it
    int32_t sacc = 0;
    uint32_t top = 0x80000000u, low = 0x7FFFFFFFu;
    if constexpr (SIGNS) asm volatile("" : "+s"(top), "+s"(low));   // (SGPR operands: VOP3 takes no literal)
#pragma unroll
    for (int e = 0; e < SPL; e += 2) {
        int32_t r0 = a[e], r1 = a[e + 1];
        // warm-up entries carry no residual (`order` is wave-uniform: the condition is a scalar mask)
        if (e < MAXORD) r0 = (lane0 && (uint32_t)e < order) ? 0 : r0;
        if (e + 1 < MAXORD) r1 = (lane0 && (uint32_t)(e + 1) < order) ? 0 : r1;
        int32_t s0 = r0 >> 31, s1 = r1 >> 31;
        asm volatile("" : "+v"(s0), "+v"(s1));   // (keeps them the values the xor below uses)
        uint32_t t0 = (uint32_t)(r0 ^ s0), tt;
        if constexpr (SIGNS) {
            // (formed HERE, over r's register: left to the compiler the merge is sunk to the word's next use, and r, t and
            // the merged word of every sample are alive together)
            // Only the merged words stay, so the pair's second t is never formed: t0 + t1 = (r1 ^ s1) + t0 is one
            // v_xad_u32 over t0's register, and the second merged word t1 | (r1 & 2^31) = r1 ^ (s1 & 0x7FFFFFFF) one
            // v_bitop3_b32 (truth table 0x78 = a ^ (b & c)) -- tests/test_xad_fold_math.py
            asm volatile("v_and_or_b32 %0, %0, %3, %2\n\t"
                         "v_xad_u32 %2, %1, %5, %2\n\t"
                         "v_bitop3_b32 %1, %1, %5, %4 bitop3:0x78"
                         : "+v"(r0), "+v"(r1), "+v"(t0) : "s"(top), "s"(low), "v"(s1));
            a[e] = r0;
            a[e + 1] = r1;
            tt = t0;
        } else {
            const uint32_t t1 = (uint32_t)(r1 ^ s1);
            a[e] = (int32_t)t0;
            a[e + 1] = (int32_t)t1;
            tt = t0 + t1;
        }
        sacc += s0 + s1;
        sum_t += tt;  // each t < 2^31
        if ((e & 7) == 6) {
            // pin the partial count: left alone, the 64 sign terms are all kept and summed at the end of the pass
            // (64 more live registers)
            asm volatile("" : "+v"(sacc));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    neg = (uint32_t)(-sacc);
}
// whole search of a stored residual (the LPC residual, computed in place over the samples)
// unchecked: the residual came out of an FIR whose i32 subtractions were not tested for overflow -- a wrapped
// difference of a <= 25-bit sample folds to >= 2^31 - 2^24 - 1, so a lane sum below 2^30 proves there was none;
// otherwise the wave reports itself (stats[3]) and the host asks for the checked re-run (Params::check_fir)
template <int SPL, int MAXORD, bool SIGNS = false>
__device__ __forceinline__ WaveRice wave_rice_stored(int32_t (&a)[SPL], uint32_t order, const Params &p,
                                                     bool unchecked = false) {
    uint64_t sum_t;
    uint32_t neg;
    wave_rice_fold<SPL, MAXORD, SIGNS>(a, order, sum_t, neg);
    if (unchecked && __any((sum_t >> p.fir_suspect_bits) != 0ull)) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&p.stats[3], 1u);
    }
    const RiceTree t = wave_rice_tree<SPL>(sum_t + neg, order, p);
    return wave_rice_exact_stored<SPL, SIGNS>(t, a, sum_t, neg);
}

// FIR of one lane's 64 samples, IN PLACE and descending (x[e] is dead once its residual exists);
// hp[MAXO] = the MAXO samples before them (zeros for lane 0); coefficients are wave-uniform.
// No overflow tracking: the caller either rules ResidualOverflow out afterwards from the folded residual
// (wave_rice_stored, `unchecked`) or has run fir64_overflows over the same samples first (Params::check_fir).
struct KeepResidual {  // fir64 consumer: just store the residual
    __device__ __forceinline__ int32_t operator()(int, int32_t d) { return d; }
};
// f(e, residual) -> value stored in x[e]: lets a caller consume each residual where it is
// produced (k_frame64 sums the code lengths there)
template <int T, int SPL, int MAXO = 16, int CBASE = 2, class F = KeepResidual>
__device__ __forceinline__ void fir64(int32_t (&x)[SPL], const int32_t (&hp)[MAXO], uint32_t lpw,
                                      uint32_t order, uint32_t shift, F &&f = F()) {
    int32_t c[T];  // wave-uniform (SGPRs): coefficient j was loaded by lane CBASE + j
#pragma unroll
    for (int j = 0; j < T; j++) c[j] = (uint32_t)j < order ? (int32_t)sread(lpw, CBASE + j) : 0;
#pragma unroll
    for (int e = SPL - 1; e >= 0; e--) {
        long long sum = 0;
#pragma unroll
        for (int j = 0; j < T; j++) {
            const int i = e - 1 - j;
            const int32_t v = i >= 0 ? x[i >= 0 ? i : 0] : hp[i >= 0 ? 0 : MAXO + i];
            sum += (long long)v * (long long)c[j];
        }
        const int32_t pred = (int32_t)(sum >> shift);
        if constexpr (std::is_same<typename std::decay<F>::type, KeepResidual>::value) {
            // the subtraction as an opaque instruction: written as x[e] - pred, the dozen tap-count instantiations
            // of the caller's switch are scheduled with all their predictions in flight and the join of their
            // result sets costs ~100 VGPRs of copies and spills
            asm("v_sub_u32 %0, %1, %2" : "=v"(x[e]) : "v"(x[e]), "v"(pred));
        } else {
            x[e] = f(e, (int32_t)((uint32_t)x[e] - (uint32_t)pred));
        }
        if ((e & 3) == 0) __builtin_amdgcn_sched_barrier(0);
    }
}
// The same FIR with the tap count a RUN-TIME (wave-uniform) value -- r05.  The twelve fir64<T> instantiations behind a
// switch are, after the compiler's control-flow structurisation, a chain of predicated regions: nothing tells the register
// allocator that only one of them runs, so every original sample stays live THROUGH a region (the next one reads it) beside
// that region's 64 results -- 154-162 live VGPRs, 64 phi copies at the join, and at MAXO = 32 (32 history registers) 48
// bytes of scratch per lane.  Here there is ONE region: the block is walked BS samples at a time (descending, in place);
// the BS predictions of a turn are BS independent i64 accumulator chains (no serial mad chain: 1.87 instead of 2.07 ns
// per mad, profiles/r03_issue_rate_ubench.json), tap pairs are added under NESTED scalar tests `order > J` (small orders
// leave at the first test, large ones fall through not-taken branches), and a sample is overwritten once, where its
// residual is formed.  Taps are rounded up to a multiple of 2 at every order (the switch rounded to 4 above 16).
// Two taps of four consecutive samples -- acc[i] += s[i + 1] * c0 + s[i] * c1, s[k] = the sample 2 - k places before the
// quad's first sample's first tap -- as EIGHT v_mad_i64_i32 in one asm statement (sample in a VGPR, coefficient in an SGPR,
// carry-out to vcc).  Written out because (1) left to the compiler a pair of taps becomes mad + mad + a 64-bit add into the
// accumulator, and taps whose sign extensions it has hoisted become 64 x 64-bit products (v_mad_u64_u32 + two v_mul_lo_u32 +
// v_add3_u32); (2) one mad per asm statement gets an s_nop behind every one of them (the hazard recogniser pads what it
// cannot see into): +25 % on the FIR.
__device__ __forceinline__ void mad_quad(long long &a0, long long &a1, long long &a2, long long &a3, int32_t s0, int32_t s1,
                                         int32_t s2, int32_t s3, int32_t s4, int32_t c0, int32_t c1) {
    asm("v_mad_i64_i32 %0, vcc, %5, %9, %0\n\t"
        "v_mad_i64_i32 %1, vcc, %6, %9, %1\n\t"
        "v_mad_i64_i32 %2, vcc, %7, %9, %2\n\t"
        "v_mad_i64_i32 %3, vcc, %8, %9, %3\n\t"
        "v_mad_i64_i32 %0, vcc, %4, %10, %0\n\t"
        "v_mad_i64_i32 %1, vcc, %5, %10, %1\n\t"
        "v_mad_i64_i32 %2, vcc, %6, %10, %2\n\t"
        "v_mad_i64_i32 %3, vcc, %7, %10, %3"
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
        : "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "s"(c0), "s"(c1)
        : "vcc");
}
// the same for the first two taps: the accumulators start here (early-clobber outputs: written before the last input is read)
__device__ __forceinline__ void mul_quad(long long &a0, long long &a1, long long &a2, long long &a3, int32_t s0, int32_t s1,
                                         int32_t s2, int32_t s3, int32_t s4, int32_t c0, int32_t c1) {
    asm("v_mad_i64_i32 %0, vcc, %5, %9, 0\n\t"
        "v_mad_i64_i32 %1, vcc, %6, %9, 0\n\t"
        "v_mad_i64_i32 %2, vcc, %7, %9, 0\n\t"
        "v_mad_i64_i32 %3, vcc, %8, %9, 0\n\t"
        "v_mad_i64_i32 %0, vcc, %4, %10, %0\n\t"
        "v_mad_i64_i32 %1, vcc, %5, %10, %1\n\t"
        "v_mad_i64_i32 %2, vcc, %6, %10, %2\n\t"
        "v_mad_i64_i32 %3, vcc, %7, %10, %3"
        : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3)
        : "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "s"(c0), "s"(c1)
        : "vcc");
}
// sample `t` of the lane's run, t < 0: the previous lane's
template <int SPL, int MAXO>
__device__ __forceinline__ int32_t fir_tap(const int32_t (&x)[SPL], const int32_t (&hp)[MAXO], int t) {
    return t >= 0 ? x[t >= 0 ? t : 0] : hp[t >= 0 ? 0 : MAXO + t];
}
// taps J, J + 1 of the BS samples from `base` on (INIT: the accumulators start with them)
template <int J, bool INIT, int BS, int SPL, int MAXO>
__device__ __forceinline__ void fir_tap_pair(long long (&acc)[BS], const int32_t (&x)[SPL], const int32_t (&hp)[MAXO],
                                             const int32_t (&c)[MAXO], int base) {
    static_assert(BS % 4 == 0 || BS == 6, "quads (turns of 6: a quad and a pair)");
#pragma unroll
    for (int q = 0; q + 4 <= BS; q += 4) {
        const int t = base + q - 2 - J;   // s[k] = sample t + k
        if constexpr (INIT)
            mul_quad(acc[q], acc[q + 1], acc[q + 2], acc[q + 3], fir_tap<SPL, MAXO>(x, hp, t), fir_tap<SPL, MAXO>(x, hp, t + 1),
                     fir_tap<SPL, MAXO>(x, hp, t + 2), fir_tap<SPL, MAXO>(x, hp, t + 3), fir_tap<SPL, MAXO>(x, hp, t + 4), c[J], c[J + 1]);
        else
            mad_quad(acc[q], acc[q + 1], acc[q + 2], acc[q + 3], fir_tap<SPL, MAXO>(x, hp, t), fir_tap<SPL, MAXO>(x, hp, t + 1),
                     fir_tap<SPL, MAXO>(x, hp, t + 2), fir_tap<SPL, MAXO>(x, hp, t + 3), fir_tap<SPL, MAXO>(x, hp, t + 4), c[J], c[J + 1]);
    }
    if constexpr (BS % 4 != 0) {   // the last two samples of a turn of 6 (18 and 36 samples per lane), left to the compiler
#pragma unroll
        for (int i = BS - 2; i < BS; i++) {
            const int e = base + i;
            const long long pr = (long long)fir_tap<SPL, MAXO>(x, hp, e - 1 - J) * (long long)c[J] +
                                 (long long)fir_tap<SPL, MAXO>(x, hp, e - 2 - J) * (long long)c[J + 1];
            acc[i] = INIT ? pr : acc[i] + pr;
        }
    }
}
template <int J, int BS, int SPL, int MAXO>
__device__ __forceinline__ void fir_taps_from(long long (&acc)[BS], const int32_t (&x)[SPL], const int32_t (&hp)[MAXO],
                                              const int32_t (&c)[MAXO], int base, uint32_t order) {
    if constexpr (J < MAXO) {
        if (order > (uint32_t)J) {   // wave-uniform: a scalar branch
            fir_tap_pair<J, false, BS, SPL, MAXO>(acc, x, hp, c, base);
            fir_taps_from<J + 2, BS, SPL, MAXO>(acc, x, hp, c, base, order);
        }
    }
}
template <int J, int MAXO, int CBASE>
__device__ __forceinline__ void fir_coeffs_from(int32_t (&c)[MAXO], uint32_t lpw, uint32_t order) {
    if constexpr (J < MAXO) {
        if (order > (uint32_t)J) {
            c[J] = (int32_t)sread(lpw, CBASE + J);
            c[J + 1] = order > (uint32_t)(J + 1) ? (int32_t)sread(lpw, CBASE + J + 1) : 0;
            fir_coeffs_from<J + 2, MAXO, CBASE>(c, lpw, order);
        }
    }
}
template <int SPL, int MAXO = 16, int CBASE = 2, int BS = 8>
__device__ __forceinline__ void fir64_dyn(int32_t (&x)[SPL], const int32_t (&hp)[MAXO], uint32_t lpw, uint32_t order,
                                          uint32_t shift) {
    static_assert(SPL % BS == 0 && MAXO % 2 == 0, "whole turns, tap pairs");
    int32_t c[MAXO];  // wave-uniform (SGPRs): coefficient j was loaded by lane CBASE + j; only c[< order rounded up to 2] is read
#pragma unroll
    for (int j = 0; j < MAXO; j++) c[j] = 0;
    c[0] = (int32_t)sread(lpw, CBASE);
    c[1] = order > 1u ? (int32_t)sread(lpw, CBASE + 1) : 0;
    fir_coeffs_from<2, MAXO, CBASE>(c, lpw, order);
#pragma unroll
    for (int b = SPL / BS - 1; b >= 0; b--) {
        const int base = b * BS;
        // (an opaque copy of the order per turn: with one condition for all turns the optimiser merges the turns' regions
        // -- "taps 2..3 of ALL 64 samples" -- and every accumulator of the block is alive at once)
        asm volatile("" : "+s"(order));
        long long acc[BS];
        fir_tap_pair<0, true, BS, SPL, MAXO>(acc, x, hp, c, base);
        fir_taps_from<2, BS, SPL, MAXO>(acc, x, hp, c, base, order);
        // (every prediction of the turn is formed from ORIGINAL samples before the first of them is overwritten)
#pragma unroll
        for (int i = BS - 1; i >= 0; i--) {
            const int32_t pred = (int32_t)(acc[i] >> shift);
            // (volatile: a plain subtraction is SUNK to the residual's first use behind the whole FIR -- with it the
            // shift and the turn's accumulators, 128 registers of them by the last turn)
            asm volatile("v_sub_u32 %0, %1, %2" : "=v"(x[base + i]) : "v"(x[base + i]), "v"(pred));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// The overflow test of that FIR alone (ResidualOverflow, encode.rs:3190-3197): true on a lane where an i32
// subtraction x - pred outside the warm-up wraps.  The samples are only READ -- a tracking variant of the
// in-place FIR beside the plain one made the compiler keep the two result sets in different registers
// (+40 VGPRs) -- so a candidate the bound cannot clear pays a second pass over its taps.
template <int SPL, int MAXO, int CBASE = 2>
__device__ __forceinline__ bool fir64_overflows(const int32_t (&x)[SPL], const int32_t (&hp)[MAXO], uint32_t lpw,
                                                uint32_t order, uint32_t shift) {
    int32_t c[MAXO];
#pragma unroll
    for (int j = 0; j < MAXO; j++) c[j] = (uint32_t)j < order ? (int32_t)sread(lpw, CBASE + j) : 0;
    // bit e set: sample e of this lane is warm-up (lane 0 only)
    const uint32_t warm = (threadIdx.x & 63) == 0 ? (order >= 32 ? 0xFFFFFFFFu : (1u << order) - 1u) : 0u;
    uint32_t ovf = 0;
#pragma unroll
    for (int e = SPL - 1; e >= 0; e--) {
        long long sum = 0;
#pragma unroll
        for (int j = 0; j < MAXO; j++) {
            const int i = e - 1 - j;
            const int32_t v = i >= 0 ? x[i >= 0 ? i : 0] : hp[i >= 0 ? 0 : MAXO + i];
            sum += (long long)v * (long long)c[j];
        }
        const int32_t pred = (int32_t)(sum >> shift);
        const int32_t d = (int32_t)((uint32_t)x[e] - (uint32_t)pred);
        uint32_t o = (uint32_t)(x[e] ^ pred) & (uint32_t)(x[e] ^ d);  // sign bit: x - pred overflowed
        if (e < MAXO) o &= ~(warm << (31 - e));
        ovf |= o;
        if ((e & 3) == 0) {
            asm volatile("" : "+v"(ovf));   // pinned: else all 64 terms are OR-ed at the end (64 live registers)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    return (ovf >> 31) != 0;
}

__device__ __forceinline__ void store_plan_wave(SubPlan *dst, uint32_t type, uint32_t wasted,
                                                uint32_t bps, uint32_t order, uint32_t precision,
                                                uint32_t shift, uint32_t source, uint32_t bits,
                                                const WaveRice *w, uint32_t coeff /* of `lane` */,
                                                uint32_t N) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    if (lane == 0) {
        const uint32_t method = w ? w->method : 0u;
        const uint32_t count = w ? w->count : 0u;
        const uint32_t porder = count ? 31u - (uint32_t)__builtin_clz(count) : 0u;
        d[0] = type | (wasted << 8) | (bps << 16) | (order << 24);
        d[1] = precision | (shift << 8) | (method << 16) | (porder << 24);
        d[2] = source;                                       // source, reserved[3]
        d[3] = count;                                        // n_partitions
        d[4] = w ? (w->bp >= 0 ? N >> w->bp : N) : 0u;       // part_len
        d[5] = bits;
    }
    if (lane < 32) d[6 + lane] = lane < order ? coeff : 0u;  // coeffs
    uint8_t *b = reinterpret_cast<uint8_t *>(dst);
    const bool live = w && lane < w->count;
    b[24 + 128 + lane] = live ? w->price : 0;        // rice[lane]
    b[24 + 128 + 64 + lane] = live ? w->pesc : 0;    // escape_bits[lane]
}

// the choice a candidate wave ends with (wave_cand_body.inc), kept in registers until it is stored
struct FinalPlan {
    uint32_t type, wasted, bps, order, prec, shift, bits, coeff /* of `lane` */;
    bool has_w;
    WaveRice w;
};
__device__ __forceinline__ void store_final(SubPlan *dst, const FinalPlan &f, uint32_t source, uint32_t N) {
    store_plan_wave(dst, f.type, f.wasted, f.bps, f.order, f.prec, f.shift, source, f.bits, f.has_w ? &f.w : nullptr,
                    f.coeff, N);
}

// this lane's SPL consecutive samples of a row (16-byte loads when SPL is a multiple of 4,
// 8-byte loads otherwise: a lane starts SPL * 4 bytes after its neighbour)
// LAST_FIRST: the lane's last four samples are requested first (the next lane's history needs them
// before anything else can start; loads return in order)
template <int SPL, bool LAST_FIRST = false>
__device__ __forceinline__ void load_lane(const int32_t *row, uint32_t lane, int32_t (&v)[SPL]) {
    if constexpr (SPL % 4 == 0) {
        const int4 *pp = reinterpret_cast<const int4 *>(row) + (SPL / 4) * lane;
        constexpr int NQ = SPL / 4;
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            const int q = LAST_FIRST ? (i == 0 ? NQ - 1 : i - 1) : i;
            const int4 a = pp[q];
            v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
        }
    } else {
        static_assert(SPL % 2 == 0, "samples per lane must be even");
        const int2 *pp = reinterpret_cast<const int2 *>(row) + (SPL / 2) * lane;
        constexpr int NQ = SPL / 2;
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            const int q = LAST_FIRST ? (i < 2 ? NQ - 2 + i : i - 2) : i;
            const int2 a = pp[q];
            v[2 * q] = a.x; v[2 * q + 1] = a.y;
        }
    }
}

// ---- transposing load (3, 4 or 8 independent channels of 4096-sample blocks, read IN PLACE from the caller's interleaved
// batch, Params::split_src = [frame][sample][channel]; VERDICT r03 item 2b): the CW waves of a workgroup are CW CONSECUTIVE
// channels c0 .. c0 + CW - 1 of one frame -- the whole frame (CW == C: 3 or 4 channels; 5 and 6 work and were measured slower than
// the planar rows: five or six 152-register waves do not pack onto four SIMDs) or half of it (CW = 4 of C = 8).
// Turn k moves samples 4 k .. 4 k + 3 of every lane's run.  The 4 samples x CW channels of lane l are CW aligned 16-byte
// pieces of memory -- contiguous for a whole frame (4 C dwords: piece j = dwords 4 j .. 4 j + 3, dword d = sample d / C,
// channel d % C), one piece per sample for the half frame -- and thread t = CW l + j loads piece j: a wave instruction reads
// whole 128-byte lines (the half frame: half of each, the other half being the sibling workgroup's, which runs on the same
// XCD).  The thread writes its four dwords into the channel planes of LDS (plane c, dword 4 l + e: at most 2-way bank
// conflicts) and wave w reads plane w back sixteen bytes per lane (the lane's four samples, conflict-free).  Two plane sets
// alternate, so one barrier per turn; AHEAD turns of loads are in flight in registers.  The planar rows nobody else wants are
// never written (the planar copy -- half of k_autocorr4's HBM traffic for these batches -- is gone).
// buf: xpose_buf_dwords(CW) dwords, free again once the last barrier below is passed.
// 8 (and 6) channels: the two workgroups of a frame share every cache line they load; workgroups go round the 8 XCDs by their id, so
// ids i and i + 8 (same XCD, same L2) take the two halves of one frame: 16 consecutive ids = 8 frames x 2 halves
__device__ __forceinline__ uint32_t xpose_workgroup(uint32_t id, uint32_t count, uint32_t channels) {
    if ((channels != 8 && channels != 6) || id >= (count & ~15u)) return id;
    const uint32_t r = id & 15u;
    return (id & ~15u) + 2u * (r & 7u) + (r >> 3);
}
constexpr int xpose_plane(int cw) { return cw == 4 ? 256 : 260; }    // dwords per channel plane (padded where pieces straddle samples)
constexpr int xpose_buf_dwords(int cw) { return 2 * cw * xpose_plane(cw); }
template <int SPL, int CW, int C>
__device__ __forceinline__ void load_lane_xpose(const int32_t *__restrict__ frame_c0 /* the frame's sample 0, channel c0 */,
                                                int32_t *buf, uint32_t tid, int32_t (&x)[SPL]) {
    static_assert(SPL % 4 == 0 && (CW == C || (CW == 4 && C == 8)), "whole frames, or half of an 8-channel frame");
    constexpr int NP = SPL / 4, AHEAD = 4, PLANE = xpose_plane(CW), SET = CW * PLANE;
    const uint32_t wave = tid / 64u, lane = tid & 63u;
    const uint32_t l = tid / (uint32_t)CW, j = tid - l * (uint32_t)CW;
    // the thread's piece of turn 0, and where its four dwords go (plane of the channel, dword 4 l + sample)
    const int32_t *g = frame_c0 + (size_t)SPL * l * C + (CW == C ? 4u * j : j * (uint32_t)C);
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t d = 4u * j + i;
        const uint32_t e = CW == C ? d / (uint32_t)C : j, c = CW == C ? d % (uint32_t)C : (uint32_t)i;
        o[i] = c * PLANE + 4u * l + e;
    }
    int4 st[AHEAD];
#pragma unroll
    for (int k = 0; k < AHEAD && k < NP; k++) st[k] = *reinterpret_cast<const int4 *>(g + (size_t)(4 * k) * C);
#pragma unroll
    for (int k = 0; k < NP; k++) {
        int32_t *b = buf + (k & 1) * SET;
        const int4 v = st[k % AHEAD];
        b[o[0]] = v.x; b[o[1]] = v.y; b[o[2]] = v.z; b[o[3]] = v.w;
        if (k + AHEAD < NP) st[k % AHEAD] = *reinterpret_cast<const int4 *>(g + (size_t)(4 * (k + AHEAD)) * C);
        __syncthreads();
        const int4 a = *reinterpret_cast<const int4 *>(b + PLANE * wave + 4 * lane);
        x[4 * k] = a.x; x[4 * k + 1] = a.y; x[4 * k + 2] = a.z; x[4 * k + 3] = a.w;
    }
}
// 6 channels as two workgroups of three waves (5.1 material; six-wave workgroups do not pack onto the SIMDs, see above): three
// channels of a sample are 12 bytes -- no 16-byte piece --, so each workgroup loads the WHOLE frame's pieces (two per thread and
// turn: 64 lanes x 6 pieces; the sibling workgroup, same XCD, loads the same lines) and keeps the dwords of its own three
// channels; the others go to a per-thread dummy word.  Twice the LDS writes of the whole-frame load, the same line traffic
// per workgroup as the half frame of 8 channels.
constexpr int XPOSE6_BUF_DWORDS = 2 * 3 * 260 + 192;
template <int SPL>
__device__ __forceinline__ void load_lane_xpose_half6(const int32_t *__restrict__ frame0 /* the frame's sample 0, channel 0 */,
                                                      uint32_t c0 /* 0 or 3 */, int32_t *buf, uint32_t tid, int32_t (&x)[SPL]) {
    constexpr int NP = SPL / 4, AHEAD = 2, PLANE = 260, SET = 3 * PLANE;
    const uint32_t wave = tid / 64u, lane = tid & 63u;
    const int32_t *g[2];
    uint32_t o[2][2][4];   // [plane set of the turn][piece][dword]: where the dword goes (a foreign channel's: the thread's dummy word)
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t idx = tid + 192u * h, l = idx / 6u, j = idx - 6u * l;
        g[h] = frame0 + (size_t)SPL * l * 6u + 4u * j;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t d = 4u * j + i, e = d / 6u, c = d - 6u * e;
            const bool mine = c - c0 < 3u;
            const uint32_t at = (c - c0) * PLANE + 4u * l + e;
            o[0][h][i] = mine ? at : 2u * SET + tid;
            o[1][h][i] = mine ? at + SET : 2u * SET + tid;
        }
    }
    int4 st[AHEAD][2];
#pragma unroll
    for (int k = 0; k < AHEAD && k < NP; k++)
#pragma unroll
        for (int h = 0; h < 2; h++) st[k][h] = *reinterpret_cast<const int4 *>(g[h] + (size_t)(4 * k) * 6);
#pragma unroll
    for (int k = 0; k < NP; k++) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int4 v = st[k % AHEAD][h];
            buf[o[k & 1][h][0]] = v.x; buf[o[k & 1][h][1]] = v.y; buf[o[k & 1][h][2]] = v.z; buf[o[k & 1][h][3]] = v.w;
            if (k + AHEAD < NP) st[k % AHEAD][h] = *reinterpret_cast<const int4 *>(g[h] + (size_t)(4 * (k + AHEAD)) * 6);
        }
        __syncthreads();
        const int4 a = *reinterpret_cast<const int4 *>(buf + (k & 1) * SET + PLANE * wave + 4 * lane);
        x[4 * k] = a.x; x[4 * k + 1] = a.y; x[4 * k + 2] = a.z; x[4 * k + 3] = a.w;
    }
}
// the instantiation a workgroup of CW waves needs (CW == 4: the frame has 4 or 8 channels)
template <int SPL, int CW>
__device__ __forceinline__ void load_lane_xpose_cw(const int32_t *batch, uint32_t frame, uint32_t c0, uint32_t C, int32_t *buf,
                                                   uint32_t tid, int32_t (&x)[SPL]) {
    const int32_t *f = batch + (size_t)frame * (64u * SPL) * C + c0;
    if constexpr (CW == 4) {
        if (C == 8) load_lane_xpose<SPL, 4, 8>(f, buf, tid, x);
        else load_lane_xpose<SPL, 4, 4>(f, buf, tid, x);
    } else if constexpr (CW == 3) {
        if (C == 6) load_lane_xpose_half6<SPL>(f - c0, c0, buf, tid, x);
        else load_lane_xpose<SPL, 3, 3>(f, buf, tid, x);
    } else {
        load_lane_xpose<SPL, CW, CW>(f, buf, tid, x);
    }
}

// MS = false: an instantiation for independent channels (no mid / side forming: half the registers in flight
// while the samples arrive, which lets three waves share a SIMD)
// XPOSE = CW > 0 (3, 4 / 8 independent channels, 4096-sample blocks): the workgroup is CW waves whose channels come out of the
// interleaved batch through load_lane_xpose instead of planar rows somebody wrote for them
// A/B + measurement builds (-DCANDP_TIMELINE=1, tools/cand_timeline.py): lane 0 of every wave leaves 100 MHz time stamps of its
// turn's phases in the (by then consumed) autocorrelation row of its candidate -- where a persistent workgroup's time goes
#ifndef CANDP_TIMELINE
#define CANDP_TIMELINE 0
#endif
// A wave's issue priority rises with the time its turn has taken so far (one level per <us>
// microseconds, looked at behind the order statistics, the exact FIXED count and the FIR) -- a wave that is starved on its
// SIMD (the youngest of four) catches up with its frame's other three instead of keeping them at the closing barrier
constexpr uint32_t CANDP_TIME_PRIO = 5;   // us per level (r05: k_cand64p 0.159 -> 0.154 ms, 0.181 -> 0.175 on the high-order input)
#define CAND_PRIO_CHECK()                                                                               \
    do {                                                                                                \
        if (prio_t0) {                                                                                  \
            const uint32_t el_ = (uint32_t)(__builtin_amdgcn_s_memrealtime() - prio_t0);   /* 10 ns */ \
            if (el_ >= 300u * CANDP_TIME_PRIO) __builtin_amdgcn_s_setprio(3);                           \
            else if (el_ >= 200u * CANDP_TIME_PRIO) __builtin_amdgcn_s_setprio(2);                      \
            else if (el_ >= 100u * CANDP_TIME_PRIO) __builtin_amdgcn_s_setprio(1);                      \
        }                                                                                               \
    } while (0)
#if CANDP_TIMELINE
#define CAND_STAMP(k)                                                                                   \
    do {                                                                                                \
        if (tl_row) {                                                                                   \
            const uint64_t tl_t = __builtin_amdgcn_s_memrealtime();                                     \
            if (lane == 0) tl_row[k] = tl_t;                                                            \
        }                                                                                               \
    } while (0)
#else
#define CAND_STAMP(k) do { } while (0)
#endif
template <int SPL, int MAXO, bool MS = true, int XPOSE = 0>
__global__ void __launch_bounds__(XPOSE ? 64 * XPOSE : WG, 2) k_cand64(Params p) {
#if CANDP_TIMELINE
    uint64_t *const tl_row = nullptr;
#endif
    constexpr uint64_t prio_t0 = 0;
    static_assert(MAXO <= SPL && (MAXO == 16 || MAXO == 32), "history comes from the previous lane only");
    static_assert(!XPOSE || (!MS && SPL == 64), "transposing load: independent channels, 4096-sample blocks");
    constexpr uint32_t N = 64u * SPL;
    __shared__ __attribute__((aligned(16))) int32_t xbuf[XPOSE == 3 ? XPOSE6_BUF_DWORDS : XPOSE ? xpose_buf_dwords(XPOSE ? XPOSE : 4) : 4];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t wg = blockIdx.x;
    if constexpr (XPOSE) wg = xpose_workgroup(wg, gridDim.x, p.channels);
    const uint32_t local = wg * (XPOSE ? XPOSE : 4) + wave;
    if (local >= p.fcount * p.ncand) return;
    const uint32_t frame = p.f0 + local / p.ncand, cand = local % p.ncand;
    const size_t cidx = (size_t)frame * p.ncand + cand;
    // Everything the wave needs from memory is requested up front, so that one round trip is
    // exposed instead of four: candidate info, the LPC parameters (one coalesced dword per lane:
    // [0] status, [1] order | precision << 8 | shift << 16, [2..33] coefficients; handed out
    // with v_readlane later) and the samples.
    static_assert(sizeof(CandInfo) == 4 && sizeof(LpcParams) == 136, "layout");
    const uint32_t ci_raw = *reinterpret_cast<const uint32_t *>(p.cinfo + cidx);
    const uint32_t *lpw_p = reinterpret_cast<const uint32_t *>(p.lpc + cidx);
    const bool want_lpc = p.max_lpc_order > 0;
    const uint32_t lpw = (want_lpc && lane < 34) ? lpw_p[lane] : 1u;       // status 1 = no LPC
    const uint32_t qv = (want_lpc && lane < 32) ? lpw_p[2 + lane] : 0u;     // coefficient `lane`
    const CandSrc src = cand_src(p, frame, cand);
    CandInfo ci;
    memcpy(&ci, &ci_raw, 4);
    constexpr bool HAND = false;   // (Params::hand_meta: the persistent kernel's)
    bool hand_x = true;
    int32_t x[SPL], h[4];
    // the candidate's samples of this lane; mid = (l + r) >> 1 (the shift joins the wasted-bits shift),
    // side = l - r; h = the previous lane's last 4 samples (zeros before the block start)
    // (the lane's last four samples are requested first: the next lane's history needs them before
    // the order statistics can start, and those then run while the rest is still arriving)
    if constexpr (XPOSE) {
        // (whole frames only, channels a multiple of CW: the waves of a workgroup are live together and share a frame)
        load_lane_xpose_cw<SPL, XPOSE>(split_frame(p, frame, 64u * SPL * p.channels), 0u, cand - wave, p.channels, xbuf, threadIdx.x, x);
    } else {
        load_lane<SPL, true>(src.a, lane, x);
    }
    if (MS && src.mode) {
        int32_t xb[SPL];
        load_lane<SPL, true>(src.b, lane, xb);
        if (src.mode == 1) {  // wave-uniform
#pragma unroll
            for (int e = 0; e < SPL; e++) x[e] = (int32_t)((uint32_t)x[e] + (uint32_t)xb[e]);
        } else {
#pragma unroll
            for (int e = 0; e < SPL; e++) x[e] = (int32_t)((uint32_t)x[e] - (uint32_t)xb[e]);
        }
    }
    const uint32_t wasted = __builtin_amdgcn_readfirstlane((uint32_t)ci.wasted);
    const uint32_t bps_eff = __builtin_amdgcn_readfirstlane((uint32_t)ci.bps);
    if (!ci.active) return;
    SubPlan *out = p.cand_plan + cidx;
    if (ci.is_const) {  // all zero -> CONSTANT(0) at the candidate's bps (encode.rs:2883-2887)
        store_plan_wave(out, FLACGPU_SUB_CONSTANT, 0, src.bps, 0, 0, 0, src.source, 8u + src.bps, nullptr, 0, N);
        return;
    }
    FinalPlan fin;
#include "wave_cand_body.inc"
    store_final(out, fin, src.source, N);
}

// ---------------------------------------------------------------------------------
// Persistent variant with the NEXT group's rows prefetched into LDS (blocks whose lane run is a whole
// number of 16-byte pieces).  A workgroup walks groups of four candidates (g = blockIdx.x, += gridDim.x;
// stereo: the L, R, mid, side candidates of frame g).  While a group is analysed, the rows of the next
// one travel HBM -> LDS by LDS-DMA (`global_load_lds_dwordx4`: no VGPR destination, so the 230-register
// analysis keeps its registers), and its candidate info / LPC words are loaded into three registers.
// At the top of the next turn the lanes pick their samples up with conflict-free ds_read_b128 (the LDS
// image of a row is piece-major: [piece k][lane][4 samples], exactly the order the DMA writes it)
// instead of waiting 16-32 HBM round trips with only two waves per SIMD to cover them.
// STEREO: two rows per group (L by wave 0, R by wave 1; mid / side read both); else one row per wave.
// ---------------------------------------------------------------------------------
template <int SPL>
__device__ __forceinline__ void prefetch_row_lds(const int32_t *row, uint32_t lane, int32_t *lds_row) {
    static_assert(SPL % 4 == 0, "16-byte pieces");
#pragma unroll
    for (int k = 0; k < SPL / 4; k++)   // lane's piece k: samples [SPL lane + 4 k, + 4) -> lds_row[(64 k + lane) 4 ..]
        __builtin_amdgcn_global_load_lds(row + (size_t)SPL * lane + 4 * k, (__attribute__((address_space(3))) void *)(lds_row + 256 * k), 16, 0, 0);
}
template <int SPL>
__device__ __forceinline__ void read_row_lds(const int32_t *lds_row, uint32_t lane, int32_t (&v)[SPL]) {
#pragma unroll
    for (int k = 0; k < SPL / 4; k++) {
        const int4 a = *reinterpret_cast<const int4 *>(lds_row + 256 * k + 4 * lane);
        v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
    }
}

// DIRECT (stereo): the frame's INTERLEAVED PCM (Params::inter) is prefetched instead of two planar rows -- a
// lane's 64 (l, r) pairs are 32 contiguous 16-byte pieces; the 32 KB frame travels as 32 contiguous 1 KB
// segments (8 DMA instructions per wave), and a wave picks l, r, l + r or l - r out of the pieces it reads back.
// SELF (with DIRECT, streams without LPC): nobody has looked at the samples before this kernel, so the wave
// ORs its candidate itself and derives the candidate info (wasted bits, all-zero; encode.rs:2870-2898) from it.
// waves per SIMD the persistent kernel's register budget is set for (order <= 16: 165 VGPRs fit three anyway)
#define CANDP_WAVES(maxo) ((maxo) <= 16 ? 4 : 3)   // r05: 116 VGPRs at order <= 16 (fir64_dyn), 132 at order 32
// PAIR (with SELF, the fast channel choice): a workgroup is TWO waves and a turn is one frame.  encode.rs:2463-2674
// analyses only the two subframes of the assignment the abs sums choose, so of the four candidate waves two would only
// wait at the barriers: here each wave sums and ORs two candidates out of the image (wave 0: L, R; wave 1: mid,
// side), the sums meet in LDS, and wave w analyses subframe w of the chosen assignment.
// the lane's SPL samples of a direct stereo candidate fetched AGAIN from the interleaved batch (Params::defer_fixed: the
// in-place FIR has consumed the first copy; plain 16-byte loads, the frame is in this XCD's L2)
template <int SPL>
__device__ __forceinline__ void refetch_interleaved(const int32_t *frame_pcm, uint32_t mode, uint32_t cand,
                                                    uint32_t lane, int32_t (&x)[SPL]) {
    static_assert(SPL % 2 == 0, "pairs of (l, r) pairs");
    const int4 *f = reinterpret_cast<const int4 *>(frame_pcm) + (SPL / 2) * lane;
#define PICKG(EXPR0, EXPR1)                                                                  \
    _Pragma("unroll") for (int k = 0; k < SPL / 2; k++) {                                   \
        const int4 v = f[k];                                                                 \
        x[2 * k] = (EXPR0);                                                                  \
        x[2 * k + 1] = (EXPR1);                                                              \
        if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);   /* 8 pieces in flight */     \
    }
    if (mode == 1) { PICKG((int32_t)((uint32_t)v.x + (uint32_t)v.y), (int32_t)((uint32_t)v.z + (uint32_t)v.w)) }   // wave-uniform
    else if (mode == 2) { PICKG((int32_t)((uint32_t)v.x - (uint32_t)v.y), (int32_t)((uint32_t)v.z - (uint32_t)v.w)) }
    else if (cand == 1) { PICKG(v.y, v.w) }
    else { PICKG(v.x, v.z) }
#undef PICKG
}
// ... and out of the frame's LDS image, which a LATE_PREFETCH instantiation of k_cand64p keeps until the turn's last barrier:
// the same reads as the turn's first fetch (piece k of this lane at img + 4 LPS k)
template <int SPL, int LPS>
__device__ __forceinline__ void pick_from_image(const int32_t *img, uint32_t mode, uint32_t cand, int32_t (&x)[SPL]) {
    constexpr int PP = SPL / 2;
    // (one loop per mode: tested per piece, the wave-uniform mode made 2 x 32 scalar branches of the re-read -- 300 SALU
    // instructions and their bubbles, +15 % on the kernel)
#define PICKI(EXPR0, EXPR1)                                                                  \
    _Pragma("unroll") for (int k = 0; k < PP; k++) {                                        \
        const int4 v = *reinterpret_cast<const int4 *>(img + 4 * LPS * k);                  \
        x[2 * k] = (EXPR0);                                                                  \
        x[2 * k + 1] = (EXPR1);                                                              \
        if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);   /* 8 pieces in flight */     \
    }
    if (mode == 1) { PICKI((int32_t)((uint32_t)v.x + (uint32_t)v.y), (int32_t)((uint32_t)v.z + (uint32_t)v.w)) }
    else if (mode == 2) { PICKI((int32_t)((uint32_t)v.x - (uint32_t)v.y), (int32_t)((uint32_t)v.z - (uint32_t)v.w)) }
    else if (cand == 1) { PICKI(v.y, v.w) }
    else { PICKI(v.x, v.z) }
#undef PICKI
}
// A/B (compile-time, -DCANDP_LATE_PREFETCH=0): the next frame's image requested right behind the turn's first fetch (r02-r04)
// instead of behind its last barrier
// (static turns -- workgroup w takes groups w, w + grid, ... -- were r02-r05's: profiles/r05_dynamic_turns.json)

template <int SPL, int MAXO, bool STEREO, bool DIRECT = false, bool SELF = false, bool PAIR = false>
__global__ void __launch_bounds__(PAIR ? 128 : WG, CANDP_WAVES(MAXO)) k_cand64p(Params p) {
    static_assert(MAXO <= SPL && (MAXO == 16 || MAXO == 32), "history comes from the previous lane only");
    static_assert(!PAIR || (SELF && DIRECT), "two waves per frame: direct input without LPC");
    constexpr int NWAVES = PAIR ? 2 : 4;
    static_assert(!DIRECT || (STEREO && SPL % 2 == 0), "direct input: interleaved stereo, wave block lengths");
    static_assert(!SELF || DIRECT, "the candidate info comes from k_candinfo / K4 otherwise");
    constexpr uint32_t N = 64u * SPL;
    constexpr int NROWS = STEREO ? 2 : 4;
    // DIRECT: the frame as NSEG segments of <= 1 KB, 1280 bytes apart (the slack takes the per-segment shift below).
    // A consumer lane's SPL (l, r) pairs are PP = SPL / 2 contiguous 16-byte pieces; a segment is the pieces of LPS
    // whole consumer lanes (4096-sample blocks: 2 lanes = 64 pieces = 1 KB, 32 segments; 1152: 7 lanes = 63 pieces,
    // 10 segments, the last one a single lane)
    constexpr int SEG = 320;
    constexpr int PP = SPL / 2, LPS = 64 / PP, NSEG = (64 + LPS - 1) / LPS, NSW = (NSEG + NWAVES - 1) / NWAVES, SEGP = LPS * PP;
    static_assert(!DIRECT || (LPS >= 1 && LPS <= 16), "segment layout");
    // (r03's de-interleaving on landing -- dword LDS-DMA into two rows of per-lane runs -- measured 0.179 ms against 0.171-0.175
    // for the segment image: 128 dword DMA instructions per frame cost more than the L / R waves' conflicted reads and moves)
    // LATE (r05; 4096-sample direct frames with LPC): the frame's image stays in LDS through the whole turn -- the next
    // frame's DMA is requested behind the turn's LAST barrier instead of behind its first fetch -- so that a wave whose
    // exact FIXED count was put off (Params::defer_fixed) and not decided by the bound re-reads its samples from LDS, not
    // from L2 / HBM (with 1024 resident workgroups a frame has left the L2 by then: the re-fetch cost a frame 7 us, and the
    // frame's four waves meet at a barrier).  The DMA's latency is no longer hidden by this workgroup's own analysis; the
    // CU's three other workgroups cover it.
    constexpr bool LATE = DIRECT && !SELF && !PAIR && SPL == 64;
    constexpr bool HAND = LATE;   // the winners' LPC residuals handed over to k_frame64 (Params::hand_meta)
    constexpr int ROW_DW = DIRECT ? NSEG * SEG : 64 * SPL, N_ROW = DIRECT ? 1 : NROWS;
    // STEREO: the four candidates' bit counts of the frame in hand.  (4096-sample direct frames with LPC: the last segment of the
    // image ends 8 dwords short of its 1280-byte slot, which no DMA lane ever writes -- the four words live there, and the
    // workgroup's LDS is 40960 bytes sharp: four workgroups fill a CU's 160 KB exactly)
    constexpr bool WBITS_IN_TAIL = DIRECT && !SELF && SPL == 64;
    // (eight words: [0..3] the bit counts, [4] the workgroup's next turn)
    static_assert(!WBITS_IN_TAIL || ((NSEG - 1) * SEG + 4 * ((LPS * (NSEG - 1)) & 15) + 4 * SEGP <= NSEG * SEG - 8), "room behind the last segment");
    __shared__ __attribute__((aligned(16))) int32_t lds_all[N_ROW * ROW_DW + (WBITS_IN_TAIL ? 0 : 8)];
    int32_t (*const rows)[ROW_DW] = reinterpret_cast<int32_t (*)[ROW_DW]>(lds_all);
    uint32_t *const wbits = reinterpret_cast<uint32_t *>(lds_all + (N_ROW * ROW_DW + (WBITS_IN_TAIL ? 0 : 8) - 8));
    __shared__ uint64_t fast_abs[4];   // SELF, fast channel choice: the four candidates' sums of magnitudes
    __shared__ uint32_t fast_or[4];    // PAIR: their ORs
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total = p.fcount * p.ncand;
    const uint32_t groups = PAIR ? p.fcount : (total + 3) / 4;
    const bool want_lpc = p.max_lpc_order > 0;
    static_assert(sizeof(CandInfo) == 4 && sizeof(LpcParams) == 136, "layout");
    // what the next turn needs, requested one turn ahead
    uint32_t n_ci = 0, n_lpw = 1u, n_qv = 0;
    auto request = [&](uint32_t g) {
        const uint32_t local = PAIR ? g * 4 : g * 4 + wave;   // (PAIR: the frame's first candidate; which two, the turn decides)
        if (g >= groups || local >= total) return;
        const uint32_t frame = p.f0 + local / p.ncand, cand = local % p.ncand;
        const size_t cidx = (size_t)frame * p.ncand + cand;
        if constexpr (!SELF) n_ci = *reinterpret_cast<const uint32_t *>(p.cinfo + cidx);
        const uint32_t *lpw_p = reinterpret_cast<const uint32_t *>(p.lpc + cidx);
        n_lpw = (want_lpc && lane < 34) ? lpw_p[lane] : 1u;       // status 1 = no LPC
        n_qv = (want_lpc && lane < 32) ? lpw_p[2 + lane] : 0u;     // coefficient `lane`
        const CandSrc s = cand_src(p, frame, cand);
        if constexpr (DIRECT) {
            // DMA instruction j moves the contiguous segment j of the frame (pieces SEGP j .. SEGP j + SEGP - 1: the
            // (l, r) pairs of consumer lanes LPS j .. LPS j + LPS - 1) -- whole cache lines, each used once, instead of
            // 16 bytes out of 64 different lines.  Inside its segment DMA lane l fetches piece k = l / LPS of consumer
            // lane LPS j + l % LPS, and segment j lands (LPS j) mod 16 slots into its 80-slot region: piece k of
            // consumer lane c is at a lane constant + 16 LPS k bytes (immediate offsets), and the 16 lanes of a
            // ds_read_b128 pass hit bank groups (c + LPS k) mod 16 -- all different.  DMA lanes beyond a segment's
            // pieces (63 of 64 at 1152 samples) repeat piece 0 into slack slots; the last, partial segment is kept
            // inside the frame by the clamp.
            const int32_t *fsrc = inter_frame(p, frame, 2 * N) + (size_t)(4u * SEGP * NSW) * wave;   // this wave's segments
            uint32_t lpart = 4u * ((uint32_t)PP * (lane % (uint32_t)LPS) + lane / (uint32_t)LPS);
            if constexpr (SEGP != 64) lpart = lane < (uint32_t)SEGP ? lpart : 0u;
            asm volatile("" : "+v"(lpart));   // (a lane-only value: not to be hoisted out of the frame loop as NSW addresses)
#pragma unroll
            for (int k = 0; k < NSW; k++) {   // segment j = NSW wave + k
                const uint32_t j = (uint32_t)NSW * wave + k;
                if (NSEG % NWAVES == 0 || j < (uint32_t)NSEG) {
                    uint32_t lp = lpart;
                    if constexpr (64 % LPS != 0) {   // the last segment: fewer than LPS lanes
                        const uint32_t room = 2u * N - 4u - 4u * SEGP * j;
                        lp = lp < room ? lp : room;
                    }
                    __builtin_amdgcn_global_load_lds(fsrc + 4 * SEGP * k + lp,
                                                     (__attribute__((address_space(3))) void *)(&rows[0][0] + j * SEG + 4u * (((uint32_t)LPS * j) & 15u)), 16, 0, 2);   // (aux 2: non-temporal -- the frame is read once here; k_cand64p 0.1632 -> 0.1588 ms)
                }
            }
        } else if constexpr (STEREO) {
            if (wave < 2) prefetch_row_lds<SPL>(s.a, lane, rows[wave]);   // candidate 0 = L row, 1 = R row
        } else {
            prefetch_row_lds<SPL>(s.a, lane, rows[wave]);
        }
    };
    uint32_t n_decided = 0, n_refetched = 0;   // Params::defer_stats of this wave (wave-uniform)
    // DYNAMIC TURNS (r05): a workgroup's first group is blockIdx.x, every further one is drawn from the launch's counter
    // (Params::turn_counter) -- one atomic per turn by thread 0 at the turn's top, published through LDS at the barrier that
    // precedes the next image's request.  With static turns (g += gridDim.x) the four workgroups of a CU end one after the
    // other: the SIMD issues oldest wave first, so the first-launched workgroup runs its eight turns at 9-10 us each while the
    // last-launched one takes 40 us per turn, and from 60 % of the kernel's time on the SIMDs hold three, two, one wave
    // (tools/cand_timeline.py: mean workgroup 123 us, kernel 172 us).  Now the fast workgroups take more turns and all end
    // within one turn of each other.  The launch's `groups` turns draw `groups` tickets in all; whoever draws the last one
    // resets the counter for the context's next launch (the host also zeroes it with the batch's counters).
    uint32_t &next_turn = wbits[4];
    uint32_t gn = groups;
#if CANDP_TIMELINE
    uint32_t tl_turn = 0;
#endif
    request(blockIdx.x);
    for (uint32_t g = blockIdx.x; g < groups; g = gn) {
        uint32_t ticket = 0;
        // (drawn behind the turn's first barrier: in front of it the barrier's vmcnt(0) would wait for the atomic's round trip)
        auto draw_turn = [&]() {
            if (threadIdx.x == 0) ticket = atomicAdd(p.turn_counter, 1u);
        };
        auto publish_turn = [&]() {   // thread 0, before the barrier in front of the request
            if (threadIdx.x == 0) {
                next_turn = gridDim.x + ticket;
                if (ticket + 1u == groups) atomicExch(p.turn_counter, 0u);   // the launch's last draw
            }
        };
        const uint32_t local = PAIR ? g * 4 : g * 4 + wave;
        const bool have = local < total;
        const uint32_t frame = p.f0 + (have ? local : total - 1) / p.ncand;
        uint32_t cand = (have ? local : total - 1) % p.ncand;
#if CANDP_TIMELINE
        // (36 u64 per candidate row of Params::ac; [15] = HW_ID, [14] = turn index)
        uint64_t *const tl_row = (!PAIR && have) ? reinterpret_cast<uint64_t *>(p.ac) + ((size_t)frame * p.ncand + cand) * AC_LD : nullptr;
        if (tl_row && lane == 0) {
            tl_row[15] = __builtin_amdgcn_s_getreg((4 /* HW_ID */) | (0 << 6) | (31 << 11));
            tl_row[14] = tl_turn | ((uint64_t)blockIdx.x << 32);
            tl_row[13] = __builtin_amdgcn_s_getreg((20 /* XCC_ID */) | (0 << 6) | (31 << 11));
            for (int k = 3; k <= 6; k++) tl_row[k] = 0;
        }
#endif
        CAND_STAMP(0);   // turn top
        __syncthreads();   // own DMA landed (vmcnt) and everybody else's too
        CAND_STAMP(1);   // image landed
        draw_turn();
        __builtin_amdgcn_s_setprio(0);
        const uint64_t prio_t0 = __builtin_amdgcn_s_memrealtime();
        uint32_t fast_assign = FLACGPU_ASSIGN_INDEPENDENT, pair_or = 0;
        if constexpr (PAIR) {
            // sums of magnitudes and ORs of two candidates per wave, straight out of the image
            const uint32_t cj = lane / (uint32_t)LPS, cb = lane % (uint32_t)LPS;
            const int32_t *img = &rows[0][0] + cj * SEG + 4u * (((uint32_t)LPS * cj) & 15u) + 4u * cb;
            uint32_t a0 = 0, a1 = 0, o0 = 0, o1 = 0;   // <= 64 samples of <= 25 bits per lane
            if (wave == 0) {
#pragma unroll
                for (int k = 0; k < PP; k++) {
                    const int4 v = *reinterpret_cast<const int4 *>(img + 4 * LPS * k);
                    a0 += uabs(v.x) + uabs(v.z);
                    a1 += uabs(v.y) + uabs(v.w);
                    o0 |= (uint32_t)v.x | (uint32_t)v.z;
                    o1 |= (uint32_t)v.y | (uint32_t)v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < PP; k++) {
                    const int4 v = *reinterpret_cast<const int4 *>(img + 4 * LPS * k);
                    const int32_t m0 = v.x + v.y, m1 = v.z + v.w, s0 = v.x - v.y, s1 = v.z - v.w;   // <= 24-bit inputs
                    a0 += uabs(m0 >> 1) + uabs(m1 >> 1);
                    a1 += uabs(s0) + uabs(s1);
                    o0 |= (uint32_t)m0 | (uint32_t)m1;   // the OR of l + r; (l + r) >> 1 ORs to this >> 1
                    o1 |= (uint32_t)s0 | (uint32_t)s1;
                }
            }
            const uint64_t t0 = wave_sum_u64((uint64_t)a0), t1 = wave_sum_u64((uint64_t)a1);
            o0 = wave_or_u32(o0);
            o1 = wave_or_u32(o1);
            if (lane == 0) {
                fast_abs[2 * wave] = t0;
                fast_abs[2 * wave + 1] = t1;
                fast_or[2 * wave] = o0;
                fast_or[2 * wave + 1] = o1;
            }
            __syncthreads();
            fast_assign = fast_assignment(p.mid_side, fast_abs[0], fast_abs[1], fast_abs[2], fast_abs[3]);
            const uint32_t s0c = fast_assign == FLACGPU_ASSIGN_SIDE_RIGHT ? 3u : fast_assign == FLACGPU_ASSIGN_MID_SIDE ? 2u : 0u;
            const uint32_t s1c = fast_assign == FLACGPU_ASSIGN_INDEPENDENT || fast_assign == FLACGPU_ASSIGN_SIDE_RIGHT ? 1u : 3u;
            cand = wave == 0 ? s0c : s1c;   // subframe `wave` of the chosen assignment
            pair_or = fast_or[cand];
            if (threadIdx.x == 0 && have) p.finfo[frame].assignment = (uint8_t)fast_assign;
        }
        const size_t cidx = (size_t)frame * p.ncand + cand;
        const CandSrc src = cand_src(p, frame, cand);
        const uint32_t ci_raw = n_ci, lpw = n_lpw, qv = n_qv;
        bool hand_x = true;
        int32_t x[SPL], h[4];
        if constexpr (DIRECT) {
            // piece k of this lane: segment lane / LPS, shifted (LPS segment) mod 16 slots, slot LPS k + lane % LPS
            const uint32_t cj = lane / (uint32_t)LPS, cb = lane % (uint32_t)LPS;
            const int32_t *img = &rows[0][0] + cj * SEG + 4u * (((uint32_t)LPS * cj) & 15u) + 4u * cb;
#define PICK(EXPR0, EXPR1)                                                                   \
    _Pragma("unroll") for (int k = 0; k < PP; k++) {                                        \
        const int4 v = *reinterpret_cast<const int4 *>(img + 4 * LPS * k);                  \
        x[2 * k] = (EXPR0);                                                                  \
        x[2 * k + 1] = (EXPR1);                                                              \
        if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);   /* 8 pieces in flight, not 32 */ \
    }
            if (src.mode == 1) { PICK((int32_t)((uint32_t)v.x + (uint32_t)v.y), (int32_t)((uint32_t)v.z + (uint32_t)v.w)) }
            else if (src.mode == 2) { PICK((int32_t)((uint32_t)v.x - (uint32_t)v.y), (int32_t)((uint32_t)v.z - (uint32_t)v.w)) }
            else {
                // L / R: single dwords (a 16-byte read would tie x[2k], x[2k+1] to slots 0 and 2 of a register
                // quad and spread the 64 samples over 128 registers)
                const int32_t *one = img + (cand == 1 ? 1 : 0);
#pragma unroll
                for (int k = 0; k < PP; k++) {
                    x[2 * k] = one[4 * LPS * k];
                    x[2 * k + 1] = one[4 * LPS * k + 2];
                }
            }
#undef PICK
        } else if constexpr (STEREO) {
            // mid / side piece by piece (both rows read whole first would keep 128 samples alive: a third wave
            // per SIMD needs the kernel below 168 VGPRs)
#define PICK2(OP)                                                                                     \
    _Pragma("unroll") for (int k = 0; k < SPL / 4; k++) {                                            \
        const int4 a = *reinterpret_cast<const int4 *>(&rows[0][0] + 256 * k + 4 * lane);            \
        const int4 b = *reinterpret_cast<const int4 *>(&rows[1][0] + 256 * k + 4 * lane);            \
        x[4 * k] = (int32_t)((uint32_t)a.x OP (uint32_t)b.x);                                        \
        x[4 * k + 1] = (int32_t)((uint32_t)a.y OP (uint32_t)b.y);                                    \
        x[4 * k + 2] = (int32_t)((uint32_t)a.z OP (uint32_t)b.z);                                    \
        x[4 * k + 3] = (int32_t)((uint32_t)a.w OP (uint32_t)b.w);                                    \
        if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);   /* 8 pieces in flight, not 32 */      \
    }
            if (src.mode == 1) { PICK2(+) }        // wave-uniform
            else if (src.mode == 2) { PICK2(-) }
            else read_row_lds<SPL>(rows[cand], lane, x);
#undef PICK2
        } else {
            read_row_lds<SPL>(rows[wave], lane, x);
        }
        if constexpr (!LATE) {
            publish_turn();
            __syncthreads();   // every wave has its samples: the rows may be overwritten
            gn = next_turn;
            request(gn);
        }
        CAND_STAMP(2);   // samples in registers
        CandInfo ci;
        memcpy(&ci, &ci_raw, 4);
        if constexpr (PAIR) {
            uint32_t orv = pair_or;
            if (src.mode == 1) orv = (uint32_t)((int32_t)orv >> 1);
            ci = cand_info_from_or(p, cand, __builtin_amdgcn_readfirstlane(orv), true);
        } else if constexpr (SELF) {
            uint32_t orv = 0;
#pragma unroll
            for (int e = 0; e < SPL; e++) orv |= (uint32_t)x[e];
            orv = wave_or_u32(orv);
            // mid is held as l + r until the shift below: the OR of (l + r) >> 1 is the OR shifted
            if (src.mode == 1) orv = (uint32_t)((int32_t)orv >> 1);
            bool act = true;
            if (!p.exhaustive) {
                // the fast channel choice (encode.rs:2463-2674) in the workgroup as well: its four waves hold L, R,
                // mid (as l + r) and side of one frame, so each sums its magnitudes, the four sums meet in LDS and
                // every wave knows the assignment -- no k_stereo_stats pass over the batch before this kernel
                uint32_t a = 0;   // <= 64 samples of <= 25 bits
                if (src.mode == 1) {
#pragma unroll
                    for (int e = 0; e < SPL; e++) a += uabs(x[e] >> 1);
                } else {
#pragma unroll
                    for (int e = 0; e < SPL; e++) a += uabs(x[e]);
                }
                const uint64_t tot = wave_sum_u64((uint64_t)a);
                if (lane == 0) fast_abs[wave] = tot;
                __syncthreads();
                fast_assign = fast_assignment(p.mid_side, fast_abs[0], fast_abs[1], fast_abs[2], fast_abs[3]);
                act = active_in_assignment(fast_assign, cand);
                if (threadIdx.x == 0 && have) p.finfo[frame].assignment = (uint8_t)fast_assign;
            }
            ci = cand_info_from_or(p, cand, __builtin_amdgcn_readfirstlane(orv), act);
        }
        const uint32_t wasted = __builtin_amdgcn_readfirstlane((uint32_t)ci.wasted);
        const uint32_t bps_eff = __builtin_amdgcn_readfirstlane((uint32_t)ci.bps);
        FinalPlan fin;
        fin.bits = 0xFFFFFFFFu;
        const bool done = have && ci.active;
        if (done) {
            if (ci.is_const) {  // all zero -> CONSTANT(0) at the candidate's bps (encode.rs:2883-2887)
                fin = FinalPlan{FLACGPU_SUB_CONSTANT, 0, src.bps, 0, 0, 0, 8u + src.bps, 0, false, WaveRice{}};
            } else {
                // (Params::defer_fixed: direct stereo input can be fetched again)
                constexpr bool CAND_CAN_REFETCH = DIRECT && !SELF;
#define CAND_REFETCH(xs)                                                                                              \
    do {                                                                                                              \
        if constexpr (LATE) {                                                                                         \
            uint32_t l2 = lane;                                                                                       \
            asm volatile("" : "+v"(l2));   /* (a lane-only address: not to be hoisted out of the frame loop) */       \
            pick_from_image<SPL, LPS>(&rows[0][0] + (l2 / (uint32_t)LPS) * SEG + 4u * (((uint32_t)LPS * (l2 / (uint32_t)LPS)) & 15u) + \
                                          4u * (l2 % (uint32_t)LPS), src.mode, cand, xs);                             \
        } else {                                                                                                      \
            refetch_interleaved<SPL>(inter_frame(p, frame, 128 * SPL), src.mode, cand, lane, xs);                                       \
        }                                                                                                             \
    } while (0)
#define CAND_DEFER_COUNT(dec) (n_decided += (dec) ? 1u : 0u, n_refetched += (dec) ? 0u : 1u)
#include "wave_cand_body.inc"
#undef CAND_DEFER_COUNT
#undef CAND_REFETCH
            }
        }
        if constexpr (STEREO) {
            // K6 in the workgroup: its four waves are the L, R, mid and side candidates of one frame, so the
            // channel assignment (encode.rs:2747-2786 / 2803-2835: first minimum of the candidate sums) is
            // decided here, the two chosen waves write their plans straight into the frame's subframe slots
            // and no candidate plan travels through HBM to a k_decide launch
            CAND_STAMP(6);   // analysis done
            if (lane == 0) wbits[wave] = fin.bits;
            if constexpr (LATE) publish_turn();
            __syncthreads();
            CAND_STAMP(7);   // the frame's four waves met
            // the channel choice (encode.rs:2747-2786 / 2803-2835) -- every wave computes it from the four counts
            auto choose = [&]() -> uint32_t {
                uint32_t assign = FLACGPU_ASSIGN_INDEPENDENT;
                if (p.exhaustive) {
                    const uint32_t l = wbits[0], r = wbits[1], sd = wbits[3];
                    int b = 0;
                    if (p.mid_side) {
                        const uint32_t m = wbits[2];
                        const uint32_t tot[4] = {l + r, l + sd, sd + r, m + sd};
                        for (int i = 1; i < 4; i++)
                            if (tot[i] < tot[b]) b = i;
                    } else {
                        const uint32_t tot[3] = {l + r, l + sd, sd + r};
                        for (int i = 1; i < 3; i++)
                            if (tot[i] < tot[b]) b = i;
                    }
                    assign = b == 0 ? FLACGPU_ASSIGN_INDEPENDENT : b == 1 ? FLACGPU_ASSIGN_LEFT_SIDE
                           : b == 2 ? FLACGPU_ASSIGN_SIDE_RIGHT : FLACGPU_ASSIGN_MID_SIDE;
                } else {
                    if constexpr (SELF) assign = fast_assign;          // chosen above
                    else assign = p.finfo[frame].assignment;           // chosen by k_stereo_stats
                }
                return assign;
            };
            uint32_t assign = FLACGPU_ASSIGN_INDEPENDENT, sel0 = 0, sel1 = 1;
            auto selected = [&]() {
                sel0 = assign == FLACGPU_ASSIGN_SIDE_RIGHT ? 3u : assign == FLACGPU_ASSIGN_MID_SIDE ? 2u : 0u;
                sel1 = assign == FLACGPU_ASSIGN_INDEPENDENT || assign == FLACGPU_ASSIGN_SIDE_RIGHT ? 1u : 3u;
            };
            if constexpr (LATE) {   // nobody reads the image any more (wbits lie behind its last segment)
                gn = next_turn;
                request(gn);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (HAND) {
                // THE RESIDUAL HANDED OVER (Params::hand_meta): a winning wave whose registers still hold the folded residual of
                // its LPC candidate stores it for k_frame64 -- right behind the next image's request, before the plan's store
                // needs registers of its own; sixteen non-temporal kilobyte stores (nobody reads the row before the next kernel)
                assign = choose();
                selected();
                if (p.hand_meta && done && (wave == sel0 || wave == sel1)) {   // wave-uniform
                    const uint32_t sub = __builtin_amdgcn_readfirstlane(frame * 2u + (wave == sel0 ? 0u : 1u));
                    const bool ok = hand_x && fin.type == FLACGPU_SUB_LPC;
                    if (ok) {
                        int32_t *const row = p.residuals + (size_t)sub * N;   // (a scalar base + the lane's offset)
                        typedef int v4i __attribute__((ext_vector_type(4)));
#pragma unroll
                        for (int j = 0; j < SPL / 4; j++) {
                            const v4i q4 = {x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
                            __builtin_nontemporal_store(q4, reinterpret_cast<v4i *>(row) + 64 * j + lane);
                        }
                    }
                    if (lane == 0) p.hand_meta[sub] = ok ? 1u : 0u;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (PAIR) {   // both waves hold a chosen subframe: wave w is subframe w
                if (done) store_final(p.out_plan + (size_t)frame * 2 + wave, fin, src.source, N);
                if (threadIdx.x == 0) {
                    flacgpu_frame_plan fp;
                    fp.assignment = (uint8_t)fast_assign;
                    fp.channels = 2;
                    fp.block_size = (uint16_t)N;
                    fp.body_bits = wbits[0] + wbits[1];
                    p.frame_plan[frame] = fp;
                }
                continue;
            }
            if constexpr (!HAND) {
                assign = choose();
                selected();
            }
            if (done && (wave == sel0 || wave == sel1))
                store_final(p.out_plan + (size_t)frame * 2 + (wave == sel0 ? 0u : 1u), fin, src.source, N);
            if (threadIdx.x == 0) {
                flacgpu_frame_plan fp;
                fp.assignment = (uint8_t)assign;
                fp.channels = 2;
                fp.block_size = (uint16_t)N;
                fp.body_bits = wbits[sel0] + wbits[sel1];
                p.frame_plan[frame] = fp;
            }
        } else {
            if (done) store_final(p.cand_plan + cidx, fin, src.source, N);
        }
        CAND_STAMP(8);   // turn end
#if CANDP_TIMELINE
        tl_turn++;
#endif
    }
    if (lane == 0 && (n_decided | n_refetched)) {
        // (64 slots, 64 bytes apart, summed by the host: with dynamic turns the workgroups end together, and 8000 atomics on
        // one word are served one after the other -- the memory channel of that word held up the last workgroups' plan
        // stores for 35 us, tools/cand_timeline.py)
        uint32_t *slot = p.defer_stats + DEFER_SLOT_WORDS * (blockIdx.x % DEFER_SLOTS);
        if (n_decided) atomicAdd(&slot[0], n_decided);
        if (n_refetched) atomicAdd(&slot[1], n_refetched);
    }
}
