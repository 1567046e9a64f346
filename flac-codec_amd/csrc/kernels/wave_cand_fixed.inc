// wave_cand_fixed.inc -- FIXED half of a candidate wave's analysis: abs sums of the iterated differences, order
// choice, Rice search and exact bit count (encode.rs:3020-3088, 3747-3962).  Textually included (wave_cand_body.inc
// for the one-wave-per-candidate kernels, wave_cand_split.inc for the FIXED waves of the split kernel).
// In scope: p, lane, x[SPL] (shifted), h[4], wasted, bps_eff, N, SPL.  Leaves forder, fw, fixed_bits, fixed_ok.
    // ---- FIXED: abs sums of the iterated differences over [4, n) (encode.rs:3039-3073).
    // Values are biased (unsigned), |a - b| + acc is one v_sad_u32 of two values with the SAME bias.  The samples and
    // the first differences carry 2^30.  The second and third differences are formed as (p ^ 0x7FFFFFFF) + d, one
    // v_xad_u32 instead of a subtraction and a re-bias: p ^ 0x7FFFFFFF = -p - 1 + 2^31 (mod 2^32), so the result is
    // d - p + (2^31 - 1) whatever bias d and p share, and it carries 2^31 - 1 itself -- as its predecessor does, so the
    // v_sad_u32 of the two and the next level's xad hold.  |d_K| < 2^(24 + K) <= 2^27 keeps d_K + 2^31 - 1 inside u32
    // (tests/test_xad_fold_math.py: the same arithmetic in numpy).  The u32 partial sums are
    // flushed as late as the candidate width allows (<= 25 bits: |d_K| < 2^(24 + K), so 64 terms of
    // orders 0..2, 32 of order 3 and 16 of order 4 stay below 2^32).
    constexpr uint32_t BIAS = 1u << 30;
    uint32_t flip = 0x7FFFFFFFu;
    asm volatile("" : "+s"(flip));   // (an SGPR operand: VOP3 takes no literal)
    uint64_t sm[5] = {0, 0, 0, 0, 0}, leaf[5];
    uint32_t w1 = 0, w2 = 0, w3 = 0;
    {
        const uint32_t hb0 = (uint32_t)h[0] + BIAS, hb1 = (uint32_t)h[1] + BIAS, hb2 = (uint32_t)h[2] + BIAS,
                       hb3 = (uint32_t)h[3] + BIAS;
        const uint32_t d1m3 = hb1 - hb0 + BIAS, d1m2 = hb2 - hb1 + BIAS, d1m1 = hb3 - hb2 + BIAS;
        const uint32_t d2m2 = (d1m3 ^ flip) + d1m2, d2m1 = (d1m2 ^ flip) + d1m1;   // bias 2^31 - 1 from here on
        uint32_t p0 = hb3, p1 = d1m1, p2 = d2m1, p3 = (d2m2 ^ flip) + d2m1;
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4));
        uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;  // contributions of samples 0..3
#pragma unroll
        for (int e = 0; e < SPL; e++) {
            const uint32_t xb = (uint32_t)x[e] + BIAS;
            // (the first difference from the UNBIASED previous sample, which is in a register anyway: one
            // instruction instead of a subtraction and a re-bias)
            const uint32_t d1 = xb - (uint32_t)(e ? x[e ? e - 1 : 0] : h[3]);
            const uint32_t d2 = (p1 ^ flip) + d1, d3 = (p2 ^ flip) + d2;
            a0 = __usad(xb, BIAS, a0);
            a1 = __usad(xb, p0, a1);
            a2 = __usad(d1, p1, a2);
            a3 = __usad(d2, p2, a3);
            a4 = __usad(d3, p3, a4);
            p0 = xb; p1 = d1; p2 = d2; p3 = d3;
            if (e == 0) w1 = a1;   // order K's warm-up = samples 0..K-1: sum |d_K| over them
            if (e == 1) w2 = a2;
            if (e == 2) w3 = a3;
            if (e == 3) { c0 = a0; c1 = a1; c2 = a2; c3 = a3; c4 = a4; }
            // opaque zeros after a flush: with a known-zero accumulator the compiler expands the next
            // v_sad_u32 into v_min + v_max + v_sub
            if ((e & 15) == 15 || e == SPL - 1) {
                sm[4] += a4;
                a4 = 0;
                asm volatile("" : "+v"(a4));
            }
            if ((e & 31) == 31 || e == SPL - 1) {
                sm[3] += a3;
                a3 = 0;
                asm volatile("" : "+v"(a3));
            }
            if ((e & 63) == 63 || e == SPL - 1) {
                sm[0] += a0; sm[1] += a1; sm[2] += a2;
                a0 = a1 = a2 = 0;
                asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2));
            }
            if ((e & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // keep the scheduler from hoisting all 64 chains
        }
        // sm: this lane's sum |d_K| over all 64 samples = the Rice search's leaf sums once the
        // warm-up of the chosen order is taken out (lane 0); the order choice sums [4, n)
        if (lane == 0) {
            leaf[0] = sm[0]; leaf[1] = sm[1] - w1; leaf[2] = sm[2] - w2; leaf[3] = sm[3] - w3; leaf[4] = sm[4] - c4;
            sm[0] -= c0; sm[1] -= c1; sm[2] -= c2; sm[3] -= c3; sm[4] -= c4;
        } else {
#pragma unroll
            for (int k = 0; k < 5; k++) leaf[k] = sm[k];
        }
    }
    {   // wave totals of the five sums (< 2^48 each): ten 24-bit limbs scanned together
        uint32_t limb[10];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            limb[2 * k] = (uint32_t)sm[k] & 0xFFFFFFu;
            limb[2 * k + 1] = (uint32_t)(sm[k] >> 24);
        }
        wave_scan_n<10>(limb);
#pragma unroll
        for (int k = 0; k < 5; k++) sm[k] = ((uint64_t)sread(limb[2 * k + 1], 63) << 24) + sread(limb[2 * k], 63);
    }
    uint32_t forder = 0;
#pragma unroll
    for (uint32_t k = 1; k <= 4; k++)
        if (sm[k] < sm[forder]) forder = k;  // min_by_key: first minimum wins
    // The FIXED residual's partition search needs only the leaf sums the order statistics already
    // hold; its exact bit count regenerates the residual from the samples.
    uint64_t fleaf = leaf[0];
#pragma unroll
    for (uint32_t k = 1; k <= 4; k++) fleaf = forder == k ? leaf[k] : fleaf;
#ifdef CAND_REFETCH
    // Params::defer_fixed (r05): the partition TREE of this half, the exact count and with them the need for the samples are put
    // off behind the LPC half where the LPC size estimate undercuts a LOWER BOUND of this half's size by the margin; an exact
    // `lpc_bits < bound` then decides encode.rs:2929-2934 for LPC (wave_cand_body.inc), otherwise the wave builds the tree,
    // re-reads its samples and counts after all.
    // The bound needs the 64 leaf sums only.  Whatever level the search chooses, a partition (count c, sum S of |r|) costs at
    // least 4 + min_k (k c + 2 S / 2^k) bits -- a Rice partition with the rule's k: 4 + (k + 1) c + sum (u >> k), and
    // sum (u >> k) >= 2 S / 2^k - c; an escaped one (k >= 15 / 31, c >= 2) more than c (log2 (S / c) + 2); an all-zero one 4 --
    // and c g(S / c) with g(m) = min_k (k + 2 m / 2^k) is CONCAVE in m, so the leaves of a partition together cost no more
    // than the partition (Jensen): 10 + the sum over the 64 leaves of c g(S / c) bounds the residual block at ANY level.
    // Per leaf, with the rule's own k = ceil(log2(S / c)): min_k (...) >= k c + (2 S >> k) - ceil(0.0861 c) (the rule's k is
    // within 0.0861 bit per residual of the real-valued minimum, log2 m + 1.9139), and 2 S where S <= c.
    // (tests/test_leaf_bound_math.py: the same arithmetic in numpy against the exact bits at every partition order.)
    const uint32_t lst = sread(lpw, 0), est8 = sread(lpw, 1) >> 24;
    const uint32_t est_bits = (est8 * N >> 3) + 17u + wasted;   // + the subframe's fixed header bits
    const bool may_defer = CAND_CAN_REFETCH && p.defer_fixed != 0 && lst == 0 && est8 != 0;
    const uint32_t fixed_head = 8u + wasted + forder * bps_eff;
    const uint32_t need = est_bits + (p.defer_margin16 * N >> 4);   // the bound is of use from here on
    bool defer = false;
    uint32_t fixed_lb = 0;
    if (may_defer) {   // wave-uniform
        // (about what the bound can reach -- the leaves' c g(S / c) add up to at most N g(S_total / N) <= k N + 2 S_total / 2^k
        // for the rule's k of the whole block (the order statistics' total, which leaves the first four samples out: a
        // heuristic, the decision below is made on the bound itself) -- all wave-uniform: where the estimate does not get
        // there the bound is not formed)
        uint64_t stot = sm[0];
#pragma unroll
        for (uint32_t k = 1; k <= 4; k++) stot = forder == k ? sm[k] : stot;
        uint32_t kt = 0;
        if (stot > (uint64_t)N) {
            const uint32_t bs = 64u - (uint32_t)__clzll((long long)stot), bc = 32u - (uint32_t)__builtin_clz(N);
            kt = bs > bc ? bs - bc - 1 : 0;
            kt += (((uint64_t)N << kt) < stot) ? 1u : 0u;
            kt += (((uint64_t)N << kt) < stot) ? 1u : 0u;
        }
        const uint64_t reach64 = (uint64_t)fixed_head + 10u + (uint64_t)kt * N + ((2 * stot) >> kt);
        const uint32_t reach = reach64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)reach64;
        // The TIGHT bound (whole leaves of 64 samples; tests/test_leaf_bound_tight_math.py, the same arithmetic in numpy in
        // tests/_leaf_bound_tight.py): the leaf sums cannot know sum (u mod 2^k) and give away half a bit per residual, as much
        // as LPC gains over FIXED on a low-order signal.  Where the bound above does not get there, one more pass over the
        // FIXED residual gives the leaf's quotient sums at its own k (the rule's, from its sum) and at k - 1 EXACTLY
        // (wave_leaf_quotients): the leaf's cost at those two is known, at k + 1 it is at least c (k + 2) + ceil((Q - c) / 2)
        // (a quotient halves to no less than (q - 1) / 2), further up no less than that (Q <= 2 c under the rule's k), at
        // k - 1 - d at least c (k - d) + 2^d Q' (a quotient at least doubles per step down; the d that minimises it: the first
        // with 2^d Q' >= c); an escaped partition costs its leaf more than c (k + 3) >= the exact cost at k (its escape_bits
        // are ilog2 of a sum >= S, plus 2), the 31-bit fallback 31 c.  The minimum of these bounds the leaf under ANY
        // parameter, and a partition of several leaves has one parameter: it costs at least the sum of their minima.
        // It can reach one bit per residual above the leaf sums' bound (Q <= 2 S / 2^k, where that one has 2 S / 2^k - c).
        constexpr bool TIGHT = SPL == 64;
        const uint32_t reach_t = TIGHT ? (reach > 0xFFFFFFFFu - N ? 0xFFFFFFFFu : reach + N) : reach;
        if (p.defer_fixed >= 2 || need <= reach_t) {
            // (an opaque copy of the leaf sum, made HERE: otherwise the per-lane part below is speculated above the two
            // wave-uniform tests and every candidate pays for it)
            uint32_t fl_lo = (uint32_t)fleaf, fl_hi = (uint32_t)(fleaf >> 32);
            asm volatile("" : "+v"(fl_lo), "+v"(fl_hi));
            const uint64_t fl = ((uint64_t)fl_hi << 32) | fl_lo;
            const uint32_t lcnt = (uint32_t)SPL - (lane == 0 ? forder : 0u);
            uint32_t lbl, k = 0;
            if (fl >> 40) {
                lbl = 0u;   // (no such sums from <= 32-bit residuals of 64 samples)
            } else if (fl <= (uint64_t)lcnt) {
                lbl = (uint32_t)(2 * fl);
            } else {
                const uint32_t bs = 64u - (uint32_t)__clzll((long long)fl), bc = 32u - (uint32_t)__builtin_clz(lcnt);
                k = bs > bc ? bs - bc - 1 : 0;
                k += (((uint64_t)lcnt << k) < fl) ? 1u : 0u;
                k += (((uint64_t)lcnt << k) < fl) ? 1u : 0u;
                lbl = k * lcnt + (uint32_t)((2 * fl) >> k) - 6u;   // (ceil(0.0861 * 64) = 6; k c >= 12 here)
            }
            uint32_t lb0 = fixed_head + 10u + wave_total_u32(lbl);
            // (2, TEST: every candidate with LPC parameters, on the leaf sums' bound; 3, TEST: the same on the tight one)
            bool go = p.defer_fixed == 2 || (p.defer_fixed == 1 && need <= lb0);
            if constexpr (TIGHT) {
                if (!go) {   // wave-uniform (1: need <= reach_t holds here)
                    const uint32_t rice_max = p.use_rice2 ? 31u : 15u;
                    const uint32_t sh = k >= 2u ? k - 2u : 0u;
                    uint32_t ys = 0, odd = 0;
                    switch (forder) {
                    case 0: wave_leaf_quotients<SPL, 4>(FixedSrc<0, SPL>{x, h}, 0, sh, ys, odd); break;
                    case 1: wave_leaf_quotients<SPL, 4>(FixedSrc<1, SPL>{x, h}, 1, sh, ys, odd); break;
                    case 2: wave_leaf_quotients<SPL, 4>(FixedSrc<2, SPL>{x, h}, 2, sh, ys, odd); break;
                    case 3: wave_leaf_quotients<SPL, 4>(FixedSrc<3, SPL>{x, h}, 3, sh, ys, odd); break;
                    default: wave_leaf_quotients<SPL, 4>(FixedSrc<4, SPL>{x, h}, 4, sh, ys, odd); break;
                    }
                    // k >= 2: ys = sum (u >> (k - 1)), odd its odd terms; k < 2: ys = sum t, and sum u = S + sum t
                    const uint32_t s32 = (uint32_t)fl;
                    const uint32_t q0 = k >= 2u ? (ys - odd) >> 1 : k == 1u ? ys : s32 + ys;    // sum (u >> k)
                    const uint32_t qm = k >= 2u ? ys : s32 + ys;                                // sum (u >> (k - 1)), k >= 1
                    uint32_t lt = lcnt * (k + 1u) + q0;
                    if (k + 1u < rice_max) {
                        const uint32_t up = q0 > lcnt ? (q0 - lcnt + 1u) >> 1 : 0u;
                        lt = min(lt, lcnt * (k + 2u) + up);
                    }
                    if (k >= 1u) {
                        // the first d with qm << d >= c, at most k - 1 (qm = 0: k - 1)
                        const uint32_t bq = 32u - (uint32_t)__builtin_clz(qm | 1u), bc = 32u - (uint32_t)__builtin_clz(lcnt);
                        uint32_t d = bc > bq ? bc - bq : 0u;
                        d += ((qm << d) < lcnt) ? 1u : 0u;
                        d = qm == 0u ? k - 1u : min(d, k - 1u);
                        lt = min(lt, lcnt * (k - d) + (qm << d));
                    }
                    // (an all-zero leaf costs nothing; a leaf whose rule asks for an escape, or with an impossible sum,
                    // keeps the leaf sums' bound; no leaf costs more than in the 31-bit fallback partition)
                    if (s32 == 0u && fl_hi == 0u) lt = 0u;
                    if (k >= rice_max || (fl >> 40)) lt = lbl;
                    lt = min(lt, 31u * lcnt);
                    const uint32_t lbt = fixed_head + 10u + wave_total_u32(lt);
                    lb0 = max(lb0, lbt);
                    go = p.defer_fixed == 3 || need <= lb0;
                }
            }
            if (go) {
                defer = true;
                fixed_lb = lb0;
            }
        }
    }
    RiceTree ft{};   // (deferred: stays zero -- a decided candidate that ends VERBATIM stores it with its plan; otherwise it is
                     // read again only behind the late wave_rice_tree of wave_cand_body.inc)
    if (!defer) ft = wave_rice_tree<SPL>(fleaf, forder, p);
#else
    const RiceTree ft = wave_rice_tree<SPL>(fleaf, forder, p);
    constexpr bool defer = false;
#endif
    WaveRice fw = ft.w;
    CAND_STAMP(3);   // order statistics + FIXED partition tree done
    CAND_PRIO_CHECK();
    // the exact count regenerates the FIXED residual from the samples (x, h): before the in-place FIR -- or behind it from
    // re-fetched samples (wave_cand_body.inc)
#define FIXED_EXACT_COUNT()                                                                      \
    switch (forder) {                                                                            \
    case 0: fw = wave_rice_exact_gen<SPL, 4>(ft, FixedSrc<0, SPL>{x, h}, 0); break;             \
    case 1: fw = wave_rice_exact_gen<SPL, 4>(ft, FixedSrc<1, SPL>{x, h}, 1); break;             \
    case 2: fw = wave_rice_exact_gen<SPL, 4>(ft, FixedSrc<2, SPL>{x, h}, 2); break;             \
    case 3: fw = wave_rice_exact_gen<SPL, 4>(ft, FixedSrc<3, SPL>{x, h}, 3); break;             \
    default: fw = wave_rice_exact_gen<SPL, 4>(ft, FixedSrc<4, SPL>{x, h}, 4); break;            \
    }
    if (!defer) { FIXED_EXACT_COUNT() }
    CAND_STAMP(4);   // exact FIXED count done (or deferred)
    CAND_PRIO_CHECK();
    uint32_t fixed_bits = 8u + wasted + forder * bps_eff + fw.bits;
    bool fixed_ok = fw.ok;
