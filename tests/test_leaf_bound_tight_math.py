"""The TIGHT lower bound of a FIXED residual block behind Params::defer_fixed (kernels/wave_cand_fixed.inc), restated in numpy
(tests/_leaf_bound_tight.py) and held against the exact Rice sizes by brute force: every partition order 0..6, and in every
partition EVERY parameter 0 .. rice_max - 1, the escape code (escape_bits = ilog2(sum) + 2, encode.rs:3787-3800) and the
31-bit fallback partition -- the cheapest way any encoder could code the block, which no plan of the reference undercuts.
Three forms of the bound are held to it: exact at the rule's parameter only, exact at that and the one below it, and the
closed form the kernel evaluates (`kernel_tight_bound`, the same integer steps as the device code).
"The bound equals the leaf's brute-force cost where the rule's parameter is the optimum" holds only as far as a MINIMUM of lower
bounds can: the terms at the rule's parameter and below it are exact, the term at the parameter above is a lower bound and may
undercut them (a leaf of one outlier among zeros: cost 206 at the rule's k = 1, bounded 199 from k = 2) -- the test holds the
bound to exactly that: min(the optimum, the bound one parameter up), and counts thousands of leaves where the two are equal.  CPU only: the arithmetic,
not the kernel (tests/test_gpu_leaf_bound_tight.py runs the kernel)."""
import numpy as np
import pytest

import _leaf_bound_tight as lbt

N, LEAF, NLEAF = lbt.N, lbt.LEAF, lbt.NLEAF


def quotient_table(r, order, rice_max):
    """q[k][leaf] = sum (u >> k) over the leaf's residuals; c[leaf], s[leaf]"""
    c, s, u, _ = lbt.leaf_tables(r, order)
    q = np.stack([(u >> k).sum(axis=1) for k in range(rice_max)])
    return q, c, s


def cheapest_block(r, order, rice_max):
    """the fewest bits the residual block can take: 6 + min over the partition orders of the sum over the partitions of
    4 + min(every Rice parameter, 5 + the escape)"""
    q, c, s = quotient_table(r, order, rice_max)
    ks = np.arange(rice_max)[:, None]
    best = 6 + 4 + 5 + 31 * (N - order)                       # the fallback partition
    for level in range(7):
        g = NLEAF >> level
        qp = q.reshape(rice_max, -1, g).sum(axis=2)
        cp = c.reshape(-1, g).sum(axis=1)
        sp = s.reshape(-1, g).sum(axis=1)
        rice = (cp[None, :] * (ks + 1) + qp).min(axis=0)
        esc = np.array([5 + (cc * (int(ss).bit_length() + 1) if ss else 0) for cc, ss in zip(cp.tolist(), sp.tolist())])
        best = min(best, 6 + int((4 + np.minimum(rice, esc)).sum()))
    return best


def blocks(rng):
    for scale in (0.3, 0.7, 1.0, 1.6, 3, 11, 100, 5000, 2 ** 12 - 1, 2 ** 12, 2 ** 20, 2 ** 27):
        yield "geometric", np.rint(rng.laplace(0, scale, N))
        yield "uniform", np.rint(rng.uniform(-scale * 2, scale * 2, N))
        yield "random", np.rint(rng.normal(0, scale, N))
        yield "sparse", np.rint(rng.laplace(0, scale, N)) * (rng.random(N) < 0.06)
        x = np.rint(rng.laplace(0, 1.5, N))
        x[rng.integers(0, N, 5)] = int(scale * 64) + 1          # single outliers: one value carries a leaf's sum
        yield "outlier", x
        env = np.repeat(rng.random(NLEAF) ** 6, LEAF) * scale * 40   # loud and quiet leaves side by side
        yield "envelope", np.rint(rng.laplace(0, 1, N) * env)
        yield "constant", np.full(N, int(scale) + 1) * rng.choice([-1, 1], N)
    yield "zero", np.zeros(N)
    z = np.zeros(N)
    z[700] = 1
    yield "one", z
    for top in (2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1):          # at the 31-bit escape boundary
        yield "escape", np.full(N, top) * rng.choice([-1, 1], N)
        yield "escape", rng.integers(top // 2, top + 1, N) * rng.choice([-1, 1], N)
        x = np.rint(rng.laplace(0, 3, N))
        x[64:128] = top                                                   # one such leaf in a quiet block
        yield "escape", x


@pytest.mark.parametrize("rice_max", [15, 31])
def test_tight_bounds_never_exceed_the_cheapest_coding(rice_max):
    rng = np.random.default_rng(20261019)
    checked = equal = at_rule = exact_terms = 0
    for name, r in blocks(rng):
        r = np.clip(np.asarray(r, dtype=np.int64), -(2 ** 31) + 1, 2 ** 31 - 1)
        for order in (0, 2, 4):
            r2 = r.copy()
            r2[:order] = 0
            least = cheapest_block(r2, order, rice_max)
            one = lbt.tight_leaf_bound(r2, order, rice_max)
            two = lbt.tight_leaf_bound(r2, order, rice_max, below=1)
            kern = lbt.kernel_tight_bound(r2, order, rice_max)
            assert one <= two <= least, (name, order, one, two, least)
            assert kern <= least, (name, order, kern, least)
            assert kern >= min(lbt.present_leaf_bound(r2, order), 10 + 31 * (N - order))
            # any other choice of the exact parameter gives a bound too
            shifted = lbt.tight_leaf_bound(r2, order, rice_max, k0_of=lambda c, s: min(lbt.leaf_k0(c, s, rice_max) + 2, rice_max - 1))
            assert shifted <= least, (name, order, shifted, least)
            # leaf by leaf: where the rule's parameter IS the leaf's cheapest coding, the bound is that cost exactly
            q, c, s = quotient_table(r2, order, rice_max)
            t = lbt.zigzag(r2).reshape(NLEAF, LEAF) >> 1
            t[0, :order] = 0
            for i in range(NLEAF):
                cc, ss = int(c[i]), int(s[i])
                if ss == 0:
                    continue
                k = lbt.rule_k(cc, ss) if ss > cc else 0
                cost = cc * (np.arange(rice_max) + 1) + q[:, i]
                low = min(int(cost.min()), cc * (ss.bit_length() + 1), 31 * cc)
                y = t[i] >> max(k - 2, 0)
                kl = lbt.kernel_leaf(cc, ss, k, int(y.sum()), int((y & 1).sum()), rice_max)
                assert kl <= low, (name, order, i, kl, low)
                if k < rice_max:
                    ol = lbt.tight_leaf(cc, ss, {k: int(q[k, i])}, rice_max)
                    assert ol <= kl, (name, order, i, ol, kl)
                    # the two quotient sums the kernel derives from its pass ARE the exact ones: its terms at the rule's
                    # parameter and at the one below are the brute-force costs there
                    q0, qm = lbt.kernel_quotients(ss, k, int(y.sum()), int((y & 1).sum()))
                    assert cc * (k + 1) + q0 == int(cost[k])
                    if k >= 1:
                        assert cc * k + qm == int(cost[k - 1])
                    exact_terms += 1
                    # ... so where the rule's parameter is the leaf's cheapest coding the bound can only fall short of it
                    # through the one term it bounds from below on the likely side, the parameter above (any further one
                    # costs more than that, any lower one more than the exact k - 1)
                    if int(cost[k]) == low:
                        up = cc * (k + 2) + lbt.above_k0(q0, cc, 1) if k + 1 < rice_max else low
                        assert kl == min(low, up), (name, order, i, k, kl, low, up)
                        equal += kl == low
                        at_rule += 1
            checked += 1
    assert checked > 250 and exact_terms > 10000 and at_rule > 5000
    assert equal > 5000, (equal, at_rule)


@pytest.mark.parametrize("q0", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("k0", [0, 3, 12, 29])
def test_bound_above_the_exact_parameter_clamp_and_ceil(q0, k0):
    """sum (q >> d) over 64 quotients with sum Q0 is at least ceil((Q0 - 64 (2^d - 1)) / 2^d) and never negative: the figures
    at the clamp and at the first step of the ceiling, and that some 64 quotients reach them"""
    c = 64
    for d in (1, 2, 31 - k0):
        got = lbt.above_k0(q0, c, d)
        want = {(65, 1): 1}.get((q0, d), 0)     # 65 = 63 ones and a two: (2 >> 1) = 1; everything else fits below 2^d each
        assert got == want, (q0, d, got)
        # reached: fill every quotient up to 2^d - 1 first, the rest on one of them
        q = np.zeros(c, dtype=np.int64)
        left = q0
        for i in range(c):
            q[i] = min(left, (1 << d) - 1)
            left -= int(q[i])
        q[0] += left
        assert int(q.sum()) == q0 and int((q >> d).sum()) == got
        # never undercut
        rng = np.random.default_rng(q0 * 100 + d)
        for _ in range(50):
            cut = np.sort(rng.integers(0, q0 + 1, c - 1))
            parts = np.diff(np.concatenate([[0], cut, [q0]]))
            assert int((parts >> d).sum()) >= got
    # the kernel's form of the first step up
    assert ((q0 - c + 1) >> 1 if q0 > c else 0) == lbt.above_k0(q0, c, 1)


def test_bounds_on_the_bench_signals_record():
    """profiles/leaf_bound_tight.json (tools/leaf_bound_tight.py) holds the shares the device test relies on"""
    import json
    import os

    rec = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                      "leaf_bound_tight.json")))
    shares = {m["signal"]: m for m in rec["cpu_shares"]}
    assert shares["ar2"]["present_bound_share"] == 0.0          # what the device counted before: none defers
    assert shares["ar2"]["tight_bound_share"] > 0.9 and shares["hi"]["tight_bound_share"] > 0.9
