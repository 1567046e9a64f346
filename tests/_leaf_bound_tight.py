"""The lower bounds of a FIXED subframe's size behind `Params::defer_fixed` (kernels/wave_cand_fixed.inc), restated in numpy
for blocks of 4096 samples: the PRESENT bound, made of the 64 leaf sums alone, and the TIGHT one, which also knows one exact
quotient sum per leaf.  Shared by tools/leaf_bound_tight.py (the shares on the bench's signals) and
tests/test_leaf_bound_tight_math.py (the bound against brute force).

Notation: r = a residual, u = zigzag(r) = 2 r (r >= 0) / -2 r - 1 (r < 0), t = u >> 1 = r ^ (r >> 31) (the FOLDED residual),
|r| = t + [r < 0].  A Rice code with parameter k costs (k + 1) + (u >> k) bits, and u >> k = t >> (k - 1) for k >= 1.
A leaf is 64 consecutive samples (leaf 0: minus the warm-up), c its residual count, S its sum of |r|.

Tight bound of a leaf:
  k0 = the rule's parameter of (c, S) (encode.rs:3777-3780: 0 where S <= c, else the smallest k with c 2^k >= S), clamped
       below rice_max;
  Q0 = sum (u >> k0), exact (on the device: sum (t >> (k0 - 1)), and S + sum t where k0 = 0);
  at k0      the leaf costs exactly c (k0 + 1) + Q0;
  at k > k0  (d = k - k0) sum (u >> k) = sum ((u >> k0) >> d) >= ceil((Q0 - c (2^d - 1)) / 2^d), not below 0;
  at k < k0  (d = k0 - k) sum (u >> k) >= 2^d Q0;
  escaped    (Partition::new, :3787-3800: escape_bits = ilog2(sum of the PARTITION) + 2 >= ilog2(S) + 2) at least
             c (ilog2(S) + 2); an all-zero leaf costs nothing inside an escaped or constant partition;
  fallback   the single 31-bit escaped partition of :3887-3895 costs 31 c.
The leaf's bound is the minimum of all of these over the legal k (0 .. rice_max - 1).  A partition of several leaves has ONE
parameter, so it costs at least the sum of its leaves' minima; every residual block carries the method, the partition order
and at least one partition header: 2 + 4 + 4 = 10 bits."""
import numpy as np

N, LEAF = 4096, 64
NLEAF = N // LEAF


def fixed_order(x):
    """encode.rs:3064-3075: the order 0..4 whose differences have the smallest abs sum over [4, n), first minimum"""
    x = np.asarray(x, dtype=np.int64)
    best, best_sum = 0, None
    for k in range(5):
        s = int(np.abs(np.diff(x, n=k)[4 - k:]).sum())
        if best_sum is None or s < best_sum:
            best, best_sum = k, s
    return best


def fixed_residual(x, order):
    """the residual block of FIXED `order` as an array of N entries, warm-up entries 0"""
    x = np.asarray(x, dtype=np.int64)
    r = np.zeros(len(x), dtype=np.int64)
    r[order:] = np.diff(x, n=order)
    return r


def zigzag(r):
    r = np.asarray(r, dtype=np.int64)
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def rule_k(c, s):
    k = 0
    while (c << k) < s:
        k += 1
    return k


def leaf_tables(r, order):
    """per leaf: count c, S = sum |r|, and the zigzag values as a [NLEAF][LEAF] array with warm-up entries masked"""
    a = np.abs(np.asarray(r, dtype=np.int64)).reshape(NLEAF, LEAF)
    u = zigzag(r).reshape(NLEAF, LEAF)
    live = np.ones((NLEAF, LEAF), dtype=bool)
    live[0, :order] = False
    c = live.sum(axis=1)
    s = np.where(live, a, 0).sum(axis=1)
    return c, s, np.where(live, u, 0), live


def present_leaf_bound(r, order):
    """10 + sum over the leaves of k c + (2 S >> k) - 6 with the rule's k (2 S where S <= c): the bound of r05"""
    c, s, _, _ = leaf_tables(r, order)
    lb = 10
    for cc, ss in zip(c.tolist(), s.tolist()):
        if ss <= cc:
            lb += 2 * ss
        else:
            k = rule_k(cc, ss)
            lb += k * cc + ((2 * ss) >> k) - 6
    return lb


def above_k0(q0, c, d):
    """lower bound of sum (q >> d) over c values q >= 0 with sum q = q0: ceil((q0 - c (2^d - 1)) / 2^d), not below 0"""
    num = q0 - c * ((1 << d) - 1)
    return 0 if num <= 0 else -((-num) >> d)


def tight_leaf(c, s, exact, rice_max):
    """the bound of ONE leaf from its count, its sum of |r| and the exact quotient sums it knows: exact = {k: sum (u >> k)} for
    one parameter or for several consecutive ones; parameters above the largest are bounded from it, those below the smallest
    from that one"""
    if c == 0 or s == 0:
        return 0
    lo, hi = min(exact), max(exact)
    best = 31 * c                                        # the 31-bit fallback partition
    best = min(best, c * (int(s).bit_length() - 1 + 2))  # escaped
    for k in range(rice_max):
        if k in exact:
            q = exact[k]
        elif k > hi:
            q = above_k0(exact[hi], c, k - hi)
        else:
            q = exact[lo] << (lo - k)
        best = min(best, c * (k + 1) + q)
    return best


def leaf_k0(c, s, rice_max):
    return min(rule_k(c, s) if s > c else 0, rice_max - 1)


def tight_leaf_bound(r, order, rice_max=31, k0_of=None, below=0):
    """10 + the sum of the 64 leaves' tight bounds.  k0_of(c, S): another choice of the parameter (the bound holds for any);
    below: how many parameters under k0 are exact as well"""
    c, s, u, _ = leaf_tables(r, order)
    lb = 10
    for i in range(NLEAF):
        cc, ss = int(c[i]), int(s[i])
        k0 = leaf_k0(cc, ss, rice_max) if k0_of is None else k0_of(cc, ss)
        exact = {k: int((u[i] >> k).sum()) for k in range(max(k0 - below, 0), k0 + 1)}
        lb += tight_leaf(cc, ss, exact, rice_max)
    return lb


def kernel_quotients(s, k, ysum, odd):
    """(sum (u >> k), sum (u >> (k - 1))) from the pass's two figures; the second is meaningless at k = 0"""
    q0 = (ysum - odd) >> 1 if k >= 2 else ysum if k == 1 else s + ysum
    qm = ysum if k >= 2 else s + ysum
    return q0, qm


def kernel_leaf(c, s, k, ysum, odd, rice_max):
    """the leaf's bound as kernels/wave_cand_fixed.inc computes it, in closed form: k = the rule's parameter (not clamped);
    ysum = sum (t >> max(k - 2, 0)) and odd = the odd terms of that sum, the two figures of wave_leaf_quotients"""
    if s == 0:
        return 0
    if k >= rice_max:
        return min(k * c + ((2 * s) >> k) - 6, 31 * c)    # the leaf sums' bound (an escape is possible)
    q0, qm = kernel_quotients(s, k, ysum, odd)
    lt = c * (k + 1) + q0
    if k + 1 < rice_max:
        lt = min(lt, c * (k + 2) + ((q0 - c + 1) >> 1 if q0 > c else 0))
    if k >= 1:
        bq, bc = max(qm, 1).bit_length(), c.bit_length()
        d = max(bc - bq, 0)
        if (qm << d) < c:
            d += 1
        d = k - 1 if qm == 0 else min(d, k - 1)
        lt = min(lt, c * (k - d) + (qm << d))
    return min(lt, 31 * c)


def kernel_tight_bound(r, order, rice_max=31):
    """10 + the sum of kernel_leaf over the block, or the leaf sums' bound where that is larger (the kernel holds both; the
    leaf sums' bound is capped here at the 31-bit fallback partition's cost, which it passes only with mean residuals beyond
    2^28 under Rice parameters below 15 -- nothing the kernel's 16-bit candidates can hold)"""
    c, s, u, _ = leaf_tables(r, order)
    t = u >> 1
    lb = 10
    for i in range(NLEAF):
        cc, ss = int(c[i]), int(s[i])
        k = rule_k(cc, ss) if ss > cc else 0
        y = t[i] >> max(k - 2, 0)
        lb += kernel_leaf(cc, ss, k, int(y.sum()), int((y & 1).sum()), rice_max)
    return max(lb, min(present_leaf_bound(r, order), 10 + 31 * (N - order)))


def wasted_bits(x):
    o = int(np.bitwise_or.reduce(np.asarray(x, dtype=np.int64)))
    if o == 0:
        return 0
    return (o & -o).bit_length() - 1


def fixed_bounds(x, bps, rice_max=31, below=0):
    """(order, present bound, tight bound) of the whole FIXED subframe of candidate x: the subframe header (8 + wasted bits'
    unary count) and the warm-up samples counted exactly, as the kernel counts them"""
    w = wasted_bits(x)
    xs = np.asarray(x, dtype=np.int64) >> w
    order = fixed_order(xs)
    r = fixed_residual(xs, order)
    head = 8 + w + order * (bps - w)
    if below == "kernel":
        return order, head + present_leaf_bound(r, order), head + kernel_tight_bound(r, order, rice_max)
    return order, head + present_leaf_bound(r, order), head + tight_leaf_bound(r, order, rice_max, below=below)


# ---- exact subframe sizes of BOTH halves (the oracle records the winner's only): what the near-tie cases of
# tests/test_gpu_leaf_bound_tight.py are built with, each figure held to the oracle's wherever the oracle shows it
def rice_block_bits(res, order, use_rice2=True, max_po=6):
    """write_residuals (encode.rs:3862-3962) for a block of N residuals (warm-up entries 0): the partition order with the
    first smallest ESTIMATE, every partition with the rule's parameter, then the exact bits"""
    rice_max = 31 if use_rice2 else 15
    a = np.abs(np.asarray(res, dtype=np.int64))
    u = zigzag(res)
    best = None
    for level in range(max_po + 1):
        plen = len(a) >> level
        est, parts, bad = 0, [], False
        for p in range(1 << level):
            lo, hi = max(p * plen, order), (p + 1) * plen
            c, s = hi - lo, int(a[lo:hi].sum())
            if s == 0:
                parts.append(("constant", 0, lo, hi))
                continue
            k = rule_k(c, s) if s > c else 0
            if k >= rice_max:
                e = s.bit_length() + 1
                bad = bad or e > 31
                est += e * c
                parts.append(("escaped", e, lo, hi))
            else:
                est += 4 + (1 + k) * c + ((s >> (k - 1)) if k else (s << 1)) - c // 2
                parts.append(("rice", k, lo, hi))
        if not bad and (best is None or est < best[0]):
            best = (est, parts)
    if best is None:
        return 6 + 4 + 5 + 31 * (len(a) - order)
    parts = best[1]
    hb = 5 if use_rice2 and any(kind == "rice" and k >= 15 for kind, k, _, _ in parts) else 4
    bits = 6
    for kind, k, lo, hi in parts:
        if kind == "rice":
            bits += hb + (1 + k) * (hi - lo) + int((u[lo:hi] >> k).sum())
        elif kind == "escaped":
            bits += hb + 5 + k * (hi - lo)
        else:
            bits += hb + 5
    return bits


def fixed_subframe_bits(x, bps, use_rice2=True):
    w = wasted_bits(x)
    xs = np.asarray(x, dtype=np.int64) >> w
    order = fixed_order(xs)
    return 8 + w + order * (bps - w) + rice_block_bits(fixed_residual(xs, order), order, use_rice2)


def lpc_subframe_bits(orc, opts, x, bps, use_rice2=True):
    """the LPC subframe of candidate x as encode_lpc_subframe (encode.rs:3090-3172) sizes it, through the oracle's stage
    functions; None where it fails (no order, zero coefficients, residual overflow)"""
    n = len(x)
    w = wasted_bits(x)
    xs = (np.asarray(x, dtype=np.int64) >> w).astype(np.int32)
    window = orc.window(opts.window_kind, opts.window_param, n)
    ac = orc.autocorrelate(xs.astype(np.float64) * window, opts.max_lpc_order)
    coeffs, errs = orc.lp_coefficients(ac)
    precision = orc.lib().orc_lpc_precision(n)
    order = orc.compute_best_order(bps - w, precision, n, errs)
    if order <= 0:
        return None
    rc, q, shift = orc.quantize(coeffs[order - 1], precision)
    if rc != 0:
        return None
    rc, res = orc.encode_residuals(q, shift, xs)
    if rc != 0:
        return None
    r = np.zeros(n, dtype=np.int64)
    r[order:] = res
    return 8 + w + order * (bps - w) + 4 + 5 + order * precision + rice_block_bits(r, order, use_rice2)
