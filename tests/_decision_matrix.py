"""The matrix of hand-built frames behind test_decision_matrix_oracle.py (CPU) and test_gpu_decisions.py (GPU): inputs
that sit ON the encoder's decision boundaries -- an exact tie, or one sample's magnitude either side of a threshold --
where the synthetic music and the seeded sweeps of the other tests land only by luck.  Byte identity with the reference
is a chain of integer decisions (first minimum of the five fixed-order sums, first minimum of the partition-order
estimates, "smallest k with cnt << k >= sum", sum > cnt, sum == 0, k >= rice_max, ilog2(sum) + 2 > 31, rice >= 15,
bits >= n * bps, FIXED before LPC and the earlier channel assignment on equal bits, checked_sub ending the ladder);
every case here declares which of them it sits on and what the reference does there (`expect`, `tie`), and the CPU
test proves that from the oracle alone before the GPU test may rely on it.

A case is one frame of planar int32 [channels][n] with its width, the partition-order limit it was built for, a name and
the declared property.  mono_cases(n, max_po) / stereo_cases(n, max_po) build the cases of one block length: a case is
scaled by building it anew for that length (tiled per partition), never by padding with silence.  Both are cached and
their arrays are read-only.

Building blocks: alt(mags) is an alternating-sign signal -- its differences are larger than itself, so FIXED order 0 is
the first minimum and a partition's sum is simply the sum of the magnitudes, which spread() sets exactly (mixing odd
values: no wasted bits by accident).

Families, and what they hold per block length (counts: summary()):
  rice      frame-wide sum = (n << k) - 1 / n << k / (n << k) + 1 at 8, 16, 24 and 32 bits for every k from 0 up to the last
            at which the oracle still takes FIXED for all three (8: 0..5, 16: 0..13, 24: 0..21, 32: 0..29),
            and n - 1 / n / n + 1 (the sum > cnt test); a silent partition inside a loud frame; k = 14 against the
            escape (escape_bits = ilog2(sum) + 2) in one loud partition of a silent 16-bit frame; FIXED orders 1..4 with
            cnt = n - order residuals as the only partition, and with plen - order residuals in partition 0 next to
            full-length partitions, at every order whose polynomial fits 32 bits at that block length.
  method    above 16 bits: the largest Rice parameter 14 / 15 one sample apart, frame-wide and in one partition only.
  dropped   32 bits: a loud partition needing k = 30, then k = 31 (its level is dropped, the next coarser one wins); a
            frame of mean exactly 2^30 (k = 30 at every level), then one more (every level dropped; VERBATIM wins both).  The 31-bit
            fallback partition cannot hold what reaches it at 32 bits: Partition::new fails at level 0 only when the
            mean |residual| exceeds 2^30, and then some residual exceeds 2^30 - 1 -- so "the fallback's largest residual
            is 2^30 - 1" does not exist; the frame ends VERBATIM, which is what the second case pins.  At 16 bits the
            fallback is reached by sum >= 2^30 alone: big_block_cases() holds 65535-sample frames with sum 2^30 - 1
            (escape of 31 bits by the ordinary route) and 2^30 (by the fallback): the same partition either way, and
            VERBATIM wins both.
  po_tie    two partition orders with equal estimates (the lower one wins): +-4 / +-9 at 64 samples, and pairs found by
            tie_pairs() -- a bounded deterministic search over the two halves' sums -- at levels 0/1, at a
            middle pair and at the two finest levels (partition lengths 18, 36 and 64 at blocks 1152, 2304 and 4096).
            A three-level tie is searched for within the same bound (three_level_tie()); where none exists at a block
            length, none is emitted, and summary() says so.
  fixed_tie the period-6 pattern (five-way tie, order 0; only where n - 4 is a multiple of 3, or the phases break it),
            constant non-zero (orders 1..4 tie at 0: order 1, and not CONSTANT), ramp (2..4 tie), quadratic (3 and 4
            tie), and each with one of the first samples perturbed so that the tie of the orders it does not reach
            exists only over the common tail.
  ladder    32 bits: a first difference of exactly 2^31 - 1, then 2^31, at the first, a middle and the last position;
            a spike on a cubic whose height puts the overflow into the second, third or fourth difference only.
  verbatim  bits = n * bps - 1 / n * bps / n * bps + 1 one sample's magnitude apart at 8, 16 and 24 bits, and the same
            with two wasted bits.
  wasted    wasted = bps - 1 (only 0 and -2^(bps-1)); one non-zero sample (first, middle, last; odd and even).
Stereo (stereo_cases): L == R, R == 0, R == -L, R == -L - 1, a pair whose two best assignments cost the same bits with no
channel silent (found by a seeded search with the oracle, each candidate encoded mono at its own width), and wasted-bit
counts per candidate.  side = L - R has min(wasted L, wasted R) wasted bits whenever those differ, so "four different
counts" does not exist: one case has L = R = 2 with mid 4 and side 3, the other L 1, R 3, mid 0, side 1.

COUNTS below holds the cases per family at each (block, max partition order); the CPU test holds summary() against it.
On the GPU (test_gpu_decisions.py, SHAPES) every mono case runs at 64 and 192 (mono, stereo), 1152 with the fast preset
and with max_lpc 0 (mono, stereo), 2304 (mono), 4096 (mono and stereo with max_lpc 0 and 12; as channel 5 of 8; all of
these again under three deferral modes and through the generic kernels) and 16384 (mono); the assignment cases at 64,
1152 and 4096 with max_lpc 0 and 12.

Ties between a FIXED and an LPC bit count are not in the matrix, and no search was run, because the oracle cannot show
one: FIXED wins on equal bits, so a frame whose LPC candidate costs exactly the FIXED bits and one whose LPC candidate
costs more give the same plan and the same bytes -- encoding a candidate with max_lpc 0 and again with max_lpc 12 and
comparing type and bits tells "LPC cheaper" from "LPC not cheaper" and nothing finer, since the loser's bit count is
never recorded.  Telling them apart needs the oracle to report both counts, which this change does not add."""
import functools

import numpy as np

import _oracle as orc

TIE_BOUND = 64        # tie_pairs(): mean magnitudes 1..TIE_BOUND per half
PAIR_SEEDS = 4000     # assignment_tie_pair(): seeds tried at most

# (block, max partition order) the mono cases are built for
MONO_SHAPES = [(64, 3), (192, 3), (1152, 3), (1152, 6), (2304, 6), (4096, 6), (16384, 6)]
STEREO_SHAPES = [(64, 3), (1152, 3), (4096, 6)]

# {family: {(block, max partition order): cases}}: what summary() must give
COUNTS = {'assignment': {(64, 3): 7, (1152, 3): 7, (4096, 6): 7},
 'dropped': {(64, 3): 4,
             (192, 3): 4,
             (1152, 3): 4,
             (1152, 6): 4,
             (2304, 6): 4,
             (4096, 6): 4,
             (16384, 6): 4,
             (65535, 6): 2},
 'fixed_tie': {(64, 3): 10, (192, 3): 6, (1152, 3): 6, (1152, 6): 6, (2304, 6): 6, (4096, 6): 10, (16384, 6): 10},
 'ladder': {(64, 3): 12, (192, 3): 12, (1152, 3): 12, (1152, 6): 12, (2304, 6): 12, (4096, 6): 12, (16384, 6): 12},
 'method': {(64, 3): 6, (192, 3): 6, (1152, 3): 6, (1152, 6): 6, (2304, 6): 6, (4096, 6): 6, (16384, 6): 6},
 'po_tie': {(64, 3): 5, (192, 3): 4, (1152, 3): 3, (1152, 6): 3, (2304, 6): 3, (4096, 6): 3, (16384, 6): 3},
 'rice': {(64, 3): 292,
          (192, 3): 292,
          (1152, 3): 274,
          (1152, 6): 274,
          (2304, 6): 274,
          (4096, 6): 271,
          (16384, 6): 256},
 'verbatim': {(64, 3): 15, (192, 3): 15, (1152, 3): 15, (1152, 6): 15, (2304, 6): 15, (4096, 6): 15, (16384, 6): 15},
 'wasted': {(64, 3): 10, (192, 3): 10, (1152, 3): 10, (1152, 6): 10, (2304, 6): 10, (4096, 6): 10, (16384, 6): 10}}


class Case:
    def __init__(self, family, name, bps, planar, max_po, expect=None, tie=None, near=None):
        self.family, self.name, self.bps, self.max_po = family, name, bps, max_po
        self.near = near              # the threshold this case is below / at / above: its neighbours differ in one sample by 1
        self.planar = np.ascontiguousarray(planar, dtype=np.int32)
        assert self.planar.ndim == 2
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        assert lo <= int(self.planar.min()) and int(self.planar.max()) <= hi, name
        self.planar.setflags(write=False)
        self.expect = expect or {}    # fields of channel 0's SubframePlan (or "assignment") the reference must show
        self.tie = tie                # {"kind": "fixed" | "porder", "among": [...], "taken": x}

    def __repr__(self):
        return f"{self.family}/{self.name}@{self.planar.shape[1]}x{self.bps}"


# ---------------------------------------------------------------- integer building blocks
def spread(cnt, total):
    """cnt magnitudes >= 0 that sum to exactly `total`, as equal as integers allow, with an odd value among them."""
    base, rem = divmod(total, cnt)
    m = [base + 1] * rem + [base] * (cnt - rem)
    if rem == 0 and base % 2 == 0 and base > 0 and cnt >= 2:
        m[0], m[1] = base + 1, base - 1
    return m


def around(cnt, total, d):
    """spread(cnt, total) with its last magnitude moved by d: the cases of a threshold differ in that one sample, by 1."""
    m = spread(cnt, total)
    m[-1] += d
    return m


def alt(mags, first=1):
    return [(first if i % 2 == 0 else -first) * m for i, m in enumerate(mags)]


def partition_new(s, cnt, rice_max):
    """Partition::new on cnt residuals with sum |r| = s: (estimate, rice, escape_bits) or None; "smallest k with
    cnt 2^k >= sum" for ceil(log2(sum / cnt)).  The one restatement: the searches here use it, and
    test_decision_matrix_oracle.py checks it against the oracle's plan on every case."""
    if s == 0:
        return 0, 255, 0
    k = 0
    while s > cnt and (cnt << k) < s:
        k += 1
    if k >= rice_max:
        e = (s.bit_length() - 1) + 2
        return None if e > 31 else (e * cnt, 255, e)
    t = (s >> (k - 1)) if k else (s << 1)
    return 4 + (1 + k) * cnt + t - cnt // 2, k, 0


def fixed_sums(x):
    """encode_fixed_subframe: the difference ladder (checked_sub ends it) and each order's sum |r| over the common tail."""
    seqs = [np.asarray(x, dtype=np.int64)]
    while len(seqs) < 5 and seqs[-1].size > 1:
        d = seqs[-1][1:] - seqs[-1][:-1]
        if d.min() < -(1 << 31) or d.max() > (1 << 31) - 1:
            break
        seqs.append(d)
    tail = seqs[-1].size
    return seqs, [int(np.abs(q[q.size - tail:]).sum()) for q in seqs]


def _est(s, cnt, rice_max=15):
    return partition_new(s, cnt, rice_max)[0]


def ladder(x):
    """The number of fixed orders the reference has for x."""
    return len(fixed_sums(x)[0])


def narrowest(x, widths=(16, 24, 32)):
    top = max(abs(int(min(x))), abs(int(max(x))) + 1)
    for b in widths:
        if top <= 1 << (b - 1):
            return b
    raise ValueError("does not fit 32 bits")


# ---------------------------------------------------------------- searches
@functools.lru_cache(maxsize=None)
def tie_pairs(h, rice_max=15):
    """(sa, sb): two halves of h residuals with sums sa and sb cost the same as one partition or as two.  sa = h a and
    sb = h b + r for a, b in 1..TIE_BOUND and 32 evenly spaced r below h, in that order of search."""
    out = []
    step = max(1, h // 32)
    for a in range(1, TIE_BOUND + 1):
        sa = h * a
        ea = _est(sa, h, rice_max)
        for b in range(1, TIE_BOUND + 1):
            for sb in range(h * b, h * b + h, step):
                if sb != sa and _est(sa + sb, 2 * h, rice_max) == ea + _est(sb, h, rice_max):
                    out.append((sa, sb))
    return out


@functools.lru_cache(maxsize=None)
def three_level_tie(h, rice_max=15):
    """(sa, sb, sc, sd): four quarters of h residuals whose one-, two- and four-partition estimates are all equal; the
    first in the order of tie_pairs(h) x tie_pairs(h), or None when the bound holds none."""
    pairs = tie_pairs(h, rice_max)
    for a, b in pairs:
        eab = _est(a + b, 2 * h, rice_max)
        for c, d in pairs:
            if _est(a + b + c + d, 4 * h, rice_max) == eab + _est(c + d, 2 * h, rice_max):
                return a, b, c, d
    return None


def _mono_bits(x, bps, n, max_po):
    o = orc.options("default", block_size=n, max_partition_order=max_po, max_lpc_order=0, mid_side=0, exhaustive=0)
    rc, _, plan = orc.encode_frame(o, 44100, bps, np.asarray(x, dtype=np.int32).reshape(1, -1))
    assert rc == 0
    return plan.sub[0].bits, plan.sub[0].type


@functools.lru_cache(maxsize=None)
def assignment_tie_pair(n, max_po, bps=16):
    """(L, R, seed): the first seeded pair of quiet noises whose cheapest total -- over independent, left/side,
    side/right and mid/side, each candidate encoded mono at its own width -- is reached by two assignments, with no
    candidate CONSTANT.  At most PAIR_SEEDS seeds."""
    for seed in range(PAIR_SEEDS):
        rng = np.random.Generator(np.random.PCG64(9000 + seed))
        amp = 3 + seed % 5
        left = rng.integers(-amp, amp + 1, size=n, dtype=np.int64)
        right = left + rng.integers(-2, 3, size=n, dtype=np.int64)
        mid, side = (left + right) >> 1, left - right
        got = [_mono_bits(c, w, n, max_po) for c, w in ((left, bps), (right, bps), (mid, bps), (side, bps + 1))]
        if any(t == orc.SUB_CONSTANT for _, t in got):
            continue
        (lb, _), (rb, _), (mb, _), (sb, _) = got
        tot = [lb + rb, lb + sb, sb + rb, mb + sb]
        if sorted(tot)[0] == sorted(tot)[1]:
            return left.astype(np.int32), right.astype(np.int32), seed
    raise AssertionError(f"no assignment tie within {PAIR_SEEDS} seeds at block {n}")


# ---------------------------------------------------------------- the mono families
def _rice(n, P, out):
    for bps in (8, 16, 24, 32):
        # every k the width allows: upward from 0 while the oracle still takes FIXED for the whole triple (beyond, VERBATIM
        # is cheaper); magnitudes of 2^k + 1 fit up to k = bps - 2, and at 32 bits k = 30 belongs to `dropped`
        for k in range(min(bps - 1, 30)):
            triple = [alt(around(n, n << k, d)) for d in (-1, 0, 1)]
            if any(_mono_bits(x, bps, n, P)[1] != orc.SUB_FIXED for x in triple):
                break
            for d, x in zip((-1, 0, 1), triple):
                rice = k + (d > 0)
                exp = dict(type=orc.SUB_FIXED, order=0, partition_order=0, rice=[rice],
                           coding_method=int(bps > 16 and rice >= 15))
                out.append(Case("rice", f"wide-k{k}{d:+d}", bps, [x], P, exp, near=f"wide-k{k}"))
    parts = 1 << P
    plen = n >> P
    if P >= 2:   # three loud quarters of mean exactly 2^6 and a silent one
        q = n // 4
        x = alt(spread(q, q << 6)) + alt(spread(q, q << 6)) + [0] * q + alt(spread(q, q << 6))
        out.append(Case("rice", "silent-partition", 16, [x], P,
                        dict(type=orc.SUB_FIXED, order=0, partition_order=2, rice=[6, 6, 255, 6], escape_bits=[0] * 4)))
    if P >= 1:
        for d in (-1, 0, 1):   # one loud partition (not the first) of a silent 16-bit frame: k = 14 or the escape
            s = (plen << 14) + d
            x = [0] * plen + alt(around(plen, plen << 14, d)) + [0] * (n - 2 * plen)
            rice = [255] * parts
            esc = [0] * parts
            rice[1], esc[1] = (14, 0) if d <= 0 else (255, s.bit_length() + 1)
            out.append(Case("rice", f"loud-partition-k14{d:+d}", 16, [x], P,
                            dict(type=orc.SUB_FIXED, order=0, partition_order=P, rice=rice, escape_bits=esc), near="loud-k14"))
    # orders 1..4, wherever the polynomial fits 32 bits: the only partition (max_po 0) has n - order residuals; and with
    # the shape's max_po, partition 0 has plen - order residuals on the threshold next to full-length partitions that are
    # loud and quiet in turn (the finest level wins)
    for order in (1, 2, 3, 4):
        for po in sorted({0, P}):
            for k in (1, 2, 3):
                for d in (-1, 0, 1):
                    cnt = (n >> po) - order
                    mags = around(cnt, cnt << k, d)
                    for i in range(1, 1 << po):
                        mags += spread(n >> po, (n >> po) << (k + 4 if i % 2 else k))
                    x = np.array([0] * order + alt(mags), dtype=np.int64)
                    x[order - 1] = 1 << (k + 6 if po else 6)   # where the (order-1)-th difference starts: every lower order pays
                    for _ in range(order):
                        x = np.cumsum(x)
                    try:
                        bps = narrowest(x)
                    except ValueError:
                        continue
                    exp = dict(type=orc.SUB_FIXED, order=order, partition_order=po, rice_first=k + (d > 0))
                    out.append(Case("rice", f"order{order}-po{po}-k{k}{d:+d}", bps, [x], po, exp, near=f"order{order}-po{po}-k{k}"))


def _method(n, P, out):
    parts, plen = 1 << P, n >> P
    for bps in (20, 24):
        for d in (0, 1):
            exp = dict(type=orc.SUB_FIXED, order=0, partition_order=0, rice=[14 + d], coding_method=d)
            out.append(Case("method", f"wide-{14 + d}", bps, [alt(around(n, n << 14, d))], P, exp, near="wide-14"))
    if P >= 1:
        for d in (0, 1):   # a quiet frame (mean 2^3, k = 3) with one partition at k = 14 / 15
            x = alt(spread(plen, plen << 3)) + alt(around(plen, plen << 14, d)) + alt(spread(n - 2 * plen, (n - 2 * plen) << 3))
            rice = [3] * parts
            rice[1] = 14 + d
            out.append(Case("method", f"one-partition-{14 + d}", 24, [x], P,
                            dict(type=orc.SUB_FIXED, order=0, partition_order=P, rice=rice, coding_method=d), near="one-partition-14"))


def _dropped(n, P, out):
    parts, plen = 1 << P, n >> P
    if P >= 1:
        for d in (0, 1):   # +-2^30: the first difference overflows, order 0 is all there is
            x = [0] * plen + alt(around(plen, plen << 30, d)) + [0] * (n - 2 * plen)
            if d == 0:
                rice = [255] * parts
                rice[1] = 30
                exp = dict(type=orc.SUB_FIXED, order=0, partition_order=P, rice=rice, coding_method=1)
            else:      # level P is dropped; P - 1 holds the loud partition with as much silence: k = 30 there
                rice = [255] * (parts // 2)
                rice[0] = 30
                exp = dict(type=orc.SUB_FIXED, order=0, partition_order=P - 1, rice=rice, coding_method=1)
            out.append(Case("dropped", f"finest-level-k{30 + d}", 32, [x], P, exp, near="finest-level-k30"))
    # (k = 30 costs 32.5 bits a sample: VERBATIM wins either way; what differs is whether FIXED had a partitioning at all)
    out.append(Case("dropped", "every-level-k30+0", 32, [alt(around(n, n << 30, 0))], P, dict(type=orc.SUB_VERBATIM, levels_alive=True), near="every-level-k30"))
    out.append(Case("dropped", "every-level-k30+1", 32, [alt(around(n, n << 30, 1))], P, dict(type=orc.SUB_VERBATIM, levels_alive=False), near="every-level-k30"))


def _tied_frame(n, q, pairs):
    """2^q stretches of two halves of h = n >> (q + 1) samples with the sums of a tie pair, the pairs taken in turn."""
    h = n >> (q + 1)
    x = []
    for i in range(1 << q):
        sa, sb = pairs[i % len(pairs)]
        x += alt(spread(h, sa) + spread(h, sb))
    return x


def _po_tie(n, P, out):
    if n == 64:
        out.append(Case("po_tie", "four-nine", 16, [alt([4] * 32 + [9] * 32)], P,
                        dict(type=orc.SUB_FIXED, order=0, partition_order=0), dict(kind="porder", among=[0, 1], taken=0)))
    for q in sorted({0, P // 2, P - 1}):
        h = n >> (q + 1)
        found = tie_pairs(h)
        assert found, f"no tie pair of length {h} within the bound"
        quiet, loud = found[0], found[-1]
        x = _tied_frame(n, q, [quiet, loud] if q else [quiet])
        out.append(Case("po_tie", f"levels-{q}-{q + 1}", 16, [x], P, dict(type=orc.SUB_FIXED, order=0, partition_order=q),
                        dict(kind="porder", among=[q, q + 1], taken=q)))
    if P >= 2:
        t = three_level_tie(n >> 2)
        if t:
            h = n >> 2
            x = alt(spread(h, t[0]) + spread(h, t[1]) + spread(h, t[2]) + spread(h, t[3]))
            out.append(Case("po_tie", "levels-0-1-2", 16, [x], P, dict(type=orc.SUB_FIXED, order=0, partition_order=0),
                            dict(kind="porder", among=[0, 1, 2], taken=0)))


def _fixed_tie(n, P, out):
    i = np.arange(n, dtype=np.int64)
    shapes = [("constant", np.full(n, 5, dtype=np.int64), [1, 2, 3, 4], 1),
              ("ramp", 3 * i + 1, [2, 3, 4], 2),
              ("quadratic", i * i + 1, [3, 4], 3)]
    if (n - 4) % 3 == 0:
        shapes.insert(0, ("period6", np.array(([1, 1, 0, -1, -1, 0] * (n // 6 + 1))[:n], dtype=np.int64), [0, 1, 2, 3, 4], 0))
    for name, x, among, taken in shapes:
        out.append(Case("fixed_tie", name, narrowest(x), [x], P, dict(type=orc.SUB_FIXED, order=taken),
                        dict(kind="fixed", among=among, taken=taken)))
        # ties that exist only over the common tail: sample j reaches the tails of the orders from 4 - j up and leaves
        # those below untouched (so orders 3 and 4 can never be left tied: no such case for the quadratic)
        for j in (0, 1, 2):
            kept = [o for o in among if o < 4 - j]
            if len(kept) < 2:
                continue
            for p in (2, -2, 3, -3, 5, -5, 9, -9):      # the first perturbation that leaves the tie the strict minimum
                y = x.copy()
                y[j] += p
                sums = fixed_sums(y)[1]
                if len({sums[o] for o in kept}) == 1 and all(v > sums[kept[0]] for o, v in enumerate(sums) if o not in kept):
                    break
            else:
                raise AssertionError(f"no tail-only perturbation of sample {j} of {name}")
            out.append(Case("fixed_tie", f"{name}-tail-only-x{j}", narrowest(y), [y], P, dict(type=orc.SUB_FIXED, order=taken),
                            dict(kind="fixed", among=kept, taken=taken)))


def _ladder(n, P, out):
    for where, p in (("first", 1), ("middle", n // 2), ("last", n - 1)):
        for d in (0, 1):   # a step of 2^31 - 1 + d on a level with +-1 on it elsewhere
            x = np.array([-(1 << 30) + (1 if k % 2 else -1) for k in range(n)], dtype=np.int64)
            x[p:] += (1 << 31) - 2
            x[p - 1] = -(1 << 30)
            x[p] = (1 << 31) - 1 + d - (1 << 30)
            out.append(Case("ladder", f"first-difference-{where}{'-overflows' if d else ''}", 32, [x], P,
                            dict(ladder=1 if d else ladder(x))))
            assert ladder(x) == 1 if d else ladder(x) > 1
    c, w = n // 2, min(n // 2, 1024)
    a = max(1, (1 << 29) // w ** 3) | 1
    bg = a * np.clip(np.arange(n, dtype=np.int64) - c, -w, w) ** 3
    for j in (2, 3, 4):   # the smallest spike whose j-th difference overflows, and one less
        lo, hi = 1, (1 << 31) - 1
        while lo < hi:
            mid = (lo + hi) // 2
            x = bg.copy()
            x[c] += mid
            if ladder(x) <= j:
                hi = mid
            else:
                lo = mid + 1
        for d in (-1, 0):
            x = bg.copy()
            x[c] += lo + d
            assert ladder(x) == (j if d == 0 else j + 1), (n, j, d, ladder(x))
            out.append(Case("ladder", f"difference-{j}{'-overflows' if d == 0 else '-fits'}", 32, [x], P,
                            dict(ladder=ladder(x))))


def _verbatim(n, P, out):
    for bps, wasted in ((8, 0), (16, 0), (24, 0), (16, 2), (24, 2)):
        eb = bps - wasted
        k = eb - 3
        fixed = 8 + wasted + 6 + (5 if bps > 16 and k >= 15 else 4)
        deficit = 1 + fixed           # bits = fixed + n (1 + k) + sum of quotients = n * eb - 1
        if n // 2 < deficit + 1:
            continue
        pos = [4 << (k - 1)] * (n // 2)          # quotient 4 (x = q 2^(k-1): u = 2x = q 2^k)
        for i in range(deficit):
            pos[i] = 3 << (k - 1)                # quotient 3
        pos[0] = pos[1] = (4 << (k - 1)) - 1     # quotient 3, one below quotient 4
        pos[2] += 1                              # an odd value that stays
        for step in range(3):
            p = list(pos)
            for i in (0, 1)[:step]:
                p[i] += 1
            x = [0] * n
            x[0::2] = p
            x = [v << wasted for v in x]
            exp = dict(type=orc.SUB_FIXED, order=0, partition_order=0, rice=[k], wasted=wasted, bits=n * eb - 1) if step == 0 \
                else dict(type=orc.SUB_VERBATIM, wasted=wasted, bits=8 + wasted + n * eb)
            exp["fixed_bits"] = n * eb - 1 + step
            out.append(Case("verbatim", f"bits{step - 1:+d}-w{wasted}", bps, [x], P, exp, near=f"bits-w{wasted}"))


def _wasted(n, P, out):
    for bps in (8, 16, 24, 32):
        lo = -(1 << (bps - 1))
        x = [lo if (i * 7 // 3) % 3 == 0 else 0 for i in range(n)]
        out.append(Case("wasted", "all-but-one-bit", bps, [x], P, dict(wasted=bps - 1, bps=1)))
    for where, p in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        for v, w in ((-77, 0), (12, 2)):
            x = [0] * n
            x[p] = v
            out.append(Case("wasted", f"one-sample-{where}-w{w}", 16, [x], P, dict(wasted=w)))


@functools.lru_cache(maxsize=None)
def mono_cases(n, max_po):
    out = []
    for fam in (_rice, _method, _dropped, _po_tie, _fixed_tie, _ladder, _verbatim, _wasted):
        fam(n, max_po, out)
    names = [(c.family, c.name, c.bps) for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def big_block_cases():
    """65535 samples at 16 bits: the partition's sum is 2^30 - 1 (escape_bits = 31 by the ordinary route), then 2^30
    (ilog2(sum) + 2 = 32: None at the only level, the fallback).  VERBATIM wins both."""
    n, out = 65535, []
    for d in (-1, 0):
        x = alt(around(n, 1 << 30, d))
        out.append(Case("dropped", f"sum-2^30{d:+d}", 16, [x], 6, dict(type=orc.SUB_VERBATIM, sum=(1 << 30) + d), near="sum-2^30"))
    return tuple(out)


# ---------------------------------------------------------------- stereo
@functools.lru_cache(maxsize=None)
def stereo_cases(n, max_po):
    """Each case is run with exhaustive on and off and mid_side on and off; `tie` maps (exhaustive, mid_side) to
    (the tied assignments in the reference's order of trying them, the one it takes)."""
    rng = np.random.Generator(np.random.PCG64(4711 + n))
    left = (rng.integers(-40, 41, size=n, dtype=np.int64) | 1)       # odd: no wasted bits, never silent
    IND, LS, SR, MS = 0, 8, 9, 10
    out = []

    def add(name, l, r, tie=None, expect=None):
        out.append(Case("assignment", name, 16, [l, r], max_po, expect, tie))

    add("L==R", left, left, {(1, 1): ([LS, SR, MS], LS), (1, 0): ([LS, SR], LS), (0, 1): ([LS, SR, MS], LS), (0, 0): ([LS, SR], LS)})
    # R == 0: the fast rule sums |x|: independent = side/right = sum |L|; its no-mid-side order tries side/right first
    add("R==0", left, np.zeros(n, dtype=np.int64), {(0, 1): ([IND, SR], IND), (0, 0): ([SR, IND], SR)})
    add("R==-L", left, -left, {(0, 1): ([IND, MS], IND)})
    add("R==-L-1", left, -left - 1)
    l, r, _ = assignment_tie_pair(n, max_po)
    add("equal-bits-pair", l, r, {(1, 1): ("search", None)})
    # wasted bits per candidate
    add("wasted-2-2-4-3", 4 * np.where(np.arange(n) % 2 == 0, 5, -5), 4 * np.where(np.arange(n) % 2 == 0, 3, -3),
        expect=dict(wasted_by_source={0: 2, 1: 2, 8: 4, 9: 3}))
    add("wasted-1-3-0-1", 2 * left, 8 * np.roll(left, 3), expect=dict(wasted_by_source={0: 1, 1: 3, 8: 0, 9: 1}))
    return tuple(out)


def summary():
    """{family: {(block, max_po): count}} of the whole matrix."""
    out = {}
    for n, p in MONO_SHAPES:
        for c in mono_cases(n, p):
            out.setdefault(c.family, {}).setdefault((n, p), 0)
            out[c.family][(n, p)] += 1
    for n, p in STEREO_SHAPES:
        out.setdefault("assignment", {})[(n, p)] = len(stereo_cases(n, p))
    out.setdefault("dropped", {})[(65535, 6)] = len(big_block_cases())
    return out
