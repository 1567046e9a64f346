"""The u32 arithmetic of the candidate wave's order statistics (kernels/wave_cand_fixed.inc) and of the pair form of the
fold (kernels/wave_cand.inc wave_rice_fold<SIGNS>), checked in numpy on the CPU -- no GPU, no oracle:

  order statistics   per sample |x|, |d1| .. |d4| are five v_sad_u32 of two values with the SAME unsigned bias.  x and d1 carry
                     2^30; d2 = (p1 ^ 0x7FFFFFFF) + d1 and d3 = (p2 ^ 0x7FFFFFFF) + d2 (one v_xad_u32 each, p the previous
                     sample's difference of the level below) carry 2^31 - 1: p ^ 0x7FFFFFFF = -p - 1 + 2^31 (mod 2^32)
  pair form          t0 + t1 = (r1 ^ s1) + t0 (one v_xad_u32, t1 never formed); the second merged word
                     t1 | (r1 & 2^31) = r1 ^ (s1 & 0x7FFFFFFF) (v_bitop3_b32, truth table 0x78); negatives = -(s0 + s1)

The loop is restated literally -- the history values in front of it, the opaque u32 accumulators and their flush schedule
included -- over lanes of 64 samples, and compared with plain abs sums of the iterated differences in int64.  Inputs sit at
the edges of the range argument |d_K| < 2^(24 + K) for candidates of at most 25 bits."""
import numpy as np
import pytest

SPL = 64
M32 = np.uint64(0xFFFFFFFF)
BIAS = np.uint64(1 << 30)
FLIP = np.uint64(0x7FFFFFFF)


def u32(v):
    """int64 / uint64 array -> the value mod 2^32, as uint64"""
    return np.asarray(v).astype(np.int64).astype(np.uint64) & M32


def xad(a, b, c):
    return ((a ^ b) + c) & M32


def usad(a, b, acc):
    return (np.maximum(a, b) - np.minimum(a, b) + acc) & M32


def order_statistics_u32(x, h):
    """wave_cand_fixed.inc's loop: x [lanes, 64], h [lanes, 4] (the four samples before the lane's; zeros for lane 0).
    Returns sm [lanes, 5] = the lane's sums of |d_K| over its 64 samples, and the largest accumulator value met."""
    lanes = x.shape[0]
    xu, hu = u32(x), u32(h)
    hb = [(hu[:, k] + BIAS) & M32 for k in range(4)]
    d1m3, d1m2, d1m1 = [(hb[k + 1] - hb[k] + BIAS) & M32 for k in range(3)]
    d2m2, d2m1 = xad(d1m3, FLIP, d1m2), xad(d1m2, FLIP, d1m1)
    p0, p1, p2, p3 = hb[3], d1m1, d2m1, xad(d2m2, FLIP, d2m1)
    a = [np.zeros(lanes, dtype=np.uint64) for _ in range(5)]
    sm = np.zeros((lanes, 5), dtype=np.uint64)
    exact = np.zeros((lanes, 5), dtype=np.uint64)     # the same sums without the mod: the flush schedule must not wrap
    for e in range(SPL):
        xb = (xu[:, e] + BIAS) & M32
        prev = xu[:, e - 1] if e else hu[:, 3]
        d1 = (xb - prev) & M32
        d2 = xad(p1, FLIP, d1)
        d3 = xad(p2, FLIP, d2)
        pairs = ((xb, np.full(lanes, BIAS)), (xb, p0), (d1, p1), (d2, p2), (d3, p3))
        for k, (u, v) in enumerate(pairs):
            exact[:, k] += np.maximum(u, v) - np.minimum(u, v)
            a[k] = usad(u, v, a[k])
        p0, p1, p2, p3 = xb, d1, d2, d3
        for k, every in ((4, 16), (3, 32), (0, 64), (1, 64), (2, 64)):
            if e % every == every - 1:
                sm[:, k] += a[k]
                a[k] = np.zeros(lanes, dtype=np.uint64)
    return sm, exact


def reference_sums(sig):
    """sig: int64 [64 * lanes].  sum |d_K| per lane, d_K the K-th iterated difference with zeros in front of the signal."""
    d = np.concatenate([np.zeros(4, dtype=np.int64), sig.astype(np.int64)])
    out = []
    for k in range(5):
        out.append(np.abs(d[4:]).reshape(-1, SPL).sum(axis=1))
        d = np.concatenate([np.zeros(1, dtype=np.int64), np.diff(d)])
    return np.stack(out, axis=1), None


def signals():
    n = SPL * 6
    rng = np.random.Generator(np.random.PCG64(2407))
    k = np.arange(n, dtype=np.int64)
    alt = np.where(k & 1, -((1 << 24) - 1), (1 << 24) - 1)
    left = np.where(k & 1, -(1 << 23), (1 << 23) - 1)                  # L = -R = full scale, swapping every sample
    right = np.where(k & 1, (1 << 23) - 1, -(1 << 23))
    imp = np.zeros(n, dtype=np.int64)
    imp[SPL + 1] = -(1 << 24)
    steps = np.where((k // 3) & 1, -(1 << 24), (1 << 24) - 1)          # full-scale jumps at lane boundaries too
    return {
        "alternating_25bit": alt,
        "alternating_25bit_whole_range": np.where(k & 1, (1 << 24) - 1, -(1 << 24)),
        "constant_minus_2_24": np.full(n, -(1 << 24), dtype=np.int64),
        "side_of_opposite_full_scale": left - right,
        "ramp_up": k * 30000 - (1 << 23),
        "ramp_down_steep": (1 << 24) - 1 - k * 87000,
        "zeros": np.zeros(n, dtype=np.int64),
        "impulse": imp,
        "steps": steps,
        "random16": rng.integers(-(1 << 15), 1 << 15, size=n, dtype=np.int64),
        "random24": rng.integers(-(1 << 23), 1 << 23, size=n, dtype=np.int64),
        "random25": rng.integers(-(1 << 24), 1 << 24, size=n, dtype=np.int64),
    }


SIGNALS = signals()


def lanes_of(sig):
    x = sig.reshape(-1, SPL)
    pad = np.concatenate([np.zeros(4, dtype=np.int64), sig])
    h = np.stack([pad[i * SPL:i * SPL + 4] for i in range(x.shape[0])])
    return x, h


@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_order_statistics_are_the_abs_sums(name):
    sig = SIGNALS[name]
    assert np.abs(sig).max() <= (1 << 24)                              # a candidate of at most 25 bits
    x, h = lanes_of(sig)
    sm, exact = order_statistics_u32(x, h)
    want, _ = reference_sums(sig)
    assert (exact == want.astype(np.uint64)).all(), name               # every v_sad_u32 term is |d_K|: no bias mismatch, no wrap
    assert (sm == want.astype(np.uint64)).all(), name                  # ... and no partial sum wrapped before its flush


def test_the_edge_inputs_reach_the_range_bound():
    """the alternating signal's differences double per level: |d_K| = 2^K (2^24 - 1), the largest a 25-bit candidate gives"""
    want, _ = reference_sums(SIGNALS["alternating_25bit"])
    for k in range(1, 5):
        assert want[2, k] == SPL * ((1 << 24) - 1) * (1 << k)
    assert want[2, 4] // 4 < (1 << 32) <= want[2, 4] // 2              # 16 terms of order 4 fit a u32, 32 would not


def test_biased_values_stay_inside_u32():
    """d_K + 2^31 - 1 with |d_K| < 2^(24 + K) <= 2^27 neither falls below 0 nor reaches 2^32, for K = 2 and 3"""
    for k in (2, 3):
        lim = 1 << (24 + k)
        assert (1 << 31) - 1 - lim >= 0 and (1 << 31) - 1 + lim < (1 << 32)
    # the identity itself, for values of ANY common bias
    rng = np.random.Generator(np.random.PCG64(2408))
    d = rng.integers(-(1 << 27), 1 << 27, size=4096, dtype=np.int64)
    p = rng.integers(-(1 << 27), 1 << 27, size=4096, dtype=np.int64)
    for bias in (0, 1 << 30, (1 << 31) - 1, 12345):
        got = xad(u32(p + bias), FLIP, u32(d + bias))
        assert (got == u32(d - p + (1 << 31) - 1)).all()


# ---- the fold's pair form ----------------------------------------------------------------------------------------------------
def bitop3(a, b, c, table):
    """v_bitop3_b32: bit i of the result is bit (a_i << 2 | b_i << 1 | c_i) of the truth table"""
    out = np.zeros_like(a)
    for idx in range(8):
        if (table >> idx) & 1:
            m = (a if idx & 4 else ~a & M32) & (b if idx & 2 else ~b & M32) & (c if idx & 1 else ~c & M32)
            out |= m
    return out & M32


def residuals():
    rng = np.random.Generator(np.random.PCG64(2409))
    edge = np.array([0, -1, 1, -(1 << 31), (1 << 31) - 1, -(1 << 30), (1 << 30) - 1, 1 << 30, -(1 << 30) - 1,
                     (1 << 28) - 1, -(1 << 28)], dtype=np.int64)
    out = {"edges": rng.choice(edge, size=4096),
           "edge_pairs": np.stack(np.meshgrid(edge, edge), axis=-1).reshape(-1),
           "small": rng.integers(-300, 300, size=4096, dtype=np.int64),
           "negative": -rng.integers(1, 1 << 28, size=4096, dtype=np.int64),
           "wide": rng.integers(-(1 << 31), 1 << 31, size=4096, dtype=np.int64)}
    for name in ("alternating_25bit", "side_of_opposite_full_scale", "impulse", "random24"):
        d = SIGNALS[name]
        for k in range(4):
            d = np.diff(d, prepend=0)
        out["d4_" + name] = d[: d.size & ~1]
    return out


RESIDUALS = residuals()


@pytest.mark.parametrize("name", sorted(RESIDUALS))
def test_pair_form_of_the_fold(name):
    r = RESIDUALS[name]
    assert r.size % 2 == 0 and r.min() >= -(1 << 31) and r.max() < (1 << 31)
    r0, r1 = r[0::2], r[1::2]
    s0, s1 = r0 >> 63, r1 >> 63                                        # the sign masks (0 / -1)
    ru0, ru1, su0, su1 = u32(r0), u32(r1), u32(s0), u32(s1)
    # the present definitions (tests/test_hand_over_math.py)
    t0, t1 = ru0 ^ su0, ru1 ^ su1
    w1 = t1 | (ru1 & np.uint64(0x80000000))
    neg = (r0 < 0).astype(np.int64) + (r1 < 0).astype(np.int64)
    assert (t0 < (1 << 31)).all() and (t1 < (1 << 31)).all()
    # the pair form
    assert (xad(ru1, su1, t0) == t0 + t1).all()                        # (no wrap: each t < 2^31)
    assert (bitop3(ru1, su1, np.full_like(ru1, FLIP), 0x78) == w1).all()
    assert ((ru1 ^ (su1 & FLIP)) == w1).all()
    assert (-(s0 + s1) == neg).all()
    # the lane's sum over 32 pairs stays what the 64-bit accumulation of t0 + t1 gave
    lanes = r.size // 64
    if lanes:
        pair = xad(ru1, su1, t0)[: lanes * 32].reshape(lanes, 32).sum(axis=1)
        tt = np.abs(r[: lanes * 64] + (r[: lanes * 64] < 0)).reshape(lanes, 64).sum(axis=1)   # t = |r| - (r < 0)
        assert (pair == tt.astype(np.uint64)).all()
