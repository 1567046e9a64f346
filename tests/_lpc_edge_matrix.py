"""The LPC parameter stage (K4: Levinson-Durbin, compute_best_order, quantize -- encode.rs:3536-3580, 3656-3702,
3334-3401) at its edges: autocorrelation ROWS no natural signal gives, and integer PCM that reaches the failure and
clamp branches.  The stage exists three times -- the oracle (oracle/flac_oracle.c), the device (lpc_candidate,
csrc/kernels/lpc.inc) and the host re-decision (lpc_from_autocorr, csrc/host/lpc_host.cpp) -- and the three must agree
bit for bit.

Expected values ALWAYS come from the oracle chain run on the very f64 row (oracle_record), never from how the row was
built.  Every case names its family, and prove(case) asserts -- on the CPU, with the oracle alone -- that the case lands
in it.  Outside the tie families the oracle's two best order estimates differ by >= 1e-6 relative (1000 x the
production tie band of 1e-9): asserted by prove for every such row; the builders replace a row that misses it (another
bps), they never skip it.

No GPU call in this module (host_record calls the library's host hook, which needs no device)."""
import math
import struct
from collections import namedtuple

import numpy as np

import _oracle as orc

ORDERS = (1, 2, 7, 8, 9, 12, 13, 16, 17, 31, 32)      # max_lpc_order: every LMAX (8, 12, 16, 32) at its top and one above the previous
PRECISION_N = (192, 193, 384, 385, 576, 577, 1152, 1153, 2304, 2305, 4608, 4609, 65535)
TIE_FAMILIES = ("near_tie", "equal_minima")
MARGIN = 1e-6
STATUS = {0: "ok", 1: "InsufficientLpcSamples", 2: "NoBestLpcOrder", 3: "ZeroLpCoefficients", 4: "LpNegativeShiftError"}

Case = namedtuple("Case", "family L n bps ac want note")        # want: family-specific expectation checked by prove
Record = namedtuple("Record", "status order precision shift qlp bits best_bits l true_shift coeffs errors")


def lmax_of(L):
    return 8 if L <= 8 else 12 if L <= 12 else 16 if L <= 16 else 32


def precision_of(n):
    return int(orc.lib().orc_lpc_precision(int(n)))


def oracle_record(ac, L, n, bps):
    """The oracle chain on one row: lp_coefficients, compute_best_order, quantize."""
    ac = np.ascontiguousarray(ac[: L + 1], dtype=np.float64)
    if n <= L:
        return Record(1, 0, 0, 0, (), (), None, None, None, (), ())
    precision = precision_of(n)
    coeffs, errors = orc.lp_coefficients(ac)
    bits = orc.subframe_bits_by_order(bps, precision, n, errors)
    order = orc.compute_best_order(bps, precision, n, errors)
    if order == 0:
        return Record(2, 0, precision, 0, (), tuple(bits), None, None, None, (), tuple(errors))
    c = coeffs[order - 1]
    l = float("nan") if np.isnan(c).any() else float(np.max(np.abs(c)))
    rc, q, shift = orc.quantize(c, precision)
    best = float(bits[order - 1])
    if rc:
        return Record(2 + rc, order, precision, 0, (), tuple(bits), best, l, None, tuple(c), tuple(errors))
    true_shift = precision - 2 - math.floor(math.log2(l))       # before the cap at 15 and the "stored as 0" of a negative shift
    return Record(0, order, precision, shift, tuple(int(v) for v in q), tuple(bits), best, l, min(true_shift, 15), tuple(c),
                  tuple(errors))


def two_best_gap(bits):
    """Relative distance of the two smallest estimates, as the device's note_order_tie measures it (None: fewer than two;
    nan where they are not finite)."""
    if len(bits) < 2:
        return None
    b = sorted(bits)[:2]
    with np.errstate(all="ignore"):
        return float(np.float64(abs(b[1] - b[0])) / np.float64(abs(b[0])))


def est8_rule(best_bits, n):
    """lpc_est8 (csrc/kernels/lpc.inc): (the value, whether e lies within 1e-6 of an integer)."""
    e = best_bits * 8.0 / float(n)
    v = 255 if e >= 255.0 else int(e) + 1 if e >= 1.0 else 1
    return v, (math.isfinite(e) and abs(e - round(e)) <= 1e-6)


def log2_edge(l):
    """True where the host libm's floor(log2(l)) is not the exponent of l, inside the device table's range."""
    if l is None or not (l > 0.0) or math.isinf(l):
        return False
    e = math.frexp(l)[1] - 1
    return -64 <= e < 64 and math.floor(math.log2(l)) != e


def _ulps_below(x, k):
    (b,) = struct.unpack("<q", struct.pack("<d", x))
    return struct.unpack("<d", struct.pack("<q", b - k))[0]


def host_record(case_ac, L, n, bps):
    """lpc_from_autocorr (csrc/host/lpc_host.cpp) on one row, through its hook flacenc_lpc_host_row: an LPC_DTYPE record."""
    import ctypes as C

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import LPC_DTYPE

    ac = np.zeros(36, dtype=np.float64)
    ac[: L + 1] = case_ac[: L + 1]
    out = np.zeros(1, dtype=LPC_DTYPE)
    _lib.lib().flacenc_lpc_host_row(ac.ctypes.data_as(C.POINTER(C.c_double)), L, n, bps, out.ctypes.data)
    return out[0]


def same_record(got, want):
    """An LPC_DTYPE record against an oracle Record: status, and behind status 0 order, precision, shift, qlp[0..order)."""
    if int(got["status"]) != want.status:
        return False
    if want.status != 0:
        return True
    return ((int(got["order"]), int(got["precision"]), int(got["shift"])) == (want.order, want.precision, want.shift)
            and tuple(int(v) for v in got["qlp"][: want.order]) == want.qlp)


# ---------------------------------------------------------------------------------------------------------------------
# row builders
# ---------------------------------------------------------------------------------------------------------------------
def from_reflection(ks, ac0=1.0):
    """Inverse Levinson: the row whose recursion meets the reflection coefficients ks (up to rounding -- what the row
    does is the oracle's to say)."""
    ac = [float(ac0)]
    a, err = [], float(ac0)
    for i, k in enumerate(ks):
        s = -0.0
        for j in range(i):
            s = s + ac[i - j] * a[j]
        ac.append(k * err + s)
        a = [a[j] - k * a[i - 1 - j] for j in range(i)] + [k]
        err = err * (1.0 - k * k)
    return np.array(ac, dtype=np.float64)


def extend_flat(prefix, L):
    """prefix (lags 0 .. m) extended to lags 0 .. L so that every further reflection coefficient is EXACTLY zero: lag
    i + 1 is the very sum the recursion subtracts from it, computed in the recursion's order.  The errors of orders
    m + 1 .. L then equal order m's, and the coefficients get zeros appended."""
    ac = [float(v) for v in prefix]
    coeffs, _ = orc.lp_coefficients(np.array(ac)) if len(ac) >= 2 else ([], None)
    c = [float(v) for v in coeffs[-1]] if len(ac) >= 2 else []
    while len(ac) < L + 1:
        i = len(ac) - 1
        s = -0.0
        for j in range(i):
            s = s + ac[i - j] * c[j]
        ac.append(s)
        c = c + [0.0]
    out = np.array(ac, dtype=np.float64)
    return out if np.isfinite(out).all() else None


def _flat_row(prefix, want_L):
    """extend_flat at want_L, or at the largest order of ORDERS below it that stays finite (K^L overflows for huge K)."""
    for L in sorted((o for o in ORDERS if len(prefix) - 1 <= o <= want_L), reverse=True):
        row = extend_flat(prefix, L)
        if row is not None:
            return L, row
    raise AssertionError(("no finite extension", prefix))


def _with_margin(family, L, n, ac, want, note):
    """The case at the first bps that keeps the two best estimates MARGIN apart (a row that misses it is replaced)."""
    for bps in (16, 24, 8, 32, 12, 20):
        gap = two_best_gap(oracle_record(ac, L, n, bps).bits)
        if gap is None or not (gap < MARGIN):
            return Case(family, L, n, bps, np.ascontiguousarray(ac, dtype=np.float64), want, note)
    raise AssertionError(("no bps keeps the margin", family, note))


def one_lag(l_value, negative=False):
    """The one-lag prefix whose order-1 coefficient has magnitude l_value exactly: [1, k] (positive definite) below 1,
    [-1, K] (err = K^2 - 1 > 0) above."""
    s = -1.0 if negative else 1.0
    return [1.0, s * l_value] if l_value < 1.0 else [-1.0, s * l_value]


_cycle = [0]


def _next_L(lo=1):
    while True:
        _cycle[0] += 1
        L = ORDERS[_cycle[0] % len(ORDERS)]
        if L >= lo:
            return L


def first_negative_shift_l(precision):
    """The smallest double whose floor(log2) (host libm) is precision + 15: shift -17, the first LpNegativeShiftError."""
    target = precision + 15
    lo, hi = struct.unpack("<q", struct.pack("<d", 2.0 ** (target - 1)))[0], struct.unpack("<q", struct.pack("<d", 2.0 ** target))[0]
    while lo < hi:
        mid = (lo + hi) // 2
        if math.floor(math.log2(struct.unpack("<d", struct.pack("<q", mid))[0])) < target:
            lo = mid + 1
        else:
            hi = mid
    return struct.unpack("<d", struct.pack("<q", lo))[0]


def failure_rows():
    out = []
    for L in ORDERS:
        n = 4096
        z = np.zeros(L + 1)
        out.append(Case("fail_all_zero", L, n, 16, z.copy(), 2, "0/0"))
        a = z.copy()
        a[0] = 3.5
        if L >= 2:
            a[2::2] = -0.0
        out.append(Case("fail_zero_coeffs", L, n, 16, a, 3, "[a, 0, -0.0, ...]"))
        out.append(Case("fail_k_one", L, n, 16, np.ones(L + 1), 2, "k = 1"))
        out.append(Case("fail_k_one", L, n, 16, np.array([(-1.0) ** j for j in range(L + 1)]), 2, "k = -1"))
        for theta in (0.3, 1.0, 2.5):
            ac = np.cos(np.arange(L + 1) * theta)
            out.append(_with_margin("cosine_rank2", L, n, ac, None, f"theta {theta}"))
        base = from_reflection([0.6 * (-0.8) ** j for j in range(L)])
        inf0, inf1, nan0, nan1 = base.copy(), base.copy(), base.copy(), base.copy()
        inf0[0], inf1[1], nan0[0], nan1[1] = np.inf, np.inf, np.nan, np.nan
        out.append(Case("nonfinite", L, n, 16, inf0, None, "ac[0] = inf"))
        out.append(Case("nonfinite", L, n, 16, inf1, None, "ac[1] = inf"))
        out.append(Case("nonfinite", L, n, 16, nan0, None, "ac[0] = nan"))
        out.append(Case("nonfinite", L, n, 16, nan1, None, "ac[1] = nan"))
        if L >= 2:
            nl = base.copy()
            nl[L] = np.nan
            out.append(_with_margin("nan_last_lag", L, n, nl, None, "nan arrives at the last order"))
        out.append(Case("fail_negative_ac0", L, n, 16, -base, 2, "ac[0] < 0"))
        out.append(_with_margin("subnormal", L, n, base * 1e-310, None, "subnormal lags"))
        out.append(_with_margin("subnormal", L, n, base * 5e-324, None, "the smallest subnormal"))
        out.append(_with_margin("huge", L, n, base * 1e300, None, "1e300"))
        out.append(Case("insufficient", L, L, 16, base, 1, "n = L"))
        out.append(_with_margin("sufficient", L, L + 1, base, None, "n = L + 1"))
    return out


def take_while_rows():
    out = []
    for j in (2, 3, 8, 9, 16, 17, 31, 32):
        for L in sorted({min(o for o in ORDERS if o >= j), 32}):
            ks = [0.7 * (-0.85) ** i for i in range(j - 1)] + [1.5] + [1.5, 0.3] * 16
            out.append(_with_margin("take_while", L, 4096, from_reflection(ks[:L]), j, f"first non-positive error at order {j}"))
    return out


def precision_rows():
    out = []
    for n in PRECISION_N:
        L = _next_L()
        out.append(_with_margin("precision", L, n, from_reflection([0.9 * (-0.7) ** i for i in range(L)]), precision_of(n), f"n {n}"))
        L, row = _flat_row(one_lag(0.7), _next_L())
        out.append(_with_margin("precision", L, n, row, precision_of(n), f"n {n}, one lag"))
    return out


def shift_rows():
    out = []
    for n in (192, 384, 576, 1152, 2304, 4608, 65535):                 # precision 7 .. 13
        p = precision_of(n)
        for shift in range(15, -17, -1):
            l_value = 1.5 * 2.0 ** (p - 2 - shift)
            L, row = _flat_row(one_lag(l_value, negative=shift & 1), _next_L())
            out.append(_with_margin("shift_ladder", L, n, row, shift, f"precision {p} shift {shift}"))
        first = first_negative_shift_l(p)
        L, row = _flat_row(one_lag(first), 2)
        out.append(_with_margin("shift_first_error", L, n, row, 4, f"precision {p}: the first l with shift -17"))
        L, row = _flat_row(one_lag(_ulps_below(first, 1)), 2)
        out.append(_with_margin("shift_last_ok", L, n, row, -16, f"precision {p}: one ulp below it"))
    out.append(Case("shift_inf", 1, 4096, 16, np.array([-1.0, np.inf]), 4, "l = inf"))
    out.append(Case("shift_inf", 1, 192, 16, np.array([-1.0, -np.inf]), 4, "l = inf, precision 7"))
    for e in range(-40, 41):
        for ulps in (0, 1, 2, 3, 8, 64):
            l_value = _ulps_below(2.0 ** e, ulps)
            if l_value == 1.0:
                continue                                                    # k = 1: err = 0, not reachable
            L, row = _flat_row(one_lag(l_value, negative=(e + ulps) & 1), _next_L())
            out.append(_with_margin("log2_sweep", L, 4096, row, None, f"2^{e} - {ulps} ulps"))
    for e in (-1074, -1000, -300, -100, -70, -65, 64, 65, 100, 300, 500):
        for ulps in (0, 1):
            l_value = _ulps_below(2.0 ** e, ulps) if e > -1074 else 5e-324
            L, row = _flat_row(one_lag(l_value), 2)
            inside = -64 <= math.frexp(l_value)[1] - 1 < 64                  # (2^64 - 1 ulp has exponent 63)
            out.append(_with_margin("log2_sweep" if inside else "log2_outside_table", L, 4096, row, None, f"2^{e} - {ulps} ulps"))
    # multi-lag rows of negative shift: reflection coefficients -k repeated
    for k in (0.54, 0.6, 0.66, 0.7, 0.75):
        for n in (192, 4096):
            out.append(_with_margin("negative_shift_multi", 32, n, from_reflection([-k] * 32), None, f"k = -{k} x 32"))
    out.append(_with_margin("negative_shift_multi", 16, 192, from_reflection([0.875] + [-0.875] * 15), None, "reflection [7/8, -7/8 x 15]"))
    return out


def from_coefficients(c):
    """Step-down: the reflection coefficients of the predictor c (then the row by from_reflection)."""
    a = [float(v) for v in c]
    ks = []
    while a:
        k = a[-1]
        ks.append(k)
        m = len(a) - 1
        d = 1.0 - k * k
        a = [(a[j] + k * a[m - 1 - j]) / d for j in range(m)]
    return from_reflection(ks[::-1])


def quantiser_rows():
    out = []
    n = 4096                                                                # precision 12; l in [0.5, 1): shift 11
    for m in (1024, 1025, 1500, 1501, 2046):
        for sign in (1.0, -1.0):
            L, row = _flat_row([1.0, sign * (2 * m + 1) / 4096.0], _next_L())
            out.append(_with_margin("round_tie", L, n, row, int(sign) * (m + 1), f"{sign:+.0f}({m} + 1/2)"))
    for i, L in enumerate(ORDERS):                                          # one tie that rint() would round the other way at every order
        sign = 1.0 - 2.0 * (i & 1)
        row = extend_flat([1.0, sign * (2 * (1100 + 2 * i) + 1) / 4096.0], L)
        out.append(_with_margin("round_tie", L, n, row, int(sign) * (1100 + 2 * i + 1), f"{sign:+.0f}({1100 + 2 * i} + 1/2) at order {L}"))
    # c = [k1 / 2, 1 / 2] exactly: c[0] * 2048 = 500.5 (a tie), and its error -0.5 makes c[1] * 2048 - 0.5 a tie as well
    L, row = _flat_row([1.0, 1001.0 / 2048.0, (1001.0 / 2048.0) ** 2 + 0.5 * (1.0 - (1001.0 / 2048.0) ** 2)], _next_L(2))
    out.append(_with_margin("tie_feeds_next", L, n, row, (501, 1024), "the error of one tie makes the next"))
    L, row = _flat_row([1.0, -1001.0 / 2048.0, (1001.0 / 2048.0) ** 2 + 0.5 * (1.0 - (1001.0 / 2048.0) ** 2)], _next_L(2))
    out.append(_with_margin("tie_feeds_next", L, n, row, (-501, 1025), "negative first tie"))
    for c in ([0.99985, -0.3], [0.99985, 0.123, -0.2]):
        L, row = _flat_row(list(from_coefficients(c)), _next_L(len(c)))
        out.append(_with_margin("clamp_carries", L, n, row, None, f"c ~ {c}"))
    L, row = _flat_row([1.0, 4095.0 / 4096.0], _next_L())
    out.append(_with_margin("clamp_carries", L, n, row, None, "2047.5 -> 2048 -> 2047, one coefficient"))
    L, row = _flat_row([1.0, -4095.0 / 4096.0], _next_L())
    out.append(_with_margin("min_not_clamped", L, n, row, -2048, "-2047.5 -> -2048"))
    L, row = _flat_row([1.0, -127.0 / 128.0], _next_L())
    out.append(_with_margin("min_not_clamped", L, 192, row, -64, "precision 7: -63.5 -> -64"))
    for k in (2.0 ** -20, -2.0 ** -22, 2.0 ** -17 - 2.0 ** -40):
        L, row = _flat_row([1.0, k], _next_L())
        out.append(_with_margin("all_zero_at_15", L, n, row, None, f"k = {k}"))
    L, row = _flat_row([1.0, 0.0625 - 2.0 ** -30], _next_L())
    out.append(_with_margin("cap_15_full", L, n, row, 2047, "0.0625 - 2^-30: shift 15, q 2047"))
    # c = [1/2, -1/4, 1/2]: two equal maxima, the last one is max_by's
    for L in (7, 12, 16, 32):
        out.append(_with_margin("equal_maxima", L, n, extend_flat([1.0, 0.5, 0.25, 0.5], L), None, "c = [1/2, -1/4, 1/2]"))
    return out


def _bisect_last_lag(L, n, bps, ks):
    """Moves the last lag of the reflection-built row until order L and the best of the lower orders tie: [(row, gap)],
    the smallest gap reached and, where that is an exact tie, the smallest gap above zero as well."""
    def f(x):
        row[L] = x
        b = oracle_record(row, L, n, bps).bits
        return (b[L - 1] - min(b[: L - 1])) if len(b) == L else float("inf")

    row = from_reflection(ks[:L - 1] + [0.0])
    x_lo = float(row[L])                                                    # k_L = 0: order L pays its header for nothing
    row_hi = from_reflection(ks[:L - 1] + [0.5])
    x_hi = float(row_hi[L])
    assert f(x_lo) > 0 and f(x_hi) < 0, (L, f(x_lo), f(x_hi))
    best, best_nz = (float("inf"), None), (float("inf"), None)
    for _ in range(200):
        mid = x_lo + (x_hi - x_lo) / 2
        if mid == x_lo or mid == x_hi:
            break
        v = f(mid)
        gap = two_best_gap(oracle_record(row, L, n, bps).bits)
        if gap < best[0]:
            best = (gap, mid)
        if 0 < gap < best_nz[0]:
            best_nz = (gap, mid)
        if v > 0:
            x_lo = mid
        else:
            x_hi = mid
    for x in (x_lo, x_hi):
        f(x)
        gap = two_best_gap(oracle_record(row, L, n, bps).bits)
        if gap < best[0]:
            best = (gap, x)
        if 0 < gap < best_nz[0]:
            best_nz = (gap, x)
    out = []
    for gap, x in (best, best_nz) if best[0] == 0 else (best,):
        row[L] = x
        out.append((row.copy(), gap))
    return out


NEAR_TIE_GAPS = {}      # (L, n) -> the gaps the bisection reached (kept rows and dropped ones)


def order_choice_rows():
    out = []
    for L in ORDERS:
        base = from_reflection([0.8 * (-0.75) ** i for i in range(L)])
        out.append(_with_margin("negative_estimates", L, 4096, base * 1e-30, None, "tiny ac: every estimate below zero"))
    # every order's estimate the same number: err = n 2^(2H + 1) exactly at every order (flat extension), so
    # log(err / 2n) / (2 ln 2) is H where the libm's log() is exact there, and H (n - i) + i H = H n for every i
    for L, bps in ((2, 8), (8, 8), (12, 4), (32, 8)):
        n, H = 4096, bps + 12
        A = 2.0 ** (12 + 2 * H + 1 - 3)
        row = extend_flat([-A, 3.0 * A], L)                                # k = -3: err = 8 A
        out.append(Case("equal_minima", L, n, bps, row, None, "bit-equal estimates: the first must win"))
    for L in ORDERS[1:]:
        for n, bps in ((4096, 16), (1000, 24)):
            for row, gap in _bisect_last_lag(L, n, bps, [0.5 * (-1.0) ** i for i in range(L)]):
                NEAR_TIE_GAPS.setdefault((L, n), []).append(gap)
                if gap <= 1e-10:
                    out.append(Case("near_tie", L, n, bps, row, gap, f"two best estimates {gap:.3g} apart"))
    return out


_rows = None


def rows():
    global _rows
    if _rows is None:
        _cycle[0] = 0
        _rows = failure_rows() + take_while_rows() + precision_rows() + shift_rows() + quantiser_rows() + order_choice_rows()
    return _rows


def prove(case):
    """Asserts with the oracle alone that the case lands in its family; returns its oracle record."""
    r = oracle_record(case.ac, case.L, case.n, case.bps)
    f, w = case.family, case.want
    gap = two_best_gap(r.bits)
    if f in TIE_FAMILIES:
        assert gap is not None and gap <= 1e-10, (case.note, gap)
    else:
        assert gap is None or not (gap < MARGIN), (f, case.note, gap)
    if f.startswith("fail_") or f in ("insufficient", "shift_first_error", "shift_inf"):
        assert r.status == w, (f, case.note, r.status)
    if f == "fail_zero_coeffs":
        assert any(math.copysign(1.0, v) < 0 and v == 0 for v in case.ac) or case.L < 2
    elif f == "cosine_rank2":
        assert r.errors[0] > 0 and not any(abs(e) >= 1e-12 for e in r.errors[1:3]), r.errors[:3]
    elif f == "nonfinite":
        assert not np.isfinite(case.ac).all()
    elif f == "nan_last_lag":
        assert r.status == 0 and r.order < case.L and len(r.bits) == case.L - 1
    elif f == "subnormal":
        assert 0 < abs(case.ac[1]) < 2.3e-308
    elif f == "huge":
        assert abs(case.ac[0]) >= 1e299 and r.status == 0
    elif f == "sufficient":
        assert case.n == case.L + 1 and r.status != 1
    elif f == "take_while":
        assert len(r.bits) == w - 1 and not (r.errors[w - 1] > 0) and all(e > 0 for e in r.errors[: w - 1]), (case.note, r.errors)
        if case.L > w:
            assert r.errors[w] > 0, "a positive error behind the first non-positive one: take_while must not look at it"
        assert r.status == 0 and r.order <= w - 1
    elif f == "precision":
        assert r.status == 0 and r.precision == w
    elif f == "shift_ladder":
        assert r.status == 0 and r.true_shift == w and r.shift == max(w, 0), (case.note, r.true_shift, r.shift)
    elif f == "shift_last_ok":
        assert r.status == 0 and r.true_shift == -16 and r.shift == 0
    elif f == "log2_sweep":
        assert r.status in (0, 4)
    elif f == "log2_outside_table":
        e = math.frexp(r.l)[1] - 1
        assert (e < -64 or e >= 64) and r.status in (0, 4)
    elif f == "negative_shift_multi":
        assert r.status == 0 and r.true_shift < 0 and r.order > 1, (case.note, r.true_shift, r.order)
    elif f == "round_tie":
        assert r.status == 0 and r.shift == 11 and r.qlp[0] == w and abs(r.coeffs[0] * 2048.0) % 1.0 == 0.5, (case.note, r.qlp[:1])
    elif f == "tie_feeds_next":
        assert r.status == 0 and r.order == 2 and r.shift == 11 and r.qlp == w, (case.note, r.qlp)
        assert abs(r.coeffs[0] * 2048.0) % 1.0 == 0.5 and (r.coeffs[1] * 2048.0) % 1.0 == 0.0
    elif f == "clamp_carries":
        mx = (1 << (r.precision - 1)) - 1
        assert r.status == 0 and r.qlp[0] == mx and math.floor(r.coeffs[0] * 2.0 ** r.shift + 0.5) == mx + 1, (case.note, r.qlp, r.coeffs)
    elif f == "min_not_clamped":
        assert r.status == 0 and r.qlp[0] == w == -(1 << (r.precision - 1)) and r.coeffs[0] * 2.0 ** r.shift > w - 0.5
    elif f == "all_zero_at_15":
        assert r.status == 0 and r.shift == 15 and not any(r.qlp)
    elif f == "cap_15_full":
        assert r.status == 0 and r.shift == 15 and r.true_shift == 15 and r.qlp[0] == w
    elif f == "equal_maxima":
        a = [abs(v) for v in r.coeffs]
        assert r.status == 0 and r.order == 3 and a.count(max(a)) == 2 and a[-1] == max(a), r.coeffs
    elif f == "negative_estimates":
        assert r.status == 0 and all(b < 0 for b in r.bits)
    elif f == "equal_minima":
        assert len(r.bits) == case.L and len(set(r.bits)) == 1 and r.order == 1, (case.note, r.bits[:3], r.order)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# integer PCM that reaches the branches
# ---------------------------------------------------------------------------------------------------------------------
RECT, HANN, TUKEY = (0, 0.0), (1, 0.0), (2, 0.5)
PcmContext = namedtuple("PcmContext", "name block channels bps L window frames ragged")      # frames: [[(tag, int64 samples)] per channel]


def _signal(tag, n):
    t = np.arange(n, dtype=np.int64)
    x = np.zeros(n, dtype=np.int64)
    if tag == "imp_first":
        x[0] = 1000
    elif tag == "imp_last":
        x[n - 1] = -1000
    elif tag == "imp_mid":
        x[n // 2] = 1000
    elif tag == "dc":
        x[:] = 20000
    elif tag == "alt":
        x[:] = 20000 * (1 - 2 * (t & 1))
    elif tag == "sine30":
        x = np.rint(2.0 ** 30 * np.sin(2 * np.pi * t / 1000.0)).astype(np.int64)
    elif tag == "ramp":
        x = 7 * t - 3 * n
    elif tag == "square":
        x = t * t
    elif tag == "half_square":
        x = (t * t) >> 1
    elif tag == "zero":
        pass
    else:
        raise KeyError(tag)
    return x


def _ctx(name, block, channels, bps, L, window, frames, ragged=False):
    built = []
    for f in frames:
        tags, n = (f, block) if not isinstance(f[-1], int) else (f[:-1], f[-1])
        assert len(tags) == channels
        built.append([(tag, _signal(tag, n)) for tag in tags])
        for _, x in built[-1]:
            assert -(1 << (bps - 1)) <= x.min() and x.max() < (1 << (bps - 1)), (name, bps)
    return PcmContext(name, block, channels, bps, L, window, built, ragged)


def pcm_contexts():
    B = 4096
    return [
        _ctx("stereo16_L12_tukey", B, 2, 16, 12, TUKEY, [("imp_first", "imp_last"), ("imp_mid", "dc"), ("dc", "alt"), ("ramp", "imp_mid")]),
        _ctx("stereo24_L12_rect", B, 2, 24, 12, RECT, [("dc", "alt"), ("alt", "imp_mid"), ("half_square", "ramp"), ("imp_first", "dc")]),
        _ctx("stereo16_L32_tukey", B, 2, 16, 32, TUKEY, [("dc", "alt"), ("ramp", "imp_last"), ("imp_mid", "ramp")]),
        _ctx("stereo24_L32_hann", B, 2, 24, 32, HANN, [("imp_first", "imp_last"), ("half_square", "dc"), ("alt", "ramp")]),
        _ctx("mono24_L12_hann", B, 1, 24, 12, HANN, [("imp_first",), ("imp_last",), ("imp_mid",), ("dc",), ("half_square",)]),
        _ctx("mono32_L12_tukey", B, 1, 32, 12, TUKEY, [("sine30",), ("imp_mid",), ("square",), ("imp_last",)]),
        _ctx("mono32_L32_tukey", B, 1, 32, 32, TUKEY, [("sine30",), ("dc",), ("alt",), ("ramp",), ("square",), ("imp_first",)]),
        _ctx("three24_L8_rect", B, 3, 24, 8, RECT, [("dc", "alt", "imp_mid"), ("ramp", "half_square", "dc"), ("imp_first", "alt", "zero")]),
        _ctx("stereo16_b192_rect", 192, 2, 16, 12, RECT, [("dc", "alt"), ("alt", "imp_mid"), ("ramp", "dc")]),
        _ctx("stereo16_b192_hann", 192, 2, 16, 12, HANN, [("imp_first", "imp_last"), ("imp_mid", "dc")]),
        _ctx("stereo24_b1000_tukey", 1000, 2, 24, 12, TUKEY, [("dc", "imp_mid"), ("imp_first", "ramp"), ("alt", "half_square")]),
        _ctx("stereo16_ragged_tukey", B, 2, 16, 12, TUKEY, [("dc", "alt", 13), ("ramp", "imp_mid", 192), ("imp_first", "dc", 193),
                                                           ("dc", "imp_last", 4096), ("alt", "dc", 12)], ragged=True),
    ]


def candidates_of(ctx, frame):
    """[(samples after the wasted-bits shift, effective bps) or None for an all-zero row] in the device's candidate order."""
    rows = [x for _, x in frame]
    bps = [ctx.bps] * len(rows)
    if ctx.channels == 2 and ctx.bps < 32:
        l, r = rows
        rows, bps = [l, r, (l + r) >> 1, l - r], [ctx.bps, ctx.bps, ctx.bps, ctx.bps + 1]
    out = []
    for x, b in zip(rows, bps):
        orv = int(np.bitwise_or.reduce(x))
        if orv == 0:
            out.append(None)
            continue
        w = (orv & -orv).bit_length() - 1
        out.append((x >> w, b - w))
    return out


_windows = {}


def pcm_records(ctx):
    """The oracle chain of every candidate of every frame ([frame][candidate] Record, None for an all-zero candidate)."""
    out = []
    for frame in ctx.frames:
        recs = []
        for cand in candidates_of(ctx, frame):
            if cand is None:
                recs.append(None)
                continue
            x, bps = cand
            n = len(x)
            if n <= ctx.L:
                recs.append(oracle_record(np.zeros(ctx.L + 1), ctx.L, n, bps))
                continue
            key = (ctx.window, n)
            if key not in _windows:
                _windows[key] = orc.window(ctx.window[0], ctx.window[1], n)
            ac = orc.autocorrelate(x.astype(np.float64) * _windows[key], ctx.L)
            recs.append(oracle_record(ac, ctx.L, n, bps))
        out.append(recs)
    return out


def prove_pcm(ctx, frame_index, channel, rec):
    """What the issue's table says of this channel's signal under this context, asserted on the oracle's record.
    Returns True where a claim was checked."""
    tag, x = ctx.frames[frame_index][channel]
    n, w, L = len(x), ctx.window, ctx.L
    if n <= L:
        assert rec.status == 1
        return True
    if tag in ("imp_first", "imp_last") and w in (HANN, TUKEY) and n in (16, 192, 4096):
        assert rec.status == 2 and not (rec.errors[0] > 0), (ctx.name, tag, rec.status)      # the window is 0 there: ac all zero
    elif tag == "imp_mid" and n >= 2 * L + 2:
        assert rec.status == 3 and len(set(rec.errors)) == 1, (ctx.name, tag, rec.status)
    elif tag in ("dc", "alt") and w == TUKEY and n == 4096 and L == 32:
        assert rec.status == 0 and len(rec.bits) == 4 and rec.order == 4 and rec.shift == 8 and abs(rec.l - 5.22) < 0.01, (ctx.name, rec.order, rec.l)
    elif tag == "sine30" and w == TUKEY and L == 32:
        assert rec.status == 0 and len(rec.bits) == 2 and rec.order == 2 and rec.shift == 10 and 2047 in rec.qlp, (rec.order, rec.shift, rec.qlp)
    elif tag == "ramp" and w == TUKEY and n == 4096 and L == 32:
        assert len(rec.bits) == 12, len(rec.bits)
    elif tag == "square" and w == TUKEY and n == 4096 and L == 32:
        assert len(rec.bits) == 8, len(rec.bits)
    elif tag in ("dc", "alt") and w == RECT and n in (192, 4096):
        p = 12 if n == 4096 else 7
        want = ((1 << (p - 1)) - 1) if tag == "dc" else -(1 << (p - 1))
        assert rec.status == 0 and rec.order == 1 and rec.precision == p and rec.shift == p - 1 and rec.qlp[0] == want, (ctx.name, tag, rec)
        assert rec.l == (n - 1) / n and math.floor(abs(rec.coeffs[0]) * 2.0 ** rec.shift + 0.5) == (1 << (p - 1))   # 2047.5 -> 2048: clamped / not
    else:
        return False
    return True
