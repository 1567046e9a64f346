"""The autocorrelation kernels (K3: csrc/kernels/autocorr.inc, launched by csrc/autocorr.hip as plan_autocorr in
csrc/host/batch_route.cpp chooses) at their tile, lag and length edges: the CASES.  Every case names the instantiation
it means to reach; tests/test_autocorr_edge_matrix_oracle.py proves on the CPU that the dispatcher agrees and that the
case's aim holds, tests/test_gpu_autocorr_edges.py compares what the kernels leave with the oracle bit for bit.

A case is: channels, bps, block length, length of the last frame (or a list of ragged lengths), frames, max LPC order,
window (kind, parameter), the door it enters by, knobs / lag split, and what it declares: the route's input, the kernel of
the whole blocks (`reach`), the kernel of a short last frame (`reach_last`), whether fused tiles run, and how many
candidates the reference does not analyse.

SHARED CONSTRUCTION.  A frame's samples are a function of (channels, bps, length, slot) alone (frame_rows): seeded PCM of
_pcm.synth_fast, two wasted bits on channel 0, and on the last channel a rail for HALF the frame -- slot 0 the positive
rail and slot 1 the negative one over [n/4, n/4 + n/2), slot -1 (one-frame cases, short last frames, ragged frames) the
positive rail over [0, n/2) and the negative one over [n/2, n).  No frame is constant.  Frame f of a batch has slot
f % 16 (a short last frame: -1), so a batch of 1025 frames costs the oracle 16.  Channel choice is exhaustive throughout:
every candidate is analysed.

FAMILIES (DESIGN.md "The autocorrelation edge matrix"): tiles, groups, lags, fused, generic, ragged.

No GPU call in this module."""
import ctypes as C
import functools
from collections import Counter, namedtuple

import numpy as np

import _oracle as orc
from _pcm import synth_fast

RATE = 48000
FN = 4096
AC_LD = 36
PERIOD = 16
RECT, HANN, TUKEY = 0, 1, 2
ROUTES = ("K0_COPY", "K0_PACKED", "PLANAR_IN_PLACE", "DIRECT_STEREO", "SPLIT", "SPLIT_XPOSE")
HOST, DEVICE, RAGGED = "analyze", "encode_device", "encode_ragged_device"

Case = namedtuple("Case", "name family ch bps block last frames order window door env lag_split route reach reach_last fused "
                          "skipped lengths aim")


# ------------------------------------------------------------------------------------------------ the kernels' own numbers
def nl_of(order):
    """k_autocorr4's lag count for a max order of 1 .. 16"""
    return 5 if order <= 4 else 9 if order <= 8 else 13 if order <= 12 else 17


def h_of(order):
    """the generic kernels' lag count: order + 1 rounded up to four"""
    return (order + 1 + 3) & ~3


def ts_of(H):
    """samples per tile of k_autocorr2 / k_autocorr_ragged: H * (64 // H)"""
    return H * max(64 // H, 1)


HS = (4, 8, 12, 16, 20, 24, 28, 32, 36)
assert [ts_of(h) for h in HS] == [64, 64, 60, 64, 60, 48, 56, 64, 36]


def ac4(order, ns, producer):
    return f"k_autocorr4<{nl_of(order)},{ns},{producer}>"


def deep(producer):
    return f"k_autocorr4_deep<{producer}>"


def ac2(order):
    return f"k_autocorr2<{h_of(order)}>"


def ragged_kernel(order):
    return f"k_autocorr_ragged<{h_of(order)}>"


def generic_tile_paths(n, H):
    """ac_wave's two paths, tile by tile: 'f' the unguarded blocks (a full tile behind the first: tbase + TS <= n && t > 0),
    'g' the guarded ones (the first tile -- its first block drops the terms before the frame -- and a short last tile)"""
    TS = ts_of(H)
    out = []
    for t in range((n + TS - 1) // TS):
        out.append("f" if t * TS + TS <= n and t > 0 else "g")
    return "".join(out)


# ------------------------------------------------------------------------------------------------ samples
def rail_spans(n, slot):
    """[(lo, hi, value sign)] of the last channel's rails in a frame of n samples"""
    if slot == -1:
        return [(0, n // 2, +1), (n // 2, n, -1)]
    if slot in (0, 1):
        return [(n // 4, n // 4 + n // 2, +1 if slot == 0 else -1)]
    return []


@functools.lru_cache(maxsize=None)
def frame_rows(ch, bps, n, slot):
    """[ch][n] int64, read-only"""
    seed = 7 + 1000003 * n + 101 * (slot + 1) + 13 * ch + bps
    x = synth_fast(seed, ch, bps, max(n, 8))[: n * ch].reshape(n, ch).astype(np.int64)
    for lo, hi, sign in rail_spans(n, slot):
        x[lo:hi, ch - 1] = (1 << (bps - 1)) - 1 if sign > 0 else -(1 << (bps - 1))
    x[:, 0] = (x[:, 0] >> 2) << 2                       # two wasted bits on channel 0 (one channel: the rails keep them)
    out = np.ascontiguousarray(x.T)
    out.setflags(write=False)
    return out


def slot_of(case, f):
    if case.lengths is not None or case.frames == 1 or (f == case.frames - 1 and case.last != case.block):
        return -1
    return f % PERIOD


def length_of(case, f):
    if case.lengths is not None:
        return case.lengths[f]
    return case.last if f == case.frames - 1 else case.block


def frame_of(case, f):
    return frame_rows(case.ch, case.bps, length_of(case, f), slot_of(case, f))


def pcm_of(case):
    """the batch as the doors take it: interleaved int32, frame after frame, nothing behind the last sample"""
    return np.ascontiguousarray(np.concatenate([frame_of(case, f).T.reshape(-1) for f in range(case.frames)]).astype(np.int32))


def candidates_of(rows):
    """a frame's candidate rows in the device's order (stereo below 32 bits: L, R, mid, side), before the wasted-bits shift"""
    if rows.shape[0] == 2:
        l, r = rows[0], rows[1]
        return [l, r, (l + r) >> 1, l - r]
    return list(rows)


def ncand_of(case):
    return 4 if case.ch == 2 and case.bps < 32 else case.ch


@functools.lru_cache(maxsize=None)
def window(kind, param, n):
    w = orc.window(kind, param, n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def shifted_windowed(ch, bps, n, slot, window_):
    """per candidate: None when the reference analyses none of it (all zero, or constant), else the f64 row it sums"""
    w = window(window_[0], window_[1], n)
    out = []
    for row in candidates_of(frame_rows(ch, bps, n, slot)):
        orv = int(np.bitwise_or.reduce(row))
        if orv == 0 or bool(np.all(row == row[0])):
            out.append(None)
            continue
        wasted = (orv & -orv).bit_length() - 1
        out.append((row >> wasted).astype(np.float64) * w)
    return out


@functools.lru_cache(maxsize=None)
def frame_sums(ch, bps, n, slot, order, window_):
    """per candidate: None, or orc.autocorrelate's lags 0 .. min(order, n - 1).  Computed once, shared, read-only."""
    out = []
    for xw in shifted_windowed(ch, bps, n, slot, window_):
        if xw is None or n <= order:                     # (n <= order: the reference does no LPC analysis of the frame)
            out.append(None)
            continue
        s = orc.autocorrelate(xw, order)
        s.setflags(write=False)
        out.append(s)
    return tuple(out)


def sums_of(case, f):
    return frame_sums(case.ch, case.bps, length_of(case, f), slot_of(case, f), case.order, case.window)


def left_fold(rows, order):
    """The statement of what the kernels must reproduce, with nothing of higher precision in it: per lag, a left fold from
    -0.0 with one rounded multiply and one rounded add per term, in increasing sample index.  (All rows and lags advance
    together -- numpy's element-wise f64 multiply and add round each element on its own, so every lag's chain is the scalar
    one.)"""
    W = np.stack(rows)
    n = W.shape[1]
    lags = min(order, n - 1) + 1
    acc = np.full((W.shape[0], lags), -0.0)
    pad = np.concatenate([np.zeros((W.shape[0], lags - 1)), W], axis=1)     # pad[:, j + lags - 1] = W[:, j]
    for j in range(n):
        k = min(j, lags - 1) + 1                                             # lags 0 .. k - 1 have a partner at j - lag >= 0
        acc[:, :k] = acc[:, :k] + W[:, j:j + 1] * pad[:, j + lags - 1 - np.arange(k)]
    return acc


def oracle_frame_bytes(case, f, number=None):
    from _compare import orc_options_for

    opts = orc_options_for(case.block, 6, case.order, True, True, case.window[0], case.window[1])
    rc, data, _ = orc.encode_frame(opts, RATE, case.bps, frame_of(case, f).astype(np.int32), frame_number=f if number is None else number)
    assert rc == 0
    return data


# ------------------------------------------------------------------------------------------------ windows
@functools.lru_cache(maxsize=None)
def flat_run(kind, param, n):
    """[lo, hi): the first run of window values that are exactly 1.0, as the context finds it"""
    w = window(kind, param, n)
    lo = 0
    while lo < n and w[lo] != 1.0:
        lo += 1
    hi = lo
    while hi < n and w[hi] == 1.0:
        hi += 1
    return lo, hi


def fused_tiles(case_or_tuple):
    """(t0, t1) of Params::fma_t0 / fma_t1 from the oracle's window alone"""
    bps, ch, order, window_, block, env = case_or_tuple
    lo, hi = flat_run(window_[0], window_[1], block)
    stereo4 = 1 if ch == 2 and bps < 32 else 0
    if "FLACGPU_NO_AC_FMA" in env or bps + stereo4 > 26 or hi <= lo:
        return 0, 0
    maxlag = 16 if order <= 16 else 32
    return (lo + maxlag + 31) // 32, hi // 32


def tiles_of(case):
    return fused_tiles((case.bps, case.ch, case.order, case.window, case.block, case.env))


@functools.lru_cache(maxsize=None)
def find_tukey(n, end, residue):
    """the smallest Tukey parameter k / 2000 (an exact float32) whose flat run's start (end: its end) is `residue` mod 32 and
    that leaves at least eight tiles flat"""
    for k in range(100, 1900):
        p = float(np.float32(k / 2000.0))
        lo, hi = flat_run(TUKEY, p, n)
        if hi - lo >= 8 * 32 + 64 and (lo if end == "lo" else hi) % 32 == residue:
            return p
    raise AssertionError((n, end, residue))


@functools.lru_cache(maxsize=None)
def find_tukey_unfused(n, order):
    """the largest Tukey parameter k / 2000 that has a flat run and still fuses no tile at this order"""
    for k in range(1999, 1000, -1):
        p = float(np.float32(k / 2000.0))
        lo, hi = flat_run(TUKEY, p, n)
        if hi > lo:
            t0, t1 = fused_tiles((24, 1, order, (TUKEY, p), n, ()))
            assert t0 >= t1, (n, order, p)
            return p
    raise AssertionError((n, order))


# ------------------------------------------------------------------------------------------------ the cases
def case(name, family, ch, bps, block, frames, order, route, reach, last=None, window_=(TUKEY, 0.5), door=DEVICE, env=(),
         lag_split=4, reach_last=None, fused=None, lengths=None, aim=None):
    last = block if last is None else last
    c = Case(name, family, ch, bps, block, last, frames, order, window_, door, tuple(env), lag_split, route, reach, reach_last,
             False, 0, None if lengths is None else tuple(lengths), aim)
    if fused is None:                                    # the default declaration: Tukey(0.5) fuses wherever the width allows
        t0, t1 = tiles_of(c)
        fused = t0 < t1 and not reach.startswith(("k_autocorr2", "k_autocorr_ragged"))
    return c._replace(fused=fused)


def _tiles():
    out = []
    for chn, ch, bps in (("stereo", 2, 16), ("3ch", 3, 20)):
        prod = "planar-stereo" if ch == 2 else "planar-indep"
        for n in (32, 64, 96, 128, 160):                 # 1 .. 5 tiles: tile(0) alone, a tail, one pair, a pair and a tail, two pairs
            for order in (4, 8, 12, 16):
                for ns in (4, 2):
                    out.append(case(f"tiles-{chn}-n{n}-o{order}-ns{ns}", "tiles", ch, bps, n, 3, order, "K0_COPY", ac4(order, ns, prod),
                                    lag_split=ns, door=DEVICE if ns == 4 else HOST))
        for n in (64, 128, 192):
            for order in (17, 32):
                out.append(case(f"tiles-deep-{chn}-n{n}-o{order}", "tiles", ch, bps, n, 3, order, "K0_COPY", deep(prod), door=HOST))
        out.append(case(f"tiles-{chn}-n96-o32-falls-to-generic", "tiles", ch, bps, 96, 3, 32, "K0_COPY", ac2(32)))
    out.append(case("tiles-mono-n65504-2047-tiles", "tiles", 1, 24, 65504, 1, 12, "PLANAR_IN_PLACE", ac4(12, 4, "planar-indep")))
    for n in (4608, 16384, 576):
        out.append(case(f"tiles-stereo-n{n}-o12", "tiles", 2, 16, n, 3, 12, "K0_COPY", ac4(12, 4, "planar-stereo")))
    return out


def _groups():
    out = []
    w16 = (TUKEY, find_tukey(FN, "lo", 16))
    # 1024 frames: 64 candidate groups, the last batch of the eight-wave kernel; 1025: 65 groups and a sixteenth of one, the
    # four-wave direct kernel of the benchmark's large batches
    out.append(case("groups-stereo-1024-frames-eight-waves", "groups", 2, 24, FN, 1024, 12, "DIRECT_STEREO", ac4(12, 8, "direct"), window_=w16))
    out.append(case("groups-stereo-1025-frames-four-waves", "groups", 2, 24, FN, 1025, 12, "DIRECT_STEREO", ac4(12, 4, "direct"), window_=w16))
    out.append(case("groups-stereo-17-frames-last-group-one-frame", "groups", 2, 24, FN, 17, 8, "DIRECT_STEREO", ac4(8, 4, "direct")))
    # independent channels: 64 is no multiple of ncand, so the second group starts inside a frame; 5 x 13 = 65: it is one candidate
    for ch, frames in ((3, 23), (5, 13), (6, 11), (7, 10)):      # (3 channels need 22 frames for a second group: the one case above 17)
        split = "SPLIT_XPOSE" if ch in (3, 6) else "SPLIT"
        out.append(case(f"groups-{ch}ch-{frames}-frames-split", "groups", ch, 16, FN, frames, 12, split, ac4(12, 4, "split")))
        out.append(case(f"groups-{ch}ch-{frames}-frames-planar", "groups", ch, 16, FN, frames, 12, "K0_COPY", ac4(12, 4, "planar-indep"),
                        env=("FLACGPU_NO_DIRECT",)))
    out.append(case("groups-5ch-13-frames-generic", "groups", 5, 16, 1000, 13, 12, "K0_COPY", ac2(12)))
    return out


LAG_ORDERS = (1, 4, 5, 8, 9, 12, 13, 16)                 # the last order of one NL and the first of the next


def _lags():
    out = []
    split_ch = dict(zip(LAG_ORDERS, (1, 3, 5, 6, 7, 3, 5, 1)))
    for order in LAG_ORDERS:
        ns = 8 if nl_of(order) == 13 else 4              # (a few frames of NL 13: the eight-wave kernel; 4 waves: groups-...-1025)
        out.append(case(f"lags-direct-4096-o{order}", "lags", 2, 24, FN, 3, order, "DIRECT_STEREO", ac4(order, ns, "direct")))
        ch = split_ch[order]
        route = "SPLIT_XPOSE" if ch in (3, 6) else "SPLIT"
        out.append(case(f"lags-split-{ch}ch-4096-o{order}", "lags", ch, 20, FN, 3, order, route, ac4(order, 4, "split")))
        out.append(case(f"lags-split4-4096-o{order}", "lags", 4, 16, FN, 3, order, "SPLIT_XPOSE", ac4(order, 4, "split4")))
        out.append(case(f"lags-split8-4096-o{order}", "lags", 8, 16, FN, 3, order, "SPLIT_XPOSE", ac4(order, 4, "split8")))
        out.append(case(f"lags-planar-stereo-4096-o{order}", "lags", 2, 24, FN, 3, order, "K0_COPY", ac4(order, 4, "planar-stereo"),
                        env=("FLACGPU_NO_DIRECT",)))
        out.append(case(f"lags-planar-3ch-4096-o{order}", "lags", 3, 20, FN, 3, order, "K0_COPY", ac4(order, 4, "planar-indep"),
                        env=("FLACGPU_NO_DIRECT",), door=HOST))
        for block in (1024, 1152, 2048, 2304):
            out.append(case(f"lags-direct-{block}-o{order}", "lags", 2, 24, block, 3, order, "DIRECT_STEREO", ac4(order, ns, "direct")))
    for order in (4, 8, 12, 16):                         # the two-way lag split at 4096 (it takes the copying K0 path)
        out.append(case(f"lags-planar-stereo-4096-o{order}-ns2", "lags", 2, 24, FN, 3, order, "K0_COPY", ac4(order, 2, "planar-stereo"), lag_split=2))
        out.append(case(f"lags-planar-5ch-4096-o{order}-ns2", "lags", 5, 16, FN, 3, order, "K0_COPY", ac4(order, 2, "planar-indep"), lag_split=2))
    out.append(case("lags-split4-keeps-rows-4096-o12", "lags", 4, 16, FN, 3, 12, "SPLIT", ac4(12, 4, "split4"), env=("FLACGPU_NO_XPOSE",)))
    out.append(case("lags-split8-keeps-rows-4096-o12", "lags", 8, 16, FN, 3, 12, "SPLIT", ac4(12, 4, "split8"), env=("FLACGPU_NO_XPOSE",)))
    return out


def _fused_kernel(block, order):
    """stereo 24-bit, three frames, by the device door"""
    if block == FN:
        if order > 16:
            return "DIRECT_STEREO", deep("direct")
        return "DIRECT_STEREO", ac4(order, 8 if nl_of(order) == 13 else 4, "direct")
    if order > 16:                                       # the shorter wave blocks are read in place up to order 16 only
        return "K0_COPY", deep("planar-stereo")
    return "DIRECT_STEREO", ac4(order, 8 if nl_of(order) == 13 else 4, "direct")


def _fused():
    out = []
    for block in (FN, 1152):
        def add(tag, order, window_, aim, fused):
            route, reach = _fused_kernel(block, order)
            out.append(case(f"fused-{block}-{tag}-o{order}", "fused", 2, 24, block, 3, order, route, reach, window_=window_, fused=fused, aim=aim))

        for r in (15, 16, 17):                           # flat_lo + 16 one short of a tile boundary, on it, one past it
            for order in (12, 16):
                add(f"lo{r}", order, (TUKEY, find_tukey(block, "lo", r)), ("lo", r), True)
        for r in (31, 0, 1):                             # the same under the deep kernel's margin of 32
            add(f"lo{r}", 32, (TUKEY, find_tukey(block, "lo", r)), ("lo", r), True)
        for r in (31, 0, 1):
            for order in (16, 32):
                add(f"hi{r}", order, (TUKEY, find_tukey(block, "hi", r)), ("hi", r), True)
        for order in (12, 32):
            add("flat-run-too-short", order, (TUKEY, find_tukey_unfused(block, order)), ("none",), False)
            add("rectangular", order, (RECT, 0.0), ("rect",), True)
            add("hann", order, (HANN, 0.0), ("hann",), False)
    # the width threshold bps + stereo4 <= 26, mono: 25 and 26 fuse, 27 and 32 do not (at 32 bits the rail products reach 2^62
    # and are inexact: a fused term there would be another number)
    for bps, fused in ((25, True), (26, True), (27, False), (32, False)):
        route = "SPLIT" if bps <= 25 else "PLANAR_IN_PLACE"
        reach = ac4(12, 4, "split" if bps <= 25 else "planar-indep")
        out.append(case(f"fused-4096-mono-{bps}-bits", "fused", 1, bps, FN, 3, 12, route, reach, fused=fused, aim=("width", bps)))
    return out


def generic_lengths(order):
    """{length: [labels]} of the issue's list for this order's H (lengths the reference analyses: > order)"""
    H = h_of(order)
    TS = ts_of(H)
    named = {"order+1": order + 1, "order+2": order + 2, "H-1": H - 1, "H": H, "TS-1": TS - 1, "TS": TS, "TS+1": TS + 1,
             "2TS-1": 2 * TS - 1, "2TS+1": 2 * TS + 1, "31": 31, "33": 33}
    out = {}
    for label, n in named.items():
        if n > order:
            out.setdefault(n, []).append(label)
    return out


GENERIC_ORDERS = (2, 6, 10, 14, 18, 22, 26, 30, 32)      # one order per H (order + 1 = H - 1 keeps the frame inside the FIRST block)
assert [h_of(o) for o in GENERIC_ORDERS] == list(HS)


def _generic_shape(i, block, last, order):
    """mono, stereo and 8 channels in turn; a length k_autocorr4 / _deep would take (a multiple of 32, of 64 above order 16)
    goes as 26-bit stereo, whose four candidates only the generic kernel computes"""
    def tiled(n):
        return n >= 32 and n % (64 if order > 16 else 32) == 0
    if tiled(block) or tiled(last):
        return "stereo26", 2, 26
    return (("mono", 1, 16), ("stereo", 2, 16), ("8ch", 8, 16))[i % 3]


def _generic():
    out = []
    for order in GENERIC_ORDERS:
        lens = sorted(generic_lengths(order))
        lens_big = [n for n in lens if n >= 16]
        k = (len(lens) + 1) // 2
        lasts, blocks = lens[:k], lens[k:]
        for i, last in enumerate(lasts):
            block = blocks[min(i, len(blocks) - 1)]
            if block <= last:
                block = lens_big[-1]
            chn, ch, bps = _generic_shape(i, block, last, order)
            out.append(case(f"generic-o{order}-{chn}-block{block}-last{last}", "generic", ch, bps, block, 3, order, "K0_COPY", ac2(order),
                            last=last, reach_last=ac2(order), door=HOST if i % 2 else DEVICE, aim=("paths",)))
    for order, ch, bps, block, last in ((14, 2, 16, 1000, 33), (14, 8, 16, 4095, 31), (32, 2, 16, 4095, 1000), (14, 1, 16, 1000, 999)):
        out.append(case(f"generic-o{order}-{ch}ch-block{block}-last{last}", "generic", ch, bps, block, 3, order, "K0_COPY", ac2(order),
                        last=last, reach_last=ac2(order), aim=("paths",)))
    return out


def ragged_lengths(order):
    """17 lengths, not sorted: the edges around the order, the 32-sample tile and this H's tile, whole and almost whole blocks,
    and two lengths <= order that the reference does not analyse"""
    TS = ts_of(h_of(order))
    base = [order + 1, 31, 32, 33, TS - 1, TS + 1, 4095, 4096, order, 1]
    lens = base + [33, order + 1, 4096, TS + 1, 31, 2 * TS + 1, order + 2]
    perm = [11, 3, 16, 7, 0, 9, 14, 5, 2, 12, 8, 1, 15, 6, 10, 4, 13]
    return [lens[i] for i in perm]


def _ragged():
    out = []
    for i, order in enumerate(GENERIC_ORDERS):
        chn, ch, bps = (("stereo", 2, 16), ("8ch", 8, 16), ("mono", 1, 24))[i % 3]     # 68, 136 and 17 candidates
        lens = ragged_lengths(order)
        out.append(case(f"ragged-o{order}-{chn}", "ragged", ch, bps, FN, len(lens), order, "K0_COPY", ragged_kernel(order), door=RAGGED,
                        lengths=lens, fused=False))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _tiles() + _groups() + _lags() + _fused() + _generic() + _ragged()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case_named(name):
    return next(c for c in cases() if c.name == name)


def summary():
    cs = cases()
    fam = Counter(c.family for c in cs)
    reached = Counter()
    for c in cs:
        reached[c.reach] += 1
        if c.reach_last and c.reach_last != c.reach:
            reached[c.reach_last] += 1
    return dict(fam), dict(reached)


# what the dispatcher can launch and the matrix must reach (k_autocorr_mfma is not bit-exact by design and is left out)
def every_instantiation():
    out = set()
    for nl_order in (4, 8, 12, 16):
        for prod in ("direct", "split", "split4", "split8", "planar-stereo", "planar-indep"):
            out.add(ac4(nl_order, 4, prod))
        for prod in ("planar-stereo", "planar-indep"):
            out.add(ac4(nl_order, 2, prod))
    out.add(ac4(12, 8, "direct"))
    out |= {deep("direct"), deep("planar-stereo"), deep("planar-indep")}
    out |= {f"k_autocorr2<{h}>" for h in HS} | {f"k_autocorr_ragged<{h}>" for h in HS}
    return out


# ------------------------------------------------------------------------------------------------ the library's hooks (no device)
def _hook(name, vin, nout):
    from flac_codec_amd import _lib

    fn = getattr(_lib.lib(), name)
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    a = (C.c_int32 * len(vin))(*vin)
    out = (C.c_uint32 * nout)()
    fn(a, out)
    return list(out)


KNOB_BITS = {"FLACGPU_NO_DIRECT": 1, "FLACGPU_NO_XPOSE": 32}


def route_of(case):
    """plan_route's input for the case's door"""
    if case.door == RAGGED:
        return "K0_COPY"                                 # (plan_route: a ragged batch is gathered and split by K0; asserted in the C++)
    knobs = sum(KNOB_BITS.get(e, 0) for e in case.env)
    row = [case.ch, case.bps, case.block, case.order, 6, 1, 0, 1, case.last, case.frames, 0, case.lag_split, 0, 0, knobs, -1, 0,
           1 if case.door == DEVICE else 0]
    return ROUTES[_hook("flacenc_plan_route_row", row, 9)[0]]


def kernel_of(case, last_frame=False):
    """(name, fused tiles on, fma_t0, fma_t1) of plan_autocorr for the launch of the case's whole blocks (last_frame: of its
    short last frame)"""
    route = route_of(case)
    stereo4 = 1 if case.ch == 2 and case.bps < 32 else 0
    lo, hi = flat_run(case.window[0], case.window[1], case.block)
    whole = case.last == case.block
    full = case.frames if whole else case.frames - 1
    n, nframes, covers = (case.last, 1, False) if last_frame else (case.block, full, whole)
    row = [ncand_of(case), stereo4, case.ch, case.bps, case.order, n, case.block, int(route == "DIRECT_STEREO"),
           int(route in ("SPLIT", "SPLIT_XPOSE")), case.lag_split, nframes, int(covers), 0, lo, hi,
           int("FLACGPU_NO_AC_FMA" in case.env), int(case.door == RAGGED)]
    family, size, ns, producer, stereo, k4, fused, t0, t1 = _hook("flacenc_plan_autocorr_row", row, 9)
    prod = ("planar-stereo" if stereo else "planar-indep", "direct", "split", "split4", "split8")[producer]
    if family == 0:
        name = f"k_autocorr4<{size},{ns},{prod}>"
        assert bool(k4) == (producer != 0)
    elif family == 1:
        name = f"k_autocorr4_deep<{prod}>"
        assert not k4
    else:
        name = ("k_autocorr2<%d>", "k_autocorr_ragged<%d>", "k_autocorr_mfma<%d>")[family - 2] % size
        assert not k4
    return name, bool(fused), t0, t1


# summary() as it stands: cases per family, cases per reached instantiation
FAMILIES = {'tiles': 98, 'groups': 12, 'lags': 90, 'fused': 46, 'generic': 47, 'ragged': 9}
REACHED = {'k_autocorr2<12>': 5,
 'k_autocorr2<16>': 9,
 'k_autocorr2<20>': 5,
 'k_autocorr2<24>': 5,
 'k_autocorr2<28>': 5,
 'k_autocorr2<32>': 4,
 'k_autocorr2<36>': 7,
 'k_autocorr2<4>': 5,
 'k_autocorr2<8>': 5,
 'k_autocorr4<13,2,planar-indep>': 6,
 'k_autocorr4<13,2,planar-stereo>': 6,
 'k_autocorr4<13,4,direct>': 1,
 'k_autocorr4<13,4,planar-indep>': 15,
 'k_autocorr4<13,4,planar-stereo>': 10,
 'k_autocorr4<13,4,split4>': 3,
 'k_autocorr4<13,4,split8>': 3,
 'k_autocorr4<13,4,split>': 7,
 'k_autocorr4<13,8,direct>': 23,
 'k_autocorr4<17,2,planar-indep>': 6,
 'k_autocorr4<17,2,planar-stereo>': 6,
 'k_autocorr4<17,4,direct>': 22,
 'k_autocorr4<17,4,planar-indep>': 7,
 'k_autocorr4<17,4,planar-stereo>': 7,
 'k_autocorr4<17,4,split4>': 2,
 'k_autocorr4<17,4,split8>': 2,
 'k_autocorr4<17,4,split>': 2,
 'k_autocorr4<5,2,planar-indep>': 6,
 'k_autocorr4<5,2,planar-stereo>': 6,
 'k_autocorr4<5,4,direct>': 10,
 'k_autocorr4<5,4,planar-indep>': 7,
 'k_autocorr4<5,4,planar-stereo>': 7,
 'k_autocorr4<5,4,split4>': 2,
 'k_autocorr4<5,4,split8>': 2,
 'k_autocorr4<5,4,split>': 2,
 'k_autocorr4<9,2,planar-indep>': 6,
 'k_autocorr4<9,2,planar-stereo>': 6,
 'k_autocorr4<9,4,direct>': 11,
 'k_autocorr4<9,4,planar-indep>': 7,
 'k_autocorr4<9,4,planar-stereo>': 7,
 'k_autocorr4<9,4,split4>': 2,
 'k_autocorr4<9,4,split8>': 2,
 'k_autocorr4<9,4,split>': 2,
 'k_autocorr4_deep<direct>': 9,
 'k_autocorr4_deep<planar-indep>': 6,
 'k_autocorr4_deep<planar-stereo>': 15,
 'k_autocorr_ragged<12>': 1,
 'k_autocorr_ragged<16>': 1,
 'k_autocorr_ragged<20>': 1,
 'k_autocorr_ragged<24>': 1,
 'k_autocorr_ragged<28>': 1,
 'k_autocorr_ragged<32>': 1,
 'k_autocorr_ragged<36>': 1,
 'k_autocorr_ragged<4>': 1,
 'k_autocorr_ragged<8>': 1}
