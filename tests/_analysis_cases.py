"""The frames behind test_frame_analysis_host.py (CPU) and test_gpu_frame_analysis.py (GPU), with the two references
that are independent of the code under test (TEST INFRASTRUCTURE ONLY):

  syn_cases()     frames written by _flacsyn from explicit choices, the Frame objects kept: the analysis must return
                  exactly the choices that were written (check_choices).  These hold what the encoder never writes:
                  more than 64 partitions (FLACGPU_AN_PARTS_CLIPPED) and 33-bit side channels (FLACGPU_AN_WIDE).
  oracle_cases()  frames written by the oracle (orc.encode_frame), each with the oracle's own plan and the planar PCM:
                  the analysis must pass _compare.compare_frame against that plan.

Every case is one stream (all its frames share rate, sample size and channels) at the smallest shape that reaches its
branch, at most 8 frames.  A case has .name, .rate, .bps, .channels, .frame_bytes, .sizes, .blob (a .flac container:
marker, STREAMINFO without MD5, the frames) and .raw (the frames alone); syn cases add .frames (the _flacsyn Frames),
oracle cases .plans and .planar.  Both lists are cached and never modified by a test.
"""
import functools
import random
from types import SimpleNamespace

import numpy as np

import _flacsyn as fs
import _foreign_matrix as fm
import _oracle as orc

KIND_OF_TYPE = {0: "constant", 1: "verbatim", 2: "fixed", 3: "lpc"}


def _case(name, rate, bps, channels, frame_bytes, sizes, **kw):
    si = fs.Bits()
    si.put(16, min(max(sizes), 65535))   # a fixed-blocksize stream: only its last frame may be shorter
    si.put(16, min(max(sizes), 65535))
    si.put(24, 0)
    si.put(24, 0)
    si.put(20, rate)
    si.put(3, channels - 1)
    si.put(5, bps - 1)
    si.put(36, sum(sizes))
    raw = b"".join(frame_bytes)
    blob = b"fLaC" + fs.metadata_block(0, si.getvalue() + bytes(16), last=True) + raw
    return SimpleNamespace(name=name, rate=rate, bps=bps, channels=channels, frame_bytes=list(frame_bytes),
                           sizes=list(sizes), blob=blob, raw=raw, **kw)


# ---- (a) explicit choices ---------------------------------------------------------------------------------------
def _syn(name, rate, bps, frames):
    feats = set()
    coded = [fs.write_frame(rate, bps, f, feats) for f in frames]
    return _case(name, rate, bps, len(frames[0].pcm), coded, [f.n for f in frames], frames=frames)


def _mono_frames(items, rate, blocking=1):
    """Frames whose headers code their own sample rate and size, so that a raw frame scan keeps them."""
    frames, at = [], 0
    for k, (v, sub) in enumerate(items):
        frames.append(fs.Frame([v], [sub], blocking=blocking, number=at if blocking else k, rcode=fs.RATE_CODES[rate]))
        at += len(v)
    return frames


@functools.lru_cache(maxsize=1)
def syn_cases():
    rng = random.Random(2501)
    out = []
    # every kind, with wasted bits, both methods, escapes of several widths (0 included) beside Rice partitions
    items = [([-77] * 5, fs.constant()), ([12 << 3] * 17, fs.constant(wasted=3)),
             ([rng.randint(-30000, 30000) for _ in range(17)], fs.verbatim()),
             ([rng.randint(-3000, 3000) << 2 for _ in range(5)], fs.verbatim(wasted=2))]
    sub = fs.fixed(3, method=1, porder=2)
    v = fm._predicted(rng, 16, 16, sub)
    items.append((v, fm.fit_k(v, sub)))
    sub = fs.fixed(2, wasted=1, porder=3, params=(3, ("escape", 9), 0, ("escape", 0), 5, ("escape", 12), 2, 14))
    v = _with_zero_partition(rng, 64, 16, sub, zero_part=3)
    items.append((v, sub))
    sub = fs.lpc(8, 12, 10, fm.small_coefs(rng, 8), porder=1, method=1)
    v = fm._predicted(rng, 32, 16, sub)
    items.append((v, fm.fit_k(v, sub)))
    sub = fs.lpc(32, 15, 14, fm.small_coefs(rng, 32, 15, 14))
    v = fm._predicted(rng, 33, 16, sub)
    items.append((v, fm.fit_k(v, sub)))
    out.append(_syn("syn-kinds", 44100, 16, _mono_frames(items, 44100)))

    # more than 64 partitions: 2^7 of two samples each and 2^8 of one; parameters differ beyond entry 63 as well
    items = []
    for po, n, order in ((7, 256, 1), (8, 256, 0), (7, 128, 1)):
        sub = fs.fixed(order, porder=po, method=po & 1)
        v = fm._predicted(rng, n, 16, sub, amp=200)
        fm.fit_k(v, sub)
        params = list(sub["params"])
        for part in (1, 63, 64, 65, (1 << po) - 1):
            params[part] = ("escape", 10)
        sub["params"] = tuple(params)
        items.append((v, sub))
    out.append(_syn("syn-clipped", 48000, 16, _mono_frames(items, 48000, blocking=0)))

    # 33-bit side channels: every assignment, every kind, values that need the 33rd bit
    sb = 33
    frames, at = [], 0
    for a in (8, 9, 10):
        specs = [([fm.HI[sb]] * 5, fs.constant()),
                 ([rng.randint(fm.LO[sb] + 1, fm.HI[sb]) for _ in range(17)], fs.verbatim()),
                 ([rng.randint(fm.LO[sb - 2] + 1, fm.HI[sb - 2]) << 2 for _ in range(5)], fs.verbatim(wasted=2))]
        for sub, n in ((fs.fixed(2, method=1), 17), (fm._unit_lpc(rng, 3, method=1, porder=2), 16)):
            level = fm.HI[sb] if a != 9 else fm.LO[sb] + 1
            v = [level - (1 if a != 9 else -1) * rng.randint(0, 1 << 20) for _ in range(n)]
            v[0] = level
            specs.append((v, fm.fit_k(v, sub)))
        for side, sub in specs:
            left, right = fm.stereo_from_side(rng, side, 32)
            subs = [fs.verbatim(), fs.verbatim()]
            subs[fs.SIDE_OF[a]] = sub
            frames.append(fs.Frame([left, right], subs, assignment=a, blocking=1, number=at, rcode=fs.RATE_CODES[96000]))
            at += len(side)
    out.append(_syn("syn-wide-a", 96000, 32, frames[:8]))
    out.append(_syn("syn-wide-b", 96000, 32, frames[8:]))
    return tuple(out)


@functools.lru_cache(maxsize=1)
def raw_invalid_cases():
    """_foreign_matrix.invalid_cases() written again with headers that code their own sample rate: the matrix's frames
    leave the rate to the STREAMINFO, so a raw frame scan passes them over, and decode_frames -- which gives a status
    per frame -- never sees them.  Same malformed subframes (fmx.INVALID), same shapes, one between two valid frames."""
    rng = random.Random(77)
    out = []
    for reason, kw, kind in fm.INVALID:
        n = 100 if kw.get("invalid") == "porder_nodiv" else 16
        frames = []
        for k in range(3):
            if k != 1:
                sub = fs.fixed(2)
                v = fm._predicted(rng, 192, 16, sub)
                frames.append(fs.Frame([v], [fm.fit_k(v, sub)], number=k, rcode=9))
                continue
            if kind == "lpc":
                sub = fs.lpc(8, 12, 10, fm.small_coefs(rng, 8), **kw)
            elif kind == "fixed":
                sub = fs.fixed(2, **kw)
            else:
                sub = fs.verbatim(**kw)
            v = fm._predicted(rng, n, 16, sub, amp=12) if kind != "verbatim" else [rng.randint(-99, 99) for _ in range(n)]
            frames.append(fs.Frame([v], [sub], number=k, rcode=9))
        out.append(_syn("raw invalid: " + reason, 44100, 16, frames))
    return tuple(out)


def _with_zero_partition(rng, n, bps, sub, zero_part):
    """A signal of n samples that `sub`'s predictor follows with small residuals, and exactly in partition zero_part."""
    order, po, wasted = sub["order"], sub["porder"], sub["wasted"]
    coefs = fs.FIXED_COEFS[order]
    plen = n >> po
    v = [rng.randint(-100, 100) for _ in range(order)]
    for i in range(order, n):
        s = sum(a * b for a, b in zip(v[i - order:i], coefs[::-1]))
        v.append(s + (0 if i // plen == zero_part else rng.randint(-60, 60)))
    assert max(abs(x) for x in v) < 1 << (bps - wasted - 1)
    return [x << wasted for x in v]


def check_choices(model, frame, where=""):
    """The model's parse of a written frame against the choices _flacsyn was given."""
    assert model is not None, f"{where} did not parse"
    assert (model.acode, model.n, model.channels) == (frame.assignment, frame.n, len(frame.pcm)), f"{where} header"
    for c, (m, sub) in enumerate(zip(model.subs, frame.subs)):
        w = f"{where} ch{c}"
        assert KIND_OF_TYPE[m.type] == sub["kind"], f"{w} kind"
        assert m.wasted == sub["wasted"], f"{w} wasted"
        if sub["kind"] in ("constant", "verbatim"):
            continue
        assert m.order == sub["order"], f"{w} order"
        if sub["kind"] == "lpc":
            assert (m.precision, m.shift) == (sub["precision"], sub["shift"]), f"{w} precision / shift"
            assert tuple(m.coeffs[:m.order]) == tuple(sub["coefs"]), f"{w} coefs"
        assert (m.coding_method, m.partition_order) == (sub["method"], sub["porder"]), f"{w} method / porder"
        assert tuple(m.all_params) == tuple(sub["params"]), f"{w} params"


# ---- (b) the oracle -------------------------------------------------------------------------------------------------
def _tone(rng, n, bps, noise=0.002, freqs=(0.031, 0.11)):
    t = np.arange(n)
    x = sum(np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) for f in freqs) / len(freqs)
    x = x * 0.4 + rng.normal(0, noise, n)
    return np.clip(np.round(x * (1 << (bps - 1))), -(1 << (bps - 1)), (1 << (bps - 1)) - 1).astype(np.int32)


def _oracle_case(name, bps, frames, rate=44100, **opt):
    """frames: planar int32 arrays [C][n]; the first one's n is the stream's block size."""
    block = max(frames[0].shape[1], 16)
    o = dict(block_size=block, max_partition_order=6, max_lpc_order=8, mid_side=0, exhaustive=0)
    o.update(opt)
    opts = orc.options("default", **o)
    coded, plans = [], []
    for k, planar in enumerate(frames):
        rc, data, plan = orc.encode_frame(opts, rate, bps, planar, frame_number=k)
        assert rc == 0 and data, f"{name}: the oracle refused frame {k} (rc {rc})"
        coded.append(data)
        plans.append(plan)
    return _case(name, rate, bps, frames[0].shape[0], coded, [f.shape[1] for f in frames], plans=plans,
                 planar=[np.ascontiguousarray(f, dtype=np.int32) for f in frames], options=o)


def reached(case, what):
    """The set of `what` over a case's subframes: an attribute of the oracle's subframe plans, or "assignment"."""
    if what == "assignment":
        return {p.assignment for p in case.plans}
    return {getattr(p.sub[c], what) for p in case.plans for c in range(case.channels)}


@functools.lru_cache(maxsize=1)
def oracle_cases():
    rng = np.random.default_rng(2502)
    out = []
    mono = lambda n, bps=16, **kw: _tone(rng, n, bps, **kw)[None, :]
    # block sizes; below 16 a frame is the short last frame behind one of 16
    for n in (1, 2, 3, 5):
        out.append(_oracle_case(f"n={n}", 16, [mono(16), mono(n)]))
    for n in (16, 17, 192):
        out.append(_oracle_case(f"n={n}", 16, [mono(n), mono(n)]))
    # 4096: an envelope that changes 2^6 times makes every finer partitioning pay, up to the 64 partitions allowed
    x = _tone(rng, 4096, 16, noise=0.0).astype(np.float64)
    env = np.repeat(2.0 ** rng.integers(-9, 0, 64), 64)
    y = np.round(x * 0.2 + rng.normal(0, 1, 4096) * env * 8000).astype(np.int32)
    c = _oracle_case("n=4096 po6", 16, [y[None, :]])
    assert 64 in reached(c, "n_partitions"), reached(c, "n_partitions")
    out.append(c)
    out.append(_oracle_case("n=4608 + short", 16, [mono(4608), mono(1000)]))
    # stereo: each of the four assignments
    # a smooth channel (a slow sine: FIXED follows it), and two independent noises
    a = np.round(12000 * np.sin(2 * np.pi * 0.004 * np.arange(192))).astype(np.int64)
    n1, n2 = rng.integers(-300, 300, 192), rng.integers(-300, 300, 192)
    pair = lambda l, r: np.stack([l, r]).astype(np.int32)
    for name, planar, want in (
            ("left/side", pair(a, a + n1), 8),                   # the clean left is cheaper than mid = left + noise / 2
            ("side/right", pair(a + n1, a), 9),
            ("mid/side correlated", pair(a + n1, a + n2), 10),   # independent noises halve in the mid channel
            ("mid/side anti-correlated", pair(a + n1, -a - n1), 10),   # the mid channel is silence
            ("independent: one silent channel", pair(a + n1, 0 * a), 0)):
        c = _oracle_case("stereo " + name, 16, [planar, planar[:, ::-1].copy()][:1], mid_side=1, exhaustive=1)
        assert reached(c, "assignment") == {want}, (name, reached(c, "assignment"))
        out.append(c)
    out.append(_oracle_case("8 channels", 16, [np.stack([_tone(rng, 192, 16) for _ in range(8)])] * 2))
    for bps in (8, 24, 32):
        c = _oracle_case(f"{bps} bits", bps, [np.stack([_tone(rng, 192, bps, noise=0.01) for _ in range(2)])])
        assert reached(c, "coding_method") == {1 if bps > 16 else 0}
        out.append(c)
    # predictors
    # (an AR(1) process, and k sinusoids, which take an order of 2k to predict)
    x = np.zeros(192)
    e = rng.normal(0, 800, 192)
    for i in range(1, 192):
        x[i] = 0.6 * x[i - 1] + e[i]

    def tones(n, k):
        t = np.arange(n)
        y = sum(np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) for f in 0.05 + 0.4 * np.arange(k) / k) / k * 0.5
        return np.round((y + rng.normal(0, 1e-4, n)) * 32767).astype(np.int32)[None, :]

    for order, planar in ((1, np.round(x).astype(np.int32)[None, :]), (8, tones(192, 4)), (32, tones(4096, 12))):
        c = _oracle_case(f"lpc order {order}", 16, [planar], max_lpc_order=order)
        assert (orc.SUB_LPC, order) in {(p.sub[0].type, p.sub[0].order) for p in c.plans}, c.plans[0].sub[0].order
        out.append(c)
    c = _oracle_case("fixed only", 16, [mono(192), mono(192)], max_lpc_order=0)
    assert reached(c, "type") == {orc.SUB_FIXED}
    out.append(c)
    c = _oracle_case("silence", 16, [np.zeros((2, 192), dtype=np.int32)])
    assert reached(c, "type") == {orc.SUB_CONSTANT}
    out.append(c)
    c = _oracle_case("full-scale noise", 16, [rng.integers(-32768, 32768, (1, 192)).astype(np.int32)])
    assert reached(c, "type") == {orc.SUB_VERBATIM}
    out.append(c)
    c = _oracle_case("two wasted bits", 16, [mono(192, 14) << 2])
    assert reached(c, "wasted") == {2}
    out.append(c)
    click = np.zeros((1, 192), dtype=np.int32)
    click[0, 100] = 20000
    c = _oracle_case("a click in silence", 16, [click])
    assert any(p.sub[0].rice[i] == 0xFF for p in c.plans for i in range(p.sub[0].n_partitions)), "no escaped partition"
    out.append(c)
    return tuple(out)
