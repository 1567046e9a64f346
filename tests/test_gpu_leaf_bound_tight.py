"""The tight lower bound of the FIXED size on the device (Params::defer_fixed, kernels/wave_cand_fixed.inc): where the leaf sums'
bound does not reach the LPC estimate, the candidate wave takes one more pass over its FIXED residual for two exact quotient sums
per leaf, and an exact `lpc_bits < bound` then skips the FIXED half's partition tree and exact count.  Whatever defers, is decided
or re-fetches, the frames must be the ORACLE's bytes; the counters (GpuAnalyzer.stats(): fixed_decided = skipped,
fixed_refetched) show which paths ran.  Stereo, 24 bits, 4096-sample blocks, 64 frames a case, LPC order 12 and 32.

Shares (of the 4 candidates of every frame, by the LPC estimate: mode 1, the default):
  AR(2), the bench's signal   tools/leaf_bound_tight.py finds `bound > exact LPC bits` for 256 of 256 candidates of the bench's first
                              64 frames (profiles/leaf_bound_tight.json; the leaf sums' bound: 0); the estimate's margin may
                              keep a few points of them from deferring: at least 0.95
  high-order (synth_hi)       at least what the build before the tight bound skipped on the same frames (PARENT_HI below)
  white noise                 nothing defers
Modes 0 (never), 2 (every candidate with LPC parameters, leaf sums' bound) and 3 (the same, tight bound) and FLACGPU_NO_HAND are run
on a mixture; the near-tie frames -- an AR(2) frame under dither scaled until FIXED and LPC are a handful of bits apart -- are
proved on the CPU first (both sizes restated in tests/_leaf_bound_tight.py and held to the oracle's)."""
import functools

import numpy as np
import pytest

import _leaf_bound_tight as lbt
import _oracle as orc
from _compare import orc_options_for, planar_frames
from _pcm import synth_fast, synth_hi

pytestmark = pytest.mark.gpu
B, BPS, FRAMES, RATE = 4096, 24, 64, 48000
BENCH_SEED, BENCH_DISTINCT = 1000 + 16 * 3, 512        # bench.py: config 3, context 0
AR2_CPU_SHARE = 1.0                                    # profiles/leaf_bound_tight.json, tight_bound_share of "ar2"
MARGIN_POINTS = 0.05
# fixed_decided of the parent build (leaf sums' bound only) on signal("hi"), of 256 candidates: measured once on an MI355X
PARENT_HI = {12: 182, 32: 183}
HANDFUL = 16                                           # bits


@functools.lru_cache(maxsize=None)
def signal(name):
    if name == "ar2":      # the first frames of the bench's distinct frames
        x = synth_fast(BENCH_SEED, 2, BPS, B * BENCH_DISTINCT)
    elif name == "hi":
        x = synth_hi(BENCH_SEED, 2, BPS, B * BENCH_DISTINCT, sections=6)
    elif name == "noise":
        rng = np.random.Generator(np.random.PCG64(77))
        x = rng.integers(-(1 << (BPS - 1)), 1 << (BPS - 1), size=2 * B * FRAMES)
    else:                  # "mix": both kinds in one batch
        x = np.concatenate([signal("ar2")[:B * FRAMES], signal("hi")[:B * FRAMES]])
    x = np.ascontiguousarray(x[:2 * B * FRAMES], dtype=np.int32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle_frames(name, max_lpc):
    oopts = orc_options_for(B, 6, max_lpc, True, True)
    out = []
    for f, planar in enumerate(planar_frames(pcm_of(name), 2, B)):
        rc, fb, _ = orc.encode_frame(oopts, RATE, BPS, planar, frame_number=f)
        assert rc == 0
        out.append(fb)
    return out


def gpu_frames(pcm, max_lpc):
    from flac_codec_amd.gpu import GpuAnalyzer

    n = pcm.size // (2 * B)
    an = GpuAnalyzer(B, 6, max_lpc, True, True, 2, 0.5, BPS, 2, max_frames=n)
    data, off = an.encode_frames(pcm, n, B, 0, RATE)
    st = an.stats()
    handed = an.handed_subframes()
    an.close()
    return [bytes(data[off[f]:off[f + 1]]) for f in range(n)], st, handed


def check(name, max_lpc):
    got, st, handed = gpu_frames(pcm_of(name), max_lpc)
    want = oracle_frames(name, max_lpc)
    print(f"leaf_bound_tight {name} lpc {max_lpc}: skipped {st.fixed_decided} refetched {st.fixed_refetched} "
          f"of {4 * len(want)} candidates, handed {handed}")
    for f in range(len(want)):
        assert got[f] == want[f], f"{name}, LPC order {max_lpc}: frame {f} differs from the oracle"
    return st, handed, 4 * len(want)


def clean(monkeypatch):
    for k in ("FLACGPU_DEFER_FIXED", "FLACGPU_DEFER_MARGIN16", "FLACGPU_NO_HAND"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("max_lpc", [12, 32])
@pytest.mark.parametrize("name", ["ar2", "hi", "noise"])
def test_share_by_the_estimate(monkeypatch, name, max_lpc):
    clean(monkeypatch)
    st, _, cands = check(name, max_lpc)
    deferred = st.fixed_decided + st.fixed_refetched          # every wave that defers ends in exactly one of the two
    assert deferred <= cands
    if name == "ar2":
        assert st.fixed_decided >= (AR2_CPU_SHARE - MARGIN_POINTS) * cands, (st.fixed_decided, cands)
    elif name == "hi":
        assert st.fixed_decided >= PARENT_HI[max_lpc], (st.fixed_decided, PARENT_HI[max_lpc])
    else:
        assert deferred == 0, (st.fixed_decided, st.fixed_refetched)


@pytest.mark.parametrize("mode", ["0", "2", "3"])
def test_modes_on_a_mixture(monkeypatch, mode):
    clean(monkeypatch)
    monkeypatch.setenv("FLACGPU_DEFER_FIXED", mode)
    st, _, cands = check("mix", 12)
    deferred = st.fixed_decided + st.fixed_refetched
    if mode == "0":
        assert deferred == 0
    else:
        assert deferred == cands                  # every candidate of these signals has LPC parameters, and all of them defer
        if mode == "3":                           # (2: the leaf sums' bound leaves the AR(2) half to the re-fetch)
            assert st.fixed_decided >= (AR2_CPU_SHARE - MARGIN_POINTS) * (cands // 2)


def test_without_the_hand_over(monkeypatch):
    clean(monkeypatch)
    monkeypatch.setenv("FLACGPU_NO_HAND", "1")
    st, handed, cands = check("ar2", 12)
    assert handed[0] == 0 and not handed[2]
    assert st.fixed_decided + st.fixed_refetched <= cands
    assert st.fixed_decided >= (AR2_CPU_SHARE - MARGIN_POINTS) * cands


# ---- near ties
def ar2_under_dither(seed, g):
    """the generator's AR(2) resonator under uniform dither of amplitude g: the larger g, the less LPC gains"""
    from scipy.signal import lfilter

    rng = np.random.Generator(np.random.PCG64(seed))
    e = rng.uniform(-float(1 << (BPS - 9)), float(1 << (BPS - 9)), size=B + 512)
    y = np.rint(lfilter([1.0], [1.0, -58000 / 32768.0, 29491 / 32768.0], e))[512:].astype(np.int64)
    d = np.rint(g * rng.uniform(-1, 1, size=B)).astype(np.int64)
    return np.clip(y + d, -(1 << (BPS - 1)), (1 << (BPS - 1)) - 1).astype(np.int32)


TIE_SEEDS, TIE_SCALES = range(1, 9), (0.7e6, 1e6, 1.4e6, 2e6, 2.8e6, 4e6, 5.6e6)


@functools.lru_cache(maxsize=None)
def near_ties(max_lpc):
    """(channels LPC wins by 1..HANDFUL bits, channels FIXED wins by 0..HANDFUL bits), each proved with the oracle: its plan
    must be the winner named here at the smaller of the two sizes computed here"""
    oopts = orc_options_for(B, 6, max_lpc, True, True)
    lpc_by, fixed_by = [], []
    for seed in TIE_SEEDS:
        for g in TIE_SCALES:
            x = ar2_under_dither(seed, g)
            fb = lbt.fixed_subframe_bits(x, BPS)
            lb = lbt.lpc_subframe_bits(orc, oopts, x, BPS)
            if lb is None or abs(fb - lb) > HANDFUL:
                continue
            rc, _, plan = orc.encode_frame(oopts, RATE, BPS, x[None, :])
            assert rc == 0
            sub = plan.sub[0]
            if lb < fb:
                assert sub.type == orc.SUB_LPC and sub.bits == lb, (seed, g, sub.type, sub.bits, lb, fb)
                lpc_by.append(x)
            else:
                assert sub.type == orc.SUB_FIXED and sub.bits == fb, (seed, g, sub.type, sub.bits, lb, fb)
                fixed_by.append(x)
    return lpc_by, fixed_by


@functools.lru_cache(maxsize=None)
def tie_pcm(max_lpc):
    lpc_by, fixed_by = near_ties(max_lpc)
    assert len(lpc_by) >= 4 and len(fixed_by) >= 4, (len(lpc_by), len(fixed_by))
    frames = []
    for a in lpc_by + fixed_by:                  # the channel with itself: left, right and mid are the near tie, side is silent
        frames.append(np.stack([a, a], axis=1))
    for a, b in zip(lpc_by, fixed_by):           # one of each kind in a frame
        frames.append(np.stack([a, b], axis=1))
        frames.append(np.stack([b, a], axis=1))
    x = np.ascontiguousarray(np.concatenate(frames).reshape(-1), dtype=np.int32)
    x.setflags(write=False)
    return x


def pcm_of(name):
    if isinstance(name, tuple):
        return tie_pcm(name[1])
    return signal(name)


@pytest.mark.parametrize("mode", ["1", "2", "3"])
@pytest.mark.parametrize("max_lpc", [12, 32])
def test_near_ties_either_way(monkeypatch, mode, max_lpc):
    clean(monkeypatch)
    monkeypatch.setenv("FLACGPU_DEFER_FIXED", mode)
    st, _, cands = check(("ties", max_lpc), max_lpc)
    lpc_by, fixed_by = near_ties(max_lpc)
    deferred = st.fixed_decided + st.fixed_refetched
    assert deferred <= cands
    if mode != "1":
        # every near-tie candidate defers; no bound can decide for LPC where FIXED is not the larger: three candidates of the
        # frames made of such a channel alone, one of each mixed frame
        assert deferred >= 3 * (len(lpc_by) + len(fixed_by))
        assert st.fixed_refetched >= 3 * len(fixed_by) + 2 * min(len(lpc_by), len(fixed_by))
