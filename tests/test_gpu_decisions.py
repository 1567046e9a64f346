"""The decision matrix (_decision_matrix.py: exact ties and thresholds one sample apart, each proven on the oracle by
test_decision_matrix_oracle.py) through GpuAnalyzer: encode_frames' bytes are the oracle's, the fetched plans equal the
oracle's field by field (_compare.compare_frame), and verify_device gives the PCM back.  Cases that share block, width,
channels and options are the frames of one call, one case per frame.  The shapes put every case in front of every
kernel family that makes the decision: the generic kernels (64, 192, 2304 as mono, 16384), the wave kernels' PAIR
(1152, fast preset) and SELF (1152, max_lpc 0) instantiations, k_cand64p / k_frame64 (4096, mono and stereo, with and
without LPC -- with LPC the winner may be LPC: parity all the same), k_decide / k_sub64 (4096, the case as channel 5 of
8 with other cases around it), the 4096 set again under each deferral mode of the fixed count and with the wave
kernels switched off."""
import numpy as np
import pytest

import _decision_matrix as dm
import _oracle as orc
from _compare import compare_frame, frames_the_reference_cannot_decode, orc_options_for

pytestmark = pytest.mark.gpu

RATE, FIRST = 48000, 5

# name: (block, max_po, channels, max_lpc, mid_side, exhaustive)
SHAPES = {
    "64-mono": (64, 3, 1, 0, False, False),
    "64-stereo": (64, 3, 2, 0, True, True),
    "192-mono": (192, 3, 1, 0, False, False),
    "192-stereo": (192, 3, 2, 8, True, False),
    "1152-fast-mono": (1152, 3, 1, 0, False, False),
    "1152-fast-stereo": (1152, 3, 2, 0, False, False),
    "1152-self-mono": (1152, 6, 1, 0, True, True),
    "1152-self-stereo": (1152, 6, 2, 0, True, True),
    "2304-mono": (2304, 6, 1, 0, True, True),
    "4096-mono-fixed": (4096, 6, 1, 0, True, True),
    "4096-mono-lpc": (4096, 6, 1, 12, True, True),
    "4096-stereo-fixed": (4096, 6, 2, 0, True, True),
    "4096-stereo-lpc": (4096, 6, 2, 12, True, True),
    "4096-8ch": (4096, 6, 8, 0, True, True),
    "16384-mono": (16384, 6, 1, 0, True, True),
}
SET_4096 = [s for s in SHAPES if s.startswith("4096")]

_expected = {}


def batches(shape):
    """[(bps, max_po, [case], planar frames)]: frame f holds case f at its home channel (5 of 8, else 0) and the cases
    3, 6, ... places on around it."""
    block, max_po, channels = SHAPES[shape][:3]
    groups = {}
    for case in dm.mono_cases(block, max_po):
        groups.setdefault((case.bps, case.max_po), []).append(case)
    home = 5 if channels == 8 else 0
    out = []
    for (bps, po), cases in sorted(groups.items()):
        frames = [np.stack([cases[(f + 3 * (c - home)) % len(cases)].planar[0] for c in range(channels)])
                  for f in range(len(cases))]
        out.append((bps, po, cases, frames))
    return out


def expected(key, opts, bps, frames):
    if key not in _expected:
        enc = [orc.encode_frame(opts, RATE, bps, planar, frame_number=FIRST + f) for f, planar in enumerate(frames)]
        assert all(rc == 0 for rc, _, _ in enc)
        _expected[key] = [(data, plan) for _, data, plan in enc]
    return _expected[key]


def run_batch(key, cases, frames, block, max_po, channels, max_lpc, mid_side, exhaustive, bps):
    from flac_codec_amd.gpu import GpuAnalyzer

    n = len(frames)
    want = expected(key, orc_options_for(block, max_po, max_lpc, mid_side, exhaustive), bps, frames)
    pcm = np.ascontiguousarray(np.stack(frames).transpose(0, 2, 1)).reshape(-1)
    an = GpuAnalyzer(block, max_po, max_lpc, mid_side, exhaustive, 2, 0.5, bps, channels, max_frames=n)
    try:
        data, off = an.encode_frames(pcm, n, block, FIRST, RATE)
        for f in range(n):
            assert data[off[f]:off[f + 1]] == want[f][0], f"{key}: {cases[f]} (frame {f}): bytes differ from the oracle's"
        res, _ = an.verify_device(RATE, FIRST)
        plans, subs, rows = an.analyze(pcm, n, block)
        undecodable = frames_the_reference_cannot_decode(subs, n, channels, block, block)
        assert not undecodable, f"{key}: {[cases[f] for f in undecodable]}"
        assert (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs, res.samples_differ) == (n, 0, 0, 0, 0), key
        assert np.array_equal(an.fetch_decoded(n, block), pcm), key
        for f in range(n):
            compare_frame(plans[f], subs[f * channels:(f + 1) * channels], rows[f], want[f][1], frames[f], block,
                          where=f"{key}: {cases[f]} (frame {f})")
    finally:
        an.close()


def run_shape(shape):
    block, max_po, channels, max_lpc, mid_side, exhaustive = SHAPES[shape]
    total = 0
    for bps, po, cases, frames in batches(shape):
        run_batch((shape, bps, po), cases, frames, block, po, channels, max_lpc, mid_side, exhaustive, bps)
        total += len(cases)
    assert total == len(dm.mono_cases(block, max_po))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_case_at_every_shape(shape):
    run_shape(shape)


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_the_4096_set_under_each_deferral_mode(monkeypatch, mode):
    """FLACGPU_DEFER_FIXED (test_gpu_taps.py::test_deferred_fixed_count_gives_the_same_bytes): the FIXED half's exact
    count put off never, by the estimate, or whenever LPC parameters exist."""
    monkeypatch.setenv("FLACGPU_DEFER_FIXED", mode)
    for shape in SET_4096:
        run_shape(shape)


def test_the_4096_set_through_the_generic_kernels(monkeypatch):
    monkeypatch.setenv("FLACGPU_NO_W64", "1")
    monkeypatch.setenv("FLACGPU_NO_FRAME64", "1")
    for shape in SET_4096:
        run_shape(shape)


@pytest.mark.parametrize("max_lpc", [0, 12])
@pytest.mark.parametrize("block,max_po", dm.STEREO_SHAPES)
def test_channel_assignment_ties(block, max_po, max_lpc):
    """L == R, R == 0, R == -L, R == -L - 1, the equal-bits pair and the wasted-bit pairs, exhaustive on and off and
    mid_side on and off: the earlier assignment on equal totals."""
    cases = dm.stereo_cases(block, max_po)
    frames = [c.planar for c in cases]
    for exhaustive in (True, False):
        for mid_side in (True, False):
            run_batch(("assignment", block, max_po, max_lpc, exhaustive, mid_side), cases, frames, block, max_po, 2, max_lpc,
                      mid_side, exhaustive, 16)


def test_sum_of_2_to_the_30_in_a_65535_sample_block():
    """16 bits: escape_bits = ilog2(sum) + 2 is 31 at sum 2^30 - 1 and does not exist at 2^30 (the fallback partition)."""
    cases = dm.big_block_cases()
    run_batch(("65535",), cases, [c.planar for c in cases], 65535, 6, 1, 0, False, False, 16)
