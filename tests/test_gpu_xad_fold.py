"""The candidate kernels' order statistics with the second and third differences formed by v_xad_u32 (bias 2^31 - 1,
kernels/wave_cand_fixed.inc) and the pair form of wave_rice_fold<SIGNS> (kernels/wave_cand.inc), against the ORACLE's bytes:
batches of 16 frames (one autocorrelation group) whose signals sit at the edges of the range argument -- a side candidate of
25 bits swinging over its whole range every sample, full-scale constants, a silent channel, wasted bits, ramps, an impulse --
beside inputs that LPC wins (the fold, the hand-over).  One batch per kernel instantiation that includes the two files:
k_cand64p<64,16> (stereo, 4096), its SELF form (LPC off), <64,32> (orders up to 32), <18,16> (1152 samples) and
k_cand64<64,16,false,4> (8 channels).  The arithmetic itself is checked on the CPU in tests/test_xad_fold_math.py."""
import numpy as np
import pytest

import _oracle as orc
from _compare import orc_options_for, planar_frames
from _pcm import synth_fast, synth_hi

pytestmark = pytest.mark.gpu
N_FRAMES = 16


def extreme_pair(bps, B, n_frames, seed):
    """[n_frames * B, 2] int64: one extreme signal per frame, the rest LPC material (synth_hi, orders 2-12)"""
    hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.arange(B, dtype=np.int64)
    x = synth_hi(seed, 2, bps, B * n_frames, segment=B, orders=[2, 12, 5, 8]).reshape(-1, 2).astype(np.int64)
    alt = np.where(k & 1, lo, hi)
    frames = [
        (alt, hi + lo - alt),                                    # L = -R - 1 = full scale: side swings +-(2^bps - 1) every sample
        (np.full(B, lo), np.full(B, hi)),                        # side = -2^bps + 1, constant
        (alt, np.zeros(B, dtype=np.int64)),                      # full-scale alternation beside a silent channel
        (alt, alt),                                              # side zero, mid at the rails
        ((x[3 * B:4 * B, 0] >> 3) << 3, (x[3 * B:4 * B, 1] >> 3) << 3),   # three wasted bits on every candidate
        (k * ((hi - lo) // B) + lo, hi - k * ((hi - lo) // B)),  # full-range ramps, opposite
        (np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)),
        (np.where(k == 70, lo, 0), np.where(k == B - 1, hi, 0)), # single impulses
        (rng.integers(lo, hi + 1, size=B), rng.integers(lo, hi + 1, size=B)),         # full-scale noise
        (rng.integers(-(1 << 15), 1 << 15, size=B), rng.integers(-(1 << 15), 1 << 15, size=B)),   # 16-bit noise
        (np.where((k // 64) & 1, lo, hi), np.where((k // 3) & 1, hi, lo)),            # rail-to-rail steps
    ]
    for f, (l, r) in enumerate(frames[:n_frames - 3]):           # (frames 11.. stay LPC material)
        x[(f + 1) * B:(f + 2) * B, 0] = l
        x[(f + 1) * B:(f + 2) * B, 1] = r
    return np.clip(x, lo, hi)


def gpu_and_oracle(pcm, channels, bps, B, max_lpc, rate=48000, first=3):
    from flac_codec_amd.gpu import GpuAnalyzer

    pcm = np.ascontiguousarray(pcm.reshape(-1), dtype=np.int32)
    n = pcm.size // (channels * B)
    an = GpuAnalyzer(B, 6, max_lpc, True, True, 2, 0.5, bps, channels, max_frames=n)
    data, off = an.encode_frames(pcm, n, B, first, rate)
    handed = an.handed_subframes()
    an.close()
    oopts = orc_options_for(B, 6, max_lpc, True, True)
    types = []
    for f, planar in enumerate(planar_frames(pcm, channels, B)):
        rc, fb, plan = orc.encode_frame(oopts, rate, bps, planar, frame_number=first + f)
        assert rc == 0
        assert bytes(data[off[f]:off[f + 1]]) == fb, f
        types += [plan.sub[c].type for c in range(channels)]
    return types, handed


def test_stereo_24bit_extremes(monkeypatch):
    monkeypatch.delenv("FLACGPU_NO_HAND", raising=False)
    types, (handed, subs, on) = gpu_and_oracle(extreme_pair(24, 4096, N_FRAMES, 5100), 2, 24, 4096, 12)
    assert on and subs == 2 * N_FRAMES and 0 < handed < subs
    assert len(set(types)) >= 3                                  # the oracle's plans are mixed: FIXED and LPC both win


def test_stereo_16bit_lpc_off():
    """max LPC order 0: the SELF instantiation, whose whole analysis is the order statistics"""
    types, _ = gpu_and_oracle(extreme_pair(16, 4096, N_FRAMES, 5200), 2, 16, 4096, 0)
    assert orc.SUB_LPC not in types and orc.SUB_FIXED in types


def test_orders_up_to_32(monkeypatch):
    monkeypatch.delenv("FLACGPU_NO_HAND", raising=False)
    x = extreme_pair(24, 4096, N_FRAMES, 5300)
    x[12 * 4096:] = synth_hi(5301, 2, 24, 4096 * 4, segment=4096, orders=[32, 27, 22, 17]).reshape(-1, 2)
    types, (handed, subs, on) = gpu_and_oracle(x, 2, 24, 4096, 32)
    assert orc.SUB_LPC in types and orc.SUB_FIXED in types
    assert on and handed > 0


def test_eight_channels():
    B, ch = 4096, 8
    x = synth_fast(5400, ch, 24, B * N_FRAMES).reshape(-1, ch).astype(np.int64)
    e = extreme_pair(24, B, N_FRAMES, 5401)
    x[:, 1], x[:, 6] = e[:, 0], e[:, 1]                          # the extreme signals on two of the channels
    x[:, 3] = (x[:, 3] >> 3) << 3                                # three wasted bits
    x[:, 4] = 0                                                  # a silent channel
    types, _ = gpu_and_oracle(x, ch, 24, B, 12)
    assert orc.SUB_LPC in types and orc.SUB_FIXED in types


def test_short_blocks_1152(monkeypatch):
    monkeypatch.delenv("FLACGPU_NO_HAND", raising=False)
    types, _ = gpu_and_oracle(extreme_pair(24, 1152, N_FRAMES, 5500), 2, 24, 1152, 12)
    assert orc.SUB_LPC in types and orc.SUB_FIXED in types


def test_every_subframe_won_by_lpc_is_handed(monkeypatch):
    """the 2-pole resonator signal: every subframe is an LPC subframe, and the wave that wins it hands its residual over --
    the merged words of the pair form are what k_frame64 emits from"""
    monkeypatch.delenv("FLACGPU_NO_HAND", raising=False)
    pcm = synth_fast(5600, 2, 24, 4096 * N_FRAMES)
    types, (handed, subs, on) = gpu_and_oracle(pcm, 2, 24, 4096, 12)
    assert all(t == orc.SUB_LPC for t in types)
    assert on and subs == 2 * N_FRAMES and handed == subs
