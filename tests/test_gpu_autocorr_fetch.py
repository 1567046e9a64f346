"""k_autocorr4 / k_autocorr4_deep with their input requested ahead through rotating staging sets (kernels/shape.h,
ac4_fetch_slot): the sums every candidate leaves are the oracle's BIT FOR BIT and the frames built from them are the
oracle's bytes -- at the frame counts where a workgroup's 16 frames are partly there (the last group clamps its frame
index: 1, 15, 16, 17, 33), for both kernels (orders 12 and 32), for the split producers of an 8-channel batch (8 frames
per group) and under a window whose flat part starts and ends inside a tile.  The input is a device tensor that ends
exactly at the batch's last sample: a request past a frame's end must read the frame's last tile again, never beyond."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as orc
from _compare import orc_options_for, planar_frames
from _pcm import synth_fast, synth_hi

pytestmark = pytest.mark.gpu
B = 4096
AC_LD = 36
RATE = 48000


@functools.lru_cache(maxsize=None)
def pcm_of(ch, bps, frames):
    x = (synth_hi(300 + ch + bps, ch, bps, B * frames, sections=4) if ch <= 2 else synth_fast(300 + ch, ch, bps, B * frames))
    x = x.reshape(-1, ch).astype(np.int64)
    x[:, 0] = (x[:, 0] >> 3) << 3                          # wasted bits on channel 0 (the in-place kernels scale the sums)
    x[B:2 * B, ch - 1] = (1 << (bps - 1)) - 1              # rail DC: the largest products
    x[(frames - 1) * B:, ch - 1] = -(1 << (bps - 1))       # and the other rail in the LAST frame, up to the tensor's end
    out = np.ascontiguousarray(x.astype(np.int32).reshape(-1))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(ch, bps, frames, lpc, window):
    """(sums per frame and candidate, frame bytes) of the oracle for every frame of pcm_of(ch, bps, frames); computed once,
    a batch of fewer frames is a prefix of it"""
    pcm = pcm_of(ch, bps, frames)
    w = orc.window(window[0], window[1], B)
    oopts = orc_options_for(B, 6, lpc, True, True, window[0], window[1])
    sums, blobs = [], []
    for f, planar in enumerate(planar_frames(pcm, ch, B)):
        rows = [r.astype(np.int64) for r in planar]
        if ch == 2:
            rows = [rows[0], rows[1], (rows[0] + rows[1]) >> 1, rows[0] - rows[1]]
        per = []
        for row in rows:
            orv = int(np.bitwise_or.reduce(row))
            if orv == 0:
                per.append(None)                           # an all-zero candidate gets no LPC analysis
                continue
            wasted = (orv & -orv).bit_length() - 1
            per.append(orc.autocorrelate((row >> wasted).astype(np.float64) * w, lpc))
        sums.append(per)
        rc, fb, _ = orc.encode_frame(oopts, RATE, bps, planar, frame_number=f)
        assert rc == 0
        blobs.append(fb)
    return sums, blobs


def device_ac(an, rows):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty((rows, AC_LD), dtype=np.float64)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(an.device_buffer(6)), out.nbytes, 2) == 0
    return out


def run_case(ch, bps, n, total, lpc, window):
    import torch

    from flac_codec_amd.gpu import GpuAnalyzer

    pcm = pcm_of(ch, bps, total)[: n * B * ch]
    want_sums, want_frames = reference(ch, bps, total, lpc, window)
    d = torch.from_numpy(pcm.copy()).cuda()                # exactly n * B * ch samples: nothing of ours lies behind them
    assert d.numel() == n * B * ch
    ncand = 4 if ch == 2 else ch
    an = GpuAnalyzer(B, 6, lpc, True, True, window[0], window[1], bps, ch, max_frames=n)
    try:
        an.encode_device(d.data_ptr(), n, B, 0, RATE)
        torch.cuda.synchronize()
        got = device_ac(an, n * ncand)[:, : lpc + 1].copy()
        data, off = an.fetch_frames(n)
        checked = 0
        for f in range(n):
            for c in range(ncand):
                want = want_sums[f][c]
                if want is None:
                    continue
                have = got[f * ncand + c][: len(want)]
                assert np.array_equal(have.view(np.int64), want.view(np.int64)), (f, c, have, want)
                checked += 1
            assert data[off[f]:off[f + 1]] == want_frames[f], f"frame {f} differs from the oracle's bytes"
        assert checked >= n * ncand - 2
        res, _ = an.verify_device(RATE, 0)
        assert (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs) == (n, 0, 0, 0)
    finally:
        an.close()


@pytest.mark.parametrize("lpc", [12, 32])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_stereo_frame_counts_around_a_workgroups_sixteen(n, lpc):
    run_case(2, 24, n, 33, lpc, (2, 0.5))


@pytest.mark.parametrize("n", [9, 17])
def test_eight_channels_through_the_split_producers(n):
    """64 candidates = 8 frames of 8 channels per workgroup: 9 and 17 frames leave the last group one frame"""
    run_case(8, 24, n, 17, 12, (2, 0.5))


@pytest.mark.parametrize("lpc", [12, 32])
def test_flat_part_that_starts_and_ends_inside_a_tile(lpc):
    """Tukey(0.3): the taper is 614.4 samples long, so the window reaches 1.0 inside tile 19 and leaves it inside tile 108"""
    w = orc.window(2, 0.3, B)
    flat = np.flatnonzero(w == 1.0)
    assert flat.size and flat[0] % 32 != 0 and (flat[-1] + 1) % 32 != 0
    run_case(2, 24, 17, 17, lpc, (2, 0.3))
