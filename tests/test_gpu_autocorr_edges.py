"""The autocorrelation kernels at their tile, lag and length edges (tests/_autocorr_edge_matrix.py: the cases, proven on the
CPU by tests/test_autocorr_edge_matrix_oracle.py): after every case's analysis the sums the device leaves for the Levinson
stage (flacgpu_device_buffer 6) are the oracle's BIT FOR BIT -- lags 0 .. order of every analysed candidate, compared as
int64, no tolerance -- and the frames built from them are the oracle's bytes.  The frame bytes alone forgive a wrong last bit
of a sum whenever the quantised coefficients come out the same; the sums do not.

Device-door inputs are tensors that end at the batch's last sample.  The fused cases run twice, with the fused tiles and with
FLACGPU_NO_AC_FMA=1."""
import ctypes as C

import numpy as np
import pytest

import _autocorr_edge_matrix as m

pytestmark = pytest.mark.gpu
KNOBS = ("FLACGPU_NO_DIRECT", "FLACGPU_NO_XPOSE", "FLACGPU_NO_AC_FMA", "FLACGPU_NO_W64", "FLACGPU_NO_DIRECT_SHORT")


def device_ac(an, rows):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty((rows, m.AC_LD), dtype=np.float64)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(an.device_buffer(6)), out.nbytes, 2) == 0
    return out


def run(case, monkeypatch, extra_env=()):
    """the case through its door: (sums [frames * ncand][AC_LD], frame bytes, offsets)"""
    import torch

    from flac_codec_amd.gpu import GpuAnalyzer

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k in tuple(case.env) + tuple(extra_env):
        monkeypatch.setenv(k, "1")
    pcm = m.pcm_of(case)
    ncand = m.ncand_of(case)
    an = GpuAnalyzer(case.block, 6, case.order, True, True, case.window[0], case.window[1], case.bps, case.ch, max_frames=case.frames)
    try:
        if case.lag_split != 4:
            an.set_tuning(an.TUNE_LAG_SPLIT, case.lag_split)
        if case.door == m.HOST:
            an.analyze(pcm, case.frames, case.last)          # (returns with the plans: the analysis is over)
            got = device_ac(an, case.frames * ncand)
            an.pack_device(0, m.RATE)
        else:
            d = torch.from_numpy(pcm).cuda()                 # exactly the batch: nothing of ours lies behind its last sample
            assert d.numel() == pcm.size
            if case.door == m.RAGGED:
                at, frames = 0, []
                for f, n in enumerate(case.lengths):
                    frames.append((d.data_ptr() + 4 * at, n, f))
                    at += n * case.ch
                assert at == pcm.size
                an.encode_ragged_device(frames, m.RATE)
            else:
                an.encode_device(d.data_ptr(), case.frames, case.last, 0, m.RATE)
            torch.cuda.synchronize()
            got = device_ac(an, case.frames * ncand)
        data, off = an.fetch_frames(case.frames)
        if case.door != m.HOST:
            res, _ = an.verify_device(m.RATE, 0)
            assert (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs) == (case.frames, 0, 0, 0)
    finally:
        an.close()
    return got, data, off


def check_sums(case, got):
    ncand = m.ncand_of(case)
    checked = 0
    for f in range(case.frames):
        for c, want in enumerate(m.sums_of(case, f)):
            if want is None:
                continue
            have = got[f * ncand + c][: len(want)]
            assert np.array_equal(have.view(np.int64), want.view(np.int64)), (case.name, case.reach, f, c, have, want)
            checked += 1
    analysed = sum(ncand for f in range(case.frames) if m.length_of(case, f) > case.order) - case.skipped
    assert checked == analysed
    return checked


def check_bytes(case, data, off):
    assert len(off) == case.frames + 1 and off[-1] == len(data)
    for f in range(case.frames):
        assert data[off[f]:off[f + 1]] == m.oracle_frame_bytes(case, f), f"{case.name}: frame {f} differs from the oracle's bytes"


@pytest.mark.parametrize("name", [c.name for c in m.cases()])
def test_sums_and_frames_are_the_oracles(monkeypatch, name):
    case = m.case_named(name)
    got, data, off = run(case, monkeypatch)
    check_sums(case, got)
    check_bytes(case, data, off)
    if case.family == "fused":
        plain, data2, off2 = run(case, monkeypatch, extra_env=("FLACGPU_NO_AC_FMA",))
        check_sums(case, plain)
        assert np.array_equal(plain[:, : case.order + 1].view(np.int64), got[:, : case.order + 1].view(np.int64))
        assert (data2, off2) == (data, off)
