"""k_sub64 / k_sub_finish (csrc/kernels/sub64.inc) held to the oracle at their word, CRC and placement edges
(tests/_sub64_edge_matrix.py; every case proven on the CPU by test_sub64_edge_matrix_oracle.py).

Every case goes byte for byte -- the whole batch, offsets included -- through every instantiation (k_sub64<64,16> on planar
rows for 5 and 7 channels and for 4-bit samples, <64,16,3> / <64,16,4> in place for 6 / 8 channels and <64,16> under
FLACGPU_NO_XPOSE), both upload doors twice on one context, the pinned host output, ranges cut by
FLACGPU_TUNE_CHUNK_MSAMPLES and by FLACGPU_TUNE_TWO_RANGES with a case frame either side of the cut, flacgpu_pack_plans
for the hand-built plans (expected: the host packer), and once through the generic packer (FLACGPU_NO_FRAME64).  A failure
prints the model's geometry of the first frame that differs."""
import numpy as np
import pytest

import _sub64_edge_matrix as M

pytestmark = pytest.mark.gpu

B = M.B
CASES = M.cases()


def analyzer(case, n_frames=None):
    from flac_codec_amd.gpu import GpuAnalyzer

    return GpuAnalyzer(B, M.OPTS["max_po"], M.OPTS["max_lpc"], True, True, 2, 0.5, case.bps, case.C,
                       max_frames=n_frames or len(case.frames))


def same(case, got, where, want=None, frames=None):
    """The batch's bytes and offsets against the expected ones; the geometry of the first differing frame on a miss."""
    data, off = got
    want_data, want_off = want or M.batch_bytes(case)
    if list(off) == list(want_off) and data == want_data:
        return
    for f in range(len(want_off) - 1):
        if list(off[f:f + 2]) != list(want_off[f:f + 2]) or data[off[f]:off[f + 1]] != want_data[want_off[f]:want_off[f + 1]]:
            a, b = data[off[f]:off[f + 1]], want_data[want_off[f]:want_off[f + 1]]
            at = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), -1)
            if frames is None:
                print(M.describe(case, f))
            raise AssertionError("%s, %s: frame %d differs at byte %d of %d (offsets %s, expected %s)" %
                                 (case.name, where, f, at, len(b), list(off[f:f + 2]), list(want_off[f:f + 2])))
    raise AssertionError("%s, %s: bytes behind the last frame" % (case.name, where))


def clean(an, case, n, where):
    res, _ = an.verify_device(case.rate, case.first)
    assert (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs) == (n, 0, 0, 0), (case.name, where)


def to_device(pcm):
    import torch

    try:
        d = torch.from_numpy(pcm).cuda()
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.skip(f"torch cannot use the GPU here: {e}")
    return d


def packed_by_plans(an, case):
    plans, subs, _ = M.hand_plans(case)
    return an.pack_plans(M.interleaved(case), len(case.frames), B, plans, subs, case.first, case.rate)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.cls + "-" + c.name)
def test_every_instantiation_and_both_doors(monkeypatch, case):
    import torch

    n = len(case.frames)
    pcm = M.interleaved(case)
    if case.plans is not None:           # hand-built plans: flacgpu_pack_plans (planar rows: k_sub64<64,16>), twice
        an = analyzer(case)
        try:
            for rep in range(2):
                same(case, packed_by_plans(an, case), "pack_plans, call %d" % rep)
            clean(an, case, n, "pack_plans")
        finally:
            an.close()
        return
    if case.bps == 4:                    # below the transposing loads' width: the rows route, never the generic packer
        from test_route_table import SPLIT, route

        r = route(M.route_inputs(case))
        assert r[0] == SPLIT and r[3] == n, (case.name, r)
    dev = to_device(pcm)
    modes = ["default"] + (["FLACGPU_NO_XPOSE"] if case.C in (6, 8) and case.bps >= 8 else [])
    for mode in modes:
        monkeypatch.delenv("FLACGPU_NO_XPOSE", raising=False)
        if mode != "default":
            monkeypatch.setenv(mode, "1")
        an = analyzer(case)
        try:
            for rep in range(2):         # the second batch meets the first one's output bytes and edge records
                same(case, an.encode_frames(pcm, n, B, case.first, case.rate), "%s, encode_frames, call %d" % (mode, rep))
            clean(an, case, n, mode + ", encode_frames")
            for rep in range(2):
                an.encode_device(dev.data_ptr(), n, B, case.first, case.rate)
                torch.cuda.synchronize()
                same(case, an.fetch_frames(n), "%s, encode_device, call %d" % (mode, rep))
            clean(an, case, n, mode + ", encode_device")
        finally:
            an.close()
    del dev


@pytest.mark.parametrize("case", [c for c in CASES if c.cls in "bc" and c.plans is None], ids=lambda c: c.cls + "-" + c.name)
def test_pinned_host_output(case):
    """The kernels' stores go over the link into pinned memory: a dword where bytes were due is a changed neighbour."""
    n = len(case.frames)
    an = analyzer(case)
    try:
        data, off, _ = an.encode_frames_pinned(M.interleaved(case), n, B, case.first, case.rate, repeat=2)
        same(case, (data, off), "encode_frames_pinned")
    finally:
        an.close()


def test_generic_packer_gives_the_same_bytes(monkeypatch):
    """FLACGPU_NO_FRAME64, once over the whole matrix: k_emit / k_pack / k_crc OR shared words with atomics and have the
    same corners."""
    monkeypatch.setenv("FLACGPU_NO_FRAME64", "1")
    by_shape = {}
    try:
        for case in CASES:
            key = (case.C, case.bps)
            if key not in by_shape:
                by_shape[key] = analyzer(case, 65)
            an = by_shape[key]
            if case.plans is not None:
                same(case, packed_by_plans(an, case), "generic packer, pack_plans")
            else:
                same(case, an.encode_frames(M.interleaved(case), len(case.frames), B, case.first, case.rate), "generic packer")
    finally:
        for an in by_shape.values():
            an.close()


# ---------------------------------------------------------------------------------------------------------------------
# a cut between two ranges: the frames either side of it are written by different launches (on two streams for
# FLACGPU_TUNE_TWO_RANGES), and where a frame does not end on a dword the two sides share one
# ---------------------------------------------------------------------------------------------------------------------
def silent_batch(C_, bps, n, case_frames, at, rate, first, cut, cut_mod):
    """n frames, silent but for `case_frames` from frame `at` on, and frame 0 a spacer picked by its length so that frame
    `cut` begins at byte cut_mod modulo 4: (pcm, expected bytes, offsets)"""
    frames = [np.zeros((C_, B), dtype=np.int32) for _ in range(n)]
    for i, x in enumerate(case_frames):
        frames[at + i] = x
    lens = [len(M.oracle_frame(planar, bps, rate, first + f)[0]) for f, planar in enumerate(frames[:cut])]
    frames[0] = M.spacer(C_, bps, rate, first, 4, (cut_mod - sum(lens[1:])) & 3)
    data, off = [], [0]
    for f, planar in enumerate(frames):
        d, _ = M.oracle_frame(planar, bps, rate, first + f)
        data.append(d)
        off.append(off[-1] + len(d))
    assert off[cut] & 3 == cut_mod
    pcm = np.ascontiguousarray(np.stack(frames).transpose(0, 2, 1)).astype(np.int32).reshape(-1)
    return pcm, b"".join(data), off


def cut_case_frames(C_, bps):
    """class (a) / (b) frames: one loud channel and a run of silent ones to the frame's end; a run at the start"""
    tail_run = M.frame_of(["noise" if bps == 4 else "synth"] + ["zeros"] * (C_ - 1), bps, 21)
    head_run = M.frame_of(["zeros"] * (C_ - 1) + ["quiet"], bps, 22)
    return [tail_run, tail_run, head_run, tail_run]


# (channels, bps, FLACGPU_TUNE_CHUNK_MSAMPLES, where the frame behind the cut begins modulo 4: the two sides share a dword).
# The smallest setting plan_route accepts is a range of 256 frames (chunk = (M << 20) / (4096 C) rounded down to 64 frames,
# >= 256), and a batch is cut from 1.5 ranges on: 384 frames, the cut in front of frame 256.
@pytest.mark.parametrize("C_,bps,chunk_m,cut_mod", [(8, 4, 8, 1), (8, 4, 8, 3), (5, 16, 5, 2), (6, 16, 6, 3)])
def test_a_cut_between_ranges(C_, bps, chunk_m, cut_mod):
    import torch

    from test_route_table import route

    n, cut, rate, first = 384, 256, 48000, 5
    pcm, want, want_off = silent_batch(C_, bps, n, cut_case_frames(C_, bps), cut - 2, rate, first, cut, cut_mod)
    case = M.Case("cut_c%d_b%d" % (C_, bps), "b", C_, bps, rate, first, [None] * n, [], None, None)
    r = route(dict(M.route_inputs(case), chunk=chunk_m))
    assert r[5] == cut, r                                                # range_frames: the cut position, from plan_route
    assert route(dict(M.route_inputs(case), chunk=chunk_m - 1))[5] == 0   # ... and no smaller setting cuts
    dev = to_device(pcm)
    an = analyzer(case, n)
    try:
        an.set_tuning(an.TUNE_CHUNK_MSAMPLES, chunk_m)
        for rep in range(2):
            an.encode_device(dev.data_ptr(), n, B, first, rate)
            torch.cuda.synchronize()
            same(case, an.fetch_frames(n), "ranges of %d frames, call %d" % (cut, rep), (want, want_off), frames=n)
        clean(an, case, n, "ranges")
    finally:
        an.close()
    del dev


@pytest.mark.parametrize("C_,bps,cut_mod", [(8, 4, 1), (8, 4, 2), (5, 16, 3), (7, 24, 1)])
def test_a_cut_between_two_streams(C_, bps, cut_mod):
    from test_route_table import route

    n, rate, first = 272, 48000, 5
    cut = ((n // 2) + 15) & ~15                                          # flacgpu_encode_device's two-ranges branch
    pcm, want, want_off = silent_batch(C_, bps, n, cut_case_frames(C_, bps), cut - 2, rate, first, cut, cut_mod)
    case = M.Case("two_c%d_b%d" % (C_, bps), "b", C_, bps, rate, first, [None] * n, [], None, None)
    assert route(dict(M.route_inputs(case), two_ranges=1))[6] == 1
    an = analyzer(case, n)
    try:
        an.set_two_ranges(True)
        for rep in range(2):
            same(case, an.encode_frames(pcm, n, B, first, rate), "two ranges, call %d" % rep, (want, want_off), frames=n)
        clean(an, case, n, "two ranges")
    finally:
        an.close()
