"""The copy rule of k_place_runs (csrc/kernels/place_rule.h) through its host export flacgpu_place_runs_host, which runs
the kernel's per-group code over host memory one "lane" after another.  The expected bytes come from plain numpy slicing.
Every destination is pre-filled with a canary: the run's bytes must arrive and every other byte must stay.  (What the
rule READS cannot be asserted here; every source has bytes of its own array in front of src and behind src + n.)
No GPU call."""
import ctypes as C

import numpy as np
import pytest

CANARY = 0xA5


def _L():
    from flac_codec_amd import encode

    return encode._stream_lib()


def _aligned(n, fill):
    """n bytes that start on a 64-byte boundary (a view; the owner stays alive through .base)."""
    raw = np.empty(n + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + n]
    a[:] = fill
    assert a.ctypes.data % 64 == 0
    return a


def _source(n):
    """distinct neighbouring bytes: a period of 251 never lines up with the 16-byte groups"""
    a = _aligned(n, 0)
    a[:] = (np.arange(n) * 7 + 3) % 251
    return a


def _place(src, dst, runs):
    """runs: [(src index, dst index, n)] -> the return code; dst is written in place"""
    from flac_codec_amd import _lib

    tab = (_lib.PlaceRun * max(len(runs), 1))()
    for r, (s, d, n) in zip(tab, runs):
        r.src, r.dst, r.n = src.ctypes.data + s, dst.ctypes.data + d, n
    return _L().flacgpu_place_runs_host(tab, len(runs))


def _expect(src, size, runs):
    want = np.full(size, CANARY, dtype=np.uint8)
    for s, d, n in runs:
        want[d:d + n] = src[s:s + n]
    return want


def _check(src, size, runs):
    dst = _aligned(size, CANARY)
    assert _place(src, dst, runs) == 0
    want = _expect(src, size, runs)
    bad = np.flatnonzero(dst != want)
    assert bad.size == 0, f"first wrong byte at {bad[0]}: {dst[bad[0]]:#x}, want {want[bad[0]]:#x}; runs {runs[:4]}"


def test_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacgpu_place_runs_host", "flacgpu_place_workgroup", "flacgpu_place_frames", "flacgpu_frame_offsets",
            "flacgpu_ingest_scratch", "flacgpu_ingest_place"} <= _lib.exported_symbols()


@pytest.mark.parametrize("src_residue", range(16))
def test_every_residue_pair_and_length(src_residue):
    """16 source residues x 16 destination residues x lengths 0..49, every run alone in its table and all 50 lengths of a
    residue pair in one table."""
    stride = 96   # a run's place: 16 bytes of margin, the residue, up to 49 bytes, margin again
    src = _source(50 * stride)
    for dst_residue in range(16):
        runs = [(n * stride + 16 + src_residue, n * stride + 16 + dst_residue, n) for n in range(50)]
        _check(src, 50 * stride, runs)
        for r in runs:
            _check(src[: r[0] + r[2] + 16], r[1] + r[2] + 32, [r])


def test_adjacent_runs_share_a_group():
    """5, 3 and 20 bytes back to back from residue 13: the first two runs and the head of the third lie in two groups
    that each of them only partly owns"""
    src = _source(400)
    for s0, s1, s2 in [(17, 100, 200), (31, 96, 205), (16, 111, 192)]:
        at = 16 + 13
        runs = [(s0, at, 5), (s1, at + 5, 3), (s2, at + 8, 20)]
        _check(src, 96, runs)
        _check(src, 96, runs[::-1])          # the table's order is not the memory's
        _check(src, 96, [runs[1]])           # the middle run alone: its neighbours' bytes stay canary


def test_empty_runs_at_the_front_in_the_middle_and_at_the_end():
    src = _source(600)
    body = [(20, 37, 40), (101, 150, 7), (300, 200, 33)]
    empty = [(5, 3, 0), (0, 0, 0), (599, 255, 0)]
    runs = [empty[0], empty[1], body[0], empty[2], body[1], empty[0], empty[1], body[2], empty[2], empty[0]]
    _check(src, 256, runs)
    _check(src, 256, empty)                  # nothing but empty runs: no byte is written
    _check(src, 256, [])
    assert _L().flacgpu_place_runs_host(None, 0) == 0
    assert _L().flacgpu_place_runs_host(None, 1) != 0


@pytest.mark.parametrize("dst_residue,src_residue", [(0, 0), (0, 5), (9, 0), (13, 6)])
def test_a_table_one_group_longer_than_a_workgroup(dst_residue, src_residue):
    wg = _L().flacgpu_place_workgroup()
    assert wg >= 64 and wg % 64 == 0
    # one run of WG groups + 1: from the residue to one byte behind the WG-th boundary
    n = 16 * wg - dst_residue + 1
    src = _source(n + 64)
    _check(src, n + 64, [(16 + src_residue, 16 + dst_residue, n)])
    # the same group count from several runs, the workgroup's edge inside the last of them
    third = (16 * wg) // 3
    runs = [(16 + src_residue, 16 + dst_residue, third), (16 + src_residue + third, 16 + dst_residue + third, 11),
            (40 + src_residue + third, 16 + dst_residue + third + 11, n - third - 11)]
    _check(src, n + 64, runs)


def test_random_tables():
    rng = np.random.default_rng(18)
    src = _source(1 << 14)
    for _ in range(40):
        runs, at = [], int(rng.integers(0, 20))
        for _ in range(int(rng.integers(1, 40))):
            n = int(rng.choice([0, 1, 2, 15, 16, 17, 31, 32, 33, int(rng.integers(0, 300))]))
            at += int(rng.choice([0, 0, 1, int(rng.integers(0, 40))]))   # back to back, or a gap
            runs.append((int(rng.integers(1, src.size - n - 1)), at, n))
            at += n
        order = rng.permutation(len(runs))
        _check(src, at + 48, [runs[i] for i in order])
