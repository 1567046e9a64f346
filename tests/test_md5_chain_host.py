"""The rule of the resumable MD5 chains (csrc/kernels/md5_feed_rule.h) through its host exports flacgpu_md5_init_host /
feed_host / final_host, which run the kernel's window-by-window pass over host memory.  Expected digests are hashlib.md5
of the samples' low `width` bytes, little-endian.  Also: the same rule in a stand-alone program under AddressSanitizer and
UBSan (tools/md5_chain_check.cpp), every piece in a heap block that ends where the piece ends.  No GPU call."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "flac-codec_amd", "csrc", "kernels")
INVALID_ARG = -1


def _L():
    from flac_codec_amd import _lib

    return _lib.lib()


def le_bytes(samples, width):
    """int32 samples -> the bytes the chain hashes: the low `width` bytes of each, little-endian"""
    return np.ascontiguousarray(samples, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :width].tobytes()


def check_samples(n, first=0):
    """tools/md5_chain_check.cpp's md5_check_sample(first .. first + n)"""
    x = (np.arange(first, first + n, dtype=np.uint64) * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 2246822519) & 0xFFFFFFFF
    x ^= x >> 13
    return x.astype(np.uint32).view(np.int32)


def interesting_counts(width):
    stage = _L().flacgpu_md5_stage_bytes()
    counts = {c for c in range(200 // width + 1)}
    for edge in (stage, 2 * stage):
        for b in (edge - 1, edge, edge + 1):
            counts |= {b // width, (b + width - 1) // width}
    return sorted(counts)


class Chain:
    def __init__(self):
        from flac_codec_amd import _lib

        self.s = _lib.Md5State()
        _L().flacgpu_md5_init_host(C.byref(self.s))

    def feed(self, samples, width):
        a = np.ascontiguousarray(samples, dtype=np.int32)
        assert _L().flacgpu_md5_feed_host(C.byref(self.s), a.ctypes.data if a.size else None, a.size, width) == 0

    def final(self):
        out = (C.c_uint8 * 16)()
        assert _L().flacgpu_md5_final_host(C.byref(self.s), out) == 0
        return bytes(out)


def test_symbols_and_the_staging_quantum():
    from flac_codec_amd import _lib

    assert {"flacgpu_md5_chains_create", "flacgpu_md5_chains_destroy", "flacgpu_md5_chains_update",
            "flacgpu_md5_chains_final", "flacgpu_md5_stage_bytes", "flacgpu_md5_init_host", "flacgpu_md5_feed_host",
            "flacgpu_md5_final_host", "flacgpu_ingest_move"} <= _lib.exported_symbols()
    stage = _L().flacgpu_md5_stage_bytes()
    assert stage >= 64 and stage % 64 == 0
    assert C.sizeof(_lib.Md5State) == 88 and C.sizeof(_lib.Md5Piece) == 24


def test_negative_samples_are_masked():
    a = np.array([-1, -2, -129, -32769, -8388609, -(1 << 31), 5], dtype=np.int32)
    for width in (1, 2, 3, 4):
        c = Chain()
        c.feed(a, width)
        assert c.final() == hashlib.md5(le_bytes(a, width)).digest()
    assert le_bytes(a[:1], 3) == b"\xff\xff\xff"


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_every_length_whole_and_one_sample_at_a_time(width):
    """message lengths 0..200 bytes (55, 56, 63, 64, 119, 120: the padding's edges) and around the staging quantum"""
    for n in interesting_counts(width):
        a = check_samples(n)
        want = hashlib.md5(le_bytes(a, width)).digest()
        c = Chain()
        c.feed(a, width)
        assert c.final() == want, (width, n)
        for e in range(n):   # the chain is initial again after final; the buffer fills over many calls
            c.feed(a[e:e + 1], width)
        assert c.final() == want, (width, n, "one sample at a time")
    assert Chain().final() == hashlib.md5(b"").digest()


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_every_cut_point(width):
    stage = _L().flacgpu_md5_stage_bytes()
    c = Chain()
    for n in interesting_counts(width):
        a = check_samples(n)
        want = hashlib.md5(le_bytes(a, width)).digest()
        if n * width <= 200:
            cuts = range(n + 1)
        else:   # the long ones: cuts near either end and round every window's edge
            near = [0, n, stage // width, 2 * stage // width]
            cuts = sorted({k for m in near for k in range(m - 70, m + 71) if 0 <= k <= n})
        for cut in cuts:
            c.feed(a[:cut], width)
            c.feed(a[cut:], width)
            assert c.final() == want, (width, n, cut)


def test_three_pieces_with_a_short_middle_and_an_empty_piece():
    a = check_samples(700)
    for width in (1, 2, 3, 4):
        want = hashlib.md5(le_bytes(a, width)).digest()
        for first, mid in [(5, 3), (21, 1), (300, 20 // width), (341, 63 // width)]:
            c = Chain()
            c.feed(a[:first], width)
            c.feed(a[:0], width)
            c.feed(a[first:first + mid], width)
            c.feed(a[first + mid:], width)
            assert c.final() == want, (width, first, mid)


def test_refusals_leave_the_state_alone():
    from flac_codec_amd import _lib

    c = Chain()
    a = check_samples(10)
    c.feed(a, 2)
    before = bytes(c.s)
    for width in (0, 5):
        assert _L().flacgpu_md5_feed_host(C.byref(c.s), a.ctypes.data, 10, width) == INVALID_ARG
    assert _L().flacgpu_md5_feed_host(C.byref(c.s), None, 10, 2) == INVALID_ARG
    assert _L().flacgpu_md5_feed_host(None, a.ctypes.data, 10, 2) == INVALID_ARG
    assert bytes(c.s) == before
    assert c.final() == hashlib.md5(le_bytes(a, 2)).digest()
    assert isinstance(c.s, _lib.Md5State)


def test_under_address_sanitizer(tmp_path):
    """tools/md5_chain_check.cpp: every count, every cut point, every piece's source ending at its allocation's end"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + san + [str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True,
                           text=True)
    if probe.returncode:
        pytest.skip("the sanitizer runtime cannot be linked here: " + (probe.stderr.strip().splitlines() or ["?"])[-1])
    exe = tmp_path / "md5_chain_check"
    made = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + san + [
        "-I" + KERNELS, os.path.join(ROOT, "tools", "md5_chain_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [ln.split() for ln in run.stdout.splitlines()]
    seen = {}
    for w, n, digest in lines:
        seen.setdefault(int(w), []).append(int(n))
        assert digest == hashlib.md5(le_bytes(check_samples(int(n)), int(w))).hexdigest(), (w, n)
    assert {w: sorted(v) for w, v in seen.items()} == {w: interesting_counts(w) for w in (1, 2, 3, 4)}
