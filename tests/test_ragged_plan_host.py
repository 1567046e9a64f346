"""flacgpu_ragged_plan (csrc/host/ragged_plan.h): the checks of a ragged batch -- every frame with a length of its own,
flacgpu_encode_ragged_device -- and the layout of its window pool.  Pure host code: no GPU call.

The expected plans are restated here in Python from the interface's words (include/flacenc_gpu.h): one window per distinct
length in first-appearance order, each followed by 64 zero doubles."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flac-codec_amd", "csrc", "host")
INVALID_ARG, UNSUPPORTED = -1, -2


def _plan(samples, block_size=4096, po=6):
    from flac_codec_amd import gpu

    return gpu.ragged_plan(samples, block_size, po)


def _refused(samples, block_size=4096, po=6):
    from flac_codec_amd import gpu

    with pytest.raises(gpu.GpuError) as e:
        gpu.ragged_plan(samples, block_size, po)
    return e.value.code, str(e.value)


def expect(samples):
    distinct = list(dict.fromkeys(int(n) for n in samples))
    return [distinct.index(int(n)) for n in samples], distinct, sum(n + 64 for n in distinct)


def test_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacgpu_ragged_plan", "flacgpu_encode_ragged_device", "flacgpu_ragged_pool_uploads"} <= _lib.exported_symbols()


def test_no_frames_is_refused():
    code, text = _refused([])
    assert code == INVALID_ARG and "no frames" in text


def test_an_empty_frame_is_refused_and_named():
    code, text = _refused([256, 17, 0, 4096, 0])
    assert code == INVALID_ARG and "frame 2 has no samples" in text


def test_a_frame_longer_than_the_block_is_refused_and_named():
    code, text = _refused([4096, 4097, 5000])
    assert code == INVALID_ARG and "frame 1 has 4097 samples" in text and "4096" in text
    code, text = _refused([17], block_size=16)
    assert code == INVALID_ARG and "frame 0 has 17 samples" in text


def test_a_refused_batch_writes_nothing():
    from flac_codec_amd import _lib

    o = _lib.GpuOptions(4096, 6, 0, 0, 0, 0, 0, 0.0)
    lens = np.array([5, 0], dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    win, dist = np.full(2, 99, dtype=np.uint32), np.full(2, 99, dtype=np.uint32)
    nd, pool = C.c_uint32(99), C.c_uint64(99)
    rc = _lib.lib().flacgpu_ragged_plan(C.byref(o), lens.ctypes.data_as(u32p), 2, win.ctypes.data_as(u32p),
                                        dist.ctypes.data_as(u32p), C.byref(nd), C.byref(pool))
    assert rc == INVALID_ARG
    assert list(win) == [99, 99] and list(dist) == [99, 99] and nd.value == 99 and pool.value == 99
    assert _lib.lib().flacgpu_ragged_plan(None, lens.ctypes.data_as(u32p), 2, None, None, None, None) == INVALID_ARG


def test_pool_layout_with_duplicates():
    samples = [256, 17, 256, 4096, 1, 17, 17, 4095, 1, 256]
    window_of, distinct, pool = _plan(samples)
    assert distinct == [256, 17, 4096, 1, 4095]                   # first-appearance order
    assert window_of == [0, 1, 0, 2, 3, 1, 1, 4, 3, 0]
    assert pool == sum(n + 64 for n in distinct) == 256 + 17 + 4096 + 1 + 4095 + 5 * 64
    assert (window_of, distinct, pool) == expect(samples)


def test_every_out_pointer_may_be_null():
    from flac_codec_amd import _lib

    o = _lib.GpuOptions(4096, 6, 0, 0, 0, 0, 0, 0.0)
    lens = np.array([3, 3, 9], dtype=np.uint32)
    rc = _lib.lib().flacgpu_ragged_plan(C.byref(o), lens.ctypes.data_as(C.POINTER(C.c_uint32)), 3, None, None, None, None)
    assert rc == 0


def test_random_batches_against_the_restated_rule():
    rng = np.random.default_rng(20)
    for _ in range(50):
        block = int(rng.choice([16, 1152, 4096, 65535]))
        n = int(rng.integers(1, 200))
        samples = [int(v) for v in rng.integers(1, block + 1, n)]
        samples += [samples[int(i)] for i in rng.integers(0, n, n // 2)]   # duplicates
        assert _plan(samples, block, 0) == expect(samples)


def test_partition_order_rule():
    """min(ctz(n), max_partition_order) > 6 is refused, naming the first such frame: what analyze_impl says of a short last
    frame.  128 = 2^7 samples under max_partition_order 8: order 7.  Under 6: order 6, accepted."""
    code, text = _refused([100, 129, 128, 256], block_size=65535, po=8)
    assert code == UNSUPPORTED
    assert "frame 2 (128 samples)" in text and "partition order" in text
    assert _plan([100, 129, 128, 256], block_size=65535, po=6) == expect([100, 129, 128, 256])
    assert _plan([64, 192, 65535], block_size=65535, po=8) == expect([64, 192, 65535])   # ctz 6, 6, 0
    code, text = _refused([4096], block_size=4096, po=15)
    assert code == UNSUPPORTED and "frame 0 (4096 samples)" in text


ROWS = [
    (4096, 6, [256]),
    (4096, 6, [1]),
    (4096, 6, [256, 17, 256, 4096, 1, 17, 17, 4095, 1, 256]),
    (16, 0, list(range(1, 17)) + list(range(16, 0, -1))),
    (65535, 8, [100, 129, 128, 256]),
    (65535, 6, [100, 129, 128, 256, 65535, 65535]),
    (4096, 6, [5, 0]),
    (4096, 6, [4097]),
    (4096, 6, []),
    (15, 6, [3]),          # an invalid block size
    (4096, 16, [3]),       # an invalid partition order
]


def test_under_address_sanitizer(tmp_path):
    """tools/ragged_plan_check.cpp, a stand-alone program built with ASan and UBSan, runs the plan on tables that end exactly at
    their allocations' ends; its rows must be the library's."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + san + [str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True,
                           text=True)
    if probe.returncode:
        pytest.skip("the sanitizer runtime cannot be linked here: " + (probe.stderr.strip().splitlines() or ["?"])[-1])
    exe = tmp_path / "ragged_plan_check"
    made = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + san + [
        "-I" + HOST, os.path.join(ROOT, "tools", "ragged_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    (tmp_path / "rows.txt").write_text("".join(" ".join(str(v) for v in [b, po, len(s)] + s) + "\n" for b, po, s in ROWS))
    run = subprocess.run([str(exe), str(tmp_path / "rows.txt")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(ROWS)
    from flac_codec_amd import gpu

    for (block, po, samples), line in zip(ROWS, lines):
        try:
            window_of, distinct, pool = gpu.ragged_plan(samples, block, po)
        except gpu.GpuError as e:
            assert line.split()[0] == str(e.code), (line, str(e))
            assert line.split(" ", 1)[1] in str(e)
            continue
        want = "0 %d %d | %s | %s" % (len(distinct), pool, " ".join(map(str, window_of)), " ".join(map(str, distinct)))
        assert " ".join(line.split()) == " ".join(want.split()), (block, po, samples)
