"""CPU-side checks of the batch decoder's sample windows (flacgpu_decoder_plan_windows, flacgpu_decoder_decode_windows,
flacgpu_window_frames): the exports, the ctypes layout of flacgpu_window and flacgpu_window_result against the header,
the frame selection against a model that sums the block sizes and searches linearly (_windows.py), and what
plan_windows -- a pure host function -- answers for hand-made records.  No GPU call."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import _foreign_matrix as fm
import _windows as wn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
I32, I16, F32 = 0, 1, 2
FLAT, PADDED = 0, 1


def test_window_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacgpu_decoder_plan_windows", "flacgpu_decoder_decode_windows",
            "flacgpu_window_frames"} <= _lib.exported_symbols()


def test_window_layouts_match_header(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_gpu.h"\n'
        "int main() { printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(flacgpu_window),"
        " offsetof(flacgpu_window, stream), offsetof(flacgpu_window, reserved), offsetof(flacgpu_window, start),"
        " offsetof(flacgpu_window, length), sizeof(flacgpu_window_result), offsetof(flacgpu_window_result, rc),"
        " offsetof(flacgpu_window_result, frames), offsetof(flacgpu_window_result, bad_frames),"
        " offsetof(flacgpu_window_result, bad_crc16), offsetof(flacgpu_window_result, samples)); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    W, R = _lib.Window, _lib.WindowResult
    assert got == [C.sizeof(W), W.stream.offset, W.reserved.offset, W.start.offset, W.length.offset,
                   C.sizeof(R), R.rc.offset, R.frames.offset, R.bad_frames.offset, R.bad_crc16.offset, R.samples.offset]
    assert got[0] == 24 and got[5] == 24


# ---- flacgpu_window_frames against the model ----
def _matrix_block_sizes():
    from flac_codec_amd.gpu import scan_stream_host

    lists = []
    for st in fm.valid_cases():
        info, _, sizes = scan_stream_host(st.blob)
        assert info.frames == len(st.frame_sizes) and sizes.tolist() == list(st.frame_sizes), st.name
        lists.append((st.name, sizes.tolist()))
    return lists


def _check_list(name, sizes, seed):
    from flac_codec_amd.gpu import window_frames

    T = sum(sizes)
    rng = wn.rng_of(seed)
    windows = wn.fixed_windows(sizes) + wn.random_windows(rng, sizes, 200)
    assert (0, T) in windows and (T, 4) in windows and (T + 100, 3) in windows and (0, 0) in windows
    for start, length in windows:
        got = window_frames(sizes, start, length)
        assert got == wn.model_frames(sizes, start, length), (name, start, length)
        if length == 0 or start >= T:
            assert got == (0, 0, 0), (name, start, length)
        else:   # the frames selected hold the window's samples and not one frame more
            first, count, skip = got
            assert count >= 1 and skip < sizes[first]
            held = sum(sizes[first:first + count]) - skip
            assert held >= min(length, T - start) > held - sizes[first + count - 1], (name, start, length)


def test_window_frames_on_fixed_blocks():
    _check_list("16 x 200", [200] * 16, 1)


def test_window_frames_on_a_single_frame_and_on_none():
    _check_list("single", [4096], 2)
    _check_list("single sample", [1], 3)
    _check_list("none", [], 4)


def test_window_frames_on_the_matrix_block_sizes():
    lists = _matrix_block_sizes()
    assert len(lists) == 133
    assert any(len(set(sizes[:-1])) > 1 for _, sizes in lists), "no variable-block-size stream"
    for k, (name, sizes) in enumerate(lists):
        _check_list(name, sizes, 100 + k)


def test_window_frames_every_boundary_pair():
    """Every straddle of the variable-block stream: the pair across boundary k takes frames k - 1 and k."""
    from flac_codec_amd.gpu import window_frames

    st = next(s for s in fm.valid_cases() if s.name == "variable-block-size")
    sizes = list(st.frame_sizes)
    assert sizes == [16, 4096, 1, 577, 192]
    at = 0
    for k, n in enumerate(sizes[:-1]):
        at += n
        assert window_frames(sizes, at - 1, 2) == (k, 2, n - 1)
    assert window_frames(sizes, 16 + 4096 - 1, 3) == (1, 3, 4095)   # across the one-sample frame


def test_window_frames_refuses_overflow_and_null():
    from flac_codec_amd import _lib

    L = _lib.lib()
    sizes = (C.c_uint32 * 2)(100, 100)
    first, count, skip = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    args = (C.byref(first), C.byref(count), C.byref(skip))
    assert L.flacgpu_window_frames(sizes, 2, (1 << 64) - 1, 1, *args) == INVALID_ARG
    assert L.flacgpu_window_frames(sizes, 2, 1 << 63, 1 << 63, *args) == INVALID_ARG
    assert L.flacgpu_window_frames(None, 2, 0, 1, *args) == INVALID_ARG
    assert L.flacgpu_window_frames(sizes, 2, 0, 1, None, C.byref(count), C.byref(skip)) == INVALID_ARG
    assert (first.value, count.value, skip.value) == (7, 7, 7)
    assert L.flacgpu_window_frames(sizes, 2, (1 << 64) - 1, 0, *args) == OK     # start + length == 2^64 - 1
    assert (first.value, count.value, skip.value) == (0, 0, 0)
    assert L.flacgpu_window_frames(None, 0, 0, 10, *args) == OK


# ---- flacgpu_decoder_plan_windows on hand-made records ----
def _records(specs):
    """specs: [(rc, channels, bps, decoded_samples)] -> the records a scan would have filled."""
    from flac_codec_amd import _lib

    recs = (_lib.DecodedStream * max(len(specs), 1))()
    at = 0
    for r, (rc, ch, bps, n) in zip(recs, specs):
        r.rc, r.out_offset = rc, at
        r.info.channels, r.info.bits_per_sample, r.info.decoded_samples = ch, bps, n
        r.info.frames = 1 if n else 0
        if rc == 0:
            at += ch * n
    return recs


def _plan(specs, windows, dtype, C_pad, T_pad, layout=PADDED, reserved=0):
    """windows: [(stream, start, length)] or [(stream, start, length, reserved)]"""
    from flac_codec_amd import _lib

    fmt = _lib.OutFormat(dtype, layout, C_pad, reserved, T_pad)
    ws = (_lib.Window * max(len(windows), 1))()
    for w, t in zip(ws, windows):
        w.stream, w.start, w.length = t[:3]
        w.reserved = t[3] if len(t) > 3 else 0
    need = C.c_uint64(12345)
    rc = _lib.lib().flacgpu_decoder_plan_windows(C.byref(fmt), _records(specs), len(specs), ws, len(windows),
                                                 C.byref(need))
    return rc, need.value


#            0                  1              2              3                4                5
BATCH = [(0, 1, 16, 1000), (0, 2, 12, 77), (-1, 0, 0, 0), (0, 3, 8, 4097), (0, 2, 24, 500), (-1, 8, 24, 10 ** 9)]
NARROW = [(0, 0, 1000), (1, 70, 50), (3, 4000, 100), (2, 5, 64), (1, 0, 0), (0, 999, 1), (3, 10 ** 6, 7)]
LONGEST = 1000


@pytest.mark.parametrize("dtype,size", [(I32, 4), (I16, 2), (F32, 4)])
def test_bytes_are_windows_times_c_t_size(dtype, size):
    assert _plan(BATCH, NARROW, dtype, 3, LONGEST) == (OK, len(NARROW) * 3 * LONGEST * size)
    assert _plan(BATCH, NARROW, dtype, 8, LONGEST + 3) == (OK, len(NARROW) * 8 * (LONGEST + 3) * size)
    assert _plan(BATCH, [], dtype, 8, 100) == (OK, 0)
    assert _plan(BATCH, [], dtype, 0, 0) == (OK, 0)
    assert _plan(BATCH, [(2, 0, 0), (5, 3, 0)], dtype, 0, 0) == (OK, 0)   # failed streams need no channel


def test_window_must_name_a_stream():
    assert _plan(BATCH, NARROW + [(len(BATCH), 0, 1)], F32, 3, LONGEST)[0] == INVALID_ARG
    assert _plan(BATCH, [(0xFFFFFFFF, 0, 0)], F32, 3, LONGEST)[0] == INVALID_ARG
    assert _plan([], [(0, 0, 0)], F32, 3, LONGEST)[0] == INVALID_ARG


def test_window_reserved_must_be_zero():
    assert _plan(BATCH, NARROW + [(0, 0, 1, 1)], F32, 3, LONGEST)[0] == INVALID_ARG


def test_start_plus_length_must_not_overflow():
    assert _plan(BATCH, [(0, (1 << 64) - 1, 1)], F32, 3, LONGEST)[0] == INVALID_ARG
    assert _plan(BATCH, [(0, (1 << 64) - 5, 5)], F32, 3, LONGEST)[0] == INVALID_ARG
    assert _plan(BATCH, [(0, (1 << 64) - 6, 5)], F32, 3, LONGEST)[0] == OK   # far past the end: valid, and empty


def test_layout_must_be_padded():
    assert _plan(BATCH, NARROW, F32, 0, 0, layout=FLAT)[0] == INVALID_ARG
    assert _plan(BATCH, NARROW, F32, 3, LONGEST, layout=FLAT)[0] == INVALID_ARG
    assert _plan(BATCH, NARROW, F32, 3, LONGEST, layout=2)[0] == INVALID_ARG
    assert _plan(BATCH, NARROW, 3, 3, LONGEST)[0] == INVALID_ARG               # unknown dtype
    assert _plan(BATCH, NARROW, F32, 3, LONGEST, reserved=1)[0] == INVALID_ARG


def test_padding_must_cover_the_windows_and_the_named_streams():
    assert _plan(BATCH, NARROW, F32, 3, LONGEST - 1)[0] == INVALID_ARG   # the longest window
    assert _plan(BATCH, NARROW, F32, 2, LONGEST)[0] == INVALID_ARG       # stream 3 has 3 channels
    assert _plan(BATCH, [(3, 0, 0)], F32, 2, LONGEST)[0] == INVALID_ARG  # ... named by an empty window too
    assert _plan(BATCH, [w for w in NARROW if w[0] != 3], F32, 2, LONGEST)[0] == OK   # unnamed: does not matter
    assert _plan(BATCH, [(5, 0, 10)], F32, 1, 10)[0] == OK               # a failed stream's channels are not looked at
    assert _plan(BATCH, [(2, 5, 64)], F32, 0, 63)[0] == INVALID_ARG      # ... its window's length is


def test_int16_refuses_a_named_wide_stream_and_names_it():
    from flac_codec_amd import _lib

    assert _plan(BATCH, NARROW + [(4, 10, 20)], I16, 3, LONGEST)[0] == UNSUPPORTED
    assert b"stream 4" in _lib.lib().flacgpu_last_error()
    assert _plan(BATCH, [(4, 0, 0)], I16, 3, LONGEST)[0] == UNSUPPORTED
    assert _plan(BATCH, NARROW + [(4, 10, 20)], I32, 3, LONGEST)[0] == OK
    assert _plan(BATCH, NARROW + [(4, 10, 20)], F32, 3, LONGEST)[0] == OK


def test_int16_ignores_wide_streams_no_window_names_or_that_failed():
    assert _plan(BATCH, NARROW, I16, 3, LONGEST) == (OK, len(NARROW) * 3 * LONGEST * 2)   # stream 4 is unnamed
    assert _plan(BATCH, NARROW + [(5, 0, 9)], I16, 3, LONGEST)[0] == OK                    # stream 5 failed


def test_null_arguments_are_invalid():
    from flac_codec_amd import _lib

    L = _lib.lib()
    fmt = _lib.OutFormat(F32, PADDED, 3, 0, LONGEST)
    need = C.c_uint64(0)
    ws = (_lib.Window * 1)()
    recs = _records(BATCH)
    assert L.flacgpu_decoder_plan_windows(None, recs, len(BATCH), ws, 1, C.byref(need)) == INVALID_ARG
    assert L.flacgpu_decoder_plan_windows(C.byref(fmt), recs, len(BATCH), None, 1, C.byref(need)) == INVALID_ARG
    assert L.flacgpu_decoder_plan_windows(C.byref(fmt), recs, len(BATCH), ws, 1, None) == INVALID_ARG
    assert L.flacgpu_decoder_plan_windows(C.byref(fmt), recs, len(BATCH), None, 0, C.byref(need)) == OK
