"""CPU-side checks of the batch decoder's output formats (flacgpu_decoder_plan_output, flacgpu_decoder_decode_as):
the exports, the ctypes layout of flacgpu_out_format and the new constants against the header, and what
plan_output -- a pure host function -- answers for hand-made records.  No GPU call."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2


def test_format_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacgpu_decoder_plan_output", "flacgpu_decoder_decode_as"} <= _lib.exported_symbols()


def test_out_format_layout_and_constants_match_header(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_gpu.h"\n'
        "int main() { printf(\"%zu %zu %zu %zu %zu %zu %u %u %u %u %u\\n\", sizeof(flacgpu_out_format),"
        " offsetof(flacgpu_out_format, dtype), offsetof(flacgpu_out_format, layout),"
        " offsetof(flacgpu_out_format, channels_padded), offsetof(flacgpu_out_format, reserved),"
        " offsetof(flacgpu_out_format, samples_padded), FLACGPU_SAMPLE_I32, FLACGPU_SAMPLE_I16, FLACGPU_SAMPLE_F32,"
        " FLACGPU_LAYOUT_FLAT, FLACGPU_LAYOUT_PADDED); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    F = _lib.OutFormat
    assert got == [C.sizeof(F), F.dtype.offset, F.layout.offset, F.channels_padded.offset, F.reserved.offset,
                   F.samples_padded.offset, _lib.SAMPLE_I32, _lib.SAMPLE_I16, _lib.SAMPLE_F32, _lib.LAYOUT_FLAT,
                   _lib.LAYOUT_PADDED]
    assert got[6:] == [0, 1, 2, 0, 1]


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


def _plan(specs, dtype, layout=0, C_pad=0, T_pad=0, reserved=0):
    from flac_codec_amd import _lib

    fmt = _lib.OutFormat(dtype, layout, C_pad, reserved, T_pad)
    need = C.c_uint64(12345)
    rc = _lib.lib().flacgpu_decoder_plan_output(C.byref(fmt), _records(specs), len(specs), C.byref(need))
    return rc, need.value


BATCH16 = [(0, 1, 16, 1000), (0, 2, 12, 77), (-1, 0, 0, 0), (0, 3, 8, 4097), (0, 2, 16, 0)]   # elements: 13445
ELEMENTS16, LONGEST16, WIDEST16 = 1000 + 2 * 77 + 3 * 4097, 4097, 3
BATCH24 = BATCH16 + [(0, 2, 24, 500)]


@pytest.mark.parametrize("dtype,size", [(0, 4), (1, 2), (2, 4)])
def test_flat_bytes_are_elements_times_element_size(dtype, size):
    assert _plan(BATCH16, dtype) == (OK, ELEMENTS16 * size)


@pytest.mark.parametrize("dtype,size", [(0, 4), (1, 2), (2, 4)])
def test_padded_bytes_are_n_c_t_size(dtype, size):
    assert _plan(BATCH16, dtype, 1, 8, LONGEST16 + 5) == (OK, len(BATCH16) * 8 * (LONGEST16 + 5) * size)
    assert _plan(BATCH16, dtype, 1, WIDEST16, LONGEST16) == (OK, len(BATCH16) * WIDEST16 * LONGEST16 * size)


def test_int16_refuses_a_24_bit_stream_and_names_it():
    from flac_codec_amd import _lib

    for layout, c_pad, t_pad in ((0, 0, 0), (1, 3, 4097)):
        assert _plan(BATCH24, 1, layout, c_pad, t_pad)[0] == UNSUPPORTED
        assert b"stream 5" in _lib.lib().flacgpu_last_error()
    assert _plan(BATCH24, 0)[0] == OK and _plan(BATCH24, 2)[0] == OK   # the other types take it


def test_int16_ignores_a_24_bit_stream_that_failed():
    failed = BATCH16 + [(-1, 2, 24, 500)]
    assert _plan(failed, 1) == (OK, ELEMENTS16 * 2)
    assert _plan(failed, 1, 1, WIDEST16, LONGEST16) == (OK, len(failed) * WIDEST16 * LONGEST16 * 2)


def test_padding_must_cover_every_good_stream():
    assert _plan(BATCH16, 2, 1, WIDEST16, LONGEST16 - 1)[0] == INVALID_ARG
    assert _plan(BATCH16, 2, 1, WIDEST16 - 1, LONGEST16)[0] == INVALID_ARG
    assert _plan(BATCH16, 2, 1, 0, LONGEST16)[0] == INVALID_ARG
    assert _plan(BATCH16, 2, 1, WIDEST16, 0)[0] == INVALID_ARG
    # a failed stream's fields are not looked at
    assert _plan(BATCH16 + [(-1, 8, 16, 10 ** 9)], 2, 1, WIDEST16, LONGEST16)[0] == OK


def test_malformed_formats_are_invalid():
    assert _plan(BATCH16, 2, 1, WIDEST16, LONGEST16, reserved=1)[0] == INVALID_ARG
    assert _plan(BATCH16, 2, 0, reserved=7)[0] == INVALID_ARG
    assert _plan(BATCH16, 2, 0, C_pad=3)[0] == INVALID_ARG        # padded fields under FLAT
    assert _plan(BATCH16, 2, 0, T_pad=4097)[0] == INVALID_ARG
    assert _plan(BATCH16, 3)[0] == INVALID_ARG                    # unknown dtype
    assert _plan(BATCH16, 0, 2, WIDEST16, LONGEST16)[0] == INVALID_ARG   # unknown layout


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_batches_without_samples(dtype):
    assert _plan([], dtype) == (OK, 0)
    assert _plan([], dtype, 1, 0, 0) == (OK, 0)
    assert _plan([], dtype, 1, 8, 100) == (OK, 0)
    nothing = [(0, 2, 16, 0), (-1, 0, 0, 0)]   # no stream has samples: zero padding is valid
    assert _plan(nothing, dtype, 0) == (OK, 0)
    assert _plan(nothing, dtype, 1, 0, 0) == (OK, 0)
    assert _plan(nothing, dtype, 1, 1, 10) == (OK, 2 * 1 * 10 * (2 if dtype == 1 else 4))
