"""CPU-side checks of FLACGPU_SAMPLE_S24, the packed 24-bit element type of the batch decoder and the device encoder:
the constant against the header, what the pure host planners (flacgpu_decoder_plan_output, flacgpu_decoder_plan_windows,
flacenc_device_batch_plan) answer for it, and the conversion rule through flacenc_ingest_sample.  No GPU call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
ENC_INVALID_ARG, ENC_UNSUPPORTED = -140, -151
S24 = 24
FLAT, PADDED = 0, 1


def test_constant_matches_header(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    src = tmp_path / "s24.cpp"
    src.write_text('#include <stdio.h>\n#include "flacenc_gpu.h"\nint main() { printf("%u\\n", FLACGPU_SAMPLE_S24); }\n')
    exe = tmp_path / "s24"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert int(subprocess.check_output([str(exe)])) == _lib.SAMPLE_S24 == 24


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


def _plan(specs, dtype, layout=FLAT, C_pad=0, T_pad=0):
    from flac_codec_amd import _lib

    fmt = _lib.OutFormat(dtype, layout, C_pad, 0, T_pad)
    need = C.c_uint64(12345)
    rc = _lib.lib().flacgpu_decoder_plan_output(C.byref(fmt), _records(specs), len(specs), C.byref(need))
    return rc, need.value


def _plan_windows(specs, dtype, windows, C_pad, T_pad):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import window_array

    fmt = _lib.OutFormat(dtype, PADDED, C_pad, 0, T_pad)
    need = C.c_uint64(12345)
    w = window_array(windows)
    rc = _lib.lib().flacgpu_decoder_plan_windows(C.byref(fmt), _records(specs), len(specs), w, len(windows), C.byref(need))
    return rc, need.value


BATCH24 = [(0, 1, 24, 1000), (0, 2, 17, 77), (-1, 0, 0, 0), (0, 3, 8, 4097), (0, 2, 16, 0), (0, 8, 4, 5)]
ELEMENTS24, LONGEST24, WIDEST24 = 1000 + 2 * 77 + 3 * 4097 + 8 * 5, 4097, 8
BATCH25 = BATCH24 + [(0, 2, 25, 500)]


def test_plan_output_is_three_bytes_per_element():
    assert _plan(BATCH24, S24) == (OK, 3 * ELEMENTS24)
    assert _plan(BATCH24, S24, PADDED, WIDEST24, LONGEST24 + 5) == (OK, 3 * len(BATCH24) * WIDEST24 * (LONGEST24 + 5))
    assert _plan([], S24) == (OK, 0)
    assert _plan([(0, 1, 24, 1)], S24) == (OK, 3)   # no rounding up to a dword


def test_plan_windows_is_three_bytes_per_element():
    windows = [(0, 5, 300), (1, 70, 40), (3, 0, 0), (2, 0, 10)]
    assert _plan_windows(BATCH24, S24, windows, 3, 301) == (OK, 3 * len(windows) * 3 * 301)
    assert _plan_windows(BATCH24, S24, [], 3, 301) == (OK, 0)


def test_a_25_bit_stream_is_refused_and_named():
    from flac_codec_amd import _lib

    for layout, c_pad, t_pad in ((FLAT, 0, 0), (PADDED, WIDEST24, LONGEST24)):
        assert _plan(BATCH25, S24, layout, c_pad, t_pad)[0] == UNSUPPORTED
        assert b"stream 6" in _lib.lib().flacgpu_last_error()
    assert _plan(BATCH25, 0)[0] == OK and _plan(BATCH25, 2)[0] == OK            # the other types take it
    assert _plan(BATCH24 + [(-1, 2, 25, 500)], S24) == (OK, 3 * ELEMENTS24)     # a failed stream is not looked at
    # windows: only a window that names the stream refuses
    assert _plan_windows(BATCH25, S24, [(0, 0, 10), (1, 0, 10)], 2, 10) == (OK, 3 * 2 * 2 * 10)
    assert _plan_windows(BATCH25, S24, [(0, 0, 10), (6, 3, 4)], 2, 10)[0] == UNSUPPORTED
    assert b"stream 6" in _lib.lib().flacgpu_last_error()


@pytest.mark.parametrize("dtype", [3, 4, 23, 25])
def test_other_values_are_still_unknown(dtype):
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import Options, _stream_lib

    assert _plan(BATCH24, dtype)[0] == INVALID_ARG
    assert _plan(BATCH24, dtype, PADDED, WIDEST24, LONGEST24)[0] == INVALID_ARG
    assert _plan_windows(BATCH24, dtype, [(0, 0, 10)], 1, 10)[0] == INVALID_ARG
    co = Options.default()._c_options()
    fmt = _lib.OutFormat(dtype, PADDED, 2, 0, 100)
    jobs = (_lib.DeviceJob * 1)()
    jobs[0].samples = 100
    assert _stream_lib().flacenc_device_batch_plan(C.byref(co), C.byref(fmt), 16, 2, jobs, 1, None, None) == ENC_INVALID_ARG
    a = C.c_int(0)
    assert _stream_lib().flacenc_ingest_sample(dtype, 0x123456, 16, C.byref(a)) == 0 and a.value == 1


def _device_plan(fmt_args, bps, channels, specs):
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import Options, _stream_lib

    co = Options.default()._c_options()
    fmt = _lib.OutFormat(*fmt_args)
    jobs = (_lib.DeviceJob * max(len(specs), 1))()
    for j, (off, n) in zip(jobs, specs):
        j.in_offset, j.samples = off, n
    elements, staging = C.c_size_t(777), C.c_size_t(777)
    rc = _stream_lib().flacenc_device_batch_plan(C.byref(co), C.byref(fmt), bps, channels, jobs, len(specs),
                                                 C.byref(elements), C.byref(staging))
    return rc, elements.value, staging.value


def test_device_batch_plan_counts_three_byte_elements():
    # PADDED: the elements of the whole tensor; staging: every stream's int32 samples rounded up to 4
    assert _device_plan((S24, PADDED, 3, 0, 4102), 24, 2, [(0, 4097), (0, 1), (0, 4102)]) == \
        (0, 3 * 3 * 4102, 4 * (8196 + 4 + 8204))
    # FLAT: up to the end of the last stream, in elements (not bytes); gaps are the caller's
    assert _device_plan((S24, FLAT, 0, 0, 0), 20, 3, [(3, 100), (400, 7)]) == (0, 400 + 21, 4 * (300 + 24))
    assert _device_plan((S24, FLAT, 0, 0, 0), 24, 1, [(0, 10), (9, 5)])[0] == ENC_INVALID_ARG   # overlap, in elements
    assert _device_plan((S24, FLAT, 0, 0, 0), 24, 1, [(0, 10), (10, 5)])[0] == 0                # touching is fine
    for bps in (1, 16, 24):
        assert _device_plan((S24, PADDED, 1, 0, 10), bps, 1, [(0, 10)])[0] == 0


def test_device_batch_plan_refuses_25_bits():
    from flac_codec_amd.encode import _stream_lib

    for fmt in ((S24, PADDED, 2, 0, 100), (S24, FLAT, 0, 0, 0)):
        assert _device_plan(fmt, 25, 2, [(0, 100)])[0] == ENC_UNSUPPORTED
        assert b"25" in _stream_lib().flacenc_last_error()
        assert _device_plan(fmt, 32, 2, [(0, 100)])[0] == ENC_UNSUPPORTED


# ---- the conversion rule
def decode_bits(v, bps):
    """The decoder's side of the rule: the 24 bits of an output element."""
    return (np.asarray(v, dtype=np.int64) << (24 - bps)) & 0xFFFFFF


def ingest(raw, bps):
    """flacenc_ingest_sample(24, ...) over an array -> (samples, altered flags)."""
    from flac_codec_amd.encode import _stream_lib

    f = _stream_lib().flacenc_ingest_sample
    f.restype = C.c_int32
    a = C.c_int(0)
    out, alt = np.empty(len(raw), dtype=np.int64), np.empty(len(raw), dtype=np.int64)
    for i, r in enumerate(raw):
        out[i] = f(S24, int(r), bps, C.byref(a))
        alt[i] = a.value
    return out, alt


def test_ingest_inverts_decode_for_every_value_up_to_12_bits():
    total = 0
    for bps in range(1, 13):
        v = np.arange(-(1 << (bps - 1)), 1 << (bps - 1), dtype=np.int64)
        got, alt = ingest(decode_bits(v, bps), bps)
        assert np.array_equal(got, v) and not alt.any(), bps
        total += v.size
    assert total == 8190


@pytest.mark.parametrize("bps", range(13, 25))
def test_ingest_inverts_decode_on_seeded_values(bps):
    rng = np.random.default_rng(2400 + bps)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    v = np.concatenate([rng.integers(lo, hi + 1, 4096), [lo, hi, 0, -1]]).astype(np.int64)
    raw = decode_bits(v, bps)
    got, alt = ingest(raw, bps)
    assert np.array_equal(got, v) and not alt.any()
    drop = 24 - bps
    if drop:   # one set bit among the dropped ones: the same sample, altered
        dirty = raw | (1 << rng.integers(0, drop, raw.size))
        got, alt = ingest(dirty, bps)
        assert np.array_equal(got, v) and alt.all()
    else:      # at 24 bits nothing is dropped: every 24-bit pattern is a sample
        got, alt = ingest(raw ^ 1, bps)
        assert np.array_equal(got, v ^ 1) and not alt.any()


def test_ingest_ignores_bits_24_to_31():
    rng = np.random.default_rng(7)
    for bps in (1, 12, 20, 24):
        v = rng.integers(-(1 << (bps - 1)), 1 << (bps - 1), 512).astype(np.int64)
        raw = decode_bits(v, bps)
        for top in (0xFF000000, 0x80000000, 0x01000000, 0x5A000000):
            got, alt = ingest(raw | top, bps)
            assert np.array_equal(got, v) and not alt.any(), (bps, hex(top))


def test_ingest_refuses_more_than_24_bits():
    from flac_codec_amd.encode import _stream_lib

    a = C.c_int(0)
    for bps in (25, 32, 0, 33):
        assert _stream_lib().flacenc_ingest_sample(S24, 0x7FFFFF, bps, C.byref(a)) == 0 and a.value == 1
