"""CPU-side checks of the device encoder's back door (flacenc_encode_many_device_out): the exports, the ctypes layout of
flacenc_device_out_job and flacgpu_place_run against the headers, and what flacenc_device_out_plan -- pure host code --
refuses.  No GPU call."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED = 0, -140, -151
I16, F32 = 1, 2
FLAT, PADDED = 0, 1


def _L():
    from flac_codec_amd import encode

    return encode._stream_lib()


def test_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacenc_device_out_plan", "flacenc_encode_many_device_out"} <= _lib.exported_symbols()


def test_layouts_match_the_headers(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    job = ["in_offset", "samples", "out_offset", "out_cap", "out_len", "status", "altered", "md5"]
    run = ["src", "dst", "n"]
    src = tmp_path / "layout.cpp"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_stream.h"\nint main() {\n'
        '  printf("%zu %zu", sizeof(flacenc_device_out_job), sizeof(flacgpu_place_run));\n'
        + "".join(f'  printf(" %zu", offsetof(flacenc_device_out_job, {f}));\n' for f in job)
        + "".join(f'  printf(" %zu", offsetof(flacgpu_place_run, {f}));\n' for f in run)
        + '  printf("\\n");\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    J, R = _lib.DeviceOutJob, _lib.PlaceRun
    assert got == [C.sizeof(J), C.sizeof(R)] + [getattr(J, f).offset for f in job] + [getattr(R, f).offset for f in run]


def _last_error():
    return _L().flacenc_last_error().decode()


def _other_error():
    """leaves a text of another entry point in flacenc_last_error, so that a refusal below is seen to set its own"""
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import Options

    co = Options.default()._c_options()
    fmt = _lib.OutFormat(F32, FLAT, 0, 0, 0)
    assert _L().flacenc_device_batch_plan(C.byref(co), C.byref(fmt), 16, 2, None, 1, None, None) == INVALID_ARG
    assert "a null argument" in _last_error()


def _plan(slots, d_out_bytes, specs=None, dtype=F32, layout=FLAT, bps=16, channels=2, C_pad=0, T_pad=0):
    """slots: [(out_offset, out_cap)]; specs: [(in_offset, samples)] (default: streams of 100 samples that do not overlap)
    -> (rc, in_elements, staging_bytes, the error text)"""
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import Options

    co = Options.default()._c_options()
    fmt = _lib.OutFormat(dtype, layout, C_pad, 0, T_pad)
    specs = specs or [(i * 100 * channels, 100) for i in range(len(slots))]
    jobs = (_lib.DeviceOutJob * max(len(slots), 1))()
    for j, (off, n), (o, c) in zip(jobs, specs, slots):
        j.in_offset, j.samples, j.out_offset, j.out_cap = off, n, o, c
        j.out_len, j.status = 777, 55   # a refused call writes no job field
    need, staging = C.c_size_t(12345), C.c_size_t(54321)
    _other_error()
    rc = _L().flacenc_device_out_plan(C.byref(co), C.byref(fmt), bps, channels, jobs, len(slots), d_out_bytes,
                                      C.byref(need), C.byref(staging))
    assert all((j.out_len, j.status) == (777, 55) for j in jobs[:len(slots)])
    return rc, need.value, staging.value, _last_error()


def _refused(got, rc, text):
    assert got[:3] == (rc, 12345, 54321), got
    assert text in got[3], got[3]


def test_plan_accepts_slots_in_any_order_with_gaps():
    slots = [(1000, 500), (3, 400), (403, 1), (2001, 90), (1500, 501)]   # touching, gaps, any byte, any order
    rc, need, staging, _ = _plan(slots, 2091)
    assert (rc, need, staging) == (OK, 5 * 200, 4 * 5 * 200)
    assert _plan([], 0)[:3] == (OK, 0, 0)
    assert _plan([(0, 0)], 0)[0] == OK


def test_plan_refuses_a_slot_past_the_buffer():
    _refused(_plan([(0, 100), (100, 101)], 200), INVALID_ARG, "flacenc_device_out_plan: stream 1")
    _refused(_plan([(201, 0)], 200), INVALID_ARG, "reaches past d_out_bytes")
    assert _plan([(0, 100), (100, 100)], 200)[0] == OK
    assert _plan([(200, 0)], 200)[0] == OK


def test_plan_refuses_an_overflowing_slot():
    big = (1 << 64) - 1
    _refused(_plan([(big, 2)], 200), INVALID_ARG, "out_offset + out_cap overflows")
    _refused(_plan([(0, 10), (16, big - 3)], big), INVALID_ARG, "overflows")


def test_plan_refuses_overlapping_slots():
    _refused(_plan([(0, 100), (99, 10)], 200), INVALID_ARG, "two slots overlap")
    _refused(_plan([(150, 10), (0, 100), (120, 31)], 200), INVALID_ARG, "two slots overlap")   # in any order
    _refused(_plan([(10, 50), (20, 5)], 200), INVALID_ARG, "two slots overlap")                # one inside another
    _refused(_plan([(10, 50), (10, 50)], 200), INVALID_ARG, "two slots overlap")


def test_plan_accepts_a_zero_cap_slot_inside_another():
    assert _plan([(0, 100), (50, 0), (0, 0), (100, 0), (100, 50)], 200)[0] == OK


def test_plan_passes_the_batch_plans_refusals_through():
    _refused(_plan([(0, 10), (10, 10)], 100, dtype=I16, bps=24), UNSUPPORTED, "int16")
    _refused(_plan([(0, 10), (10, 10)], 100, specs=[(0, 100), (199, 50)]), INVALID_ARG, "FLAT streams overlap")
    _refused(_plan([(0, 10), (10, 10)], 100, layout=PADDED, C_pad=1, T_pad=100), INVALID_ARG, "channels_padded")


def test_encode_runs_the_plans_checks_first():
    """a refused call launches nothing: these return before any device is looked for"""
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import Options

    co = Options.default()._c_options()
    fmt = _lib.OutFormat(F32, FLAT, 0, 0, 0)
    jobs = (_lib.DeviceOutJob * 2)()
    for j, (off, slot) in zip(jobs, [(0, (0, 100)), (200, (99, 10))]):
        j.in_offset, j.samples, (j.out_offset, j.out_cap), j.status = off, 100, slot, 55
    _other_error()
    rc = _L().flacenc_encode_many_device_out(C.byref(co), 4096, C.byref(fmt), 44100, 16, 2, jobs, 2, 4096, 200, 0, None)
    assert rc == INVALID_ARG and "two slots overlap" in _last_error() and [j.status for j in jobs] == [55, 55]
    jobs[1].out_offset = 100
    rc = _L().flacenc_encode_many_device_out(C.byref(co), 4096, C.byref(fmt), 44100, 16, 2, jobs, 2, 4096, 200, 2, None)
    assert rc == INVALID_ARG and "unknown flags" in _last_error() and [j.status for j in jobs] == [55, 55]
