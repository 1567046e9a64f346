"""CPU-side checks of the device-resident batch encoder (flacenc_encode_many_device): the exports, the ctypes layout of
flacenc_device_job against the header, what flacenc_device_batch_plan -- pure host code -- answers, and the conversion
rule (csrc/kernels/ingest_rule.h) through its host export flacenc_ingest_sample.  No GPU call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED = 0, -140, -151
I32, I16, F32 = 0, 1, 2
FLAT, PADDED = 0, 1
ALL_BPS = [4, 8, 12, 16, 20, 24, 25, 32]


def _L():
    from flac_codec_amd import encode

    return encode._stream_lib()


def test_device_batch_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacenc_device_batch_plan", "flacenc_encode_many_device", "flacenc_ingest_sample", "flacgpu_ingest_create",
            "flacgpu_ingest_destroy", "flacgpu_ingest_submit", "flacgpu_ingest_finish"} <= _lib.exported_symbols()


def test_device_job_layout_matches_header(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    fields = ["in_offset", "samples", "out", "out_cap", "out_len", "status", "altered", "md5"]
    src = tmp_path / "layout.cpp"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_stream.h"\nint main() {\n'
        '  printf("%zu %zu %u", sizeof(flacenc_device_job), sizeof(flacenc_tensor_format), FLACENC_DEVICE_NO_MD5);\n'
        + "".join(f'  printf(" %zu", offsetof(flacenc_device_job, {f}));\n' for f in fields)
        + '  printf("\\n");\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    J = _lib.DeviceJob
    assert got == [C.sizeof(J), C.sizeof(_lib.OutFormat), _lib.DEVICE_NO_MD5] + [getattr(J, f).offset for f in fields]


def _plan(specs, dtype, layout=FLAT, bps=16, channels=2, C_pad=0, T_pad=0, reserved=0, options=None):
    """specs: [(in_offset, samples)] -> (rc, in_elements, staging_bytes)"""
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import Options

    L = _L()
    co = (options or Options.default())._c_options()
    fmt = _lib.OutFormat(dtype, layout, C_pad, reserved, T_pad)
    jobs = (_lib.DeviceJob * max(len(specs), 1))()
    for j, (off, n) in zip(jobs, specs):
        j.in_offset, j.samples = off, n
    need, staging = C.c_size_t(12345), C.c_size_t(54321)
    rc = L.flacenc_device_batch_plan(C.byref(co), C.byref(fmt), bps, channels, jobs, len(specs), C.byref(need),
                                     C.byref(staging))
    return rc, need.value, staging.value


def _model(specs, layout, channels, C_pad, T_pad):
    in_elements = len(specs) * C_pad * T_pad if layout == PADDED else max([o + n * channels for o, n in specs if n], default=0)
    staging = 4 * sum((n * channels + 3) // 4 * 4 for _, n in specs)
    return OK, in_elements, staging


LENGTHS = [0, 1, 4095, 4096, 4097, 2 * 4096 + 5]


@pytest.mark.parametrize("dtype", [I32, I16, F32])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_plan_sizes_match_the_model(dtype, channels):
    padded = [(0, n) for n in LENGTHS]
    assert _plan(padded, dtype, PADDED, 16, channels, channels + 1, max(LENGTHS) + 5) == \
        _model(padded, PADDED, channels, channels + 1, max(LENGTHS) + 5)
    flat, at = [], 3
    for n in LENGTHS:
        flat.append((at, n))
        at += n * channels + 7
    flat = flat[::-1]   # any order
    assert _plan(flat, dtype, FLAT, 16, channels) == _model(flat, FLAT, channels, 0, 0)
    assert _plan([], dtype, FLAT, 16, channels) == (OK, 0, 0)
    assert _plan([], dtype, PADDED, 16, channels, channels, 10) == (OK, 0, 0)


def test_plan_refusals_write_nothing():
    two = [(0, 100), (200, 50)]
    refused = [
        (_plan(two, F32, PADDED, 16, 2, C_pad=1, T_pad=100), INVALID_ARG),            # channels_padded < channels
        (_plan(two, F32, PADDED, 16, 2, C_pad=2, T_pad=99), INVALID_ARG),             # a stream longer than samples_padded
        (_plan([(0, 100), (199, 50)], F32, FLAT, 16, 2), INVALID_ARG),                # FLAT streams overlap
        (_plan([(300, 50), (0, 100), (100, 150)], F32, FLAT, 16, 2), INVALID_ARG),    # ... in any order
        (_plan(two, I16, FLAT, 17, 2), UNSUPPORTED),                                  # I16 above 16 bits
        (_plan(two, I16, PADDED, 24, 2, C_pad=2, T_pad=100), UNSUPPORTED),
        (_plan(two, F32, FLAT, 16, 0), INVALID_ARG),                                  # channels / bps outside flacgpu_create's
        (_plan(two, F32, FLAT, 16, 9), INVALID_ARG),
        (_plan(two, F32, FLAT, 0, 2), INVALID_ARG),
        (_plan(two, F32, FLAT, 33, 2), INVALID_ARG),
        (_plan(two, 3, FLAT, 16, 2), INVALID_ARG),                                    # unknown type, unknown layout
        (_plan(two, F32, 2, 16, 2, C_pad=2, T_pad=100), INVALID_ARG),
        (_plan(two, F32, FLAT, 16, 2, reserved=1), INVALID_ARG),
        (_plan(two, F32, FLAT, 16, 2, C_pad=2), INVALID_ARG),                         # padded fields under FLAT
        (_plan(two, F32, FLAT, 16, 2, T_pad=100), INVALID_ARG),
    ]
    for (rc, need, staging), want in refused:
        assert (rc, need, staging) == (want, 12345, 54321)
    # streams that only touch are fine, and so is I16 at 16 bits and below
    assert _plan([(0, 100), (200, 50)], F32, FLAT, 16, 2)[0] == OK
    assert _plan(two, I16, FLAT, 16, 2)[0] == OK and _plan(two, I16, FLAT, 12, 2)[0] == OK


def test_plan_refuses_invalid_options():
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import Options

    co = Options.default()._c_options()
    co.block_size = 8   # below Options::block_size's minimum: InvalidBlockSize
    fmt = _lib.OutFormat(F32, FLAT, 0, 0, 0)
    jobs = (_lib.DeviceJob * 1)()
    jobs[0].samples = 10
    assert _L().flacenc_device_batch_plan(C.byref(co), C.byref(fmt), 16, 1, jobs, 1, None, None) == -101


# ---- the conversion rule --------------------------------------------------------------------------------------------
def _ingest(sample_type, raw, bps):
    a = C.c_int(-7)
    v = _L().flacenc_ingest_sample(sample_type, int(raw) & 0xFFFFFFFF, bps, C.byref(a))
    return v, a.value


def _numpy_f32(x, bps):
    """The issue's expression: clip(rint(float64(x) * 2.0**(bps-1)), lo, hi), NaN -> 0; altered: clamped or NaN."""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(x.astype(np.float64) * 2.0 ** (bps - 1))
    nan = np.isnan(r)
    r = np.where(nan, 0.0, r)
    out = np.clip(r, lo, hi)
    return out.astype(np.int64), (nan | (out != r)).astype(np.int64)


def _f32_inputs(bps):
    scale = 2.0 ** (bps - 1)
    xs = [0.0, -0.0, 1.0, -1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))),
          float(np.nextafter(np.float32(-1.0), np.float32(0.0))), float("inf"), float("-inf"), float("nan"),
          float(np.float32(1e-45)), float(np.float32(-1e-45)), float(np.float32(1e-40)), float(np.float32(1.1754942e-38)),
          3.5, -3.5, 1e30, -1e30]
    for k in (0, 1, 2, 3, 6, 7, (1 << (bps - 1)) - 2, (1 << (bps - 1)) - 1):   # half-way cases, both parities of k
        for sign in (1.0, -1.0):
            xs.append(sign * (k + 0.5) / scale)
    rng = np.random.default_rng(1234 + bps)
    xs += list(rng.uniform(-1.25, 1.25, 700).astype(np.float32))
    xs += list((rng.integers(-(1 << (bps - 1)) - 3, (1 << (bps - 1)) + 3, 300) / scale).astype(np.float32))
    return np.array(xs, dtype=np.float32)


@pytest.mark.parametrize("bps", ALL_BPS)
def test_float32_rule_matches_numpy(bps):
    xs = _f32_inputs(bps)
    want, want_alt = _numpy_f32(xs, bps)
    bits = xs.view(np.uint32)
    for i in range(xs.size):
        assert _ingest(F32, bits[i], bps) == (int(want[i]), int(want_alt[i])), (bps, float(xs[i]))
    assert want_alt.sum() > 0 and (want_alt == 0).sum() > 0


@pytest.mark.parametrize("bps", ALL_BPS)
def test_int32_rule_clamps_to_the_range(bps):
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    cases = {0, 1, -1, lo, hi, lo + 1, hi - 1, -(1 << 31), (1 << 31) - 1}
    if bps < 32:
        cases |= {lo - 1, hi + 1}
    for x in sorted(cases):
        assert _ingest(I32, x, bps) == (min(max(x, lo), hi), int(x < lo or x > hi)), (bps, x)


@pytest.mark.parametrize("bps", [4, 8, 12, 16])
def test_int16_rule_is_an_arithmetic_shift(bps):
    drop = 16 - bps
    for x in (0, 1, -1, 32767, -32768, 32766, -32767, 1 << drop, -(1 << drop), (1 << drop) - 1, 0x1234, -0x1234, 0x7FF0):
        raw = x & 0xFFFF
        assert _ingest(I16, raw, bps) == (x >> drop, int((x & ((1 << drop) - 1)) != 0)), (bps, x)
        assert _ingest(I16, raw | 0xABCD0000, bps)[0] == x >> drop   # only the low half is an element
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    assert _ingest(I16, 32767, bps)[0] == hi and _ingest(I16, -32768 & 0xFFFF, bps)[0] == lo


def test_combinations_plan_refuses_give_zero_and_altered():
    assert _ingest(I16, 0x1234, 17) == (0, 1)
    assert _ingest(I16, 0x1234, 24) == (0, 1)
    assert _ingest(3, 5, 16) == (0, 1)
    assert _ingest(I32, 5, 0) == (0, 1) and _ingest(I32, 5, 33) == (0, 1)
    assert _L().flacenc_ingest_sample(I32, 5, 16, None) == 5   # altered may be NULL


def _decode_rule(s, bps):
    """sample_bits<DT_F32> of kernels/decode_many.inc: (float)s * 2^-(bps - 1)."""
    return np.asarray(s).astype(np.float32) * np.float32(2.0 ** -(bps - 1))


@pytest.mark.parametrize("bps", [4, 8, 12, 16, 20, 24, 25])
def test_numpy_model_inverts_the_decoders_rule(bps):
    """The model the other tests compare with is itself an inverse of the decoder's rule (exact for bps <= 25)."""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    rng = np.random.default_rng(bps)
    s = np.unique(np.concatenate([np.arange(lo, min(lo + 2000, hi + 1)), np.arange(max(hi - 2000, lo), hi + 1),
                                  np.arange(max(-2000, lo), min(2001, hi + 1)), rng.integers(lo, hi + 1, 20000)]))
    want, alt = _numpy_f32(_decode_rule(s, bps), bps)
    assert np.array_equal(want, s) and not alt.any()


def test_float32_rule_inverts_the_decoders_for_every_sample(tmp_path):
    """ingest(F32, decode_rule(s)) == s, unaltered, for EVERY s in range at every bps <= 25: 2^26 calls of the
    library's own export, made from a small C++ program (a Python loop would take minutes)."""
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    src = tmp_path / "inverse.cpp"
    src.write_text(r"""
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
typedef int32_t (*ingest_fn)(uint32_t, uint32_t, uint32_t, int *);
int main(int argc, char **argv) {
    void *h = dlopen(argv[1], RTLD_NOW);
    if (!h) { printf("dlopen: %s\n", dlerror()); return 2; }
    ingest_fn ingest = (ingest_fn)dlsym(h, "flacenc_ingest_sample");
    if (!ingest) { printf("no symbol\n"); return 2; }
    unsigned long long checked = 0;
    for (uint32_t bps = 1; bps <= 25; bps++) {
        const int64_t lo = -((int64_t)1 << (bps - 1)), hi = ((int64_t)1 << (bps - 1)) - 1;
        const uint32_t scale_bits = (128u - bps) << 23;   /* 2^-(bps - 1), as sample_bits builds it */
        float scale;
        memcpy(&scale, &scale_bits, 4);
        for (int64_t s = lo; s <= hi; s++, checked++) {
            const float x = (float)(int32_t)s * scale;
            uint32_t raw;
            memcpy(&raw, &x, 4);
            int altered = -1;
            const int32_t got = ingest(2u, raw, bps, &altered);
            if (got != s || altered != 0) { printf("bps %u sample %lld -> %d altered %d\n", bps, (long long)s, got, altered); return 1; }
        }
    }
    printf("ok %llu\n", checked);
    return 0;
}
""")
    exe = tmp_path / "inverse"
    subprocess.check_call([cxx, "-O2", "-o", str(exe), str(src), "-ldl"])
    out = subprocess.run([str(exe), _lib.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["ok", str(2 ** 26 - 2)], out.stdout + out.stderr
