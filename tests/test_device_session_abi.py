"""CPU-side checks of the device sessions (flacenc_device_session_*): the exports, the ctypes layouts of
flacenc_session_chunk, flacenc_session_final, flacgpu_md5_piece and flacgpu_md5_state against the headers, and what
flacenc_device_session_plan -- pure host code -- refuses and answers.  No GPU call."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED, INVALID_BLOCK_SIZE = 0, -140, -151, -101
NO_MD5 = 1


def _L():
    from flac_codec_amd import encode

    return encode._stream_lib()


def test_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacenc_device_session_plan", "flacenc_device_session_open", "flacenc_device_session_header_len",
            "flacenc_device_session_write", "flacenc_device_session_finalize", "flacenc_device_session_close",
            "flacgpu_ingest_move", "flacgpu_ingest_stream_of"} <= _lib.exported_symbols()


def test_layouts_match_the_headers(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    structs = [("flacenc_session_chunk", _lib.SessionChunk),
               ("flacenc_session_final", _lib.SessionFinal),
               ("flacgpu_md5_piece", _lib.Md5Piece),
               ("flacgpu_md5_state", _lib.Md5State)]
    src = tmp_path / "layout.cpp"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_stream.h"\nint main() {\n'
        + "".join(f'  printf("%zu ", sizeof({name}));\n'
                  + "".join(f'  printf("%zu ", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
                  for name, cls in structs)
        + '  printf("\\n");\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, cls in structs:
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want


def _plan(bps=16, channels=2, n=3, max_chunk=44100, flags=0, block=None, opts=None):
    from flac_codec_amd.encode import Options

    o = opts or Options.default()
    if block:
        o = o.block_size(block)
    co = o._c_options()
    out = C.c_size_t(12345)
    rc = _L().flacenc_device_session_plan(C.byref(co), bps, channels, n, max_chunk, flags, C.byref(out))
    return rc, out.value, _L().flacenc_last_error().decode()


def _staging(block, channels, max_chunk, n):
    up4 = lambda v: (v + 3) // 4 * 4   # noqa: E731
    return 2 * 4 * n * (up4((block - 1) * channels) + up4(max_chunk * channels))


def test_plan_sizes():
    """two halves; in each, per stream, block_size - 1 carried samples and a chunk, both rounded up to 16 bytes; 128
    bytes of chain state and tables per stream unless the MD5 is off"""
    assert _plan()[:2] == (OK, _staging(4096, 2, 44100, 3) + 3 * 128)
    assert _plan(flags=NO_MD5)[:2] == (OK, _staging(4096, 2, 44100, 3))
    assert _plan(channels=3, n=5, max_chunk=7, block=64)[:2] == (OK, _staging(64, 3, 7, 5) + 5 * 128)
    assert _plan(channels=1, n=1, max_chunk=1, block=16)[:2] == (OK, 2 * 4 * (16 + 4) + 128)
    assert _plan(n=0)[:2] == (OK, 0)
    from flac_codec_amd.encode import Options

    co = Options.default()._c_options()
    assert _L().flacenc_device_session_plan(C.byref(co), 16, 2, 3, 100, 0, None) == OK   # the size is optional


def test_plan_refuses_what_the_batch_plan_refuses_for_the_shape():
    for kw, rc, text in [(dict(channels=0), INVALID_ARG, "channels outside 1..8"),
                         (dict(channels=9), INVALID_ARG, "channels outside 1..8"),
                         (dict(bps=0), INVALID_ARG, "bits per sample"),
                         (dict(bps=33), INVALID_ARG, "bits per sample"),
                         (dict(max_chunk=0), INVALID_ARG, "max_chunk is 0"),
                         (dict(flags=2), INVALID_ARG, "unknown flags"),
                         (dict(max_chunk=1 << 62), UNSUPPORTED, "exceeds 2^64"),
                         (dict(n=1 << 33), UNSUPPORTED, "streams")]:
        got = _plan(**kw)
        assert got[:2] == (rc, 12345) and text in got[2], (kw, got)
    assert _L().flacenc_device_session_plan(None, 16, 2, 1, 1, 0, None) == INVALID_ARG


def test_plan_and_open_pass_the_options_errors_through():
    from flac_codec_amd.encode import Options

    co = Options.default()._c_options()
    co.block_size = 15
    out = C.c_size_t(12345)
    assert _L().flacenc_device_session_plan(C.byref(co), 16, 2, 1, 100, 0, C.byref(out)) == INVALID_BLOCK_SIZE
    assert out.value == 12345
    h = C.c_void_p(777)
    totals = (C.c_uint64 * 1)(100)
    assert _L().flacenc_device_session_open(C.byref(co), 44100, 16, 2, totals, 1, 100, 0, C.byref(h)) == INVALID_BLOCK_SIZE
    assert not h.value   # refused before any device is looked for
    co = Options.default()._c_options()
    assert _L().flacenc_device_session_open(C.byref(co), 44100, 16, 2, totals, 1, 0, 0, C.byref(h)) == INVALID_ARG
    assert _L().flacenc_device_session_open(C.byref(co), 44100, 16, 2, None, 1, 100, 0, C.byref(h)) == INVALID_ARG
    assert _L().flacenc_device_session_header_len(None, 0) == 0
    _L().flacenc_device_session_close(None)
