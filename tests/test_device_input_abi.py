"""CPU-side checks of the batch decoder's device door (include/flacenc_gpu.h "streams that already lie in device
memory"): the exports, the ctypes signatures against the header, the refusal of a NULL handle without a device, and the
metadata walk (csrc/kernels/meta_walk.h) in its host build -- flacgpu_meta_walk_host against flacgpu_scan_stream_host on
the inputs of _meta_cases.py, and under AddressSanitizer in a stand-alone program (tools/meta_walk_check.cpp).  No GPU call."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import _meta_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flac-codec_amd", "csrc", "host")
SYMBOLS = ("flacgpu_decoder_scan_device", "flacgpu_decoder_scan_frames_device", "flacgpu_decoder_slot_bytes",
           "flacgpu_meta_walk_host")
INVALID_ARG, BUFFER_TOO_SMALL = -1, -5
SI_FIELDS = ("sample_rate", "channels", "bits_per_sample", "min_block", "max_block", "total_samples")


def test_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert set(SYMBOLS) <= _lib.exported_symbols()


# the header's parameter types as ctypes spells them
_CTYPE = {"flacgpu_decoder *": C.c_void_p, "void *": C.c_void_p, "uint8_t *": C.c_void_p,
          "const uint8_t *const *": C.POINTER(C.c_void_p), "const size_t *": C.POINTER(C.c_size_t),
          "uint32_t": C.c_uint32, "size_t": C.c_size_t, "uint64_t *": C.POINTER(C.c_uint64),
          "uint32_t *": C.POINTER(C.c_uint32), "const uint8_t *": C.c_char_p}


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "flacenc_gpu.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append(re.sub(r"\s*\b\w+$", "", p).replace("* ", "*").strip())   # the type, without the parameter's name
    return out


@pytest.mark.parametrize("name", SYMBOLS)
def test_lib_signatures_match_the_header(name):
    from flac_codec_amd import _lib

    structs = {"flacgpu_decoded_stream *": C.POINTER(_lib.DecodedStream), "flacgpu_raw_stream *": C.POINTER(_lib.RawStream),
               "flacgpu_stream_info *": C.POINTER(_lib.StreamInfo)}
    want = [structs.get(t) or _CTYPE[t] for t in _header_params(name)]
    fn = getattr(_lib.lib(), name)
    assert list(fn.argtypes) == want
    assert fn.restype is C.c_int


def test_null_handle_is_refused_without_a_device():
    from flac_codec_amd import _lib

    L = _lib.lib()
    n = C.c_uint64(0)
    recs = (_lib.DecodedStream * 1)()
    raw = (_lib.RawStream * 1)()
    ptrs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    assert L.flacgpu_decoder_scan_device(None, ptrs, lens, 1, None, recs, C.byref(n)) == INVALID_ARG
    assert b"flacgpu_decoder_scan_device" in L.flacgpu_last_error()
    assert L.flacgpu_decoder_scan_frames_device(None, ptrs, lens, 1, 0, None, recs, raw, C.byref(n), C.byref(n),
                                                C.byref(n)) == INVALID_ARG
    assert b"flacgpu_decoder_scan_frames_device" in L.flacgpu_last_error()
    assert L.flacgpu_decoder_slot_bytes(None, None, 0, C.byref(n)) == INVALID_ARG


def _walk(blob):
    from flac_codec_amd import _lib

    info, min_frame, at = _lib.StreamInfo(), C.c_uint32(77), C.c_uint64(77)
    rc = _lib.lib().flacgpu_meta_walk_host(blob, len(blob), C.byref(info), C.byref(min_frame), C.byref(at))
    return rc, info, min_frame.value, at.value


def _host(blob):
    """flacgpu_scan_stream_host: (rc, info, first frame byte or None when it found no frame)."""
    from flac_codec_amd import _lib

    info, n = _lib.StreamInfo(), C.c_uint32(0)
    off, sizes = (C.c_uint64 * 1)(), (C.c_uint32 * 1)()
    rc = _lib.lib().flacgpu_scan_stream_host(blob, len(blob), C.byref(info), off, sizes, 1, C.byref(n))
    first = None
    if rc in (0, BUFFER_TOO_SMALL) and n.value:
        offs, ns = (C.c_uint64 * n.value)(), (C.c_uint32 * n.value)()
        rc = _lib.lib().flacgpu_scan_stream_host(blob, len(blob), C.byref(info), offs, ns, n.value, C.byref(n))
        first = offs[0]
    return rc, info, first


def _check(label, blob):
    rc, info, min_frame, at = _walk(blob)
    want_rc, want, first = _host(blob)
    assert rc == want_rc, label
    for f in SI_FIELDS:
        assert getattr(info, f) == getattr(want, f), (label, f)
    assert bytes(info.md5) == bytes(want.md5), label
    # everything the frame scan and the decode fill stays 0
    assert (info.frames, info.bad_frames, info.bad_crc16, info.decoded_samples, info.md5_status) == (0, 0, 0, 0, 0), label
    marker, complete, si, model_at = mc.walk(blob)
    if rc == 0:
        assert complete and si is not None and at == model_at <= len(blob), label
        assert min_frame == int.from_bytes(si[4:7], "big"), label
        if first is not None:
            assert first == at, label   # the host scan's first frame starts where the walk says the metadata end
    else:
        assert at == 0, label
        assert not (complete and si is not None) or info.max_block < 1, label
        if si is None:
            assert bytes(info) == bytes(C.sizeof(info)), label
    return rc


def test_walk_equals_the_host_parser_on_the_foreign_matrix():
    cases = mc.foreign()
    assert len(cases) == 133
    assert [_check(label, blob) for label, blob in cases + mc.foreign_invalid()] == [0] * (len(cases) + 10)


def test_walk_equals_the_host_parser_at_every_truncation():
    blob, meta = mc.small_file()
    rcs = [_check(label, cut) for label, cut in mc.truncations()]
    assert len(rcs) == meta + 3 and rcs == [INVALID_ARG] * meta + [0] * 3


def test_walk_equals_the_host_parser_at_the_edges():
    got = {label: _check(label, blob) for label, blob in mc.edges()}
    refused = {label for label, rc in got.items() if rc}
    assert all(rc in (0, INVALID_ARG) for rc in got.values())
    assert refused == {
        "length 41", "wrong marker", "lower-case marker", "no last-block flag: the walk runs off the end",
        "no last-block flag, the end inside a block header", "a block passes the end by one byte",
        "second STREAMINFO truncated: the first stays in info", "type 0 with length 33", "type 0 with length 35",
        "max_block 0: refused", "empty", "the marker alone"}
    # the consequences as literals
    by = dict(mc.edges())
    _, info, _, at = _walk(by["two STREAMINFO blocks: the second wins"])
    assert (info.sample_rate, info.channels, info.bits_per_sample) == (48000, 2, 24)
    rc, info, _, _ = _walk(by["second STREAMINFO truncated: the first stays in info"])
    assert rc == INVALID_ARG and (info.sample_rate, info.bits_per_sample) == (8000, 8)
    _, _, _, at = _walk(by["70 KB PADDING behind STREAMINFO"])
    assert at == 4 + 38 + 70004 + 15
    for label in ("metadata ends exactly at len", "metadata ends exactly at len, 42 bytes"):
        assert _walk(by[label])[3] == len(by[label])


def test_null_data_is_not_dereferenced():
    from flac_codec_amd import _lib

    info, min_frame, at = _lib.StreamInfo(), C.c_uint32(0), C.c_uint64(0)
    assert _lib.lib().flacgpu_meta_walk_host(None, 1000, C.byref(info), C.byref(min_frame), C.byref(at)) == INVALID_ARG
    assert _lib.lib().flacgpu_meta_walk_host(b"fLaC", 4, None, C.byref(min_frame), C.byref(at)) == INVALID_ARG


def test_walk_under_address_sanitizer(tmp_path):
    """tools/meta_walk_check.cpp, a stand-alone C++ program, walks every truncation and every edge case from a heap block
    of exactly the input's size."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + san + [str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True,
                           text=True)
    if probe.returncode:
        pytest.skip("the sanitizer runtime cannot be linked here: " + (probe.stderr.strip().splitlines() or ["?"])[-1])
    exe = tmp_path / "meta_walk_check"
    build = [cxx, "-std=c++17", "-O1", "-g"] + san + [
             "-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tools", "meta_walk_check.cpp"),
             os.path.join(HOST, "flac_stream.cpp"), os.path.join(HOST, "checksums.cpp"), "-o", str(exe)]
    made = subprocess.run(build, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    blobs = [blob for _, blob in mc.truncations() + mc.edges()]
    with open(tmp_path / "inputs.bin", "wb") as f:
        for blob in blobs:
            f.write(len(blob).to_bytes(4, "little") + blob)
    run = subprocess.run([str(exe), str(tmp_path / "inputs.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    accepted = [mc.walk(b) for b in blobs]
    ok = [w for w, b in zip(accepted, blobs) if _walk(b)[0] == 0]
    assert run.stdout.split() == ["inputs", str(len(blobs)), "accepted", str(len(ok)), "frames_at",
                                  str(sum(w[3] for w in ok))]
