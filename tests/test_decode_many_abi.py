"""CPU-side checks of the batch decoder (flacgpu_decoder_*): its exports, the ctypes layout of
flacgpu_decoded_stream against the header, the CRC-16 algebra its frame scan relies on, and the
mapping of a stream's record to decode.verify's result.  No GPU call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("flacgpu_decoder_create", "flacgpu_decoder_destroy", "flacgpu_decoder_scan", "flacgpu_decoder_decode")


def test_decoder_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert set(SYMBOLS) <= _lib.exported_symbols()


def test_decoded_stream_layout_matches_header(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_gpu.h"\n'
        "int main() { printf(\"%zu %zu %zu %zu %zu %u %u\\n\", sizeof(flacgpu_decoded_stream),"
        " offsetof(flacgpu_decoded_stream, rc), offsetof(flacgpu_decoded_stream, out_offset),"
        " offsetof(flacgpu_decoded_stream, info), sizeof(flacgpu_stream_info),"
        " FLACGPU_DECODE_OUT_DEVICE, FLACGPU_DECODE_NO_MD5); }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _lib.DecodedStream
    assert got == [C.sizeof(D), D.rc.offset, D.out_offset.offset, D.info.offset, C.sizeof(_lib.StreamInfo),
                   _lib.DECODE_OUT_DEVICE, _lib.DECODE_NO_MD5]


# ---- the CRC-16 algebra of kernels/frame_scan.inc (poly 0x8005, MSB first, init 0, no final XOR) ----
def _mulmod(a, b):
    r = 0
    for i in range(15, -1, -1):
        r = ((r << 1) ^ 0x8005) & 0xFFFF if r & 0x8000 else (r << 1) & 0xFFFF
        if (b >> i) & 1:
            r ^= a
    return r


def _xpow_bytes(nbytes):   # gf_xpow_bytes: x^(8 nbytes) mod P through the order 32767 of x
    e = (nbytes % 32767) * 8 % 32767
    r, v = 1, 2
    for i in range(15):
        if (e >> i) & 1:
            r = _mulmod(r, v)
        v = _mulmod(v, v)
    return r


def test_x_has_order_32767_mod_p():
    v = 1
    for k in range(1, 32768):
        v = _mulmod(v, 2)
        if v == 1:
            break
    assert k == 32767


def test_prefix_crc_identity_against_the_oracle():
    """CRC(s, e) = P(e) ^ P(s) x^(8 (e - s)) with P(k) = CRC(bytes[0, k)), and bytes [q-2, q) are the CRC-16 of
    [s, q-2) exactly when CRC(s, q) == 0 -- the two facts the link kernel's test stands on."""
    import _oracle as orc

    rng = np.random.default_rng(7)
    for trial in range(40):
        n = int(rng.integers(2, 5000))
        buf = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        P = lambda k: orc.crc16(buf[:k])  # noqa: E731
        for _ in range(5):
            s = int(rng.integers(0, n - 1))
            e = int(rng.integers(s + 1, n + 1))
            assert orc.crc16(buf[s:e]) == P(e) ^ _mulmod(P(s), _xpow_bytes(e - s))
        s = int(rng.integers(0, n - 1))
        q = int(rng.integers(s + 2, n + 1))
        ok = orc.crc16(buf[s:q - 2]) == (buf[q - 2] << 8 | buf[q - 1])
        assert ok == (orc.crc16(buf[s:q]) == 0)
        fixed = buf[:q - 2] + orc.crc16(buf[s:q - 2]).to_bytes(2, "big")
        assert orc.crc16(fixed[s:q]) == 0
        # the link kernel's form: CRC(s, q) == 0 exactly when P(q) x^(-8q) == P(s) x^(-8s)
        Pf = lambda k: orc.crc16(fixed[:k])  # noqa: E731
        A = lambda k: _mulmod(Pf(k), _xpow_bytes(32767 - k % 32767))  # noqa: E731
        assert A(q) == A(s)
        if buf[q - 1] != fixed[q - 1] or buf[q - 2] != fixed[q - 2]:
            assert _mulmod(P(q), _xpow_bytes(32767 - q % 32767)) != _mulmod(P(s), _xpow_bytes(32767 - s % 32767))
    for d in (1, 2, 63, 64, 4095, 32767, 32768, 10 ** 9 + 7, 1 << 40):   # long distances reduce through the order
        ref = 1
        for _ in range((8 * d) % 32767):
            ref = _mulmod(ref, 2)
        assert _xpow_bytes(d) == ref


@pytest.mark.parametrize("rc,bad,crc,status,want", [
    (0, 0, 0, 1, "MD5_MATCH"), (0, 0, 0, 0, "MD5_MISMATCH"), (0, 0, 0, 2, "NO_MD5"),
    (-1, 0, 0, 0, None), (0, 1, 0, 1, None), (0, 0, 1, 1, None)])
def test_verify_result_mapping(rc, bad, crc, status, want):
    from flac_codec_amd import _lib
    from flac_codec_amd.decode import DecodeError, Verified, _result

    class Rec:
        pass

    r = Rec()
    r.rc = rc
    r.info = _lib.StreamInfo()
    r.info.bad_frames, r.info.bad_crc16, r.info.md5_status, r.info.frames = bad, crc, status, 3
    got = _result(r)
    if want is None:
        assert isinstance(got, DecodeError)
    else:
        assert got is Verified[want]

