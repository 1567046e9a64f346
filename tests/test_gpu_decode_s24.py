"""flacgpu_decoder_decode_as / decode_many(dtype="int24"): packed 24-bit output of the batch decoder.

The inputs are the hand-built matrix (_foreign_matrix.py): its st.pcm is the correct answer by construction, and the
expectation is that PCM converted in numpy by the header's definition -- (sample << (24 - bps)) & 0xFFFFFF as three
little-endian bytes, element e at byte 3 * e -- never an output of the code under test.  Every buffer is pre-filled with
0x7F bytes between two 256-byte guards: after a decode the streams' bytes equal the expectation, every other byte
inside out_bytes is zero, and the guards are untouched."""
import functools

import numpy as np
import pytest

import _foreign_matrix as fm

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0x7F
S24 = 24
FLAT, PADDED = 0, 1


def pack24(pcm, bps):
    """int32 PCM of bps bits -> uint8 [..., 3]: the header's definition of an S24 element."""
    assert bps <= 24
    v = (np.asarray(pcm).astype(np.int64) << (24 - bps)) & 0xFFFFFF
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8)


@pytest.fixture(scope="module")
def dec():
    from flac_codec_amd.gpu import Decoder

    d = Decoder(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def subset():
    """The matrix's streams of at most 24 bits -- and what the filter must not lose."""
    every = list(fm.valid_cases())
    cases = [s for s in every if s.bps <= 24]
    assert len(every) == 133 and len(cases) == 133 - 8 and all(s.bps > 24 for s in every if s not in cases)
    assert {1, 2, 8} <= {s.channels for s in cases} and {4, 17, 24} <= {s.bps for s in cases}
    assert any(s.name == "wasted-16" for s in cases)
    assert any(n < 6 for s in cases for n in s.frame_sizes)   # runs shorter than one 16-byte group
    return cases


@functools.lru_cache(maxsize=None)
def expected(layout):
    """(format arguments, the out_bytes a decode of subset() must leave), computed once and never modified."""
    cases = subset()
    if layout == FLAT:
        return (S24, FLAT, 0, 0, 0), np.concatenate([pack24(s.pcm, s.bps).reshape(-1) for s in cases])
    T = max(s.pcm.size // s.channels for s in cases) + 5   # + 5: rows start at every byte phase
    assert {(3 * T * r) % 16 for r in range(16)} == set(range(16))
    want = np.zeros((len(cases), 8, T, 3), dtype=np.uint8)
    for i, s in enumerate(cases):
        n = s.pcm.size // s.channels
        want[i, :s.channels, :n] = pack24(s.pcm.reshape(n, s.channels).T, s.bps)
    return (S24, PADDED, 8, 0, T), want.reshape(-1)


def decode_raw(dec, recs, n, fmt, dest, md5=False, shift=0):
    """One decode_as into a 0x7F-filled buffer with guards, `out` shift bytes behind the first guard; returns (the
    whole buffer as host bytes, out_bytes)."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    need = Decoder.plan_output(fmt, recs, n)
    flags = 0 if md5 else _lib.DECODE_NO_MD5
    if dest == "device":
        buf = torch.full((GUARD + shift + need + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0
        try:
            dec.decode_as(buf.data_ptr() + GUARD + shift, need, fmt, flags | _lib.DECODE_OUT_DEVICE, recs)
        finally:
            raw = buf.cpu().numpy()
    else:
        raw = np.full(GUARD + shift + need + GUARD, FILL, dtype=np.uint8)
        dec.decode_as(raw.ctypes.data + GUARD + shift, need, fmt, flags, recs)
    return raw, need


def check(raw, need, want, shift=0):
    assert need == want.size
    at = GUARD + shift
    assert (raw[:at] == FILL).all() and (raw[at + need:] == FILL).all(), "a guard was written"
    got = raw[at:at + need]
    if not np.array_equal(got, want):
        where = np.flatnonzero(got != want)
        raise AssertionError(f"{where.size} bytes differ, the first at {where[:8].tolist()}: got "
                             f"{got[where[:8]].tolist()}, want {want[where[:8]].tolist()}")


def run(dec, layout, dest, md5=False, shift=0):
    from flac_codec_amd import _lib

    cases = subset()
    args, want = expected(layout)
    recs, _ = dec.scan([s.blob for s in cases])
    raw, need = decode_raw(dec, recs, len(cases), _lib.OutFormat(*args), dest, md5, shift)
    check(raw, need, want, shift)
    at = 0
    for s, r in zip(cases, recs):
        assert r.rc == 0 and r.out_offset == at and (r.info.bad_frames, r.info.bad_crc16) == (0, 0), s.name
        at += s.pcm.size
    return cases, recs


@pytest.mark.parametrize("dest", ["host", "device"])
@pytest.mark.parametrize("layout", [FLAT, PADDED])
def test_the_matrix_up_to_24_bits(dec, layout, dest):
    run(dec, layout, dest)


@pytest.mark.parametrize("shift", [1, 2])
def test_flat_to_an_unaligned_device_address(dec, shift):
    run(dec, FLAT, "device", shift=shift)


@pytest.mark.parametrize("layout,dest", [(FLAT, "device"), (PADDED, "host")])
def test_md5_is_verified_beside_the_packed_output(dec, layout, dest):
    cases, recs = run(dec, layout, dest, md5=True)
    for s, r in zip(cases, recs):
        assert r.info.md5_status == s.md5_status and bytes(r.info.decoded_md5) == s.digest, s.name
    # every stream of the subset that carries a digest verifies
    assert all(r.info.md5_status == 1 for s, r in zip(cases, recs) if s.md5_status == 1)
    assert sum(s.md5_status == 1 for s in cases) > 100


def test_python_surface_returns_byte_triples():
    from flac_codec_amd.gpu import decode_many

    cases = subset()[::9]
    blobs = [s.blob for s in cases]
    for out in ("device", "host"):
        flat, streams = decode_many(blobs, out=out, dtype="int24")
        assert str(flat.dtype).endswith("uint8") and tuple(flat.shape) == (sum(s.pcm.size for s in cases), 3)
        batch, padded = decode_many(blobs, out=out, dtype="int24", layout="padded", pad_channels=8)
        T = max(s.pcm.size // s.channels for s in cases)
        assert tuple(batch.shape) == (len(cases), 8, T, 3)
        for s, a, b in zip(cases, streams, padded):
            n = s.pcm.size // s.channels
            want = pack24(s.pcm.reshape(n, s.channels), s.bps)
            assert a.rc == 0 and tuple(a.pcm.shape) == (n, s.channels, 3) and tuple(b.pcm.shape) == (s.channels, n, 3)
            host = (lambda t: t.cpu().numpy()) if out == "device" else np.asarray
            assert np.array_equal(host(a.pcm), want) and np.array_equal(host(b.pcm), want.transpose(1, 0, 2)), s.name
            assert a.info.md5_status == s.md5_status
    with pytest.raises(ValueError, match="int24"):
        decode_many(blobs, dtype="int8")


def test_a_32_bit_stream_refuses_the_call_and_writes_nothing(dec):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import GpuError

    cases = [s for s in fm.valid_cases() if s.name in ("lpc8", "stereo-24", "stereo-32")]
    assert [s.bps for s in cases] == [16, 24, 32]
    recs, _ = dec.scan([s.blob for s in cases])
    for dest in ("device", "host"):
        for fmt in (_lib.OutFormat(S24, FLAT, 0, 0, 0), _lib.OutFormat(S24, PADDED, 8, 0, 1 << 16)):
            size = 1 << 20
            raw = np.full(GUARD + size + GUARD, FILL, dtype=np.uint8)
            if dest == "device":
                import torch

                buf = torch.from_numpy(raw).to("cuda:0")
                torch.cuda.synchronize()
                ptr = buf.data_ptr() + GUARD
            else:
                ptr = raw.ctypes.data + GUARD
            with pytest.raises(GpuError) as e:
                dec.decode_as(ptr, size, fmt, _lib.DECODE_OUT_DEVICE if dest == "device" else 0, recs)
            assert e.value.code == -2 and "stream 2" in str(e.value)
            if dest == "device":
                raw = buf.cpu().numpy()
            assert (raw == FILL).all(), dest
