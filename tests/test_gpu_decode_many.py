"""The batch decoder (flacgpu_decoder_scan / flacgpu_decoder_decode, gpu.decode_many) on the GPU: every stream's
record and samples equal flacgpu_decode_stream's for the same bytes, for fixtures, our own streams of every shape,
damaged and foreign inputs, with output to host or device memory and the MD5 on the device."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as orc
from _pcm import le_bytes as _le_bytes
from _pcm import synth_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")
FIXTURES = ["sine.flac", "all-frames.flac", "seektable.flac", "comment.flac"]
INFO_FIELDS = ["sample_rate", "channels", "bits_per_sample", "min_block", "max_block", "frames", "bad_frames",
               "bad_crc16", "total_samples", "decoded_samples", "md5", "decoded_md5", "md5_status"]
MD5_EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")

pytestmark = pytest.mark.gpu


def _fixture(name):
    with open(os.path.join(REFDATA, name), "rb") as f:
        return f.read()


def _encode(pcm, ch, bps, opts, rate=48000):
    from flac_codec_amd.encode import FlacSampleWriter

    w = FlacSampleWriter(None, opts, rate, bps, ch, pcm.size)
    w.write(pcm)
    w.finalize()
    data = w.getvalue()
    w.close()
    return data


def _metadata_end(blob):
    pos = 4
    while True:
        last, blen = blob[pos] & 0x80, int.from_bytes(blob[pos + 1:pos + 4], "big")
        pos += 4 + blen
        if last:
            return pos


def _empty_stream(blob, md5=MD5_EMPTY):
    """`blob`'s metadata alone -- a stream without frames (the writer refuses to finalize one) -- with STREAMINFO
    saying 0 samples and holding `md5`."""
    b = bytearray(blob[:_metadata_end(blob)])
    assert b[4] & 0x7F == 0
    b[8 + 13] &= 0xF0
    b[8 + 14:8 + 18] = bytes(4)
    b[26:42] = md5
    return bytes(b)


def _single(blob):
    """flacgpu_decode_stream on one stream: (rc, StreamInfo, interleaved samples)."""
    from flac_codec_amd import _lib

    L = _lib.lib()
    info = _lib.StreamInfo()
    blob = bytes(blob)
    rc = L.flacgpu_decode_stream(blob, len(blob), -1, None, 0, C.byref(info))
    if rc or info.frames == 0:
        return rc, info, np.zeros(0, np.int32)
    out = np.empty(info.decoded_samples * info.channels, dtype=np.int32)
    rc = L.flacgpu_decode_stream(blob, len(blob), -1, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size,
                                 C.byref(info))
    return rc, info, out


def _val(info, f):
    v = getattr(info, f)
    return bytes(v) if f in ("md5", "decoded_md5") else v


def _same_info(got, ref, skip=()):
    diff = {f: (_val(got, f), _val(ref, f)) for f in INFO_FIELDS if f not in skip and _val(got, f) != _val(ref, f)}
    assert not diff, diff


def _empty_md5_status(info):
    md5 = bytes(info.md5)
    return 2 if md5 == bytes(16) else (1 if md5 == MD5_EMPTY else 0)


def test_reference_fixtures_in_one_batch():
    from flac_codec_amd.gpu import decode_many

    blobs = [_fixture(n) for n in FIXTURES]
    flat, streams = decode_many(blobs, out="host")
    assert len(streams) == 4
    for name, blob, s in zip(FIXTURES, blobs, streams):
        rc, ref, oinfo = orc.decode_stream(blob)
        assert rc == 0 and s.rc == 0, name
        assert s.info.md5_status == 1 and s.info.bad_frames == 0 and s.info.bad_crc16 == 0, name
        assert s.info.frames == oinfo.frames, name
        assert np.array_equal(s.pcm.reshape(-1), ref), name
        _, sinfo, _ = _single(blob)
        _same_info(s.info, sinfo)
    assert bytes(streams[0].info.decoded_md5).hex() == "831671b807f97051301e01d68b5c54b3"
    assert flat.size == sum(s.pcm.size for s in streams)


@functools.lru_cache(maxsize=1)
def _mixed_batch():
    """(blob, pcm, bps, channels) of 200+ streams of every shape, zero-length ones included."""
    from flac_codec_amd.encode import Options

    rng = np.random.default_rng(1234)
    presets = [lambda: Options.fast(), lambda: Options.default(), lambda: Options.best(),
               lambda: Options.best().max_lpc_order(32)]
    blocks = [192, 576, 1000, 1152, 2304, 4096, 4608, 256, 333, 8192]
    widths = [8, 12, 16, 20, 24, 32]
    out = []
    for k in range(204):
        ch = 1 + k % 8
        bps = widths[k % 6]
        opts = presets[k % 4]()
        block = blocks[k % len(blocks)]
        if k % 51 == 7:
            block = 65535
        opts = opts.block_size(block)
        if k % 37 == 5:
            n = 0
        else:
            frames = 1 + int(rng.integers(0, 3 if block >= 8192 else 6))
            n = block * (frames - 1) + int(rng.integers(1, block + 1))   # a short last block most of the time
            n = min(n, 70000)
        rate = [8000, 16000, 44100, 48000, 96000][k % 5]
        if n:
            pcm = synth_fast(700 + k, ch, bps, n)
            out.append((_encode(pcm, ch, bps, opts, rate=rate), pcm, bps, ch))
        else:
            blob = _encode(synth_fast(700 + k, ch, bps, 100), ch, bps, opts, rate=rate)
            out.append((_empty_stream(blob, MD5_EMPTY if k % 2 else bytes(16)), np.zeros(0, np.int32), bps, ch))
    return out


def test_mixed_batch_of_own_streams():
    from flac_codec_amd.gpu import decode_many

    batch = _mixed_batch()
    flat, streams = decode_many([b for b, _, _, _ in batch], out="host")
    empties = 0
    for k, ((blob, pcm, bps, ch), s) in enumerate(zip(batch, streams)):
        assert s.rc == 0, k
        assert np.array_equal(s.pcm.reshape(-1), pcm), f"stream {k}: {ch} ch, {bps} bits"
        rc, sinfo, sout = _single(blob)
        assert rc == 0
        if pcm.size == 0:
            empties += 1
            _same_info(s.info, sinfo, skip=("decoded_md5", "md5_status"))
            assert s.info.frames == 0 and sinfo.md5_status == 0
            assert bytes(s.info.decoded_md5) == MD5_EMPTY and s.info.md5_status == _empty_md5_status(s.info)
        else:
            _same_info(s.info, sinfo)
            assert s.info.md5_status == 1, k
            assert bytes(s.info.decoded_md5) == orc.md5(_le_bytes(pcm, bps)), k
    assert empties >= 3
    assert flat.size == sum(p.size for _, p, _, _ in batch)


def test_device_output_and_too_small_buffer():
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, GpuError

    blobs = [_fixture(n) for n in FIXTURES] + [b for b, _, _, _ in _mixed_batch()[:24]]
    dec = Decoder(0)
    try:
        recs, total = dec.scan(blobs)
        host = np.empty(total, np.int32)
        dec.decode(host.ctypes.data, total, 0, recs)
        guard = 16
        sentinel = -0x5A5A5A5B
        buf = torch.full((total + guard,), sentinel, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(GpuError) as e:
            dec.decode(buf.data_ptr(), total - 1, _lib.DECODE_OUT_DEVICE, recs)
        assert e.value.code == -5   # FLACGPU_ERR_BUFFER_TOO_SMALL
        assert bool((buf == sentinel).all())
        recs2, total2 = dec.scan(blobs)
        assert total2 == total
        dec.decode(buf.data_ptr(), total, _lib.DECODE_OUT_DEVICE, recs2)
        got = buf.cpu().numpy()
        assert np.array_equal(got[:total], host)
        assert (got[total:] == sentinel).all()
        for a, b in zip(recs, recs2):
            assert a.rc == b.rc and a.out_offset == b.out_offset
            _same_info(a.info, b.info)
    finally:
        dec.close()


def _damaged(rng, blobs):
    """A few hundred damaged / foreign inputs derived from `blobs`."""
    cases = []
    for k in range(320):
        src = bytearray(blobs[int(rng.integers(0, len(blobs)))])
        kind = k % 8
        if kind == 0:   # bit flips anywhere, metadata included
            for _ in range(int(rng.integers(1, 4))):
                i = int(rng.integers(0, len(src)))
                src[i] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:   # bit flip in the last third (inside the frames)
            i = int(rng.integers(len(src) * 2 // 3, len(src)))
            src[i] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:   # truncation
            src = src[:int(rng.integers(0, len(src)))]
        elif kind == 3:   # inserted bytes
            i = int(rng.integers(0, len(src)))
            src[i:i] = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        elif kind == 4:   # deleted bytes
            i = int(rng.integers(0, len(src)))
            del src[i:i + int(rng.integers(1, 40))]
        elif kind == 5:   # two streams spliced
            other = blobs[int(rng.integers(0, len(blobs)))]
            src = src[:int(rng.integers(0, len(src)))] + other[int(rng.integers(0, len(other))):]
        elif kind == 6:   # garbage behind a fLaC marker and a copied STREAMINFO, or plain garbage
            g = rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8).tobytes()
            src = bytearray(src[:42] + g) if k % 16 == 6 else bytearray(g)
        else:   # empty, or a bare metadata header
            src = bytearray(b"" if k % 16 == 7 else src[:42])
        cases.append(bytes(src))
    return cases


def test_equivalence_under_damage():
    from flac_codec_amd.encode import Options
    from flac_codec_amd.gpu import decode_many

    rng = np.random.default_rng(99)
    intact = [_fixture(n) for n in FIXTURES]
    pcms = [None] * len(intact)
    for k, (ch, bps, block) in enumerate([(2, 16, 1152), (1, 24, 4096), (6, 20, 576), (2, 24, 1000), (1, 8, 192)]):
        pcm = synth_fast(50 + k, ch, bps, block * 5 + 77)
        intact.append(_encode(pcm, ch, bps, Options.default().block_size(block)))
        pcms.append(pcm)
    cases = _damaged(rng, intact)
    batch, kinds = [], []
    for k, c in enumerate(cases):   # intact streams between the damaged ones
        batch.append(c)
        kinds.append(("damaged", None))
        if k % 20 == 0:
            i = (k // 20) % len(intact)
            batch.append(intact[i])
            kinds.append(("intact", i))
    _, streams = decode_many(batch, out="host")
    compared = 0
    for k, (blob, s, (kind, i)) in enumerate(zip(batch, streams, kinds)):
        rc, sinfo, sout = _single(blob)
        assert s.rc == rc, k
        if rc != 0:
            _same_info(s.info, sinfo)
            assert s.info.md5_status == 0 and bytes(s.info.decoded_md5) == bytes(16)
            continue
        if sinfo.frames == 0:
            _same_info(s.info, sinfo, skip=("decoded_md5", "md5_status"))
            assert s.info.md5_status == _empty_md5_status(s.info)
            continue
        # the samples of a frame that does not decode are undefined in both paths: compare them where the stream's
        # own path decoded every frame it found (no bad frame, or a lost sync behind good frames that match a prefix
        # of the intact stream's samples)
        defined = sinfo.bad_frames == 0
        if not defined and sinfo.bad_frames == 1:
            refs = [orc.decode_stream(b)[1] for b in intact]
            defined = any(r.size >= sout.size and np.array_equal(r[:sout.size], sout) for r in refs)
        if defined:
            _same_info(s.info, sinfo)
            assert np.array_equal(s.pcm.reshape(-1), sout), k
            compared += 1
        else:
            _same_info(s.info, sinfo, skip=("decoded_md5", "md5_status"))
        if kind == "intact":
            assert s.info.md5_status == 1 and s.info.bad_frames == 0
            if pcms[i] is not None:
                assert np.array_equal(s.pcm.reshape(-1), pcms[i])
    assert compared >= 60


def test_false_sync_inside_a_verbatim_frame():
    """Full-scale noise is coded VERBATIM, so chosen samples put a well-formed frame header with a correct CRC-8 into
    the frame's bytes: the scan must see it as a candidate and reject it through the CRC-16 rule."""
    from flac_codec_amd.encode import Options
    from flac_codec_amd.gpu import decode_many

    hdr = bytes([0xFF, 0xF8, 0xC9, 0x08, 0x05])
    hdr += bytes([orc.crc8(hdr)])   # 4096 samples, 44.1 kHz, mono, 16 bits, frame 5
    fake = np.frombuffer(hdr, dtype=">i2").astype(np.int32)
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, 4096 * 3 + 500).astype(np.int32)
    pcm[4096 + 1001:4096 + 1004] = fake
    pcm[2 * 4096 + 17:2 * 4096 + 20] = fake
    blob = _encode(pcm, 1, 16, Options.default().block_size(4096), rate=44100)
    assert blob.count(hdr) == 2, "the encoder did not code the noise VERBATIM"
    flat, streams = decode_many([blob, blob], out="host")
    rc, sinfo, sout = _single(blob)
    for s in streams:
        assert s.rc == 0 and s.info.bad_frames == 0 and s.info.md5_status == 1
        assert np.array_equal(s.pcm.reshape(-1), pcm)
        assert s.info.frames == sinfo.frames == 4
        _same_info(s.info, sinfo)


def test_md5_statuses():
    from flac_codec_amd.encode import Options
    from flac_codec_amd.gpu import decode_many

    pcm = synth_fast(11, 2, 16, 4096 * 3 + 5)
    blob = _encode(pcm, 2, 16, Options.default())
    assert blob[:4] == b"fLaC" and blob[4] & 0x7F == 0   # STREAMINFO first: its MD5 at bytes 26..42
    zero = blob[:26] + bytes(16) + blob[42:]
    changed = bytearray(blob)
    changed[30] ^= 0x01
    empty = _empty_stream(blob)
    empty_zero = _empty_stream(blob, bytes(16))
    _, streams = decode_many([blob, zero, bytes(changed), empty, empty_zero], out="device")
    assert [s.info.md5_status for s in streams[:3]] == [1, 2, 0]
    digest = orc.md5(_le_bytes(pcm, 16))
    for s in streams[:3]:
        assert bytes(s.info.decoded_md5) == digest and s.info.bad_frames == 0
    # empty streams: the new path hashes the empty input (flacgpu_decode_stream does not hash at all)
    assert streams[3].info.frames == 0 and bytes(streams[3].info.decoded_md5) == MD5_EMPTY
    assert streams[3].info.md5_status == 1 and streams[3].info.bad_frames == 0
    assert streams[4].info.md5_status == 2
    assert _single(empty)[1].md5_status == 0
    _, nomd5 = decode_many([blob, zero, empty], out="host", verify_md5=False)
    assert [s.info.md5_status for s in nomd5] == [3, 3, 3]
    assert all(bytes(s.info.decoded_md5) == bytes(16) for s in nomd5)
    # every sample width: 8 / 12 / 20 / 24 / 32 bits
    blobs, pcms = [], []
    for k, bps in enumerate([8, 12, 20, 24, 32]):
        p = synth_fast(20 + k, 1 + k % 3, bps, 3000 + 7 * k)
        blobs.append(_encode(p, 1 + k % 3, bps, Options.best()))
        pcms.append((p, bps))
    _, streams = decode_many(blobs, out="device")
    for s, (p, bps) in zip(streams, pcms):
        assert s.info.md5_status == 1 and bytes(s.info.decoded_md5) == orc.md5(_le_bytes(p, bps)), bps
        assert np.array_equal(s.pcm.cpu().numpy().reshape(-1), p)


def test_flacverify_example(tmp_path):
    blobs = {n: _fixture(n) for n in FIXTURES}
    paths = []
    for n, b in blobs.items():
        p = tmp_path / n
        p.write_bytes(b)
        paths.append(str(p))
    sine = blobs["sine.flac"]
    broken = bytearray(sine)
    broken[len(broken) - len(broken) // 3] ^= 0x40   # inside the frames: the CRC-16 chain breaks
    (tmp_path / "broken.flac").write_bytes(bytes(broken))
    mismatch = bytearray(sine)
    mismatch[30] ^= 0x01   # STREAMINFO's MD5
    (tmp_path / "mismatch.flac").write_bytes(bytes(mismatch))
    nomd5 = sine[:26] + bytes(16) + sine[42:]
    (tmp_path / "nomd5.flac").write_bytes(nomd5)
    (tmp_path / "text.flac").write_bytes(b"not a flac file at all, just some words " * 4)
    extra = [str(tmp_path / n) for n in ("broken.flac", "mismatch.flac", "nomd5.flac", "text.flac")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "flacverify.py")] + paths + extra,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    assert lines[:4] == [f"{p}: ok" for p in paths]
    assert lines[4].startswith(f"{extra[0]}: error - ")
    assert lines[5] == f"{extra[1]}: bad - MD5 mismatch"
    assert lines[6] == f"{extra[2]}: ok - no MD5"
    assert lines[7].startswith(f"{extra[3]}: error - ")
