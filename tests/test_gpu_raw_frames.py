"""Raw frame streams through the batch decoder: flacgpu_decoder_scan_frames / _decode_frames, decode_many(raw=True) and
decode.FlacStreamReader.

The device scan is held to flacgpu_scan_frames_host (which test_scan_frames_host.py holds to the rule's Python model) on
every input of _raw_frames.all_cases() in one batch.  Expected PCM is what the hand-built frames were written from
(_flacsyn: right by construction), the input of our own FlacStreamWriter, or -- for uniform streams -- decode_many of
the regular stream made of the same frame bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import _flacsyn as fs
import _foreign_matrix as fm
import _raw_frames as rf
import _scan_model as sm
from _pcm import synth_fast

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED, TOO_SMALL = 0, -1, -2, -5
GUARD, FILL = 64, 0x5A5A5A5A   # int32 guard words around decode_frames' output


@pytest.fixture(scope="module")
def dec():
    from flac_codec_amd.gpu import Decoder

    d = Decoder(0)
    yield d
    d.close()


def host_scan(blob):
    from flac_codec_amd.gpu import scan_frames_host

    return scan_frames_host(blob)


def decode_frames_guarded(dec, frames, dest):
    """decode_frames of the scanned batch into a buffer with guard words; (samples, records)."""
    import torch

    from flac_codec_amd import _lib

    total = dec.raw_elements
    recs = frames.copy()
    if dest == "device":
        buf = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        dec.decode_frames(buf.data_ptr() + 4 * GUARD, total, _lib.DECODE_OUT_DEVICE, recs)
        buf = buf.cpu().numpy()
    else:
        buf = np.full(GUARD + total + GUARD, FILL, dtype=np.int32)
        dec.decode_frames(buf.ctypes.data + 4 * GUARD, total, 0, recs)
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + total:] == FILL).all(), "a write outside out"
    return buf[GUARD:GUARD + total], recs


def frame_pcm(samples, rec):
    at, n, ch = int(rec["out_offset"]), int(rec["block_size"]), int(rec["channels"])
    return samples[at:at + n * ch].reshape(n, ch)


def to_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def test_device_scan_equals_host_scan(dec):
    cases = rf.all_cases()
    assert len(cases) > 2000
    blobs = [b for _, b in cases]
    recs, total, raw, frames = dec.scan_frames(blobs)
    at = out = 0
    for i, (label, blob) in enumerate(cases):
        want, summary = host_scan(blob)
        want = want.copy()
        want["stream"] = i
        want["out_offset"] += out
        got = frames[at:at + len(want)]
        assert raw[i].first_frame == at, label
        assert rf.summary_tuple(raw[i]) == rf.summary_tuple(summary), label
        assert got.tobytes() == want.tobytes(), label
        at += len(want)
        out += int((want["block_size"].astype(np.int64) * want["channels"]).sum())
        want_rc = OK if summary.uniform else UNSUPPORTED if summary.frames else INVALID_ARG
        assert recs[i].rc == want_rc, label
    assert at == len(frames) and out == dec.raw_elements


@pytest.mark.parametrize("dest", ["host", "device"])
def test_decode_frames_of_the_mixed_stream(dec, dest):
    st = rf.mixed()
    recs, total, raw, frames = dec.scan_frames([st.blob])
    assert recs[0].rc == UNSUPPORTED and total == 0 and len(frames) == 12
    assert [rf.record_tuple(f) for f in frames] == [rf.record_tuple(r) for r in rf.expected_records(st)]
    samples, out = decode_frames_guarded(dec, frames, dest)
    assert (out["status"] == 0).all()
    out["status"] = 0
    assert out.tobytes() == frames.tobytes()
    for k in range(12):
        assert np.array_equal(frame_pcm(samples, out[k]), np.array(st.pcm[k], dtype=np.int64).astype(np.int32)), k


def test_public_decode_frames(dec):
    from flac_codec_amd.gpu import decode_frames

    st = rf.mixed()
    for out in ("host", "device"):
        samples, frames, raw = decode_frames([st.blob, b"", st.blob[5:]], out=out)
        samples = to_numpy(samples)
        assert [r.frames for r in raw] == [12, 0, 11] and [r.gaps for r in raw] == [0, 0, 1]
        assert frames["stream"].tolist() == [0] * 12 + [2] * 11 and (frames["status"] == 0).all()
        for k in range(12):
            assert np.array_equal(frame_pcm(samples, frames[k]), np.array(st.pcm[k], dtype=np.int64).astype(np.int32))
        for k in range(1, 12):
            assert np.array_equal(frame_pcm(samples, frames[11 + k]), frame_pcm(samples, frames[k]))


def test_a_frame_that_does_not_parse(dec):
    """A reserved subframe type under a right CRC-16: status bit 0, the neighbours decode."""
    st = rf.build([(44100, 16, 2, 16)] * 3, 31, invalid_at=1)
    recs, _, raw, frames = dec.scan_frames([st.blob])
    assert raw[0].frames == 3 and raw[0].uniform == 1 and recs[0].rc == OK
    samples, out = decode_frames_guarded(dec, frames, "host")
    assert out["status"].tolist() == [0, 1, 0]
    for k in (0, 2):
        assert np.array_equal(frame_pcm(samples, out[k]), np.array(st.pcm[k], dtype=np.int32))


def test_a_swallowed_non_subset_frame_does_not_parse(dec):
    """test_scan_frames_host.test_non_subset_frames_are_not_kept: the record in front of the odd frame runs over it."""
    blobs = [b for _, b in rf.non_subset_cases()]
    _, _, raw, frames = dec.scan_frames(blobs)
    assert [r.frames for r in raw] == [12, 12]
    samples, out = decode_frames_guarded(dec, frames, "host")
    st = rf.mixed()
    for i in range(2):
        assert out["status"][12 * i:12 * i + 12].tolist() == [0, 0, 1] + [0] * 9
        for k in range(12):
            if k != 2:
                want = np.array(st.pcm[k], dtype=np.int64).astype(np.int32)
                assert np.array_equal(frame_pcm(samples, out[12 * i + k]), want), (i, k)


def test_round_trip_of_our_stream_writer():
    from flac_codec_amd.decode import FlacStreamReader, FrameBuf
    from flac_codec_amd.encode import FlacStreamWriter, Options

    w = FlacStreamWriter(None, Options.best())
    want = []
    for rate, ch, bps, n, seed in [(44100, 2, 16, 16, 1), (48000, 1, 24, 192, 2), (96000, 2, 24, 4096, 3)]:
        pcm = synth_fast(seed, ch, bps, n)
        w.write(rate, ch, bps, pcm)
        want.append(FrameBuf(pcm, rate, ch, bps))
    data = w.getvalue()
    w.close()
    reader = FlacStreamReader(data)
    got = [reader.read() for _ in range(3)]
    assert got == want, (got, want)
    with pytest.raises(EOFError):
        reader.read()
    assert (reader.skipped_bytes, reader.gaps) == (0, 0)
    assert list(FlacStreamReader(data)) == want


def test_stream_reader_reports_a_bad_frame_and_goes_on():
    from flac_codec_amd.decode import DecodeError, FlacStreamReader

    st = rf.build([(44100, 16, 2, 16)] * 3, 31, invalid_at=1)
    reader = FlacStreamReader(st.blob)
    assert (reader.skipped_bytes, reader.gaps) == (0, 0)   # before any read
    assert np.array_equal(reader.read().samples.reshape(16, 2), np.array(st.pcm[0], dtype=np.int32))
    with pytest.raises(DecodeError):
        reader.read()
    third = reader.read()
    assert np.array_equal(third.samples.reshape(16, 2), np.array(st.pcm[2], dtype=np.int32))
    assert (third.sample_rate, third.channels, third.bits_per_sample) == (44100, 2, 16)
    with pytest.raises(EOFError):
        reader.read()


def _uniform_pairs():
    """(raw blob, regular blob, digest) of the uniform streams: the matrix's subset streams with the fLaC marker and
    metadata removed, and -- those being fewer than ten -- the hand-built uniform set."""
    matrix = rf.subset_matrix_streams()
    assert len(matrix) == 7   # counted on the CPU: fewer than 10 qualify, hence the set built from _flacsyn
    pairs = [(st.blob[sm.metadata(st.blob)[0]:], st.blob, st.digest) for st in matrix]
    pairs += [(raw.blob, regular.blob, regular.digest) for raw, regular in rf.uniform_set()]
    assert len(pairs) == 19
    return pairs


def test_uniform_streams_decode_as_regular_ones(dec):
    from flac_codec_amd.gpu import decode_many, decode_windows

    pairs = _uniform_pairs()
    raws, regulars = [p[0] for p in pairs], [p[1] for p in pairs]
    for kw in (dict(dtype="int32", layout="flat"), dict(dtype="float32", layout="padded"),
               dict(dtype="int24", layout="padded")):
        pick = range(len(pairs))
        if kw["dtype"] == "int24":   # needs at most 24 bits in every stream
            pick = [i for i in pick if host_scan(raws[i])[0]["bits_per_sample"][0] <= 24]
            assert len(pick) >= 10
        want, want_streams = decode_many([regulars[i] for i in pick], out="host", **kw)
        got, got_streams = decode_many([raws[i] for i in pick], out="host", raw=True, decoder=dec, **kw)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), kw
        for i, a, b in zip(pick, got_streams, want_streams):
            assert (a.rc, a.offset) == (b.rc, b.offset) == (OK, b.offset), (kw, i)
            for field in ("sample_rate", "channels", "bits_per_sample", "frames", "decoded_samples", "bad_frames",
                          "bad_crc16"):
                assert getattr(a.info, field) == getattr(b.info, field), (kw, i, field)
            assert a.info.total_samples == 0 and bytes(a.info.md5) == bytes(16)
            assert a.info.md5_status == 2 and b.info.md5_status == 1
            assert bytes(a.info.decoded_md5) == bytes(b.info.decoded_md5) == pairs[i][2], (kw, i)
    # sample windows: the raw scan on `dec` against a regular scan on a handle of its own
    from flac_codec_amd.gpu import Decoder

    rng = random.Random(99)
    recs, _, _, _ = dec.scan_frames(raws)
    lengths = [recs[i].info.decoded_samples for i in range(len(raws))]
    windows = []
    for _ in range(100):
        i = rng.randrange(len(raws))
        windows.append((i, rng.randrange(lengths[i] + 8), rng.choice((0, 1, 16, 100, 700))))
    other = Decoder(0)
    try:
        regular_recs, _ = other.scan(regulars)
        want, want_res = decode_windows(other, regular_recs, windows, dtype="float32", out="host")
    finally:
        other.close()
    got, got_res = decode_windows(dec, recs, windows, dtype="float32", out="host")
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    for a, b in zip(got_res, want_res):
        assert (a.rc, a.frames, a.bad_frames, a.bad_crc16, a.samples) == (b.rc, b.frames, b.bad_frames, b.bad_crc16,
                                                                          b.samples)
    assert sum(r.samples for r in got_res) > 3000


def test_a_batch_of_uniform_non_uniform_empty_and_garbage(dec):
    from flac_codec_amd.gpu import decode_many

    uni, mixed = rf.uniform(), rf.mixed()
    garbage = bytes(random.Random(3).randrange(256) for _ in range(500)) + bytes([0xFF, 0xF8]) * 20
    blobs = [uni.blob, mixed.blob, b"", garbage]
    batch, streams = decode_many(blobs, out="host", raw=True, decoder=dec, dtype="int32", layout="padded")
    assert [s.rc for s in streams] == [OK, UNSUPPORTED, INVALID_ARG, INVALID_ARG]
    total = sum(n for _, _, _, n in uni.shapes)
    assert batch.shape == (4, 2, total)
    want = np.concatenate([np.array(p, dtype=np.int32) for p in uni.pcm])   # [samples][channels]
    assert np.array_equal(batch[0], want.T)
    assert not batch[1:].any()   # the rows of the rc != 0 streams are zero
    assert streams[0].info.md5_status == 2 and streams[0].info.frames == len(uni.pcm)
    assert (streams[0].info.min_block, streams[0].info.max_block) == (16, 192)
    # decode_frames on the same scan still returns the non-uniform stream's frames (and the uniform one's)
    frames = np.zeros(len(uni.pcm) + 12, dtype=rf_dtype())
    samples, out = decode_frames_guarded(dec, frames, "host")
    assert out["stream"].tolist() == [0] * len(uni.pcm) + [1] * 12 and (out["status"] == 0).all()
    for k in range(12):
        want_k = np.array(mixed.pcm[k], dtype=np.int64).astype(np.int32)
        assert np.array_equal(frame_pcm(samples, out[len(uni.pcm) + k]), want_k), k


def rf_dtype():
    from flac_codec_amd.gpu import FRAME_DTYPE

    return FRAME_DTYPE


def test_calls_in_any_order_on_one_raw_scan_then_a_regular_scan(dec):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, decode_windows

    raw, regular = rf.uniform_set()[1]
    mixed = rf.mixed()
    recs, total, _, frames = dec.scan_frames([raw.blob, mixed.blob])
    want = regular.pcm.reshape(-1, 2)   # [samples][channels]
    assert total == want.size

    def check_frames():
        samples, out = decode_frames_guarded(dec, frames, "host")
        assert (out["status"] == 0).all()
        assert np.array_equal(np.concatenate([frame_pcm(samples, out[k]) for k in range(5)]), want)
        assert np.array_equal(frame_pcm(samples, out[5 + 3]), np.array(mixed.pcm[3], dtype=np.int32))

    check_frames()
    fmt = _lib.OutFormat(_lib.SAMPLE_I16, _lib.LAYOUT_FLAT, 0, 0, 0)
    need = Decoder.plan_output(fmt, recs, 2)
    assert need == 2 * total
    i16 = np.full(total, 0x7F7F, dtype=np.int16)
    dec.decode_as(i16.ctypes.data, need, fmt, 0, recs)
    assert np.array_equal(i16.reshape(-1, 2), want.astype(np.int16))
    batch, res = decode_windows(dec, recs, [(0, 100, 300), (1, 0, 50)], dtype="int32", out="host")
    assert np.array_equal(batch[0, :, :300], want[100:400].T) and not batch[1].any()
    assert (res[0].rc, res[0].samples, res[1].rc) == (OK, 300, UNSUPPORTED)
    check_frames()
    flat = np.empty(total, dtype=np.int32)
    dec.decode(flat.ctypes.data, total, 0, recs)
    assert np.array_equal(flat.reshape(-1, 2), want)
    # a regular scan replaces the raw one: decode_frames is refused, decode works
    recs, total = dec.scan([regular.blob])
    with pytest.raises(Exception):
        dec.decode_frames(flat.ctypes.data, flat.size, 0, frames.copy())
    flat = np.empty(total, dtype=np.int32)
    dec.decode(flat.ctypes.data, total, 0, recs)
    assert np.array_equal(flat.reshape(-1, 2), want) and recs[0].info.md5_status == 1


def test_a_byte_range_from_the_middle_of_a_file(dec):
    """3000 bytes cut out of a regular stereo stream of 4096-sample blocks with tabled rate and sample-size codes: the
    whole frames inside decode to the matching slice of the full decode, which `number` (a frame number) locates."""
    from flac_codec_amd.gpu import decode_frames, decode_many

    rng = random.Random(11)
    frames = []
    for k in range(8):
        sub = fs.fixed(1)
        v = fm._predicted(rng, 4096, 16, sub, amp=1)
        frames.append(fs.Frame([v, [k - 3] * 4096], [fm.fit_k(v, sub), fs.constant()], rcode=fs.RATE_CODES[44100],
                               number=k))
    st = fs.write_stream(44100, 16, frames)
    assert max(len(c) for c in st.frame_bytes) < 1450   # so that 3000 bytes hold a whole frame wherever they start
    _, full = decode_many([st.blob], out="host")
    pcm = full[0].pcm
    middle = len(st.blob) // 2 - 1500
    first_frame_byte = len(st.blob) - sum(len(c) for c in st.frame_bytes)
    assert middle > first_frame_byte + 10
    samples, recs, raw = decode_frames([st.blob[middle:middle + 3000]], out="host", decoder=dec)
    assert 1 <= len(recs) <= 3 and raw[0].gaps == 2 and (recs["status"] == 0).all()
    assert (recs["blocking"] == 0).all() and (recs["block_size"] == 4096).all()
    for r in recs:
        start = int(r["number"]) * 4096
        assert np.array_equal(frame_pcm(samples, r), pcm[start:start + 4096]), int(r["number"])
    assert recs["number"].tolist() == list(range(int(recs["number"][0]), int(recs["number"][0]) + len(recs)))


def test_a_32_bit_mid_side_frame_in_a_raw_stream(dec):
    """The side channel of 32-bit stereo has 33 bits: full-scale samples of opposite sign."""
    from flac_codec_amd.gpu import decode_frames

    rng = random.Random(8)
    lo, hi = -(1 << 31), (1 << 31) - 1
    left = [hi, lo, hi, lo] + [rng.randint(lo, hi) for _ in range(12)]
    right = [lo, hi, hi - 1, lo + 1] + [rng.randint(lo, hi) for _ in range(12)]
    small = [[3, -4], [5, 6]]
    blob = b""
    for number, (chans, a, rate, bits) in enumerate(((list(zip(*small)), 1, 44100, 16), ([left, right], 10, 192000, 32),
                                                      (list(zip(*small)), 1, 44100, 16))):
        chans = [list(c) for c in chans]
        fr = fs.Frame(chans, [fs.verbatim(), fs.verbatim()], assignment=a, rcode=fs.RATE_CODES[rate], number=number)
        blob += fs.write_frame(rate, bits, fr, set())
    samples, recs, raw = decode_frames([blob], out="host", decoder=dec)
    assert raw[0].frames == 3 and raw[0].gaps == 0 and (recs["status"] == 0).all()
    assert (recs["assignment"].tolist(), recs["bits_per_sample"].tolist()) == ([1, 10, 1], [16, 32, 16])
    want = np.array([left, right], dtype=np.int64).T.astype(np.int32)
    assert np.array_equal(frame_pcm(samples, recs[1]), want)
    assert np.array_equal(frame_pcm(samples, recs[0]), np.array(small, dtype=np.int32))


def test_refusals_write_nothing(dec):
    from flac_codec_amd import _lib

    L = _lib.lib()
    st = rf.mixed()
    _, _, _, frames = dec.scan_frames([st.blob])
    total = dec.raw_elements
    out = np.full(total, FILL, dtype=np.int32)
    recs = np.full(len(frames) * 64, 0xEE, dtype=np.uint8).view(rf_dtype())
    rp = recs.ctypes.data_as(C.POINTER(_lib.FrameRecord))
    assert L.flacgpu_decoder_decode_frames(dec._h, out.ctypes.data, total - 1, 0, rp, len(recs)) == TOO_SMALL
    assert L.flacgpu_decoder_decode_frames(dec._h, out.ctypes.data, total, 0, rp, len(recs) - 1) == TOO_SMALL
    assert L.flacgpu_decoder_decode_frames(dec._h, out.ctypes.data, total, 2, rp, len(recs)) == INVALID_ARG   # NO_MD5
    assert L.flacgpu_decoder_decode_frames(dec._h, out.ctypes.data, total, 0, None, 0) == INVALID_ARG
    assert L.flacgpu_decoder_frame_records(dec._h, rp, len(recs) - 1) == TOO_SMALL
    assert (out == FILL).all() and (recs.view(np.uint8) == 0xEE).all()
