"""FLACGPU_SCAN_SPECULATIVE through the batch decoder (DESIGN.md 4b "A frame's own extent"): the device scan with
k_spec_end is held to flacgpu_scan_frames_host_ex (which test_scan_frames_speculative.py holds to the rule's Python
model) on every input of _raw_frames.all_cases() and on the decoder matrix with every second frame header destroyed, in
one batch; the frames kept by their own bits decode to what they were written from; and the flag reaches decode_many,
decode_windows and decode.FlacStreamReader.

The inputs are the smallest that reach every branch of the walker: blocks of 16 to 4096 samples and one frame of 131 081
bytes; false candidates run it into foreign bytes and into the slots' zero tails."""
import numpy as np
import pytest

import _raw_frames as rf
import _spec_frames as sf

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
GUARD, FILL = 64, 0x5A5A5A5A   # int32 guard words around decode_frames' output


@pytest.fixture(scope="module")
def dec():
    from flac_codec_amd.gpu import Decoder

    d = Decoder(0)
    yield d
    d.close()


def _cases():
    return list(rf.all_cases()) + [(f"matrix {i}, parity {p}", blob) for i, p, blob in sf.alternating()]


def _device_equals_host(dec, cases, speculative):
    from flac_codec_amd.gpu import scan_frames_host

    recs, total, raw, frames = dec.scan_frames([b for _, b in cases], speculative=speculative)
    at = out = own = 0
    for i, (label, blob) in enumerate(cases):
        want, summary = scan_frames_host(blob, speculative=speculative)
        want = want.copy()
        want["stream"] = i
        want["out_offset"] += out
        got = frames[at:at + len(want)]
        assert raw[i].first_frame == at, label
        assert rf.summary_tuple(raw[i]) == rf.summary_tuple(summary), label
        assert got.tobytes() == want.tobytes(), label
        at += len(want)
        out += int((want["block_size"].astype(np.int64) * want["channels"]).sum())
        own += int(want["reserved"].sum())
        want_rc = OK if summary.uniform else UNSUPPORTED if summary.frames else INVALID_ARG
        assert recs[i].rc == want_rc, label
    assert at == len(frames) and out == dec.raw_elements
    return own


def test_device_scan_equals_host_scan_with_and_without_the_flag(dec):
    cases = _cases()
    assert len(cases) == 2253 + 214
    own = _device_equals_host(dec, cases, True)
    assert own >= 225 + 271 + 93   # the alternating inputs' frames and at least one per flip that has any
    # the same batch on the same handle afterwards, without the flag: nothing is left over
    assert _device_equals_host(dec, cases, False) == 0


@pytest.mark.parametrize("dest", ["host", "device"])
def test_frames_kept_by_their_own_bits_decode(dec, dest):
    import torch

    from flac_codec_amd import _lib

    m = sf.subset_matrix()
    alt = sf.alternating()
    _, _, raw, frames = dec.scan_frames([blob for _, _, blob in alt], speculative=True)
    total = dec.raw_elements
    out = frames.copy()
    if dest == "device":
        buf = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        dec.decode_frames(buf.data_ptr() + 4 * GUARD, total, _lib.DECODE_OUT_DEVICE, out)
        buf = buf.cpu().numpy()
    else:
        buf = np.full(GUARD + total + GUARD, FILL, dtype=np.int32)
        dec.decode_frames(buf.ctypes.data + 4 * GUARD, total, 0, out)
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + total:] == FILL).all(), "a write outside out"
    samples = buf[GUARD:GUARD + total]
    assert (out["status"] == 0).all()
    assert len(out) == 271 + 332 and int(out["reserved"].sum()) == 225 + 271
    for r in out:
        i, parity, _ = alt[int(r["stream"])]
        k = sf.true_frames(m[i])[(int(r["byte_offset"]), int(r["bytes"]))]
        assert k % 2 != parity
        at, n, ch = int(r["out_offset"]), int(r["block_size"]), int(r["channels"])
        assert np.array_equal(samples[at:at + n * ch].reshape(n, ch), m[i].pcm[k]), (m[i].name, parity, k)


def test_a_damaged_header_costs_one_frame_of_a_uniform_stream(dec):
    from flac_codec_amd.decode import FlacStreamReader
    from flac_codec_amd.gpu import decode_many, decode_windows, scan_frames_host

    raw, _ = rf.uniform_set()[1]   # 44100 Hz, 16 bits, stereo; blocks of 16, 192, 33, 576 and 17 samples
    assert [n for _, _, _, n in raw.shapes] == [16, 192, 33, 576, 17]
    b = bytearray(raw.blob)
    b[raw.at[2]] ^= 0x01   # the first sync byte of frame 2
    blob = bytes(b)
    pcm = [np.array(p, dtype=np.int32) for p in raw.pcm]   # [n][channels]
    starts = lambda frames: [int(f["byte_offset"]) for f in frames]
    assert starts(scan_frames_host(blob)[0]) == [raw.at[k] for k in (0, 3, 4)]
    assert starts(scan_frames_host(blob, speculative=True)[0]) == [raw.at[k] for k in (0, 1, 3, 4)]

    batch, streams = decode_many([blob], out="host", raw=True, speculative=True, dtype="float32", layout="padded", decoder=dec)
    want = np.concatenate([pcm[k] for k in (0, 1, 3, 4)])
    assert streams[0].rc == OK and streams[0].info.frames == 4 and batch.shape == (1, 2, len(want))
    assert np.array_equal(batch[0], (want.T / 32768.0).astype(np.float32))
    # the present rule loses frame 1 with frame 2
    batch, streams = decode_many([blob], out="host", raw=True, dtype="float32", layout="padded", decoder=dec)
    lost = np.concatenate([pcm[k] for k in (0, 3, 4)])
    assert streams[0].info.frames == 3 and batch.shape == (1, 2, len(lost))
    assert np.array_equal(batch[0], (lost.T / 32768.0).astype(np.float32))

    got = list(FlacStreamReader(blob, speculative=True))
    assert len(got) == 4
    for g, k in zip(got, (0, 1, 3, 4)):
        assert (g.sample_rate, g.channels, g.bits_per_sample) == (44100, 2, 16)
        assert np.array_equal(np.asarray(g.samples).reshape(-1, 2), pcm[k]), k
    assert len(list(FlacStreamReader(blob))) == 3

    # a window over the seam: frame 1 is samples [16, 208) of the kept stream, frame 3 follows it
    recs, total, _, frames = dec.scan_frames([blob], speculative=True)
    assert total == want.size and frames["reserved"].tolist() == [0, 1, 0, 0]
    win, res = decode_windows(dec, recs, [(0, 150, 200)], dtype="int32", out="host")
    assert (res[0].rc, res[0].frames, res[0].bad_frames, res[0].bad_crc16, res[0].samples) == (OK, 2, 0, 0, 200)
    assert np.array_equal(win[0], want[150:350].T)


def test_an_unknown_flag_is_refused_and_nothing_is_written(dec):
    import ctypes as C

    from flac_codec_amd import _lib

    L = _lib.lib()
    st = rf.mixed()
    _, _, _, frames = dec.scan_frames([st.blob], speculative=True)
    ptrs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)(len(st.blob))
    keep = C.c_char_p(st.blob)
    ptrs[0] = C.cast(keep, C.c_void_p).value
    for flags in (2, 3, 0x80000000):
        streams, raw = (_lib.DecodedStream * 1)(), (_lib.RawStream * 1)()
        C.memset(streams, 0xEE, C.sizeof(streams))
        C.memset(raw, 0xEE, C.sizeof(raw))
        counts = [C.c_uint64(0xDEAD) for _ in range(3)]
        rc = L.flacgpu_decoder_scan_frames_ex(dec._h, ptrs, lens, 1, flags, streams, raw, *[C.byref(c) for c in counts])
        assert rc == INVALID_ARG, flags
        assert bytes(streams) == b"\xee" * C.sizeof(streams) and bytes(raw) == b"\xee" * C.sizeof(raw), flags
        assert [c.value for c in counts] == [0xDEAD] * 3, flags
    again = np.zeros(len(frames), dtype=frames.dtype)   # the handle's scanned batch is still the one before
    assert L.flacgpu_decoder_frame_records(dec._h, again.ctypes.data_as(C.POINTER(_lib.FrameRecord)), len(again)) == OK
    assert again.tobytes() == frames.tobytes()
