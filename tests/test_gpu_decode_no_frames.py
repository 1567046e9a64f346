"""A batch without a single frame through every decode call of the batch decoder, on a regular scan and on a raw one.

The guards for "no frame" and "no count pair" live in the helpers the decode calls share (FramePass, OutStage and
Selected in decode_many.hip), so every call is sent a batch that reaches them: empty bytes, a bare fLaC +
STREAMINFO header with nothing behind it, and 100 bytes of noise.  What every call returns for such a batch was
recorded from the calls as they stood before the helpers were shared, and is compared exactly; every padded output is
zero in every byte, its 0xA5 fill gone, its guards intact.  Afterwards the same handle scans a two-frame stream and
decodes it to the oracle's samples: nothing of the empty batch is left on it."""
import numpy as np
import pytest

import _flacsyn as fs
import _oracle as orc

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
INVALID = -1
T, CP = 16, 1   # the padded batch: one channel row of 16 samples per stream


def two_frames():
    """Two 16-sample mono frames, 16 bits, the rate coded in every header so that the bare frames stand alone."""
    pcm = [[((37 * i * i + 11 * i) % 4001) - 2000 for i in range(k * 16, k * 16 + 16)] for k in range(2)]
    frames = [fs.Frame([v], [fs.verbatim()], rcode=fs.RATE_CODES[16000], number=k) for k, v in enumerate(pcm)]
    return fs.write_stream(16000, 16, frames)


def no_frame_batch():
    st = two_frames()
    noise = np.random.default_rng(20261019).integers(0, 256, 100, dtype=np.uint8).tobytes()
    return [b"", st.blob[:42], noise]


def guarded(nbytes, dest):
    import torch

    if dest == "device":
        buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        return buf, buf.data_ptr() + GUARD
    buf = np.full(GUARD + nbytes + GUARD, FILL, dtype=np.uint8)
    return buf, buf.ctypes.data + GUARD


def all_zero_between_guards(buf, nbytes):
    b = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
    return bool((b[:GUARD] == FILL).all() and (b[GUARD + nbytes:] == FILL).all() and not b[GUARD:GUARD + nbytes].any())


def stream_rows(recs, n):
    return [(r.rc, r.info.frames, r.info.decoded_samples, r.info.bad_frames, r.info.bad_crc16, r.info.md5_status,
             r.out_offset) for r in list(recs)[:n]]


def window_rows(results, n):
    return [(r.rc, r.frames, r.bad_frames, r.bad_crc16, r.samples) for r in list(results)[:n]]


def run_calls(dec, recs, total, raw):
    """Every decode call over the scan on `dec`; what each returned, by name."""
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import FRAME_DTYPE, Decoder, window_array

    n = 3
    got = {"scan": (stream_rows(recs, n), total)}
    fmt = _lib.OutFormat(_lib.SAMPLE_F32, _lib.LAYOUT_PADDED, CP, 0, T)
    for dest, flag in (("host", 0), ("device", _lib.DECODE_OUT_DEVICE)):
        buf, ptr = guarded(0, dest)   # a flat batch without a sample: nothing is written
        got[f"decode.{dest}"] = stream_rows(dec.decode(ptr, 0, flag, recs), n)
        assert all_zero_between_guards(buf, 0)
        need = Decoder.plan_output(fmt, recs, n)
        buf, ptr = guarded(need, dest)
        got[f"decode_as.{dest}"] = (need, stream_rows(dec.decode_as(ptr, need, fmt, flag, recs), n))
        assert all_zero_between_guards(buf, need)
        for name, wins in (("none", []), ("one_each", [(i, 0, T) for i in range(n)])):
            wins = window_array(wins)
            need = Decoder.plan_windows(fmt, recs, n, wins)
            buf, ptr = guarded(need, dest)
            results = dec.decode_windows(ptr, need, fmt, flag, wins)
            got[f"decode_windows.{name}.{dest}"] = (need, window_rows(results, len(wins)))
            assert all_zero_between_guards(buf, need)
        if not raw:
            continue
        frames = np.zeros(dec.n_raw_frames, dtype=FRAME_DTYPE)
        buf, ptr = guarded(0, dest)
        got[f"decode_frames.{dest}"] = len(dec.decode_frames(ptr, 0, flag, frames))
        assert all_zero_between_guards(buf, 0)
        results, need, mask_need = dec.plan_timeline(fmt)
        buf, ptr = guarded(need, dest)
        mask, mptr = guarded(mask_need, dest)
        results, frames = dec.decode_timeline(ptr, need, mptr, mask_need, fmt, flag)
        got[f"decode_timeline.{dest}"] = (need, mask_need, len(frames), [
            (r.rc, r.placed, r.dropped, r.concealed, r.gaps, r.timeline_samples) for r in list(results)[:n]])
        assert all_zero_between_guards(buf, need) and all_zero_between_guards(mask, mask_need)
    return got


def expected(raw):
    """What the calls returned before they shared their helpers.  The bare header is a stream without samples to the
    regular scan (rc 0; md5_status 0: STREAMINFO's MD5 is that of 32 samples, not of none) and no stream to the raw one."""
    none, header = (INVALID, 0, 0, 0, 0, 0, 0), (INVALID if raw else 0, 0, 0, 0, 0, 0, 0)
    streams = [none, header, none]
    windows = [(s[0], 0, 0, 0, 0) for s in streams]
    want = {"scan": (streams, 0)}
    for dest in ("host", "device"):
        want.update({f"decode.{dest}": streams, f"decode_as.{dest}": (3 * CP * T * 4, streams),
                     f"decode_windows.none.{dest}": (0, []), f"decode_windows.one_each.{dest}": (3 * CP * T * 4, windows)})
        if raw:
            want.update({f"decode_frames.{dest}": 0,
                         f"decode_timeline.{dest}": (3 * CP * T * 4, 3 * T, 0, [(INVALID, 0, 0, 0, 0, 0)] * 3)})
    return want


def test_a_batch_without_a_frame_through_every_decode_call():
    import torch

    from flac_codec_amd.gpu import Decoder, decode_many

    st = two_frames()
    rc, want, _ = orc.decode_stream(st.blob)
    assert rc == 0 and np.array_equal(want, st.pcm)
    blobs = no_frame_batch()
    for raw in (False, True):
        dec = Decoder(0)
        try:
            if raw:
                recs, total, _, frames = dec.scan_frames(blobs)
                assert len(frames) == 0
            else:
                recs, total = dec.scan(blobs)
            got = run_calls(dec, recs, total, raw)
            print(f"raw={raw}: {got!r}")
            assert got == expected(raw)
            # the handle afterwards: a stream with frames, decoded to the oracle's samples
            flat, streams = decode_many([st.blob[42:] if raw else st.blob], decoder=dec, raw=raw)
            torch.cuda.synchronize()
            s = streams[0]
            assert (s.rc, s.info.frames, s.info.bad_frames, s.info.bad_crc16) == (0, 2, 0, 0)
            assert s.info.md5_status == (2 if raw else 1)
            assert np.array_equal(flat.cpu().numpy(), want)
        finally:
            dec.close()
