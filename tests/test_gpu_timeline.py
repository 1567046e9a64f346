"""flacgpu_decoder_decode_timeline / gpu.decode_timeline: raw frame streams decoded onto their timelines, gaps and
frames that do not decode zeroed on the device, a validity mask beside the samples.

The expectation is _timeline.py's: every case's surviving frames, named by the case's author, placed by their coded
numbers with the writer's own PCM -- independent of any decoder -- and converted by the existing tests' models of
decode_as's conversions (test_gpu_decode_windows.convert_bits, test_gpu_decode_windows_s24.pack24).  Everything is exact
equality.  `out` and `mask` are 0xA5-filled between two 256-byte guards: after a call the guards are intact and every
byte between them equals the expectation, so nothing of the fill is left.

All cases are one scan_frames_ex batch per scan setting, decoded as int32 and float32 into host and device memory over
that one scan.  int16 and packed 24-bit refuse a batch that holds a wider stream with a timeline (that is case 10), so
they run over a scan of the same cases without the wider ones."""
import ctypes as C
import functools

import numpy as np
import pytest

import _timeline as tl
from test_gpu_decode_windows import convert_bits
from test_gpu_decode_windows_s24 import pack24

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
I32, I16, F32, S24 = 0, 1, 2, 24
FLAT, PADDED = 0, 1
ES = {I32: 4, I16: 2, F32: 4, S24: 3}
MAX_BITS = {I32: 32, F32: 32, S24: 24, I16: 16}
TOO_SMALL = -5


def piece():
    from flac_codec_amd.gpu import timeline_piece_bytes

    return timeline_piece_bytes()


@functools.lru_cache(maxsize=None)
def batch(max_bits):
    """The cases a dtype that holds max_bits can take: every refused stream, and the others up to that width."""
    return tuple(c for c in tl.cases(piece()) if c.want[False].rc != tl.OK or c.bits <= max_bits)


@functools.lru_cache(maxsize=None)
def expected(max_bits, speculative, dtype):
    """(the output's bytes, the mask's bytes, Cp, T) for batch(max_bits)."""
    cases = batch(max_bits)
    Cp, T = tl.layout(cases)
    pcm, mask = tl.expected_rows(cases, speculative, Cp, T)
    rows = []
    for c, row in zip(cases, pcm):
        ok = c.want[speculative].rc == tl.OK
        if dtype == S24:
            rows.append(pack24(row, c.bits) if ok else np.zeros(row.shape + (3,), dtype=np.uint8))
        else:
            rows.append(convert_bits(row, c.bits, dtype) if ok else np.zeros_like(convert_bits(row, 16, dtype)))
    want = np.ascontiguousarray(np.stack(rows)).view(np.uint8).reshape(-1)
    return want, mask.reshape(-1), Cp, T


@pytest.fixture(scope="module")
def decoders():
    from flac_codec_amd.gpu import Decoder

    made = {}

    def get(key):
        if key not in made:
            made[key] = Decoder(0)
        return made[key]

    yield get
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def scans(decoders):
    """(decoder, frames) of batch(max_bits) scanned with or without `speculative`: one scan per key for the module."""
    done = {}

    def get(max_bits, speculative):
        key = (max_bits, speculative)
        if key not in done:
            dec = decoders(key)
            done[key] = (dec, dec.scan_frames([c.blob for c in batch(max_bits)], speculative)[3])
        return done[key]

    return get


def guarded(nbytes, dest):
    import torch

    if dest == "device":
        buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        return buf, buf.data_ptr() + GUARD
    buf = np.full(GUARD + nbytes + GUARD, FILL, dtype=np.uint8)
    return buf, buf.ctypes.data + GUARD


def host_bytes(buf):
    return buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()


def decode_raw(dec, fmt, dest, with_mask=True):
    """One decode_timeline into 0xA5-filled buffers with guards: (out bytes, mask bytes, need, mask_need, results,
    frames); the byte arrays hold the guards."""
    import torch

    from flac_codec_amd import _lib

    _, need, mask_need = dec.plan_timeline(fmt)
    out, out_ptr = guarded(need, dest)
    mask, mask_ptr = guarded(mask_need, dest)
    torch.cuda.synchronize()
    results, frames = dec.decode_timeline(out_ptr, need, mask_ptr if with_mask else None, mask_need, fmt,
                                          _lib.DECODE_OUT_DEVICE if dest == "device" else 0)
    return host_bytes(out), host_bytes(mask), need, mask_need, results, frames


def same_bytes(got, want, what, shape=None):
    assert bool((got[:GUARD] == FILL).all()) and bool((got[GUARD + want.size:] == FILL).all()), f"{what}: a guard was written"
    body = got[GUARD:GUARD + want.size]
    if not np.array_equal(body, want):
        where = np.flatnonzero(body != want)[:5]
        raise AssertionError(f"{what} differs at bytes {where.tolist()}: got {body[where].tolist()}, want "
                             f"{want[where].tolist()}" + (f" (shape {shape})" if shape else ""))


def check_records(cases, speculative, scan_frames, results, frames, statuses=None):
    """results and frames against the cases' expectations and against the model on the scan's own records."""
    at = 0
    for i, case in enumerate(cases):
        want = case.want[speculative]
        assert tl.result_tuple(results[i]) == tl.result_tuple(want.result), case.label
        recs = [r for r in scan_frames if int(r["stream"]) == i]
        mine = frames[at:at + len(recs)]
        model, places = tl.timeline(recs)
        hidden = {a for a, _ in want.hidden}
        for (a, flags), got in zip(places, mine):
            concealed = bool(flags & tl.PLACED) and a in hidden and model["rc"] == tl.OK
            assert (int(got["at"]), int(got["flags"])) == (a, flags | (tl.CONCEALED if concealed else 0)), case.label
            assert bool(got["status"]) == concealed, case.label
        if statuses is not None:
            _, full = tl.conceal(model, places, recs, statuses[at:at + len(recs)])
            assert [(int(g["at"]), int(g["flags"]), int(g["status"])) for g in mine] == full, case.label
        at += len(recs)
    assert at == len(frames) == len(scan_frames)


def run_and_check(scans, max_bits, speculative, dtype, dest):
    from flac_codec_amd import _lib

    dec, scan_frames = scans(max_bits, speculative)
    cases = batch(max_bits)
    want, want_mask, Cp, T = expected(max_bits, speculative, dtype)
    fmt = _lib.OutFormat(dtype, PADDED, Cp, 0, T)
    out, mask, need, mask_need, results, frames = decode_raw(dec, fmt, dest)
    assert (need, mask_need) == (len(cases) * Cp * T * ES[dtype], len(cases) * T)
    same_bytes(out, want, f"out ({dtype}, {dest})", (len(cases), Cp, T))
    same_bytes(mask, want_mask, f"mask ({dtype}, {dest})", (len(cases), T))
    check_records(cases, speculative, scan_frames, results, frames)
    return out, mask, results, frames


@pytest.mark.parametrize("speculative", [False, True])
def test_every_case_in_one_batch_and_the_other_calls_beside_it(scans, speculative):
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, window_array

    first = None
    for dtype in (I32, F32):
        for dest in ("device", "host"):
            got = run_and_check(scans, 32, speculative, dtype, dest)
            first = first or (dtype, dest, got)
    dec, scan_frames = scans(32, speculative)
    cases = batch(32)
    # ---- the other calls on the same scan give what they give on a scan that never saw a timeline call
    blobs = [c.blob for c in cases]

    def run_others(d, recs):
        n = len(blobs)
        flat = np.full(d.raw_elements, 0x5A5A5A5A, dtype=np.int32)
        fr = d.decode_frames(flat.ctypes.data, flat.size, 0, np.zeros(d.n_raw_frames, dtype=scan_frames.dtype)).copy()
        fmt = _lib.OutFormat(F32, FLAT, 0, 0, 0)
        need = Decoder.plan_output(fmt, recs, n)
        as_out = np.zeros(need, dtype=np.uint8)
        d.decode_as(as_out.ctypes.data, need, fmt, _lib.DECODE_NO_MD5, recs)
        wins = window_array([(0, 100, 500), (1, 0, 300), (len(cases) - 1, 0, 10)])
        wfmt = _lib.OutFormat(I32, PADDED, 2, 0, 512)
        wneed = Decoder.plan_windows(wfmt, recs, n, wins)
        w_out = np.zeros(wneed, dtype=np.uint8)
        wres = d.decode_windows(w_out.ctypes.data, wneed, wfmt, 0, wins)
        ok = fr["status"] == 0   # the samples of a frame that does not decode are undefined
        keep = np.zeros(flat.size, dtype=bool)
        for r in fr[ok]:
            keep[int(r["out_offset"]):int(r["out_offset"]) + int(r["block_size"]) * int(r["channels"])] = True
        undefined = {int(r["stream"]) for r in fr[~ok]}
        whole = [as_out.view(np.int32)[recs[i].out_offset:recs[i].out_offset + recs[i].info.decoded_samples *
                                       recs[i].info.channels]
                 for i in range(n) if recs[i].rc == 0 and i not in undefined]
        assert len(whole) > 20 and not {0, 1, len(cases) - 1} & undefined
        return (fr, flat[keep], np.concatenate(whole), w_out,
                [(w.rc, w.frames, w.bad_frames, w.bad_crc16, w.samples) for w in wres])

    fresh = Decoder(0)
    try:
        fresh_recs = fresh.scan_frames(blobs, speculative)[0]
        want = run_others(fresh, fresh_recs)
    finally:
        fresh.close()
    # the records of the timeline's own scan: a second scan_frames would replace the batch, so they are planned anew
    recs = (_lib.DecodedStream * len(blobs))()
    C.memmove(recs, fresh_recs, C.sizeof(recs))
    got = run_others(dec, recs)
    for a, b, what in zip(got, want, ("decode_frames' records", "decode_frames' samples", "decode_as", "decode_windows",
                                      "decode_windows' results")):
        assert (np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b), what
    # decode_frames' statuses are the model's concealment
    dtype, dest, (out0, mask0, _, _) = first
    again = run_and_check(scans, 32, speculative, dtype, dest)
    assert np.array_equal(again[0], out0) and np.array_equal(again[1], mask0)
    check_records(cases, speculative, scan_frames, again[2], again[3], statuses=got[0]["status"])
    # without a mask: the same samples, and frames may be NULL
    Cp, T = tl.layout(cases)
    fmt = _lib.OutFormat(dtype, PADDED, Cp, 0, T)
    out, mask, need, _, _, _ = decode_raw(dec, fmt, "device", with_mask=False)
    assert np.array_equal(out, out0) and bool((mask == FILL).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dest", ["device", "host"])
@pytest.mark.parametrize("dtype", [I16, S24])
@pytest.mark.parametrize("speculative", [False, True])
def test_narrow_formats(scans, speculative, dtype, dest):
    run_and_check(scans, MAX_BITS[dtype], speculative, dtype, dest)


def test_whole_stream_equals_decode_many(decoders):
    from flac_codec_amd.gpu import decode_many, decode_timeline

    case = tl.cases(piece())[0]
    assert case.label == "fixed: whole"
    _, streams = decode_many([case.blob], raw=True, out="host", verify_md5=False, decoder=decoders("many"))
    buf, mask, results, frames = decode_timeline([case.blob], dtype="int32", out="host", decoder=decoders("many"))
    assert results[0].gaps == 0 and results[0].timeline_samples == streams[0].info.decoded_samples == buf.shape[2]
    assert np.array_equal(buf[0], streams[0].pcm.T) and bool(mask.all())


def small_batch(bits):
    cases = [c for c in tl.cases(piece()) if c.want[False].rc == tl.OK and c.bits <= bits][:2]
    wide = next(c for c in tl.cases(piece()) if c.want[False].rc == tl.OK and c.bits == bits)
    return cases + [wide]


def test_padding_one_sample_too_small_writes_nothing(decoders):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import GpuError

    cases = small_batch(16)
    dec = decoders("small")
    dec.scan_frames([c.blob for c in cases])
    Cp, T = tl.layout(cases)
    longest = max(c.want[False].timeline_samples for c in cases)
    for fmt in (_lib.OutFormat(I32, PADDED, Cp, 0, longest - 1), _lib.OutFormat(I32, PADDED, Cp - 1, 0, T),
                _lib.OutFormat(I32, FLAT, 0, 0, 0), _lib.OutFormat(7, PADDED, Cp, 0, T)):
        results, need, mask_need = dec.plan_timeline(fmt, check=False)
        assert need is None, "the plan accepted the format"
        assert [r.timeline_samples for r in results][:len(cases)] == [c.want[False].timeline_samples for c in cases]
        with pytest.raises(GpuError) as e:
            dec.plan_timeline(fmt)
        assert e.value.code == tl.INVALID_ARG
        nbytes = len(cases) * Cp * T * 4
        out, out_ptr = guarded(nbytes, "host")
        mask, mask_ptr = guarded(len(cases) * T, "host")
        frames = np.full(dec.n_raw_frames, 0x77, dtype=np.uint8).repeat(16).view(
            [("at", "<u8"), ("flags", "<u4"), ("status", "<u4")])
        with pytest.raises(GpuError) as e:
            dec.decode_timeline(out_ptr, nbytes, mask_ptr, len(cases) * T, fmt, 0, frames=frames)
        assert e.value.code == tl.INVALID_ARG
        assert bool((out == FILL).all()) and bool((mask == FILL).all()) and bool((frames.view(np.uint8) == 0x77).all())
    # buffers too small, an unknown flag
    fmt = _lib.OutFormat(I32, PADDED, Cp, 0, T)
    _, need, mask_need = dec.plan_timeline(fmt)
    out, out_ptr = guarded(need, "host")
    mask, mask_ptr = guarded(mask_need, "host")
    for args, code in (((out_ptr, need - 1, mask_ptr, mask_need, fmt, 0), TOO_SMALL),
                       ((out_ptr, need, mask_ptr, mask_need - 1, fmt, 0), TOO_SMALL),
                       ((out_ptr, need, mask_ptr, mask_need, fmt, 2), tl.INVALID_ARG)):
        with pytest.raises(GpuError) as e:
            dec.decode_timeline(*args)
        assert e.value.code == code
        assert bool((out == FILL).all()) and bool((mask == FILL).all())
    # no raw scan on the handle
    from flac_codec_amd.gpu import Decoder

    bare = Decoder(0)
    try:
        with pytest.raises(GpuError) as e:
            bare.plan_timeline(fmt)
        assert e.value.code == tl.INVALID_ARG
    finally:
        bare.close()


@pytest.mark.parametrize("dtype,bits", [(I16, 24), (S24, 32)])
def test_a_wider_stream_is_refused_and_named(decoders, dtype, bits):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import GpuError

    cases = small_batch(bits)
    dec = decoders("small")
    dec.scan_frames([c.blob for c in cases])
    Cp, T = tl.layout(cases)
    fmt = _lib.OutFormat(dtype, PADDED, Cp, 0, T)
    nbytes = len(cases) * Cp * T * ES[dtype]
    out, out_ptr = guarded(nbytes, "host")
    for call in (lambda: dec.plan_timeline(fmt), lambda: dec.decode_timeline(out_ptr, nbytes, None, 0, fmt, 0)):
        with pytest.raises(GpuError) as e:
            call()
        assert e.value.code == tl.UNSUPPORTED
        first_wide = next(i for i, c in enumerate(cases) if c.bits > MAX_BITS[dtype])
        assert f"stream {first_wide} has {cases[first_wide].bits} bits" in str(e.value)
    assert bool((out == FILL).all())


def test_python_surface_and_refusal_reasons(decoders):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import decode_timeline

    cases = batch(16)
    blobs = [c.blob for c in cases]
    buf, mask, results, frames = decode_timeline(blobs, decoder=decoders("surface"))   # float32, device, own maxima
    reason = _lib.lib().flacgpu_last_error().decode()
    refused = next(i for i, c in enumerate(cases) if c.want[False].rc != tl.OK)
    assert reason.startswith(f"flacgpu_decoder_decode_timeline: stream {refused}: "), reason
    Cp = max(c.channels for c in cases if c.want[False].rc == tl.OK)
    T = max(c.want[False].timeline_samples for c in cases)
    assert tuple(buf.shape) == (len(cases), Cp, T) and tuple(mask.shape) == (len(cases), T)
    pcm, want_mask = tl.expected_rows(cases, False, Cp, T)
    for i, c in enumerate(cases):
        assert results[i].rc == c.want[False].rc, c.label
        want = convert_bits(pcm[i], c.bits, F32).view(np.float32) if results[i].rc == tl.OK else np.zeros((Cp, T), np.float32)
        assert np.array_equal(buf[i].cpu().numpy().view(np.int32), want.view(np.int32)), c.label
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    host, none, _, _ = decode_timeline(blobs, dtype="int24", out="host", mask=False, pad_to=T + 3, pad_channels=Cp + 1)
    assert none is None and host.shape == (len(cases), Cp + 1, T + 3, 3)
    assert not host[:, Cp:].any() and not host[:, :, T:].any()
