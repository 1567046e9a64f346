"""flacgpu_decoder_decode_windows / gpu.decode_windows: sample windows of a scanned batch.

The reference is the existing path plus numpy, never the code under test: decode_many(dtype="int32", layout="flat",
out="host") of the same blobs, sliced and zero-padded per window and converted by the header's definitions (raw bits
compared for float32).  The expected frame count of a window comes from _windows.model_frames on the stream's block
sizes.  Every output buffer is 0x7F-filled between two 256-byte guards: after a call the guards are intact and every
byte of out_bytes equals the expectation, so nothing of the fill is left.

The matrix test holds about 3000 windows in one call, as wide as the longest stream (65536 samples) and 8 channels
deep: 5.8 GB of int32 / float32.  The comparison therefore runs on the device, against an expectation scattered into
zeros there; a host-destination buffer is uploaded for it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _foreign_matrix as fm
import _windows as wn

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0x7F
I32, I16, F32 = 0, 1, 2
FLAT, PADDED = 0, 1
SIGNED = {I32: np.int32, I16: np.int16, F32: np.int32}   # the element's bits as torch can hold them
OK, INVALID_ARG, UNSUPPORTED, TOO_SMALL = 0, -1, -2, -5


def convert_bits(pcm, bps, dtype):
    """The header's definitions of the three sample types on int32 PCM, as the element's raw bits."""
    pcm = np.asarray(pcm, dtype=np.int32)
    if dtype == I16:
        assert bps <= 16
        return (pcm << (16 - bps)).astype(np.int16)
    if dtype == F32:
        return (pcm.astype(np.float32) * np.float32(2.0 ** -(bps - 1))).view(np.int32)
    return pcm


@pytest.fixture(scope="module")
def dec():
    from flac_codec_amd.gpu import Decoder

    d = Decoder(0)
    yield d
    d.close()


def reference(blobs):
    """The existing path: every stream's int32 samples [samples, channels] (None for rc != 0), its rc, bps, sizes."""
    from flac_codec_amd.gpu import decode_many, scan_stream_host

    _, streams = decode_many(blobs, dtype="int32", layout="flat", out="host")
    out = []
    for blob, s in zip(blobs, streams):
        sizes = scan_stream_host(blob)[2].tolist() if s.rc == 0 else []
        assert s.rc != 0 or sum(sizes) == s.info.decoded_samples
        out.append((s.rc, s.pcm, s.info.bits_per_sample, sizes))
    return out


def window_array(windows):
    from flac_codec_amd.gpu import window_array as wa

    return wa(windows)


def decode_raw(dec, recs, n, fmt, wins, dest):
    """One decode_windows into a 0x7F-filled buffer with guards; (the whole buffer as a device uint8 tensor, out_bytes,
    results)."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    need = Decoder.plan_windows(fmt, recs, n, wins)
    if dest == "device":
        buf = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        res = dec.decode_windows(buf.data_ptr() + GUARD, need, fmt, _lib.DECODE_OUT_DEVICE, wins)
    else:
        raw = np.full(GUARD + need + GUARD, FILL, dtype=np.uint8)
        res = dec.decode_windows(raw.ctypes.data + GUARD, need, fmt, 0, wins)
        buf = torch.from_numpy(raw).to("cuda:0")
    return buf, need, res


def check(buf, need, fmt, windows, ref, res, undefined=(), bad=None):
    """Guards intact; out_bytes equal the reference's samples in their places and zero everywhere else; every window's
    record.  undefined: [(window, t0, t1)] not compared (a frame that does not decode); bad: {window: bad_frames}."""
    import torch

    N, Cp, T = len(windows), fmt.channels_padded, fmt.samples_padded
    es = 2 if fmt.dtype == I16 else 4
    assert need == N * Cp * T * es
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + need:] == FILL).all()), "a guard was written"
    idx, vals = [], []
    for w, (s, start, length) in enumerate(windows):
        rc, pcm, bps, sizes = ref[s]
        r = res[w]
        assert r.rc == rc, (w, s)
        if rc != 0:
            assert (r.frames, r.bad_frames, r.bad_crc16, r.samples) == (0, 0, 0, 0), (w, s)
            continue
        total, ch = pcm.shape
        samples = min(max(total - start, 0), length)
        assert r.samples == samples, (w, s, start, length)
        assert r.frames == wn.model_frames(sizes, start, length)[1], (w, s, start, length)
        assert (r.bad_frames, r.bad_crc16) == ((bad or {}).get(w, 0), 0), (w, s, start, length)
        if samples:
            part = convert_bits(pcm[start:start + samples], bps, fmt.dtype)   # [samples, ch]
            for c in range(ch):
                idx.append((w * Cp + c) * T + np.arange(samples, dtype=np.int64))
                vals.append(part[:, c])
    tdt = torch.int16 if fmt.dtype == I16 else torch.int32
    got = buf[GUARD:GUARD + need].view(tdt)
    want = torch.zeros(N * Cp * T, dtype=tdt, device="cuda:0")
    if idx:
        want[torch.from_numpy(np.concatenate(idx)).to("cuda:0")] = \
            torch.from_numpy(np.concatenate(vals).astype(SIGNED[fmt.dtype])).to("cuda:0")
    for w, t0, t1 in undefined:
        for c in range(Cp):
            a = (w * Cp + c) * T
            got[a + t0:a + t1] = 0
            want[a + t0:a + t1] = 0
    if not torch.equal(got, want):
        where = torch.nonzero(got != want)[:5].flatten().tolist()
        raise AssertionError(f"output differs from the reference at elements {where} (w, c, t = "
                             f"{[(e // (Cp * T), e // T % Cp, e % T) for e in where]})")


# ---- 1. the hand-built matrix
@functools.lru_cache(maxsize=None)
def matrix(narrow):
    """(streams, their reference), computed once and never modified; narrow: the streams of at most 16 bits."""
    cases = [s for s in fm.valid_cases() if s.bps <= 16 or not narrow]
    return cases, reference([s.blob for s in cases])


def matrix_windows(cases):
    rng = wn.rng_of(20241018)
    out = []
    for s, st in enumerate(cases):
        for start, length in wn.fixed_windows(st.frame_sizes) + wn.random_windows(rng, st.frame_sizes, 8):
            out.append((s, start, length))
    return out


@pytest.mark.parametrize("dest", ["host", "device"])
@pytest.mark.parametrize("dtype", [I32, I16, F32])
def test_every_window_shape_on_the_matrix(dec, dtype, dest):
    from flac_codec_amd import _lib

    assert len(fm.valid_cases()) == 133
    cases, ref = matrix(dtype == I16)
    # what a filter must not lose
    assert any(s.channels == 1 for s in cases) and any(s.channels > 2 for s in cases)
    assert len({f[1] for s in cases for f in s.features if f[0] == "side_bps"}) == 3   # the stereo assignments
    sizes = next(s for s in cases if s.name == "variable-block-size").frame_sizes
    assert len(set(sizes)) == len(sizes) > 2
    assert dtype == I16 or any(s.name == "stereo-32" for s in cases)
    blobs = [s.blob for s in cases]
    for st, (rc, pcm, bps, sizes) in zip(cases, ref):
        assert rc == 0 and sizes == list(st.frame_sizes), st.name
        assert np.array_equal(pcm.reshape(-1), st.pcm), st.name   # the reference is right by construction, too
    windows = matrix_windows(cases)
    longest = max(length for _, _, length in windows)
    fmt = _lib.OutFormat(dtype, PADDED, 8, 0, longest + 3)   # + 3: rows start at every alignment
    recs, _ = dec.scan(blobs)
    wins = window_array(windows)
    buf, need, res = decode_raw(dec, recs, len(cases), fmt, wins, dest)
    check(buf, need, fmt, windows, ref, res)


# ---- 2. more frames than one workgroup takes
def short_block_stream():
    import _flacsyn as fs

    rng = wn.rng_of(5)
    b = fm.Builder()
    frames, at = [], 0
    for k in range(300):
        pcm = [[rng.randint(-32768, 32767) for _ in range(16)] for _ in range(2)]
        frames.append(fs.Frame(pcm, [fs.verbatim(), fs.verbatim()], assignment=(1, 8, 9, 10)[k % 4], blocking=1,
                               number=at))
        at += 16
    st = b.add("short-blocks", 44100, 16, frames)
    assert st.valid and list(st.frame_sizes) == [16] * 300
    return st


def test_windows_over_many_short_frames(dec):
    from flac_codec_amd import _lib

    st = short_block_stream()
    ref = reference([st.blob])
    T = 300 * 16
    rng = wn.rng_of(6)
    windows = [(0, 7, 65 * 16 - 14), (0, 16 * 3, 128 * 16), (0, 16 * 100 + 15, 128 * 16 - 14), (0, 0, T)]
    counts = [wn.model_frames(st.frame_sizes, a, n)[1] for _, a, n in windows]
    assert counts == [65, 128, 129, 300]
    windows += [(0, a, n) for a, n in wn.random_windows(rng, st.frame_sizes, 296)]
    rng.shuffle(windows)
    assert len(windows) == 300
    recs, _ = dec.scan([st.blob])
    for dtype in (I16, F32):
        fmt = _lib.OutFormat(dtype, PADDED, 2, 0, T + 3)
        buf, need, res = decode_raw(dec, recs, 1, fmt, window_array(windows), "device")
        check(buf, need, fmt, windows, ref, res)


# ---- 3. damage
def test_windows_on_damaged_streams(dec):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import scan_stream_host

    blobs, windows, undefined, bad = [], [], [], {}
    for reason, st in fm.invalid_cases():   # 192 good samples, a frame that does not parse, 192 good samples
        s = len(blobs)
        blobs.append(st.blob)
        n = st.frame_sizes[1]
        assert list(st.frame_sizes) == [192, n, 192]
        windows += [(s, 3, 189), (s, 192 + n, 192), (s, 192 + n + 5, 500)]   # around the bad frame
        bad[len(windows)] = 1
        undefined.append((len(windows), 192 - 100, 192 - 100 + n))
        windows.append((s, 100, 92 + n + 50))                                # across it
        bad[len(windows)] = 1
        undefined.append((len(windows), 0, n - 1))
        windows.append((s, 193, n + 20))                                     # from inside it
    whole = next(s for s in fm.valid_cases() if s.name == "lpc8")
    off = scan_stream_host(whole.blob)[1].tolist()
    last = len(off) - 1
    assert last >= 3
    cut = whole.blob[:(off[last] + len(whole.blob)) // 2]   # ends inside the last frame: the scan loses sync there
    lost, junk = len(blobs), len(blobs) + 1
    blobs += [cut, b"not a FLAC stream"]
    ref = reference(blobs)
    kept = ref[lost][1].shape[0]
    assert ref[lost][0] == 0 and 0 < kept == sum(whole.frame_sizes[:last]) and ref[junk][0] != 0
    full = sum(whole.frame_sizes)
    windows += [(lost, 0, full), (lost, kept - 3, 10), (lost, kept, 5), (lost, kept + 40, 7), (junk, 0, 10), (junk, 5, 0)]
    recs, _ = dec.scan(blobs)
    assert recs[lost].info.bad_frames == 1 and recs[lost].info.decoded_samples == kept and recs[junk].rc == ref[junk][0]
    fmt = _lib.OutFormat(F32, PADDED, 2, 0, max(w[2] for w in windows) + 3)
    for dest in ("device", "host"):
        buf, need, res = decode_raw(dec, recs, len(blobs), fmt, window_array(windows), dest)
        check(buf, need, fmt, windows, ref, res, undefined, bad)
        k = len(windows) - 6
        assert [res[k + i].samples for i in range(6)] == [kept, 3, 0, 0, 0, 0]
        assert [res[k + i].frames for i in range(6)] == [last, 1, 0, 0, 0, 0]


# ---- 4. call order on one scan
def test_call_order_on_one_scan():
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    cases = [s for s in fm.valid_cases()
             if s.name in ("lpc8", "stereo-16", "stereo-32", "channels-3", "variable-block-size", "wasted-16")]
    assert len(cases) == 6 and all(s.md5_status == 1 for s in cases)
    blobs = [s.blob for s in cases]
    n = len(cases)
    rng = wn.rng_of(8)
    windows = [(s, a, k) for s, st in enumerate(cases) for a, k in wn.random_windows(rng, st.frame_sizes, 6)]
    windows_b = windows[::-1][:20]
    longest = max(s.pcm.size // s.channels for s in cases)
    padded = _lib.OutFormat(F32, PADDED, 3, 0, longest + 5)

    def as_padded(d, recs):
        need = Decoder.plan_output(padded, recs, n)
        raw = np.full(need, FILL, dtype=np.uint8)
        d.decode_as(raw.ctypes.data, need, padded, 0, recs)
        return raw, None

    def whole(d, recs):
        total = sum(s.pcm.size for s in cases)
        out = np.full(total, 0x7F7F7F7F, dtype=np.int32)
        mine = (_lib.DecodedStream * n)()
        C.memmove(mine, recs, C.sizeof(mine))
        d.decode(out.ctypes.data, total, 0, mine)
        assert all(mine[i].info.md5_status == 1 and mine[i].info.bad_frames == 0 for i in range(n))
        return out.view(np.uint8), None

    def windows_of(which, dtype):
        def run(d, recs):
            fmt = _lib.OutFormat(dtype, PADDED, 3, 0, max(w[2] for w in which) + 3)
            wins = window_array(which)
            need = Decoder.plan_windows(fmt, recs, n, wins)
            raw = np.full(need, FILL, dtype=np.uint8)
            res = d.decode_windows(raw.ctypes.data, need, fmt, 0, wins)
            return raw, [(r.rc, r.frames, r.bad_frames, r.bad_crc16, r.samples) for r in list(res)[:len(which)]]
        return run

    order = [as_padded, windows_of(windows, F32), whole, windows_of(windows_b, I32), as_padded]
    alone = []
    for call in order:   # each call alone on a fresh scan
        d = Decoder(0)
        try:
            recs, _ = d.scan(blobs)
            alone.append(call(d, recs))
        finally:
            d.close()
    d = Decoder(0)
    try:
        recs, _ = d.scan(blobs)
        for k, call in enumerate(order):
            raw, res = call(d, recs)
            assert np.array_equal(raw, alone[k][0]) and res == alone[k][1], f"call {k} differs from the same call alone"
    finally:
        d.close()
    assert np.array_equal(alone[2][0].view(np.int32), np.concatenate([s.pcm for s in cases]))
    assert any(r[1] for r in alone[1][1]) and any(r[1] for r in alone[3][1])   # the windows did decode frames


# ---- 5. refusals write nothing
def test_refusals_write_nothing(dec):
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, GpuError

    cases = [s for s in fm.valid_cases() if s.name in ("lpc8", "stereo-24", "channels-3")]
    assert [(s.bps, s.channels) for s in cases] == [(16, 1), (24, 2), (16, 3)]
    n = len(cases)
    good = [(0, 10, 100), (2, 0, 208), (0, 4000, 9)]
    W = _lib.Window
    size = 1 << 20
    fresh = Decoder(0)   # never scanned
    try:
        for dest in ("device", "host"):
            for what, windows, fmt, cap, code in (
                    ("stream >= n_streams", good + [(n, 0, 1)], (F32, PADDED, 3, 208), size, INVALID_ARG),
                    ("reserved != 0", [W(0, 1, 10, 100)], (F32, PADDED, 3, 208), size, INVALID_ARG),
                    ("start + length overflows", good + [(0, (1 << 64) - 4, 4)], (F32, PADDED, 3, 208), size, INVALID_ARG),
                    ("layout not PADDED", good, (F32, FLAT, 0, 0), size, INVALID_ARG),
                    ("samples_padded too small", good, (F32, PADDED, 3, 207), size, INVALID_ARG),
                    ("channels_padded too small", good, (I16, PADDED, 2, 208), size, INVALID_ARG),
                    ("out_cap_bytes too small", good, (I16, PADDED, 3, 208), 3 * 3 * 208 * 2 - 1, TOO_SMALL),
                    ("int16 of a 24-bit stream", good + [(1, 0, 5)], (I16, PADDED, 3, 208), size, UNSUPPORTED),
                    ("no scanned batch", good, (F32, PADDED, 3, 208), size, INVALID_ARG),
                    ("no windows", [], (F32, PADDED, 3, 208), size, OK)):
                d = fresh if what == "no scanned batch" else dec
                if d is dec:
                    dec.scan([s.blob for s in cases])
                wins = (W * len(windows))(*[w if isinstance(w, W) else W(w[0], 0, w[1], w[2]) for w in windows])
                raw = np.full(GUARD + size + GUARD, FILL, dtype=np.uint8)
                if dest == "device":
                    buf = torch.from_numpy(raw).to("cuda:0")
                    torch.cuda.synchronize()
                    ptr, flags = buf.data_ptr() + GUARD, _lib.DECODE_OUT_DEVICE
                else:
                    ptr, flags = raw.ctypes.data + GUARD, 0
                if code == OK:
                    d.decode_windows(ptr, cap, _lib.OutFormat(fmt[0], fmt[1], fmt[2], 0, fmt[3]), flags, wins)
                else:
                    with pytest.raises(GpuError) as e:
                        d.decode_windows(ptr, cap, _lib.OutFormat(fmt[0], fmt[1], fmt[2], 0, fmt[3]), flags, wins)
                    assert e.value.code == code, (dest, what, str(e.value))
                    if code == UNSUPPORTED:
                        assert "stream 1" in str(e.value)
                    if what == "no scanned batch":
                        assert "no scanned batch" in str(e.value)
                if dest == "device":
                    raw = buf.cpu().numpy()
                assert (raw == FILL).all(), (dest, what)
    finally:
        fresh.close()
    # a too-wide stream that no window names does not refuse int16
    recs, _ = dec.scan([s.blob for s in cases])
    fmt = _lib.OutFormat(I16, PADDED, 3, 0, 211)
    ref = reference([s.blob for s in cases])
    buf, need, res = decode_raw(dec, recs, n, fmt, window_array(good), "device")
    check(buf, need, fmt, good, ref, res)


# ---- 6. the Python surface
def test_python_surface(dec):
    import torch

    from flac_codec_amd.gpu import decode_windows

    cases = [s for s in fm.valid_cases() if s.name in ("lpc8", "stereo-16", "channels-3")]
    blobs = [s.blob for s in cases]
    ref = reference(blobs)
    recs, _ = dec.scan(blobs)
    tuples = [(0, 5, 300), (1, 20, 64), (2, 100, 1000), (1, 0, 0)]
    for windows in (tuples, np.array(tuples, dtype=np.int64)):
        for dtype, code in (("float32", F32), ("int16", I16), ("int32", I32)):
            batch, res = decode_windows(dec, recs, windows, dtype=dtype, out="device")
            assert isinstance(batch, torch.Tensor) and batch.is_cuda and batch.dtype == getattr(torch, dtype)
            assert tuple(batch.shape) == (4, 3, 1000) and len(res) == 4
            host, res_h = decode_windows(dec, recs, windows, dtype=dtype, out="host", pad_to=1003, pad_channels=5)
            assert isinstance(host, np.ndarray) and host.dtype == np.dtype(dtype) and host.shape == (4, 5, 1003)
            assert [r.samples for r in res] == [r.samples for r in res_h] == [300, 64, 108, 0]
            dev = batch.cpu().numpy()
            for w, (s, start, length) in enumerate(tuples):
                pcm, bps = ref[s][1], ref[s][2]
                k = res[w].samples
                want = convert_bits(pcm[start:start + k], bps, code).T
                for got, Cp in ((dev, 3), (host, 5)):
                    mine = got[w].view(SIGNED[code])
                    assert np.array_equal(mine[:want.shape[0], :k], want), (dtype, w)
                    assert not mine[want.shape[0]:].any() and not mine[:, k:].any(), (dtype, w)
    with pytest.raises(ValueError):
        decode_windows(dec, recs, tuples, out="nowhere")
    with pytest.raises(ValueError):
        decode_windows(dec, recs, [(0, 1)])
