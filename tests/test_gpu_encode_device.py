"""flacenc_encode_many_device / BatchEncoder.encode_device on the GPU: a device tensor (int32, int16 or float32; planar and
padded, or interleaved and flat) -> .flac files.  The expected bytes never come from the code under test: the tensor is
quantised in numpy by the conversion rule (csrc/kernels/ingest_rule.h) and the int32 streams are encoded by
BatchEncoder.encode (flacenc_encode_many, pinned to the oracle by the existing tests); every stream's bytes and status
must be equal."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I32, I16, F32 = 0, 1, 2
FLAT, PADDED = 0, 1
NP = {I32: np.int32, I16: np.int16, F32: np.float32}
B = 4096
LENGTHS = [0, 1, 4095, 4096, 4097, 2 * 4096 + 5]
NO_MD5 = 1


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible to torch")
    return torch


def quantise(x, dtype, bps):
    """The conversion rule in numpy -> (int32 samples, altered flags)."""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if dtype == F32:
        with np.errstate(invalid="ignore", over="ignore"):
            r = np.rint(x.astype(np.float64) * 2.0 ** (bps - 1))
        nan = np.isnan(r)
        r = np.where(nan, 0.0, r)
        q = np.clip(r, lo, hi)
        return q.astype(np.int32), nan | (q != r)
    if dtype == I16:
        drop = 16 - bps
        return (x.astype(np.int32) >> drop), (x.astype(np.int32) & ((1 << drop) - 1)) != 0
    q = np.clip(x.astype(np.int64), lo, hi)
    return q.astype(np.int32), q != x


def signal(seed, n, channels, bps):
    """[n, channels] int32 samples of bps bits: a slow sine plus noise, so that LPC, FIXED and the stereo modes all occur."""
    rng = np.random.default_rng(seed)
    amp = (1 << (bps - 1)) - 1
    t = np.arange(n)[:, None]
    x = 0.6 * amp * np.sin(2 * np.pi * t * (0.003 + 0.002 * np.arange(channels)[None, :]) + seed)
    x += rng.normal(0, max(amp / 64, 0.7), (n, channels))
    if channels >= 2:
        x[:, 1] = 0.7 * x[:, 0] + 0.3 * x[:, 1]
    return np.clip(np.rint(x), -amp - 1, amp).astype(np.int32)


def as_elements(q, dtype, bps):
    """int32 samples of bps bits -> tensor elements that quantise back to them."""
    if dtype == F32:   # exact for bps <= 25
        return (q.astype(np.float64) * 2.0 ** -(bps - 1)).astype(np.float32)
    if dtype == I16:
        return (q << (16 - bps)).astype(np.int16)
    return q.astype(np.int32)


def filler(dtype, shape):
    """What padding and gaps hold: NaN (F32) or 0x7F bytes -- never read, or the bytes differ."""
    if dtype == F32:
        return np.full(shape, np.nan, dtype=np.float32)
    return np.full(shape, 0x7F7F7F7F if dtype == I32 else 0x7F7F, dtype=NP[dtype])


def expected(opts, streams, rate, bps, channels):
    """[(status, bytes)] of BatchEncoder.encode's path for interleaved int32 streams (a 0-sample stream included)."""
    from flac_codec_amd.encode import BatchEncoder, _stream_lib

    enc = BatchEncoder(opts)
    h = enc.prepare([s.reshape(-1) for s in streams], rate, bps, channels)
    jobs, arrs, co = h
    _stream_lib().flacenc_encode_many(C.byref(co), jobs, len(arrs), 0)
    return [(int(jobs[i].status), enc._bufs[i][:jobs[i].out_len].tobytes()) for i in range(len(arrs))]


def run_device(opts, host, fmt_args, specs, rate, bps, channels, flags=0, caps=None, guard=64):
    """One flacenc_encode_many_device call on a host array uploaded with torch.  specs: [(in_offset, samples)].
    -> (rc, [(status, bytes, altered, md5)], guards_intact)"""
    torch = _torch()
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import _stream_lib

    L = _stream_lib()
    co = opts._c_options()
    fmt = _lib.OutFormat(*fmt_args)
    t = torch.from_numpy(host).cuda()
    jobs = (_lib.DeviceJob * max(len(specs), 1))()
    bufs = []
    for i, (off, n) in enumerate(specs):
        cap = int(L.flacenc_worst_case_bytes(C.byref(co), bps, channels, n)) if caps is None else caps[i]
        buf = np.full(cap + 2 * guard, 0xA5, dtype=np.uint8)
        bufs.append(buf)
        jobs[i].in_offset, jobs[i].samples = off, n
        jobs[i].out, jobs[i].out_cap = buf.ctypes.data + guard, cap
    rc = L.flacenc_encode_many_device(C.byref(co), t.data_ptr() if t.numel() else None, C.byref(fmt), rate, bps, channels,
                                      jobs, len(specs), flags, None)
    out, intact = [], True
    for i, buf in enumerate(bufs):
        j = jobs[i]
        out.append((int(j.status), buf[guard:guard + j.out_len].tobytes(), int(j.altered), bytes(j.md5)))
        intact &= bool((buf[:guard] == 0xA5).all() and (buf[buf.size - guard:] == 0xA5).all())
    return rc, out, intact, bufs


def padded_batch(streams, dtype, bps, channels):
    """[n, channels] int32 streams -> ([B, C + 1, longest + 5] array with filler in the padding, fmt args, specs)."""
    longest = max(len(s) for s in streams)
    T, Cp = longest + 5, channels + 1
    host = filler(dtype, (len(streams), Cp, T))
    for i, s in enumerate(streams):
        host[i, :channels, :len(s)] = as_elements(s, dtype, bps).T
    return host, (dtype, PADDED, Cp, 0, T), [(0, len(s)) for s in streams]


def flat_batch(streams, dtype, bps, channels):
    """... -> (flat array: streams at odd offsets, gaps of filler, fmt args, specs)"""
    specs, at = [], 3
    for s in streams:
        specs.append((at, len(s)))
        at += len(s) * channels + 5
    host = filler(dtype, (at,))
    for (off, n), s in zip(specs, streams):
        host[off:off + n * channels] = as_elements(s, dtype, bps).reshape(-1)
    return host, (dtype, FLAT, 0, 0, 0), specs


def check(opts, streams, dtype, layout, bps, channels, rate=44100):
    host, fmt, specs = (padded_batch if layout == PADDED else flat_batch)(streams, dtype, bps, channels)
    want = expected(opts, streams, rate, bps, channels)
    rc, got, intact, _ = run_device(opts, host, fmt, specs, rate, bps, channels)
    assert intact
    for i, ((ws, wb), (gs, gb, alt, md5)) in enumerate(zip(want, got)):
        assert gs == ws, (i, gs, ws)
        assert gb == wb, f"stream {i} ({len(streams[i])} samples): bytes differ"
        assert alt == 0
        if ws == 0:
            assert md5 == hashlib.md5(_le(streams[i], bps)).digest() == gb[26:42]
    assert rc == next((s for s, _ in want if s), 0)
    return got


def _le(pcm, bps):
    w = (bps + 7) // 8
    return np.ascontiguousarray(pcm, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :w].tobytes()


def _opts(kind="default"):
    from flac_codec_amd.encode import Options

    if kind == "best":
        return Options.best()
    o = Options.default()
    if kind in (1152, 576):
        o.block_size(kind)
    return o


@pytest.mark.parametrize("dtype", [I32, I16, F32])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("layout", [PADDED, FLAT])
def test_every_length_type_and_channel_count_16_bit(dtype, channels, layout):
    streams = [signal(10 * channels + k, n, channels, 16) for k, n in enumerate(LENGTHS)]
    check(_opts(), streams, dtype, layout, 16, channels)


@pytest.mark.parametrize("dtype,bps", [(I32, 8), (I16, 8), (F32, 8), (I32, 12), (I16, 12), (F32, 12), (I32, 24), (F32, 24),
                                       (I32, 32)])
def test_other_sample_widths(dtype, bps):
    streams = [signal(bps + k, n, 2, bps) for k, n in enumerate([4097, 1, 2 * 4096 + 5])]
    check(_opts(), streams, dtype, PADDED, bps, 2)


def test_float32_at_32_bits():
    """float32 holds 24 bits: at bps 32 the expected samples are the quantised floats, not the other way round."""
    rng = np.random.default_rng(32)
    x = (rng.uniform(-1.0, 1.0, (3, 1, 4097)) * np.sin(np.arange(4097) * 0.01)).astype(np.float32)
    x[0, 0, :4] = [1.0, -1.0, np.inf, -np.inf]
    q, alt = quantise(x, F32, 32)
    streams = [q[i].T.copy() for i in range(3)]
    want = expected(_opts(), streams, 48000, 32, 1)
    rc, got, intact, _ = run_device(_opts(), x, (F32, PADDED, 1, 0, 4097), [(0, 4097)] * 3, 48000, 32, 1)
    assert rc == 0 and intact
    assert [(s, b) for s, b, _, _ in got] == want
    # 1.0 and +-inf are clamped; -1.0 is -2^31 exactly, the range's own end: not altered
    assert [g[2] for g in got] == [int(alt[i].sum()) for i in range(3)] and got[0][2] == 3


@pytest.mark.parametrize("kind", ["best", 1152, 576])
@pytest.mark.parametrize("dtype", [I16, F32])
def test_other_options(kind, dtype):
    block = kind if isinstance(kind, int) else 4096
    streams = [signal(7 + k, n, 2, 16) for k, n in enumerate([0, 1, block - 1, block, block + 1, 2 * block + 5])]
    check(_opts(kind), streams, dtype, PADDED, 16, 2)


def test_batch_boundaries():
    """batch_frames 1: the front end's batches hold 64 frames, its smallest.  14 streams of 5 blocks are 70 frames: two
    batches -- the planner never cuts a stream of up to 32 blocks, so the boundary falls between two streams.  3 streams
    of 40 blocks are cut: 32 + 8 blocks, the boundary inside every stream."""
    o = _opts(1152).batch_frames(1)
    check(o, [signal(100 + k, 5 * 1152 + (k % 3), 2, 16) for k in range(14)], F32, PADDED, 16, 2)
    o = _opts(576).batch_frames(1)
    check(o, [signal(200 + k, 40 * 576 + 11 * k, 2, 16) for k in range(3)], I16, PADDED, 16, 2)


def test_altered_counts_and_clamping():
    rng = np.random.default_rng(5)
    n = 4096 + 77
    x = rng.uniform(-1.3, 1.3, (3, 2, n)).astype(np.float32)
    x[0, 0, ::97] = np.nan
    x[1, 1, ::89] = np.inf
    x[1, 0, ::83] = -np.inf
    x[2, :, : n // 2] = ((np.arange(n // 2) - 1000) + 0.5) / 32768.0   # exact ties, both parities
    q, alt = quantise(x, F32, 16)
    streams = [q[i].T.copy() for i in range(3)]
    want = expected(_opts(), streams, 44100, 16, 2)
    rc, got, intact, _ = run_device(_opts(), x, (F32, PADDED, 2, 0, n), [(0, n)] * 3, 44100, 16, 2)
    assert rc == 0 and intact
    assert [(s, b) for s, b, _, _ in got] == want
    assert [g[2] for g in got] == [int(alt[i].sum()) for i in range(3)] and all(g[2] > 0 for g in got[:2])
    # int16 at 12 bits with dirty low bits
    y = rng.integers(-32768, 32768, (2, 1, n)).astype(np.int16)
    y[1] &= ~0xF   # clean: nothing altered
    q, alt = quantise(y, I16, 12)
    streams = [q[i].T.copy() for i in range(2)]
    want = expected(_opts(), streams, 44100, 12, 1)
    rc, got, intact, _ = run_device(_opts(), y, (I16, PADDED, 1, 0, n), [(0, n)] * 2, 44100, 12, 1)
    assert rc == 0 and [(s, b) for s, b, _, _ in got] == want
    assert [g[2] for g in got] == [int(alt[0].sum()), 0] and got[0][2] > 0
    # int32 out of range at 16 bits
    z = rng.integers(-40000, 40000, (1, 1, n)).astype(np.int32)
    q, alt = quantise(z, I32, 16)
    want = expected(_opts(), [q[0].T.copy()], 44100, 16, 1)
    rc, got, intact, _ = run_device(_opts(), z, (I32, PADDED, 1, 0, n), [(0, n)], 44100, 16, 1)
    assert rc == 0 and [(s, b) for s, b, _, _ in got] == want and got[0][2] == int(alt.sum()) > 0


def test_md5_and_no_md5():
    from flac_codec_amd.gpu import decode_many

    streams = [signal(3 + k, n, 2, 24) for k, n in enumerate([4097, 777])]
    host, fmt, specs = padded_batch(streams, I32, 24, 2)
    rc, with_md5, _, _ = run_device(_opts(), host, fmt, specs, 48000, 24, 2)
    rc2, without, _, _ = run_device(_opts(), host, fmt, specs, 48000, 24, 2, flags=NO_MD5)
    assert rc == 0 and rc2 == 0
    for s, (st, blob, _, md5), (st2, blob2, _, md5_2) in zip(streams, with_md5, without):
        assert md5 == hashlib.md5(_le(s, 24)).digest() and md5_2 == bytes(16)
        assert len(blob) == len(blob2) and blob[:26] == blob2[:26] and blob[42:] == blob2[42:]
        assert blob[26:42] == md5 and blob2[26:42] == bytes(16)
    _, recs = decode_many([b for _, b, _, _ in with_md5] + [b for _, b, _, _ in without], out="host", verify_md5=True)
    assert [r.info.md5_status for r in recs] == [1, 1, 2, 2]
    for r, s in zip(recs, streams + streams):
        assert r.rc == 0 and np.array_equal(np.asarray(r.pcm), s)


@pytest.mark.parametrize("bps,channels", [(16, 1), (16, 2), (24, 2)])
def test_round_trip_of_the_hand_built_matrix(bps, channels):
    """decode_many(float32, padded) -> encode_device -> decode_many(int32) gives the matrix's PCM back."""
    import _foreign_matrix as fm
    from flac_codec_amd.encode import BatchEncoder
    from flac_codec_amd.gpu import decode_many

    _torch()
    cases = [s for s in fm.valid_cases() if s.bps == bps and s.channels == channels]
    cases = [s for s in cases if s.rate == cases[0].rate]   # one call takes one shape
    assert cases
    batch, recs = decode_many([s.blob for s in cases], dtype="float32", layout="padded", verify_md5=False)
    lengths = [r.info.decoded_samples for r in recs]
    enc = BatchEncoder(_opts())
    files = enc.encode_device(batch, lengths, sample_rate=cases[0].rate, bits_per_sample=bps)
    assert enc.last_altered == [0] * len(cases)
    _, back = decode_many(files, out="host")
    for s, r in zip(cases, back):
        assert r.rc == 0 and r.info.md5_status == 1 and r.info.bits_per_sample == bps
        assert np.array_equal(np.asarray(r.pcm).reshape(-1), s.pcm), s.name


def test_refused_calls_write_nothing():
    streams = [signal(k, 5000, 2, 16) for k in range(3)]
    host, fmt, specs = padded_batch(streams, I16, 16, 2)
    rc, got, intact, bufs = run_device(_opts(), host, fmt, specs, 44100, 24, 2)   # I16 at 24 bits
    assert rc == -151 and intact
    assert all((b == 0xA5).all() for b in bufs) and all(g[:3] == (0, b"", 0) for g in got)
    # an output buffer too small fails that job alone
    want = expected(_opts(), streams, 44100, 16, 2)
    caps = [len(want[0][1]), len(want[1][1]) - 1, len(want[2][1]) + 100]
    rc, got, intact, _ = run_device(_opts(), host, fmt, specs, 44100, 16, 2, caps=caps)
    assert rc == -130 and intact
    assert [g[0] for g in got] == [0, -130, 0]
    assert got[0][1] == want[0][1] and got[2][1] == want[2][1] and got[1][1] == b""


def test_calls_in_a_row_and_after_a_pool_release():
    from flac_codec_amd.encode import _stream_lib

    a = [signal(k, n, 2, 16) for k, n in enumerate([4097, 100])]
    b = [signal(9 + k, n, 1, 24) for k, n in enumerate([3 * 4096, 4095, 1])]
    first = check(_opts(), a, F32, PADDED, 16, 2)
    check(_opts(), b, I32, FLAT, 24, 1)
    _stream_lib().flacenc_release_pools()
    assert check(_opts(), a, F32, PADDED, 16, 2) == first


def test_encode_device_uses_the_tensor_and_lengths():
    torch = _torch()
    from flac_codec_amd.encode import BatchEncoder

    streams = [signal(40 + k, n, 2, 16) for k, n in enumerate([4097, 4096 + 2000, 300])]
    host, _, _ = padded_batch(streams, F32, 16, 2)
    host = np.ascontiguousarray(host[:, :2, :])   # [B, C, T]: the tensor's C is the channel count; T stays padded
    want = expected(_opts(), streams, 32000, 16, 2)
    enc = BatchEncoder(_opts())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):   # the tensor is produced on a side stream: the call must wait for it
        t = torch.from_numpy(host).cuda(non_blocking=True) * 1.0
        files = enc.encode_device(t, [len(x) for x in streams], sample_rate=32000, bits_per_sample=16)
    assert files == [b for _, b in want] and enc.last_altered == [0, 0, 0]
    with pytest.raises(ValueError):
        enc.encode_device(t[:, :, ::2], None, sample_rate=32000, bits_per_sample=16)
