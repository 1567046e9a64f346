"""flacenc_encode_many_device / BatchEncoder.encode_device with packed 24-bit input (FLACGPU_SAMPLE_S24, dtype="int24").

The expected bytes never come from the code under test: the tensor's 3-byte elements are widened and quantised in numpy
by the conversion rule (sign_extend24(x) >> (24 - bps), csrc/kernels/ingest_rule.h) and the int32 streams are encoded by
BatchEncoder.encode (flacenc_encode_many, pinned to the oracle by the existing tests); every stream's bytes, status,
altered count and MD5 must be equal.  Padding and gaps hold 0xFF bytes (-1 samples, and a carry into a neighbouring
element if a byte of them were read), which would change the files."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S24 = 24
FLAT, PADDED = 0, 1
LENGTHS = [1, 4095, 4096, 4097, 12289]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible to torch")
    return torch


def pack24(x):
    """int values -> uint8 [..., 3], the low 24 bits little-endian."""
    v = np.asarray(x).astype(np.int64) & 0xFFFFFF
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8)


def signal(seed, n, channels, bps):
    """[n, channels] int32 samples of bps bits: a slow sine plus noise, so that LPC, FIXED and the stereo modes occur."""
    rng = np.random.default_rng(seed)
    amp = (1 << (bps - 1)) - 1
    t = np.arange(n)[:, None]
    x = 0.6 * amp * np.sin(2 * np.pi * t * (0.003 + 0.002 * np.arange(channels)[None, :]) + seed)
    x += rng.normal(0, max(amp / 64, 0.7), (n, channels))
    if channels >= 2:
        x[:, 1] = 0.7 * x[:, 0] + 0.3 * x[:, 1]
    x = np.clip(np.rint(x), -amp - 1, amp).astype(np.int32)
    x[0, 0], x[n // 2, channels - 1] = -amp - 1, amp   # both ends of the range
    return x


def _opts():
    from flac_codec_amd.encode import Options

    return Options.default()


def reference_files(streams, rate, bps, channels):
    """[(status, bytes)] of flacenc_encode_many for interleaved int32 streams."""
    from flac_codec_amd.encode import BatchEncoder, _stream_lib

    enc = BatchEncoder(_opts())
    jobs, arrs, co = enc.prepare([s.reshape(-1) for s in streams], rate, bps, channels)
    _stream_lib().flacenc_encode_many(C.byref(co), jobs, len(arrs), 0)
    return [(int(jobs[i].status), enc._bufs[i][:jobs[i].out_len].tobytes()) for i in range(len(arrs))]


@functools.lru_cache(maxsize=None)
def batch(bps, channels):
    """(the int32 streams, their reference files): computed once per shape and never modified."""
    streams = [signal(100 * bps + 10 * channels + k, n, channels, bps) for k, n in enumerate(LENGTHS)]
    return streams, reference_files(streams, 48000, bps, channels)


def padded_bytes(streams, bps, channels):
    """-> (uint8 [B, C + 1, longest + 5, 3] with 0xFF in the padding, fmt args, specs)"""
    T, Cp = max(len(s) for s in streams) + 5, channels + 1
    host = np.full((len(streams), Cp, T, 3), 0xFF, dtype=np.uint8)
    for i, s in enumerate(streams):
        host[i, :channels, :len(s)] = pack24(s.T.astype(np.int64) << (24 - bps))
    return host, (S24, PADDED, Cp, 0, T), [(0, len(s)) for s in streams]


def flat_bytes(streams, bps, channels):
    """-> (uint8 [elements, 3]: the streams at odd element offsets with gaps of 0xFF, fmt args, specs)"""
    specs, at = [], 3
    for k, s in enumerate(streams):
        specs.append((at, len(s)))
        at += len(s) * channels + 1 + k % 5   # gaps of 1-5 elements: the streams start at every byte phase
    host = np.full((at, 3), 0xFF, dtype=np.uint8)
    for (off, n), s in zip(specs, streams):
        host[off:off + n * channels] = pack24(s.reshape(-1).astype(np.int64) << (24 - bps))
    return host, (S24, FLAT, 0, 0, 0), specs


def run_device(host, fmt_args, specs, rate, bps, channels, shift=0, guard=64):
    """One flacenc_encode_many_device call on host bytes uploaded with torch, the tensor `shift` bytes into its buffer.
    -> (rc, [(status, bytes, altered, md5)], output guards intact)"""
    torch = _torch()
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import _stream_lib

    L = _stream_lib()
    co = _opts()._c_options()
    fmt = _lib.OutFormat(*fmt_args)
    flat = np.concatenate([np.full(shift, 0xFF, dtype=np.uint8), host.reshape(-1)])
    t = torch.from_numpy(flat).cuda()
    jobs = (_lib.DeviceJob * len(specs))()
    bufs = []
    for i, (off, n) in enumerate(specs):
        cap = int(L.flacenc_worst_case_bytes(C.byref(co), bps, channels, n))
        buf = np.full(cap + 2 * guard, 0xA5, dtype=np.uint8)
        bufs.append(buf)
        jobs[i].in_offset, jobs[i].samples = off, n
        jobs[i].out, jobs[i].out_cap = buf.ctypes.data + guard, cap
    rc = L.flacenc_encode_many_device(C.byref(co), t.data_ptr() + shift, C.byref(fmt), rate, bps, channels, jobs,
                                      len(specs), 0, None)
    out, intact = [], True
    for i, buf in enumerate(bufs):
        j = jobs[i]
        out.append((int(j.status), buf[guard:guard + j.out_len].tobytes(), int(j.altered), bytes(j.md5)))
        intact &= bool((buf[:guard] == 0xA5).all() and (buf[buf.size - guard:] == 0xA5).all())
    return rc, out, intact


def _le(pcm, bps):
    w = (bps + 7) // 8
    return np.ascontiguousarray(pcm, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :w].tobytes()


def check(streams, want, got, rc, intact, bps, altered=None):
    assert rc == 0 and intact
    for i, ((ws, wb), (gs, gb, alt, md5)) in enumerate(zip(want, got)):
        assert (gs, ws) == (0, 0), i
        assert gb == wb, f"stream {i} ({len(streams[i])} samples): bytes differ"
        assert alt == (0 if altered is None else altered[i]), i
        assert md5 == hashlib.md5(_le(streams[i], bps)).digest() == gb[26:42], i


@pytest.mark.parametrize("layout", [PADDED, FLAT])
@pytest.mark.parametrize("bps,channels", [(24, 1), (24, 2), (24, 3), (20, 2), (16, 2), (20, 3), (16, 1)])
def test_files_equal_the_host_path(bps, channels, layout):
    streams, want = batch(bps, channels)
    host, fmt, specs = (padded_bytes if layout == PADDED else flat_bytes)(streams, bps, channels)
    rc, got, intact = run_device(host, fmt, specs, 48000, bps, channels)
    check(streams, want, got, rc, intact, bps)


@pytest.mark.parametrize("shift", [1, 2])
def test_a_tensor_at_an_unaligned_address(shift):
    streams, want = batch(24, 2)
    host, fmt, specs = flat_bytes(streams, 24, 2)
    rc, got, intact = run_device(host, fmt, specs, 48000, 24, 2, shift=shift)
    check(streams, want, got, rc, intact, 24)


def test_dropped_bits_are_counted():
    bps, channels = 20, 2
    streams, want = batch(bps, channels)
    host, fmt, specs = padded_bytes(streams, bps, channels)
    rng = np.random.default_rng(20)
    altered = []
    for i, s in enumerate(streams):   # non-zero bits below the 20 kept: the same samples, every such element counted
        dirty = rng.random((channels, len(s))) < 0.3
        dirty[0, 0] = True
        host[i, :channels, :len(s), 0] |= (dirty * rng.integers(1, 16, dirty.shape)).astype(np.uint8)
        altered.append(int(dirty.sum()))
    rc, got, intact = run_device(host, fmt, specs, 48000, bps, channels)
    check(streams, want, got, rc, intact, bps, altered)


def test_encode_device_and_back():
    """BatchEncoder.encode_device(dtype="int24") on a [B, C, T, 3] tensor and on a flat one; decode_many(dtype="int24")
    of the files returns the input bytes exactly (bps 24)."""
    torch = _torch()
    from flac_codec_amd.encode import BatchEncoder
    from flac_codec_amd.gpu import decode_many

    streams, want = batch(24, 2)
    host, _, _ = padded_bytes(streams, 24, 2)
    host = np.ascontiguousarray(host[:, :2])   # [B, C, T, 3]: the tensor's C is the channel count; T stays padded
    enc = BatchEncoder(_opts())
    t = torch.from_numpy(host).cuda()
    files = enc.encode_device(t, [len(s) for s in streams], sample_rate=48000, bits_per_sample=24, dtype="int24")
    assert files == [b for _, b in want] and enc.last_altered == [0] * len(streams)
    flat, _, specs = flat_bytes(streams, 24, 2)
    again = enc.encode_device(torch.from_numpy(flat).cuda(), [n for _, n in specs], sample_rate=48000, bits_per_sample=24,
                              dtype="int24", offsets=[o for o, _ in specs], channels=2)
    assert again == files
    batch_back, back = decode_many(files, dtype="int24", layout="padded", pad_to=host.shape[2])
    got = batch_back.cpu().numpy()
    for i, (s, r) in enumerate(zip(streams, back)):
        assert r.rc == 0 and r.info.md5_status == 1 and r.info.bits_per_sample == 24
        assert np.array_equal(got[i, :, :len(s)], host[i, :, :len(s)]), i
        assert not got[i, :, len(s):].any()
    flat_back, back = decode_many(files, dtype="int24", out="host")
    for (off, n), r in zip(specs, back):
        assert np.array_equal(r.pcm.reshape(-1, 3), flat[off:off + 2 * n])
    with pytest.raises(ValueError):
        enc.encode_device(t.view(torch.int8), None, sample_rate=48000, bits_per_sample=24, dtype="int24")
    with pytest.raises(ValueError):
        enc.encode_device(t, None, sample_rate=48000, bits_per_sample=24)   # uint8 without dtype="int24"


@pytest.mark.parametrize("name", ["int32", "int16"])
def test_encode_device_takes_flat_tensors_of_the_other_types_too(name):
    """offsets / lengths / channels describe a flat tensor of any element type, not of int24 alone."""
    torch = _torch()
    from flac_codec_amd.encode import BatchEncoder

    streams, want = batch(16, 2)
    specs, at = [], 3
    for k, s in enumerate(streams):
        specs.append((at, len(s)))
        at += s.size + 1 + k % 5
    host = np.full(at, 0x7F7F, dtype=name)   # the gaps would change the files if read
    for (off, n), s in zip(specs, streams):
        host[off:off + 2 * n] = s.reshape(-1)
    enc = BatchEncoder(_opts())
    files = enc.encode_device(torch.from_numpy(host).cuda(), [n for _, n in specs], sample_rate=48000, bits_per_sample=16,
                              offsets=[o for o, _ in specs], channels=2)
    assert files == [b for _, b in want] and enc.last_altered == [0] * len(streams)
    with pytest.raises(ValueError):   # a stream past the tensor's end
        enc.encode_device(torch.from_numpy(host).cuda(), [at], sample_rate=48000, bits_per_sample=16, offsets=[3],
                          channels=2)


def test_25_bits_refuse_the_call():
    streams, _ = batch(24, 1)
    host, fmt, specs = padded_bytes(streams, 24, 1)
    rc, got, intact = run_device(host, fmt, specs, 48000, 25, 1)
    assert rc == -151 and intact and all(g[:3] == (0, b"", 0) for g in got)
