"""flacgpu_decoder_decode_as / decode_many(dtype=, layout=): the batch decoder's int16, float32 and padded outputs.

The inputs are the hand-built matrix (_foreign_matrix.py): its st.pcm is the correct answer by construction, and every
expectation here is that PCM converted in numpy by the header's definitions -- never the int32 output of the code
under test.  Every buffer is pre-filled with 0x7F bytes between two 256-byte guards: after a decode the stream's
samples equal the expectation bit for bit, every other byte inside out_bytes is zero (so nothing of the fill is left:
the call does not depend on a cleared buffer), and the guards are untouched."""
import ctypes as C

import numpy as np
import pytest

import _flacsyn as fs
import _foreign_matrix as fm

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0x7F
I32, I16, F32 = 0, 1, 2
FLAT, PADDED = 0, 1
NP = {I32: np.int32, I16: np.int16, F32: np.float32}
BITS = {I32: np.uint32, I16: np.uint16, F32: np.uint32}
INFO_FIELDS = ["sample_rate", "channels", "bits_per_sample", "min_block", "max_block", "frames", "bad_frames",
               "bad_crc16", "total_samples", "decoded_samples", "md5", "decoded_md5", "md5_status"]


def convert(pcm, bps, dtype):
    """The header's definitions of the three sample types, on int32 PCM."""
    pcm = np.asarray(pcm, dtype=np.int32)
    if dtype == I16:
        assert bps <= 16
        return (pcm << (16 - bps)).astype(np.int16)
    if dtype == F32:
        return pcm.astype(np.float32) * np.float32(2.0 ** -(bps - 1))
    return pcm


def bits(a, dtype):
    return np.ascontiguousarray(a).view(BITS[dtype])


@pytest.fixture(scope="module")
def dec():
    from flac_codec_amd.gpu import Decoder

    d = Decoder(0)
    yield d
    d.close()


def sub16(cases):
    return [s for s in cases if s.bps <= 16]


def fmt_of(dtype, layout, cases, short=0):
    from flac_codec_amd import _lib

    if layout == FLAT:
        return _lib.OutFormat(dtype, FLAT, 0, 0, 0)
    longest = max(s.pcm.size // s.channels for s in cases)
    return _lib.OutFormat(dtype, PADDED, 8, 0, longest + 5 - short)   # + 5: rows start off 16-byte alignment


def decode_raw(dec, recs, n, fmt, dest, md5=False):
    """One decode_as into a 0x7F-filled buffer with guards; returns (the whole buffer as host bytes, out_bytes)."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    need = Decoder.plan_output(fmt, recs, n)
    flags = 0 if md5 else _lib.DECODE_NO_MD5
    if dest == "device":
        buf = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        try:
            dec.decode_as(buf.data_ptr() + GUARD, need, fmt, flags | _lib.DECODE_OUT_DEVICE, recs)
        finally:
            raw = buf.cpu().numpy()
    else:
        raw = np.full(GUARD + need + GUARD, FILL, dtype=np.uint8)
        dec.decode_as(raw.ctypes.data + GUARD, need, fmt, flags, recs)
    return raw, need


def check_output(raw, need, fmt, cases, recs, exact=None):
    """Guards intact; each stream's samples equal the converted st.pcm bit for bit (exact: per stream, None = all of
    it, or (head, tail) sample counts that must be right); every other byte of out_bytes is zero."""
    dtype, es = fmt.dtype, np.dtype(NP[fmt.dtype]).itemsize
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + need:] == FILL).all(), "a guard was written"
    body = raw[GUARD:GUARD + need]
    got = body.view(BITS[dtype])
    defined = 0   # bytes that belong to some stream's samples
    if fmt.layout == PADDED:
        Cp, Tp = fmt.channels_padded, fmt.samples_padded
        assert need == len(cases) * Cp * Tp * es
        got = got.reshape(len(cases), Cp, Tp)
    else:
        assert need == sum(s.pcm.size for s in cases) * es
    at = 0
    for i, st in enumerate(cases):
        ch, n = st.channels, st.pcm.size // st.channels
        assert recs[i].rc == 0 and recs[i].info.decoded_samples == n and recs[i].info.channels == ch, st.name
        want = bits(convert(st.pcm, st.bps, dtype), dtype).reshape(n, ch)
        if fmt.layout == PADDED:
            mine = got[i, :ch, :n].T
        else:
            assert recs[i].out_offset == at, st.name
            mine = got[at:at + n * ch].reshape(n, ch)
            at += n * ch
        part = None if exact is None else exact[i]
        if part is None:
            assert np.array_equal(mine, want), st.name
        else:   # the samples between head and tail are undefined (a frame that does not decode)
            head, tail = part
            assert np.array_equal(mine[:head], want[:head]) and np.array_equal(mine[n - tail:], want[n - tail:]), st.name
            mine[head:n - tail] = 0   # (a view of raw: not counted below)
            want = want.copy()
            want[head:n - tail] = 0
        defined += int(np.count_nonzero(np.ascontiguousarray(want).view(np.uint8)))
    # nothing but the samples is nonzero: the padding is zero and none of the fill is left
    assert int(np.count_nonzero(body)) == defined, "bytes outside the streams' samples are not zero"


def run_and_check(dec, cases, dtype, layout, dest, md5=False):
    recs, _ = dec.scan([s.blob for s in cases])
    fmt = fmt_of(dtype, layout, cases)
    raw, need = decode_raw(dec, recs, len(cases), fmt, dest, md5)
    check_output(raw, need, fmt, cases, recs)
    return recs


# ---- 1. every format, both destinations
@pytest.mark.parametrize("dest", ["host", "device"])
@pytest.mark.parametrize("layout", [FLAT, PADDED])
@pytest.mark.parametrize("dtype", [I32, I16, F32])
def test_every_format_on_the_matrix(dec, dtype, layout, dest):
    cases = list(fm.valid_cases())
    assert len(cases) == 133
    run_and_check(dec, sub16(cases) if dtype == I16 else cases, dtype, layout, dest)


def test_permuted_order_to_device(dec):
    cases = fm.valid_cases()
    order = np.random.default_rng(4321).permutation(len(cases))
    assert not np.array_equal(order, np.arange(len(cases)))
    run_and_check(dec, [cases[i] for i in order], F32, PADDED, "device")


# ---- 2. frames that begin at odd element offsets
def odd_batch():
    import random

    rng = random.Random(99)
    b = fm.Builder()
    items = []
    for n in (17, 19, 1, 4096):
        if n == 4096:
            sub = fs.fixed(2)
            v = fm._predicted(rng, n, 16, sub)
            items.append((v, fm.fit_k(v, sub)))
        else:
            items.append(([rng.randint(-32768, 32767) for _ in range(n)], fs.verbatim()))
    b.mono("odd-mono", 16, items)
    frames, at = [], 0
    for n in (17, 19, 17, 19):
        pcm = [[rng.randint(-32768, 32767) for _ in range(n)] for _ in range(3)]
        frames.append(fs.Frame(pcm, [fs.verbatim()] * 3, blocking=1, number=at))
        at += n
    b.add("odd-3-channels", 48000, 16, frames)
    frames, at = [], 0
    for k in range(5):
        pcm = [[rng.randint(-32768, 32767) for _ in range(19)] for _ in range(2)]
        pcm[0][0], pcm[1][0] = (32767, -32768) if k % 2 else (-32768, 32767)   # the side needs 17 bits
        frames.append(fs.Frame(pcm, [fs.verbatim(), fs.verbatim()], assignment=10, blocking=1, number=at))
        at += 19
    b.add("odd-mid-side", 44100, 16, frames)
    starts = {sum(st.frame_sizes[:k]) % 4 for st in b.streams for k in range(len(st.frame_sizes))}
    assert starts == {0, 1, 2, 3} and all(s.valid and s.bps == 16 for s in b.streams)
    return b.streams


ODD = None


def odd_cases():
    global ODD
    if ODD is None:
        ODD = odd_batch()
    return ODD


@pytest.mark.parametrize("dest", ["host", "device"])
@pytest.mark.parametrize("layout", [FLAT, PADDED])
@pytest.mark.parametrize("dtype", [I32, I16, F32])
def test_frames_at_odd_offsets(dec, dtype, layout, dest):
    recs = run_and_check(dec, odd_cases(), dtype, layout, dest, md5=True)
    assert all(recs[i].info.md5_status == 1 and (recs[i].info.bad_frames, recs[i].info.bad_crc16) == (0, 0)
               for i in range(3))


# ---- 3. the MD5 survives conversion
@pytest.mark.parametrize("dtype,layout", [("float32", "padded"), ("int16", "flat")])
def test_md5_survives_conversion(dtype, layout):
    from flac_codec_amd.gpu import decode_many

    cases = list(fm.valid_cases())
    if dtype == "int16":
        cases = sub16(cases)
    code = {"float32": F32, "int16": I16}[dtype]
    for verify in (True, False):
        out, streams = decode_many([s.blob for s in cases], out="device", verify_md5=verify, dtype=dtype, layout=layout)
        host = out.cpu().numpy()
        assert host.dtype == NP[code]
        if layout == "padded":
            assert host.shape == (len(cases), 8, max(s.pcm.size // s.channels for s in cases))
        for i, (st, s) in enumerate(zip(cases, streams)):
            assert s.rc == 0 and (s.info.bad_frames, s.info.bad_crc16) == (0, 0), st.name
            if verify:
                assert s.info.md5_status == st.md5_status and bytes(s.info.decoded_md5) == st.digest, st.name
            else:
                assert s.info.md5_status == 3, st.name
            n = st.pcm.size // st.channels
            want = bits(convert(st.pcm, st.bps, code), code).reshape(n, st.channels)
            assert tuple(s.pcm.shape) == ((st.channels, n) if layout == "padded" else (n, st.channels)), st.name
            mine = bits(s.pcm.cpu().numpy(), code)
            assert np.array_equal(mine.T if layout == "padded" else mine, want), st.name
            if layout == "padded":
                assert not host[i, st.channels:].any() and not host[i, :, n:].any(), st.name


# ---- 4. refusals write nothing
def test_refusals_write_nothing(dec):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import GpuError

    wide = [s for s in fm.valid_cases() if s.name in ("lpc8", "stereo-24", "channels-3")]
    assert [s.bps for s in wide] == [16, 24, 16]
    odd = odd_cases()
    for dest in ("device", "host"):
        for cases, fmt, cap_short, code in (
                (wide, _lib.OutFormat(I16, FLAT, 0, 0, 0), -1, -2),          # UNSUPPORTED: a 24-bit stream
                (wide, _lib.OutFormat(I16, PADDED, 8, 0, 1 << 16), -1, -2),
                (odd, fmt_of(F32, PADDED, odd, short=6), 0, -1),              # INVALID_ARG: pad_to = max - 1
                (odd, fmt_of(I16, PADDED, odd), 1, -5),                       # BUFFER_TOO_SMALL: out_bytes - 1
                (odd, fmt_of(F32, FLAT, odd), 1, -5)):
            recs, _ = dec.scan([s.blob for s in cases])
            size = 1 << 20   # any room: nothing may be written to it
            raw = np.full(GUARD + size + GUARD, FILL, dtype=np.uint8)
            if dest == "device":
                import torch

                buf = torch.from_numpy(raw).to("cuda:0")
                torch.cuda.synchronize()
                ptr = buf.data_ptr() + GUARD
            else:
                ptr = raw.ctypes.data + GUARD
            cap = size
            if cap_short > 0:
                from flac_codec_amd.gpu import Decoder

                cap = Decoder.plan_output(fmt, recs, len(cases)) - cap_short
                assert 0 < cap < size
            flags = _lib.DECODE_OUT_DEVICE if dest == "device" else 0
            with pytest.raises(GpuError) as e:
                dec.decode_as(ptr, cap, fmt, flags, recs)
            assert e.value.code == code, (dest, fmt.dtype, fmt.layout, str(e.value))
            if code == -2:
                assert "stream 1" in str(e.value)
            if dest == "device":
                raw = buf.cpu().numpy()
            assert (raw == FILL).all(), (dest, code)


# ---- 5. malformed frames
def test_malformed_frames_as_padded_float(dec):
    from flac_codec_amd import _lib

    bad = fm.invalid_cases()
    good = [s for s in fm.valid_cases() if s.name in ("lpc8", "stereo-32", "channels-3", "wasted-16")]
    assert len(good) == 4
    batch, kinds = [], []
    for k, (reason, st) in enumerate(bad):   # valid streams between the malformed ones
        batch.append(st)
        kinds.append(reason)
        if k % 3 == 0:
            batch.append(good[(k // 3) % 4])
            kinds.append(None)
    n = len(batch)
    recs, total = dec.scan([st.blob for st in batch])
    fmt = fmt_of(F32, PADDED, batch)
    raw, need = decode_raw(dec, recs, n, fmt, "device", md5=True)
    mine = [(recs[i].info.frames, recs[i].info.bad_frames, recs[i].info.bad_crc16) for i in range(n)]
    # the same scan through flacgpu_decoder_decode
    import torch

    flat = torch.empty(total, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ref = (_lib.DecodedStream * n)()
    dec.decode(flat.data_ptr(), total, _lib.DECODE_OUT_DEVICE, ref)
    assert mine == [(ref[i].info.frames, ref[i].info.bad_frames, ref[i].info.bad_crc16) for i in range(n)]
    assert all(m == ((3, 1, 0) if reason else (st.n_frames, 0, 0)) for m, reason, st in zip(mine, kinds, batch))
    exact = [None if reason is None else (192, 192) for reason in kinds]
    check_output(raw, need, fmt, batch, recs, exact)
    for i, reason in enumerate(kinds):
        if reason is None:
            assert recs[i].info.md5_status == batch[i].md5_status and bytes(recs[i].info.decoded_md5) == batch[i].digest


# ---- 6. one scan, many decodes
def test_one_scan_many_decodes(dec):
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import decode_many

    cases = sub16(fm.valid_cases())
    n = len(cases)
    blobs = [s.blob for s in cases]
    recs, total = dec.scan(blobs)
    first = (_lib.DecodedStream * n)()
    C.memmove(first, recs, C.sizeof(first))
    fmt = fmt_of(F32, PADDED, cases)
    raw, need = decode_raw(dec, first, n, fmt, "device", md5=True)
    check_output(raw, need, fmt, cases, first)
    flat = torch.full((total,), 0x7F7F7F7F, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    middle = (_lib.DecodedStream * n)()
    C.memmove(middle, recs, C.sizeof(middle))
    dec.decode(flat.data_ptr(), total, _lib.DECODE_OUT_DEVICE, middle)
    last = (_lib.DecodedStream * n)()
    C.memmove(last, recs, C.sizeof(last))
    fmt = fmt_of(I16, FLAT, cases)
    raw, need = decode_raw(dec, last, n, fmt, "device", md5=True)
    check_output(raw, need, fmt, cases, last)
    fresh_flat, fresh = decode_many(blobs, out="device")
    assert torch.equal(flat, fresh_flat)
    assert np.array_equal(flat.cpu().numpy(), np.concatenate([s.pcm for s in cases]))
    for i, (st, s) in enumerate(zip(cases, fresh)):
        for r in (first[i], middle[i], last[i]):
            assert (r.rc, r.out_offset) == (s.rc, s.offset), st.name
            for f in INFO_FIELDS:
                a, b = getattr(r.info, f), getattr(s.info, f)
                assert (a if isinstance(a, int) else bytes(a)) == (b if isinstance(b, int) else bytes(b)), (st.name, f)
        assert s.info.md5_status == st.md5_status and bytes(s.info.decoded_md5) == st.digest, st.name
