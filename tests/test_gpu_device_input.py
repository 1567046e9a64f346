"""The batch decoder's device door (flacgpu_decoder_scan_device, flacgpu_decoder_scan_frames_device; kernels/gather.inc,
kernels/meta_walk.h): streams that already lie in device memory.  The contract is equivalence, and the reference in
every comparison is the HOST door (flacgpu_decoder_scan, flacgpu_decoder_scan_frames_ex) on a handle of its own, given
the same bytes from host memory: the slot buffer byte for byte, every record, every decoded sample.  All comparisons
are exact."""
import ctypes as C

import numpy as np
import pytest

import _foreign_matrix as fm
import _meta_cases as mc
import _raw_frames as rf
import _scan_layout as sl
from _pcm import synth_fast

pytestmark = pytest.mark.gpu

OK, INVALID_ARG = 0, -1
DEV = "cuda:0"
SENTINEL = sl.header(16, bits=16, style="fit", number=5)   # FF F8 ...: parses as a frame header wherever it is read


@pytest.fixture(scope="module")
def doors():
    """(the handle that only ever sees device input, the handle that only ever sees host input)"""
    import torch

    from flac_codec_amd.gpu import Decoder

    torch.cuda.init()   # torch's HIP runtime first, as in decode_many
    dev, host = Decoder(0), Decoder(0)
    yield dev, host
    dev.close()
    host.close()


def _put(blob):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8).copy()).to(DEV)[:len(blob)]


def _shard(blobs, phase=lambda i: 2 * i + 1):
    """One device tensor that holds every blob, blob i at an address that is phase(i) modulo 16, SENTINEL bytes between
    them, the last blob ending with the tensor; and the views."""
    import torch

    host, at, index = bytearray(), 0, []
    for i, b in enumerate(blobs):
        gap = len(SENTINEL) + (phase(i) - (at + len(SENTINEL))) % 16
        host += (SENTINEL * 4)[:gap]
        at += gap
        assert at % 16 == phase(i) % 16
        index.append((at, len(b)))
        host += b
        at += len(b)
    shard = torch.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8).copy()).to(DEV)
    assert shard.data_ptr() % 16 == 0 and shard.numel() == at
    return shard, [shard[o:o + n] for o, n in index]


def _raw_scan(dec, ptrs, lens, flags, stream=None, device=True):
    """The raw scans through the C ABI, with pointers as given: (rc, records, raw summaries, frames, totals) as bytes."""
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import FRAME_DTYPE

    L, n = _lib.lib(), len(ptrs)
    p = (C.c_void_p * max(n, 1))(*ptrs)
    ln = (C.c_size_t * max(n, 1))(*lens)
    recs, raw = (_lib.DecodedStream * max(n, 1))(), (_lib.RawStream * max(n, 1))()
    nf, ne, nt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    if device:
        rc = L.flacgpu_decoder_scan_frames_device(dec._h, p, ln, n, flags, C.c_void_p(stream or 0), recs, raw, C.byref(nf),
                                                  C.byref(ne), C.byref(nt))
    else:
        rc = L.flacgpu_decoder_scan_frames_ex(dec._h, p, ln, n, flags, recs, raw, C.byref(nf), C.byref(ne), C.byref(nt))
    if rc:
        return rc, None, None, None, None
    frames = np.zeros(nf.value, dtype=FRAME_DTYPE)
    assert L.flacgpu_decoder_frame_records(dec._h, frames.ctypes.data_as(C.POINTER(_lib.FrameRecord)), frames.size) == 0
    return rc, bytes(recs), bytes(raw), frames.tobytes(), (nf.value, ne.value, nt.value)


def _records_bytes(recs, n):
    from flac_codec_amd import _lib

    return bytes(recs)[:n * C.sizeof(_lib.DecodedStream)]


# ---- 1. the gather, byte for byte
def test_gather_builds_the_host_doors_slot_buffer():
    """Random-byte regions (a raw scan takes any bytes) at every source alignment and the lengths around 16, 32, 48, 64
    and 128; more than 2 WG + 1 short regions, so that many slots share a workgroup; 1 MiB + 5 bytes at an odd address; a
    zero-length region and a NULL entry.  The handle is dirtied first with a larger scan of 0xFF bytes: every byte of
    the slot buffer, tails and look-ahead included, must be the gather's own."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    rng = np.random.default_rng(20261019)
    lengths = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 4097)
    regions, phases = [], []
    for a in range(16):
        for n in lengths:
            regions.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
            phases.append(a)
    for k in range(2 * sl.WG + 40):
        regions.append(rng.integers(0, 256, int(rng.integers(1, 201)), dtype=np.uint8).tobytes())
        phases.append(int(rng.integers(0, 16)))
    regions.append(rng.integers(0, 256, (1 << 20) + 5, dtype=np.uint8).tobytes())
    phases.append(7)
    regions.append(rng.integers(0, 256, 333, dtype=np.uint8).tobytes())   # the last region ends with the tensor
    phases.append(13)
    shard, views = _shard(regions, phase=lambda i: phases[i])
    assert views[-1].data_ptr() + views[-1].numel() == shard.data_ptr() + shard.numel()
    assert views[-2].data_ptr() % 2 == 1
    # a zero-length region (a valid pointer that must not be read) and a NULL entry with a length, in the middle
    dptrs = [v.data_ptr() for v in views]
    lens = [len(r) for r in regions]
    keep = [C.c_char_p(r) for r in regions]
    hptrs = [C.cast(k, C.c_void_p).value for k in keep]
    for ptrs, valid in ((dptrs, views[3].data_ptr()), (hptrs, hptrs[3])):
        ptrs[40:40] = [valid, None]
    lens[40:40] = [0, 7]

    dev = Decoder(0)
    ref = Decoder(0)
    try:
        dev.scan_frames([b"\xff" * (3 << 20)])   # dirt: the buffer is larger than the batch below and full of 0xFF
        assert set(dev.slot_bytes()[:3 << 20]) == {0xFF}
        torch.cuda.synchronize()
        for flags in (0, _lib.SCAN_SPECULATIVE):
            got = _raw_scan(dev, dptrs, lens, flags)
            want = _raw_scan(ref, hptrs, lens, flags, device=False)
            assert got[0] == want[0] == OK
            a, b = dev.slot_bytes(), ref.slot_bytes()
            assert len(a) == len(b) and len(a) % 64 == 0 and len(a) > sum(lens)
            if a != b:
                x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
                bad = np.flatnonzero(x != y)
                raise AssertionError(f"{bad.size} bytes of the slot buffer differ, the first at {bad[0]}: "
                                     f"{x[bad[0]]} for {y[bad[0]]}")
            assert got[1:] == want[1:], flags
    finally:
        dev.close()
        ref.close()


# ---- 2. regular streams
@pytest.fixture(scope="module")
def foreign(doors):
    """The 133 streams of _foreign_matrix.py at odd offsets of one device tensor, scanned through both doors."""
    dev, host = doors
    blobs = [b for _, b in mc.foreign()]
    assert len(blobs) == 133
    shard, views = _shard(blobs)
    assert all(v.data_ptr() % 2 == 1 for v in views)
    return blobs, shard, views


def _same_streams(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.rc, g.offset) == (w.rc, w.offset), i
        assert bytes(g.info) == bytes(w.info), i


def test_regular_streams_decode_as_through_the_host_door(doors, foreign):
    from flac_codec_amd.gpu import decode_many

    dev, host = doors
    blobs, shard, views = foreign
    drecs, dtotal = dev.scan(views)
    hrecs, htotal = host.scan(blobs)
    assert dtotal == htotal and _records_bytes(drecs, len(blobs)) == _records_bytes(hrecs, len(blobs))
    assert dev.slot_bytes() == host.slot_bytes()
    flat, streams = decode_many(views, out="host", verify_md5=True, decoder=dev)
    want, wstreams = decode_many(blobs, out="host", verify_md5=True, decoder=host)
    _same_streams(streams, wstreams)
    assert np.array_equal(flat, want)
    assert sum(s.rc == OK and s.info.md5_status == 1 for s in streams) > 100
    # the same scan through decode_as: padded float32
    batch, streams = decode_many(views, out="host", dtype="float32", layout="padded", decoder=dev)
    wbatch, wstreams = decode_many(blobs, out="host", dtype="float32", layout="padded", decoder=host)
    _same_streams(streams, wstreams)
    assert batch.shape == wbatch.shape and batch.tobytes() == wbatch.tobytes()


def test_windows_of_a_device_scan(doors, foreign):
    from flac_codec_amd.gpu import decode_windows

    dev, host = doors
    blobs, shard, views = foreign
    drecs, _ = dev.scan(views)
    hrecs, _ = host.scan(blobs)
    rng = np.random.default_rng(5)
    windows = []
    for _ in range(48):
        i = int(rng.integers(0, len(blobs)))
        total = max(int(hrecs[i].info.decoded_samples), 1)
        start = int(rng.integers(0, total))
        windows.append((i, start, int(rng.integers(0, 300))))
    got, gres = decode_windows(dev, drecs, windows, dtype="int32", out="host")
    want, wres = decode_windows(host, hrecs, windows, dtype="int32", out="host")
    assert [bytes(r) for r in gres] == [bytes(r) for r in wres]
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert sum(r.samples for r in gres) > 1000


# ---- 3. metadata
def test_metadata_cases_in_one_batch(doors):
    """Every input of the CPU test of the walk (_meta_cases.py: the foreign matrix, a file cut at every length of its
    metadata, the edges) through k_meta_walk: every flacgpu_decoded_stream equals the host door's."""
    dev, host = doors
    cases = mc.all_cases()
    blobs = [b for _, b in cases]
    shard, views = _shard(blobs, phase=lambda i: (5 * i + 3) % 16)
    drecs, dtotal = dev.scan(views)
    hrecs, htotal = host.scan(blobs)
    assert dtotal == htotal
    for i, (label, _) in enumerate(cases):
        assert bytes(drecs[i]) == bytes(hrecs[i]), label
    assert dev.slot_bytes() == host.slot_bytes()
    assert sum(hrecs[i].rc == OK for i in range(len(blobs))) > 133 and sum(hrecs[i].rc != OK for i in range(len(blobs))) > 40


# ---- 4. raw streams
def _raw_doors_agree(doors, blobs, speculative):
    from flac_codec_amd.gpu import decode_frames, decode_timeline

    dev, host = doors
    shard, views = _shard(blobs, phase=lambda i: (7 * i + 1) % 16)
    got = dev.scan_frames(views, speculative=speculative)
    want = host.scan_frames(blobs, speculative=speculative)
    n = len(blobs)
    assert got[1] == want[1] and _records_bytes(got[0], n) == _records_bytes(want[0], n)
    assert bytes(got[2]) == bytes(want[2])
    assert got[3].tobytes() == want[3].tobytes()
    assert dev.slot_bytes() == host.slot_bytes()
    samples, frames, _ = decode_frames(views, out="host", decoder=dev, speculative=speculative)
    wsamples, wframes, _ = decode_frames(blobs, out="host", decoder=host, speculative=speculative)
    assert frames.tobytes() == wframes.tobytes()
    ok = np.ones(samples.size, dtype=bool)   # the samples of a frame that does not decode are undefined
    for f in wframes[wframes["status"] != 0]:
        ok[int(f["out_offset"]):int(f["out_offset"]) + int(f["block_size"]) * int(f["channels"])] = False
    assert np.array_equal(samples[ok], wsamples[ok])
    batch, mask, results, tl = decode_timeline(views, dtype="int32", out="host", decoder=dev, speculative=speculative)
    wbatch, wmask, wresults, wtl = decode_timeline(blobs, dtype="int32", out="host", decoder=host, speculative=speculative)
    assert [bytes(r) for r in results] == [bytes(r) for r in wresults]
    assert tl.tobytes() == wtl.tobytes()
    assert batch.shape == wbatch.shape and batch.tobytes() == wbatch.tobytes()
    assert mask.tobytes() == wmask.tobytes()
    return len(wframes)


@pytest.mark.parametrize("speculative", [False, True])
def test_raw_frame_inputs(doors, speculative):
    blobs = [b for _, b in rf.all_cases()]
    assert _raw_doors_agree(doors, blobs, speculative) > 100


@pytest.mark.parametrize("name", [c.name for c in sl.cases()])
def test_scan_layout_cases(doors, name):
    """The cases aimed at the scan's own structure (_scan_layout.py): block phases, slots on a workgroup's edge, the
    carry with 1 to 4 workgroups per lane -- the gather runs over the same layouts."""
    from flac_codec_amd.gpu import decode_many

    case = sl.case(name)
    if case.raw:
        assert _raw_doors_agree(doors, case.blobs, case.speculative) > 0
        return
    dev, host = doors
    shard, views = _shard(case.blobs, phase=lambda i: (3 * i + 9) % 16)
    flat, streams = decode_many(views, out="host", decoder=dev)
    want, wstreams = decode_many(case.blobs, out="host", decoder=host)
    _same_streams(streams, wstreams)
    assert np.array_equal(flat, want) and flat.size
    assert dev.slot_bytes() == host.slot_bytes()


# ---- 5. round trip without a host copy
@pytest.mark.parametrize("block,frames,last", [(4096, 6, 1000), (1152, 3, 1152)])
def test_encode_scan_decode_stays_on_the_device(block, frames, last):
    """flacgpu_encode_device leaves its frames in device memory (buffers 4 and 5); they are scanned where they lie and
    decoded to the device: the PCM that went in comes out, and no compressed byte has been in host memory."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, GpuAnalyzer

    L = _lib.lib()
    samples = block * (frames - 1) + last
    pcm = torch.from_numpy(synth_fast(40 + block, 2, 16, samples).astype(np.int32)).to(DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    an = GpuAnalyzer(block, 6, 12, True, True, 2, 0.5, 16, 2, max_frames=frames)
    dec = Decoder(0)
    try:
        an.encode_device(pcm.data_ptr(), frames, last, 0, 44100, stream=side.cuda_stream)
        offsets = torch.empty(frames + 1, dtype=torch.int64, device=DEV)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        assert hip.hipMemcpyAsync(offsets.data_ptr(), an.device_buffer(5), 8 * (frames + 1), 3, side.cuda_stream) == 0
        side.synchronize()
        total = int(offsets[frames])   # 8 bytes come down: the length of the batch, not its bytes
        assert 0 < total < 4 * 2 * samples
        rc, recs, raw, fr, totals = _raw_scan(dec, [an.device_buffer(4)], [total], 0, stream=side.cuda_stream)
        assert rc == OK and totals == (frames, 2 * samples, 2 * samples)
        from flac_codec_amd.gpu import FRAME_DTYPE

        records = np.frombuffer(fr, dtype=FRAME_DTYPE).copy()
        assert list(records["block_size"]) == [block] * (frames - 1) + [last]
        out = torch.full((2 * samples + 8,), 0x55555555, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        dec.decode_frames(out.data_ptr(), 2 * samples, _lib.DECODE_OUT_DEVICE, records)
        assert (records["status"] == 0).all()
        assert torch.equal(out[:2 * samples], pcm.reshape(-1))
        assert bool((out[2 * samples:] == 0x55555555).all())
    finally:
        dec.close()
        an.close()


# ---- 6. ordering and refusals
def test_sources_filled_on_a_side_stream(doors):
    """The source is filled by a copy queued on a side stream, behind a large fill of the same tensor, and that stream is
    passed: the scan reads the bytes, not what lay there before."""
    import torch

    dev, host = doors
    blobs = [b for _, b in rf.all_cases()][:12]
    data = b"".join(blobs)
    pinned = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).pin_memory()
    shard = torch.empty(len(data), dtype=torch.uint8, device=DEV)
    big = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(4):
            big.fill_(0xFF)   # work in front of the copy
        shard.fill_(0xFF)
        shard.copy_(pinned, non_blocking=True)
    views, at = [], 0
    for b in blobs:
        views.append(shard[at:at + len(b)])
        at += len(b)
    got = dev.scan_frames(views, stream=side)
    want = host.scan_frames(blobs)
    assert got[3].tobytes() == want[3].tobytes() and len(want[3]) > 10
    assert _records_bytes(got[0], len(blobs)) == _records_bytes(want[0], len(blobs))
    side.synchronize()


def test_pinned_host_memory_is_refused(doors):
    """A pinned host address is no device memory: INVALID_ARG, the stream named, nothing launched, no scanned batch.
    (Pinned, so that a check that let it through could not fault the device.)"""
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import PinnedBuffer

    dev, host = doors
    L = _lib.lib()
    blob = rf.uniform().blob
    good = _put(blob)
    buf = PinnedBuffer(len(blob))
    try:
        buf.array[:] = np.frombuffer(blob, dtype=np.uint8)
        assert dev.scan_frames([good])[3].size > 0   # a scanned batch, which the refused call must take away
        rc = _raw_scan(dev, [good.data_ptr(), buf.address, good.data_ptr()], [len(blob)] * 3, 0)[0]
        assert rc == INVALID_ARG
        assert b"stream 1" in L.flacgpu_last_error() and b"scan_frames_device" in L.flacgpu_last_error()
        need = C.c_uint64(0)
        assert L.flacgpu_decoder_slot_bytes(dev._h, None, 0, C.byref(need)) == INVALID_ARG   # no scanned batch
        assert L.flacgpu_decoder_frame_records(dev._h, None, 0) == INVALID_ARG
        # the regular door refuses alike
        p = (C.c_void_p * 1)(buf.address)
        ln = (C.c_size_t * 1)(len(blob))
        recs, total = (_lib.DecodedStream * 1)(), C.c_uint64(0)
        assert L.flacgpu_decoder_scan_device(dev._h, p, ln, 1, None, recs, C.byref(total)) == INVALID_ARG
        assert b"stream 0" in L.flacgpu_last_error()
        # and the handle is as good as before
        assert dev.scan_frames([good])[3].tobytes() == host.scan_frames([blob])[3].tobytes()
    finally:
        buf.close()


def test_mixed_batches_and_wrong_tensors_raise(doors):
    import torch

    dev, _ = doors
    blob = rf.uniform().blob
    t = _put(blob)
    for bad in ([t, blob], [blob, t]):
        with pytest.raises(ValueError):
            dev.scan(bad)
        with pytest.raises(ValueError):
            dev.scan_frames(bad)
    for bad in (t.cpu(), t.to(torch.int8), t.reshape(1, -1), torch.stack([t, t], 1)[:, 0]):
        with pytest.raises(ValueError):
            dev.scan_frames([bad])
    with pytest.raises(ValueError):
        dev.scan([blob], stream=torch.cuda.current_stream())


def test_unknown_flag_is_refused(doors):
    from flac_codec_amd import _lib

    dev, _ = doors
    t = _put(rf.uniform().blob)
    assert _raw_scan(dev, [t.data_ptr()], [t.numel()], 2)[0] == INVALID_ARG
    assert _raw_scan(dev, [t.data_ptr()], [t.numel()], _lib.SCAN_SPECULATIVE | 4)[0] == INVALID_ARG


def test_device_only_handle_and_empty_batches(doors):
    """Empty tensors and an empty batch scan as empty bytes do."""
    import torch

    dev, host = doors
    empty = torch.empty(0, dtype=torch.uint8, device=DEV)
    got, want = dev.scan_frames([empty, empty]), host.scan_frames([b"", b""])
    assert bytes(got[2]) == bytes(want[2]) and _records_bytes(got[0], 2) == _records_bytes(want[0], 2)
    assert dev.slot_bytes() == host.slot_bytes() == b""
    got, want = dev.scan([empty]), host.scan([b""])
    assert _records_bytes(got[0], 1) == _records_bytes(want[0], 1)
