"""flacenc_encode_many_device_out / BatchEncoder.encode_device(out="device") on the GPU: a device tensor -> finished .flac
files in slots of ONE device buffer.  The expected bytes, status, altered and md5 never come from the code under test:
they are flacenc_encode_many_device's into host buffers (pinned to flacenc_encode_many and the oracle by
test_gpu_encode_device.py), run on the same tensor with the same options and flags.  The device buffer is pre-filled
with 0xA5 and downloaded whole: every byte outside [out_offset, out_offset + out_len) of the streams that succeeded (and
outside the slots of the ones that failed, whose bytes are undefined) must still be 0xA5."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_encode_device as base
from test_gpu_encode_device import FLAT, I16, I32, LENGTHS, NO_MD5, PADDED, signal

pytestmark = pytest.mark.gpu

CANARY = 0xA5
ERR_IO, INVALID_ARG = -130, -140


def _options(block=None, batch_frames=None):
    from flac_codec_amd.encode import Options

    o = Options.default()
    if block:
        o.block_size(block)
    if batch_frames:
        o.batch_frames(batch_frames)
    return o


def worst_case(opts, bps, channels, samples):
    from flac_codec_amd.encode import _stream_lib

    co = opts._c_options()
    return int(_stream_lib().flacenc_worst_case_bytes(C.byref(co), bps, channels, samples))


def run_out(opts, host, fmt_args, specs, rate, bps, channels, slots, d_out_bytes, flags=0):
    """One flacenc_encode_many_device_out call.  specs: [(in_offset, samples)], slots: [(out_offset, out_cap)].
    -> (rc, [(status, out_offset, out_len, altered, md5)], the whole device buffer as a numpy array)"""
    torch = base._torch()
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import _stream_lib

    L = _stream_lib()
    co = opts._c_options()
    fmt = _lib.OutFormat(*fmt_args)
    t = torch.from_numpy(host).cuda()
    shard = torch.full((max(d_out_bytes, 1),), CANARY, dtype=torch.uint8, device="cuda")
    jobs = (_lib.DeviceOutJob * max(len(specs), 1))()
    for j, (off, n), (o, c) in zip(jobs, specs, slots):
        j.in_offset, j.samples, j.out_offset, j.out_cap = off, n, o, c
    rc = L.flacenc_encode_many_device_out(C.byref(co), t.data_ptr() if t.numel() else None, C.byref(fmt), rate, bps,
                                          channels, jobs, len(specs), shard.data_ptr(), d_out_bytes, flags, None)
    got = [(int(j.status), int(j.out_offset), int(j.out_len), int(j.altered), bytes(j.md5)) for j in jobs[:len(specs)]]
    return rc, got, shard.cpu().numpy()[:d_out_bytes]


def compare(want_rc, want, rc, got, out, slots, want_status=None):
    """want: run_device's [(status, bytes, altered, md5)] of the host-output call.  want_status: where the slots make a
    stream fail that the host-output call (with room enough) encoded."""
    untouched = np.ones(out.size, dtype=bool)
    for i, ((ws, wb, wa, wm), (gs, off, n, ga, gm), (so, cap)) in enumerate(zip(want, got, slots)):
        ws = want_status[i] if want_status else ws
        assert gs == ws, (i, gs, ws)
        assert (ga, gm) == (wa, wm), (i, "altered / md5")
        assert off == so
        if gs == 0:
            assert n == len(wb) and out[off:off + n].tobytes() == wb, f"stream {i}: bytes differ"
            untouched[off:off + n] = False
        else:
            assert n == 0
            untouched[so:so + cap] = False   # a failed stream's slot holds undefined bytes
    assert (out[untouched] == CANARY).all(), f"bytes outside the files were written: {np.flatnonzero(untouched & (out != CANARY))[:8]}"
    statuses = [g[0] for g in got]
    assert rc == next((s for s in statuses if s), 0)
    if not want_status:
        assert rc == want_rc


def slots_in_a_row(caps, gap=0):
    slots, at = [], 0
    for c in caps:
        slots.append((at + gap, c))
        at += gap + c
    return slots, at + gap


@pytest.mark.parametrize("flags", [0, NO_MD5])
@pytest.mark.parametrize("layout", [PADDED, FLAT])
@pytest.mark.parametrize("dtype,bps,channels", [(I16, 16, 1), (I32, 24, 2)])
def test_parity_with_the_host_output_call(dtype, bps, channels, layout, flags):
    opts = _options()
    streams = [signal(30 * channels + k, n, channels, bps) for k, n in enumerate(LENGTHS)]
    host, fmt, specs = (base.padded_batch if layout == PADDED else base.flat_batch)(streams, dtype, bps, channels)
    want_rc, want, intact, _ = base.run_device(opts, host, fmt, specs, 48000, bps, channels, flags=flags)
    assert intact and [w[0] for w in want] == [INVALID_ARG, 0, 0, 0, 0, 0]
    slots, total = slots_in_a_row([worst_case(opts, bps, channels, n) for _, n in specs], gap=3)
    rc, got, out = run_out(opts, host, fmt, specs, 48000, bps, channels, slots, total, flags=flags)
    compare(want_rc, want, rc, got, out, slots)
    if flags:
        assert all(g[4] == bytes(16) for g in got)


def test_slots_at_every_residue_in_shuffled_order():
    opts = _options()
    rng = np.random.default_rng(16)
    lengths = [300 + 531 * i for i in range(16)]   # 300 .. 8265 samples: no, one and two whole blocks, with a short last one
    streams = [signal(60 + k, n, 2, 16) for k, n in enumerate(lengths)]
    host, fmt, specs = base.padded_batch(streams, I16, 16, 2)
    want_rc, want, _, _ = base.run_device(opts, host, fmt, specs, 44100, 16, 2)
    assert want_rc == 0
    slots, at = [None] * 16, 0
    for i in rng.permutation(16):
        at += int(rng.integers(1, 41))
        at += (int(i) - at) % 16   # stream i's slot starts at residue i
        slots[i] = (at, worst_case(opts, 16, 2, lengths[i]))
        at += slots[i][1]
    assert sorted(o % 16 for o, _ in slots) == list(range(16))
    rc, got, out = run_out(opts, host, fmt, specs, 44100, 16, 2, slots, at + 29)
    compare(want_rc, want, rc, got, out, slots)


def test_runs_shorter_than_a_group():
    """silence in 256-sample blocks: every frame is about ten bytes, so several frames -- batch by batch, several RUNS --
    share one 16-byte group, and a run's head and tail fall into one group"""
    opts = _options(256)
    n = 3 * 256 + 1
    streams = [np.zeros((n, 1), dtype=np.int32) for _ in range(7)]
    host, fmt, specs = base.padded_batch(streams, I16, 16, 1)
    want_rc, want, _, _ = base.run_device(opts, host, fmt, specs, 44100, 16, 1)
    assert want_rc == 0
    from flac_codec_amd.gpu import scan_stream_host

    _, frame_at, _ = scan_stream_host(want[0][1])
    sizes = np.diff(np.append(frame_at, len(want[0][1])))
    assert len(sizes) == 4 and sizes.max() < 16, sizes
    slots, at = [], 0
    for i in range(7):
        at += (5 * i + 3 - at) % 16 + 16   # residues 3, 8, 13, 2, 7, 12, 1
        slots.append((at, len(want[i][1]) + i % 2))   # exactly the file, or one byte more
        at += slots[-1][1]
    rc, got, out = run_out(opts, host, fmt, specs, 44100, 16, 1, slots, at + 17)
    compare(want_rc, want, rc, got, out, slots)


def _plan_batches_of(whole, batch_frames, per_block):
    """batches the segments of every stream arrive in (flacenc_coalesce_plan, the planner of both entry points)"""
    from flac_codec_amd.encode import _stream_lib

    L = _stream_lib()
    L.flacenc_coalesce_plan.restype = C.c_size_t
    L.flacenc_coalesce_plan.argtypes = [C.POINTER(C.c_uint64), C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t,
                                        C.POINTER(C.c_uint32)]
    w = (C.c_uint64 * len(whole))(*whole)
    cap = 4096
    st, first, n, batch = (C.c_uint32 * cap)(), (C.c_uint64 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    bc = C.c_uint32(0)
    segs = L.flacenc_coalesce_plan(w, len(whole), batch_frames, per_block, st, first, n, batch, cap, C.byref(bc))
    assert segs <= cap
    return [sorted({batch[k] for k in range(segs) if st[k] == s}) for s in range(len(whole))]


@pytest.mark.parametrize("long_blocks", [9, 150])
def test_a_stream_among_two_short_ones_with_small_batches(long_blocks):
    """batch_frames 4, one stream of long_blocks blocks + 7 samples among two short ones.  The planner's batches hold at
    least 64 frames and it never cuts a stream of up to 32 blocks, so the 9-block stream still travels in one batch; the
    150-block stream is the one whose segments arrive in three batches, on the two contexts in rotation, each batch's
    runs continuing where the batch before stopped (asserted on the plan itself)."""
    block = 256
    opts = _options(block, batch_frames=4)
    lengths = [block + 3, long_blocks * block + 7, 2 * block]
    batches = _plan_batches_of([n // block for n in lengths], 4, block * 2)
    if long_blocks == 150:
        assert len(batches[1]) >= 3, batches
    streams = [signal(80 + k, n, 2, 16) for k, n in enumerate(lengths)]
    host, fmt, specs = base.flat_batch(streams, I16, 16, 2)
    want_rc, want, _, _ = base.run_device(opts, host, fmt, specs, 44100, 16, 2)
    assert want_rc == 0
    slots, total = slots_in_a_row([worst_case(opts, 16, 2, n) for n in lengths], gap=7)
    rc, got, out = run_out(opts, host, fmt, specs, 44100, 16, 2, slots, total)
    compare(want_rc, want, rc, got, out, slots)


def test_too_small_slots_fail_alone():
    from flac_codec_amd.gpu import scan_stream_host

    opts = _options()
    lengths = [4096 + 100, 2 * 4096 + 9, 3 * 4096, 2 * 4096 + 9, 500]
    streams = [signal(90 + k, n, 2, 16) for k, n in enumerate(lengths)]
    host, fmt, specs = base.padded_batch(streams, I16, 16, 2)
    want_rc, want, _, _ = base.run_device(opts, host, fmt, specs, 44100, 16, 2)
    assert want_rc == 0
    caps = [len(w[1]) for w in want]
    _, frame_at, _ = scan_stream_host(want[1][1])
    hlen = int(frame_at[0])
    caps[1] = hlen - 1                                            # no room for the header
    _, frame_at, _ = scan_stream_host(want[3][1])
    assert len(frame_at) == 3
    caps[3] = int(frame_at[0]) + int(frame_at[1] - frame_at[0]) + 1   # header + the first frame + 1: the second overflows it
    slots, total = slots_in_a_row(caps, gap=1)                    # neighbours one canary byte apart
    rc, got, out = run_out(opts, host, fmt, specs, 44100, 16, 2, slots, total)
    compare(want_rc, want, rc, got, out, slots, want_status=[0, ERR_IO, 0, ERR_IO, 0])
    assert rc == ERR_IO
    # a slot that holds everything but the short last block's frame
    caps = [len(w[1]) for w in want]
    caps[0] -= 1
    slots, total = slots_in_a_row(caps, gap=1)
    rc, got, out = run_out(opts, host, fmt, specs, 44100, 16, 2, slots, total)
    compare(want_rc, want, rc, got, out, slots, want_status=[ERR_IO, 0, 0, 0, 0])


def test_a_refused_call_writes_nothing():
    opts = _options()
    streams = [signal(k, 5000, 2, 16) for k in range(2)]
    host, fmt, specs = base.padded_batch(streams, I16, 16, 2)
    rc, got, out = run_out(opts, host, fmt, specs, 44100, 16, 2, [(0, 40000), (39999, 40000)], 80000)
    assert rc == INVALID_ARG and (out == CANARY).all() and all(g[0] == 0 and g[2] == 0 for g in got)


@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_round_trip_without_a_host_copy(kind):
    torch = base._torch()
    from flac_codec_amd.encode import BatchEncoder
    from flac_codec_amd.gpu import decode_many

    lengths = [4097, 2 * 4096 + 5, 777, 4096]
    streams = [signal(50 + k, n, 2, 16) for k, n in enumerate(lengths)]
    dtype = I16 if kind == "int16" else base.F32
    host, _, _ = base.padded_batch(streams, dtype, 16, 2)
    t = torch.from_numpy(np.ascontiguousarray(host[:, :2, :])).cuda()
    enc = BatchEncoder(_options())
    views = enc.encode_device(t, lengths, sample_rate=32000, bits_per_sample=16, out="device")
    assert all(v.is_cuda and v.dtype == torch.uint8 and v.dim() == 1 for v in views)
    assert enc.last_status == [0] * 4 and enc.last_altered == [0] * 4
    pcm, recs = decode_many(views, out="device")
    assert pcm.is_cuda
    for s, r, md5 in zip(streams, recs, enc.last_md5):   # (the streams ARE the quantised input: as_elements is exact)
        assert r.rc == 0 and r.info.md5_status == 1 and bytes(r.info.md5) == md5
        assert np.array_equal(r.pcm.cpu().numpy(), s)
    # the encoder's shard is reused by the next call, and the caller's own shard and slots are honoured
    first = [v.cpu().numpy().tobytes() for v in views]
    again = enc.encode_device(t, lengths, sample_rate=32000, bits_per_sample=16, out="device")
    assert again[0].data_ptr() == views[0].data_ptr() and [v.cpu().numpy().tobytes() for v in again] == first
    shard = torch.full((sum(len(f) for f in first) + 4 * 9 + 5,), CANARY, dtype=torch.uint8, device="cuda")
    slots, at = [], 5
    for f in first[::-1]:
        slots.append((at, len(f)))
        at += len(f) + 9
    slots = slots[::-1]
    mine = enc.encode_device(t, lengths, sample_rate=32000, bits_per_sample=16, out="device", shard=shard, slots=slots)
    assert [v.cpu().numpy().tobytes() for v in mine] == first
    assert [v.data_ptr() - shard.data_ptr() for v in mine] == [o for o, _ in slots]
    keep = np.ones(shard.numel(), dtype=bool)
    for o, c in slots:
        keep[o:o + c] = False
    assert (shard.cpu().numpy()[keep] == CANARY).all()


def test_out_host_is_the_default_and_unchanged():
    torch = base._torch()
    from flac_codec_amd.encode import BatchEncoder

    streams = [signal(40 + k, n, 2, 16) for k, n in enumerate([4097, 300])]
    host, _, _ = base.padded_batch(streams, base.F32, 16, 2)
    t = torch.from_numpy(np.ascontiguousarray(host[:, :2, :])).cuda()
    want = base.expected(_options(), streams, 32000, 16, 2)
    enc = BatchEncoder(_options())
    lengths = [len(s) for s in streams]
    assert enc.encode_device(t, lengths, sample_rate=32000, bits_per_sample=16) == [b for _, b in want] \
        == enc.encode_device(t, lengths, sample_rate=32000, bits_per_sample=16, out="host")
