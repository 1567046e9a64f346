"""Every kind of batch behind every other kind on ONE context (csrc/flacenc_gpu.hip: the Batch record of the batch in hand).

A context keeps what it knows about the batch submitted last -- kind, frame lengths, tables, where the PCM and the frames
lie -- for the fetch, verify and re-decision entries that follow.  Nothing of the batch before may reach them: for every
ordered pair (a, b) of the kinds below, a and then b run on a shared context, and b's bytes, offsets, fetch() plans and
residual rows must be what b gives on a fresh context that makes only that call (parity with the oracle is the other
tests' job), the device verifier must find its frames clean and fetch_decoded must return its input.  Each kind's route is
asserted through flacenc_plan_route_row first, so that no kind quietly runs another path (a ragged batch has no row in the
hook: its route takes no argument but its being ragged).

A call REFUSED for its arguments launches nothing and leaves the batch in hand fetchable with the same bytes: one leg per
refusal between a and its fetch.

One shape grants every route: 16-bit stereo, blocks of 4096, LPC order 12, max_frames 384."""
import ctypes as C

import numpy as np
import pytest

from _pcm import synth_fast

pytestmark = pytest.mark.gpu

B, CH, BPS, RATE, MAX_FRAMES = 4096, 2, 16, 48000, 384
FRAME = B * CH
K0_COPY, K0_PACKED, DIRECT_STEREO = 0, 1, 3
RAGGED_LENGTHS = [1, 4096, 192, 100]
SEGMENTS = [(2, 100), (3, 0x7FFFFFF0)]      # (frames, first frame number), cut from the head of the PCM back to back


def analyzer(max_po=6):
    from flac_codec_amd.gpu import GpuAnalyzer

    return GpuAnalyzer(B, max_po, 12, True, True, 2, 0.5, BPS, CH, max_frames=MAX_FRAMES)


def route_of(**kw):
    from test_route_table import route

    row = dict(channels=CH, bps=BPS, block=B, order=12, po=6, exhaustive=1, layout=0, aligned=1, short_last=0, n_frames=6, packed=0,
               lag_split=4, timing=0, segments=0, knobs=0, chunk=-1, two_ranges=0, whole_call=1)
    row.update(kw)
    return route(row)       # [input, hand, fast_analysis, fast_pack, k4_in_autocorr, range_frames, two_ranges, host_out, in_place]


class World:
    """The PCM on the host and on the device, and the plans flacgpu_pack_plans is handed."""

    def __init__(self):
        import torch

        self.torch = torch
        self.pcm = np.ascontiguousarray(synth_fast(9100, CH, BPS, B * MAX_FRAMES), dtype=np.int32)
        try:
            self.dev = torch.from_numpy(self.pcm).cuda()
            self.odd = torch.empty(2 * FRAME + 1, dtype=torch.int32, device="cuda")   # the first segment, 4 bytes off
            self.odd[1:] = self.dev[:2 * FRAME]
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.skip(f"torch cannot use the GPU here: {e}")
        self.ptr = self.dev.data_ptr()
        assert self.ptr % 16 == 0
        self.pinned = []          # [pinned in, pinned out] of the packed segments, kept: a context may look at them until it is closed
        an = analyzer()
        an.encode_frames(self.pcm[:4 * FRAME + 1000 * CH], 5, 1000, 7, RATE)
        self.plans, self.subs, _ = an.fetch(5, want_residuals=False)
        an.close()

    def sync(self):
        self.torch.cuda.synchronize()

    def close(self):
        from flac_codec_amd import _lib

        for h in self.pinned:
            _lib.lib().flacgpu_host_free(h)
        self.pinned = []


# ---------------------------------------------------------------------------------------------------------------------
# the kinds: run(world, analyzer) -> (bytes, offsets); what the batch holds (frames, the last one's length, every
# frame's length for a ragged one, its interleaved input); what verify_device is asked (first frame number; None: the
# frames went to the caller's pinned buffer and the verifier says so)
# ---------------------------------------------------------------------------------------------------------------------
def fetched(w, an):
    w.sync()
    return an.fetch_frames()


def k_host(w, an):
    assert route_of(n_frames=5, short_last=B - 1000)[:4] == [K0_COPY, 0, 4, 4]      # four frames fast, the short one generic
    return an.encode_frames(w.pcm[:4 * FRAME + 1000 * CH], 5, 1000, 7, RATE)


def k_device(w, an):
    assert route_of()[0] == DIRECT_STEREO
    an.encode_device(w.ptr, 6, B, 11, RATE)
    return fetched(w, an)


def k_ranges(w, an):
    r = route_of(n_frames=384, chunk=2)
    assert (r[0], r[5]) == (DIRECT_STEREO, 256) and route_of(n_frames=384, chunk=1)[5] == 0
    an.set_tuning(an.TUNE_CHUNK_MSAMPLES, 2)
    try:
        an.encode_device(w.ptr, 384, B, 3, RATE)
    finally:
        an.set_tuning(an.TUNE_CHUNK_MSAMPLES, 0)      # never cut: what every other kind here gets anyway
    return fetched(w, an)


def k_two_ranges(w, an):
    assert route_of(n_frames=256, two_ranges=1, chunk=0)[6] == 1 and route_of(n_frames=255, two_ranges=1, chunk=0)[6] == 0
    an.set_two_ranges(True)
    try:
        an.encode_device(w.ptr, 256, B, 5, RATE)
    finally:
        an.set_two_ranges(False)
    return fetched(w, an)


def host_segments(w):
    out, at = [], 0
    for n, first in SEGMENTS:
        out.append((w.pcm[at * FRAME:(at + n) * FRAME], first))
        at += n
    return out


def k_host_segments(w, an):
    assert route_of(n_frames=5, whole_call=0)[0] == DIRECT_STEREO       # gathered into the context's buffer, read in place there
    return an.encode_segments(host_segments(w), RATE)


def k_device_segments(w, an):
    r = route_of(n_frames=5, segments=1, whole_call=0)
    assert (r[0], r[8]) == (DIRECT_STEREO, 1)
    an.encode_segments_device([(w.ptr, 2, SEGMENTS[0][1]), (w.ptr + 2 * FRAME * 4, 3, SEGMENTS[1][1])], RATE)
    return fetched(w, an)


def k_device_segments_gathered(w, an):
    assert route_of(n_frames=5, segments=1, whole_call=0, aligned=0)[8] == 0
    an.encode_segments_device([(w.odd.data_ptr() + 4, 2, SEGMENTS[0][1]), (w.ptr + 2 * FRAME * 4, 3, SEGMENTS[1][1])], RATE)
    return fetched(w, an)


def k_packed_segments_host(w, an):
    """GpuAnalyzer.encode_segments_packed with the pinned buffers kept until the module is done"""
    from test_gpu_packed import le_bytes

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import GpuError

    r = route_of(n_frames=5, packed=2, whole_call=0)
    assert (r[0], r[7]) == (K0_PACKED, 1)                               # ... and every frame may go straight to pinned memory
    L = _lib.lib()
    src = le_bytes(w.pcm[:5 * FRAME], 2)
    segs = (_lib.Segment * len(SEGMENTS))()
    for i, (n, first) in enumerate(SEGMENTS):
        segs[i].pcm, segs[i].n_frames, segs[i].first_frame_number = None, n, first
    cap = L.flacgpu_packed_cap(an._h)
    if not w.pinned:
        w.pinned = [L.flacgpu_host_alloc(src.size + 64), L.flacgpu_host_alloc(cap)]
        assert all(w.pinned)
    hin, hout = w.pinned
    C.memmove(hin, src.ctypes.data, src.size)
    an.last_frames = 5
    offp, total = C.POINTER(C.c_uint64)(), C.c_uint64(0)
    for where, call in (("submit", lambda: L.flacgpu_encode_segments_packed_async_host(an._h, hin, 2, segs, len(SEGMENTS), RATE, hout, cap)),
                        ("frames_ready", lambda: L.flacgpu_frames_ready(an._h, C.byref(offp), C.byref(total))),
                        ("fetch_frames_async", lambda: L.flacgpu_fetch_frames_async(an._h, hout, cap)),
                        ("wait", lambda: L.flacgpu_wait(an._h))):
        rc = call()
        if rc:
            raise GpuError(rc, where)
    return C.string_at(hout, total.value), [offp[i] for i in range(6)]


def ragged_frames(w):
    """(element offset in the PCM, samples, frame number): every frame starts off the 16-byte grid of the device buffer"""
    out, at = [], 1
    for k, n in enumerate(RAGGED_LENGTHS):
        out.append((at, n, 5000 + 11 * k))
        at += n * CH + (2 if (at + n * CH) % 4 == 0 else 0)
    assert all(a % 4 for a, _, _ in out)
    return out


def k_ragged(w, an):
    an.encode_ragged_device([(w.ptr + 4 * at, n, num) for at, n, num in ragged_frames(w)], RATE)
    return fetched(w, an)


def k_pack_plans(w, an):
    return an.pack_plans(w.pcm[:4 * FRAME + 1000 * CH], 5, 1000, w.plans, w.subs, 7, RATE)


def k_packed_async(w, an):
    from test_gpu_packed import le_bytes

    assert route_of(packed=2, whole_call=0)[0] == K0_PACKED
    return an.encode_packed(le_bytes(w.pcm[:6 * FRAME], 2), 2, 6, B, 9, RATE)


class Kind:
    def __init__(self, name, run, n, last, first, pcm, lengths=None):
        self.name, self.run, self.n, self.last, self.first, self.pcm = name, run, n, last, first, pcm
        self.lengths = lengths or [B] * (n - 1) + [last]


def head(frames, last=B):
    return lambda w: w.pcm[:(frames - 1) * FRAME + last * CH]


KINDS = [
    Kind("host", k_host, 5, 1000, 7, head(5, 1000)),
    Kind("device", k_device, 6, B, 11, head(6)),
    Kind("ranges", k_ranges, 384, B, 3, head(384)),
    Kind("two_ranges", k_two_ranges, 256, B, 5, head(256)),
    Kind("host_segments", k_host_segments, 5, B, 0, head(5)),
    Kind("device_segments", k_device_segments, 5, B, 0, head(5)),
    Kind("device_segments_gathered", k_device_segments_gathered, 5, B, 0, head(5)),
    Kind("packed_segments_host", k_packed_segments_host, 5, B, None, head(5)),
    Kind("ragged", k_ragged, 4, RAGGED_LENGTHS[-1], 0,
         lambda w: np.concatenate([w.pcm[at:at + n * CH] for at, n, _ in ragged_frames(w)]), RAGGED_LENGTHS),
    Kind("pack_plans", k_pack_plans, 5, 1000, 7, head(5, 1000)),
    Kind("packed_async", k_packed_async, 6, B, 9, head(6)),
]
NAMES = [k.name for k in KINDS]


def plan_view(kind, plans, subs, res):
    """what fetch() promises of a batch, field by field (the bytes beyond -- coefficients past the order, Rice parameters
    past the partitions, residual rows past the frame -- are whatever the buffers held)"""
    out = []
    for f, n in enumerate(kind.lengths):
        p = plans[f]
        out.append((p.assignment, p.channels, p.block_size, p.body_bits))
        for c in range(CH):
            s = subs[f * CH + c]
            key = [s.type, s.wasted, s.bps, s.bits, s.source]
            row = 1                                              # CONSTANT: the one sample
            if s.type in (2, 3):                                 # FIXED, LPC: warm-up + residuals
                key += [s.order, s.coding_method, s.partition_order, s.n_partitions, s.part_len,
                        bytes(s.rice[:s.n_partitions]), bytes(s.escape_bits[:s.n_partitions])]
                row = n
            if s.type == 3:
                key += [s.precision, s.shift, list(s.coeffs[:s.order])]
            if s.type == 1:                                      # VERBATIM
                row = n
            out.append((key, res[f, c, :row].tobytes()))
    return out


class Solo:
    def __init__(self, data, off, view):
        self.data, self.off, self.view = data, list(off), view


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.fixture(scope="module")
def solo(world):
    """every kind on a fresh context that makes only that call: computed once, never changed"""
    out = {}
    for kind in KINDS:
        an = analyzer()
        try:
            data, off = kind.run(world, an)
            assert len(off) == kind.n + 1 and off[-1] == len(data) and off[0] == 0, kind.name
            out[kind.name] = Solo(data, off, plan_view(kind, *an.fetch(kind.n)))
        finally:
            an.close()
    return out


@pytest.fixture(scope="module")
def shared(world):
    an = analyzer()
    yield an
    an.close()


def check_in_hand(world, an, kind, want, where, got=None):
    """the batch in hand is `kind`'s, whole: bytes and offsets, the verifier's word, fetch()'s plans and rows, the PCM"""
    from flac_codec_amd.gpu import GpuError

    data, off = got or an.fetch_frames()
    assert list(off) == want.off and data == want.data, where
    if kind.first is None:
        with pytest.raises(GpuError) as e:
            an.verify_device(RATE, 0)
        assert e.value.code == -2 and "host buffer" in str(e.value), where      # FLACGPU_ERR_UNSUPPORTED
    else:
        res, _ = an.verify_device(RATE, kind.first)
        assert (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs) == (kind.n, 0, 0, 0), where
    assert plan_view(kind, *an.fetch(kind.n)) == want.view, where
    if kind.first is not None:
        pcm = kind.pcm(world)
        assert np.array_equal(an.fetch_decoded(kind.n, kind.last)[:pcm.size], pcm), where


@pytest.mark.parametrize("a", NAMES)
def test_each_kind_behind_each_other_kind(world, solo, shared, a):
    first = KINDS[NAMES.index(a)]
    for kind in KINDS:
        if kind is first:
            continue
        first.run(world, shared)
        got = kind.run(world, shared)
        check_in_hand(world, shared, kind, solo[kind.name], "%s behind %s" % (kind.name, a), got)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: (name, what is called); each must raise and leave the batch in hand as it was
# ---------------------------------------------------------------------------------------------------------------------
def r_too_many_frames(w, an):
    an.encode_device(w.ptr, MAX_FRAMES + 1, B, 0, RATE)


def r_too_many_segment_frames(w, an):
    an.encode_segments_device([(w.ptr, 200, 0), (w.ptr, 185, 0)], RATE)


def r_empty_segment(w, an):
    an.encode_segments_device([(w.ptr, 2, 0), (w.ptr, 0, 9)], RATE)


def r_bad_ragged_frame(w, an):
    an.encode_ragged_device([(w.ptr + 4, 100, 0), (0, 100, 1)], RATE)


def r_ragged_frame_off_its_alignment(w, an):
    an.encode_ragged_device([(w.ptr + 4, 100, 0), (w.ptr + 2, 100, 1)], RATE)


def r_packed_width(w, an):
    from test_gpu_packed import le_bytes

    an.encode_packed(le_bytes(w.pcm[:2 * FRAME], 3), 3, 2, B, 0, RATE)       # three bytes a sample into a 16-bit context


REFUSALS = [r_too_many_frames, r_too_many_segment_frames, r_empty_segment, r_bad_ragged_frame, r_ragged_frame_off_its_alignment,
            r_packed_width]
# (the packed segments' bytes left the context with the call, for the caller's buffer: nothing to fetch again)
HELD = [k for k in KINDS if k.first is not None]


@pytest.mark.parametrize("a", [k.name for k in HELD])
def test_a_refused_call_leaves_the_batch_in_hand(world, solo, shared, a):
    from flac_codec_amd.gpu import GpuError

    kind = KINDS[NAMES.index(a)]
    kind.run(world, shared)
    for refuse in REFUSALS:
        with pytest.raises(GpuError):
            refuse(world, shared)
        shared.last_frames = kind.n       # (the Python handle counted the refused call's frames)
        data, off = shared.fetch_frames()
        assert list(off) == solo[a].off and data == solo[a].data, "%s after %s" % (a, refuse.__name__)
    check_in_hand(world, shared, kind, solo[a], "%s after every refusal" % a)


def test_a_partition_order_the_reference_cannot_take_is_refused_by_every_entry(world):
    """max_partition_order 8: a block of 4096 would be cut into 256 partitions, which the reference cannot hold, so only
    batches of short frames pass (1000 = 8 * 125: order 3; 192: order 6).  Every entry refuses the whole blocks before it
    touches the context: the short batch in hand stays fetchable."""
    from test_gpu_packed import le_bytes

    from flac_codec_amd.gpu import GpuError

    an = analyzer(max_po=8)
    ref = analyzer(max_po=8)
    short = [(world.ptr + 4, 1000, 3), (world.ptr + 4 + 8 * 1000, 192, 4)]
    try:
        for name, run in (("host", lambda x: x.encode_frames(world.pcm[:1000 * CH], 1, 1000, 7, RATE)),
                          ("ragged", lambda x: (x.encode_ragged_device(short, RATE), fetched(world, x))[1])):
            want = run(ref)
            run(an)
            for refuse in (lambda: an.encode_frames(world.pcm[:2 * FRAME], 2, B, 0, RATE),
                           lambda: an.encode_device(world.ptr, 2, B, 0, RATE),
                           lambda: an.analyze_device(world.ptr, 2, B),
                           lambda: an.encode_segments(host_segments(world), RATE),
                           lambda: an.encode_segments_device([(world.ptr, 2, 0)], RATE),
                           lambda: an.encode_ragged_device(short + [(world.ptr + 4, B, 5)], RATE),
                           lambda: an.encode_packed(le_bytes(world.pcm[:2 * FRAME], 2), 2, 2, B, 0, RATE),
                           lambda: an.encode_segments_packed(le_bytes(world.pcm[:2 * FRAME], 2), 2, [(2, 0)], RATE)):
                with pytest.raises(GpuError) as e:
                    refuse()
                assert e.value.code == -2 and "partition order" in str(e.value), name
                an.last_frames = len(want[1]) - 1
                got = an.fetch_frames()
                assert got[0] == want[0] and list(got[1]) == list(want[1]), name
    finally:
        an.close()
        ref.close()
