"""flacgpu_session_host_open_container -- the container-session rule (DESIGN.md 4b "Container sessions": regular .flac
streams fed chunk by chunk) as plain host code, the device session's counterpart -- on the CPU, against the rule as a
Python model (_container_session_model.py) feed by feed, and against the one-shot scan of the concatenation
(flacgpu_scan_stream_host): the frames, their count, the samples, lost synchronisation and the refusal must not depend
on where the chunks were cut."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import _container_session_model as cm
import _flacsyn as fs
import _meta_cases as mc
import _raw_frames as rf
import _scan_model as scm

ERR_INVALID_ARG = -1
W = 4096


class HostContainer:
    def __init__(self, n_streams, w):
        from flac_codec_amd import _lib

        self.L, self._lib, self.n = _lib.lib(), _lib, n_streams
        self.h = C.c_void_p()
        assert self.L.flacgpu_session_host_open_container(n_streams, w, C.byref(self.h)) == 0

    def _call(self, fn, args, finish):
        from flac_codec_amd.gpu import FRAME_DTYPE

        total = C.c_uint64(0xDEAD)
        raw = (self._lib.RawStream * self.n)()
        held = (C.c_uint64 * self.n)()
        frames = np.zeros(64, dtype=FRAME_DTYPE)
        rest = (raw, C.byref(total)) if finish else (raw, held, C.byref(total))
        rc = fn(*args, frames.ctypes.data_as(C.POINTER(self._lib.FrameRecord)), frames.size, *rest)
        assert rc == 0 and total.value <= frames.size
        return (list(frames[:total.value]), [(r.frames, r.skipped_bytes, r.gaps, r.uniform) for r in raw],
                [r.first_frame for r in raw], list(held))

    def feed(self, chunks):
        keep = [bytes(c) for c in chunks]
        data = (C.c_void_p * self.n)(*[C.cast(C.c_char_p(c), C.c_void_p) if c else None for c in keep])
        lens = (C.c_size_t * self.n)(*[len(c) for c in keep])
        return self._call(self.L.flacgpu_session_host_feed, (self.h, data, lens, None), False)

    def finish(self):
        return self._call(self.L.flacgpu_session_host_finish, (self.h,), True)

    def close(self):
        self.L.flacgpu_session_host_close(self.h)


def _frames(shape, count, seed, blocking=0, defer=False):
    """fs.Frame objects of one shape (rate, bits, channels, n), every subframe FIXED order 2: short frames."""
    rate, bits, channels, n = shape
    rng = random.Random(seed)
    out, samples = [], 0
    for k in range(count):
        chans = rf._channels(rng, bits, channels, n, amp=200)
        subs = rf._subs(chans, bits, channels - 1, ["fixed"] * channels)
        out.append(fs.Frame(chans, subs, rcode=0 if defer else fs.RATE_CODES[rate], bps_code=0 if defer else None,
                            blocking=blocking, number=samples if blocking else k))
        samples += n
    return out


@functools.lru_cache(maxsize=None)
def the_file(blocking=0, defer=False):
    """About 12 frames of block 192, stereo, 16 bits, behind STREAMINFO, a SEEKTABLE-sized block and PADDING."""
    return fs.write_stream(44100, 16, _frames((44100, 16, 2, 192), 12, 20261103, blocking, defer),
                           metadata=[(3, bytes(36)), (1, bytes(21))])


def one_shot(blob):
    """flacgpu_scan_stream_host: (rc, frame starts, block sizes, bad_frames, decoded_samples)."""
    from flac_codec_amd import gpu

    try:
        info, off, sizes = gpu.scan_stream_host(blob)
    except gpu.GpuError as e:
        return e.args[0] if isinstance(e.args[0], int) else ERR_INVALID_ARG, [], [], 0, 0
    return 0, [int(v) for v in off], [int(v) for v in sizes], info.bad_frames, info.decoded_samples


def _agrees(blob, cuts, w, label, want=None, model=True):
    """One stream through the host session feed by feed: against the model's feeds, and the sum against the one-shot
    scan of the concatenation.  Returns the session's last summary."""
    want = one_shot(blob) if want is None else want
    feeds, m = cm.online(blob, cuts, w) if model else (None, None)
    s = HostContainer(1, w)
    got, at, frames_so_far = [], 0, 0
    steps = [blob[a:b] for a, b in zip([0] + list(cuts), cuts)] + [None]
    for k, chunk in enumerate(steps):
        recs, raw, first, held = s.finish() if chunk is None else s.feed([chunk])
        assert first == [0] and raw[0][0] == frames_so_far + len(recs), (label, k)
        assert held == [0] if chunk is None else held[0] <= w + 15, (label, k)
        if model:
            assert cm.tuples(recs) == cm.tuples(feeds[k]), (label, k)
        out = 0
        for r in recs:   # a feed lays its frames out one after another
            assert (int(r["out_offset"]), int(r["stream"]), int(r["status"])) == (out, 0, 0), (label, k)
            out += int(r["block_size"]) * int(r["channels"])
        got += recs
        frames_so_far += len(recs)
        at += len(chunk or b"")
    s.close()
    rc, starts, sizes, bad, samples = want
    frames, skipped, gaps, uniform = raw[0]
    if model:
        assert raw[0] == m.summary(), label
    if rc:
        assert (got, frames, skipped, gaps, uniform) == ([], 0, len(blob), int(len(blob) > 0), 0), label
        return raw[0]
    assert uniform == 1 and [int(r["byte_offset"]) for r in got] == starts, label
    assert [int(r["block_size"]) for r in got] == sizes and frames == len(starts), label
    assert int(uniform and gaps) == bad, label
    end = (int(got[-1]["byte_offset"]) + int(got[-1]["bytes"])) if got else scm.metadata(blob)[0]
    assert skipped == (len(blob) - end if bad else 0), label
    return raw[0]


def test_every_single_cut():
    st = the_file()
    assert 10 <= st.n_frames <= 14 and cm.links_within(st.blob, W)
    want = one_shot(st.blob)
    assert want[0] == 0 and len(want[1]) == st.n_frames and want[3] == 0
    assert cm.tuples(cm.oneshot(st.blob)[1]) == cm.tuples([r for f in cm.online(st.blob, [len(st.blob)], W)[0] for r in f])
    for cut in range(0, len(st.blob) + 1):
        _agrees(st.blob, [cut, len(st.blob)], W, f"cut at {cut}", want)


def test_seeded_multi_cuts_with_one_byte_chunks_and_idle_feeds():
    rng = random.Random(20261104)
    st = the_file()
    want = one_shot(st.blob)
    for k in range(200):
        cuts = cm.multi_cut(rng, len(st.blob), lo=1, hi=400 if k % 4 else 30)
        _agrees(st.blob, cuts, W, f"case {k}", want)


@pytest.mark.parametrize("which", ["deferred", "blocking 1"])
def test_headers_that_defer_to_streaminfo_and_sample_numbers(which):
    st = the_file(defer=True) if which == "deferred" else the_file(blocking=1)
    rng = random.Random(7)
    for k in range(25):
        _agrees(st.blob, cm.multi_cut(rng, len(st.blob)), W, f"{which}: case {k}")
    feeds, _ = cm.online(st.blob, [len(st.blob)], W)
    recs = [r for f in feeds for r in f]
    assert {(r["sample_rate"], r["bits_per_sample"], r["blocking"]) for r in recs} == {(44100, 16, int(which != "deferred"))}
    if which != "deferred":
        assert [r["number"] for r in recs] == [192 * k for k in range(st.n_frames)]


def _lookalike(min_frame):
    """A frame whose 12th byte begins a header that parses, has the frame's blocking bit and the CRC-16 of the bytes so
    far in front of it: it ends the frame only when STREAMINFO's min_frame does not forbid it."""
    inner = cm.crcd(scm.header(number=0) + bytes(4))
    first = cm.crcd(inner + scm.header(number=1) + bytes(range(30)))
    rest = b"".join(cm.crcd(scm.header(number=k) + bytes(range(k, k + 40))) for k in (2, 3))
    si = mc.streaminfo(min_block=192, max_block=192, min_frame=min_frame, channels=1, bits=16)
    return mc.chain([(0, si)]) + first + rest, len(inner), len(first)


def test_a_lookalike_header_inside_min_frame_does_not_end_a_frame():
    rng = random.Random(11)
    for min_frame, n_frames in ((40, 3), (0, 4)):
        blob, inner, first = _lookalike(min_frame)
        want = one_shot(blob)
        assert len(want[1]) == n_frames and want[1][1] - want[1][0] == (first if min_frame else inner)
        for cut in range(len(blob) + 1):
            _agrees(blob, [cut, len(blob)], W, f"min_frame {min_frame}, cut {cut}", want)
        for k in range(20):
            _agrees(blob, cm.multi_cut(rng, len(blob), hi=40), W, f"min_frame {min_frame}, case {k}", want)


def test_an_end_exactly_W_away_is_kept_and_one_W_plus_1_away_loses_the_stream():
    st = the_file()
    sizes = [len(c) for c in st.frame_bytes]
    longest = max(sizes)
    k = sizes.index(longest)
    assert 0 < k and longest >= 16
    rng = random.Random(13)
    for w, frames in ((longest, st.n_frames), (longest - 1, k)):
        rc, recs, bad, samples, _ = cm.oneshot(st.blob, w)
        assert (rc, len(recs), bad) == (0, frames, int(frames < st.n_frames))
        want = (0, [r["byte_offset"] for r in recs], [r["block_size"] for r in recs], bad, samples)
        for case in range(12):
            _agrees(st.blob, cm.multi_cut(rng, len(st.blob)), w, f"W = {w}, case {case}", want)


def test_damage_a_wrong_first_position_and_an_empty_region():
    st = the_file()
    meta = len(st.blob) - sum(len(c) for c in st.frame_bytes)
    at = meta + sum(len(c) for c in st.frame_bytes[:5]) + 20   # a body byte of frame 5
    damaged = st.blob[:at] + bytes([st.blob[at] ^ 0x5A]) + st.blob[at + 1:]
    rng = random.Random(17)
    for label, blob, frames, bad in (("a damaged frame in the middle", damaged, 5, 1),
                                     ("a first position that is no candidate", st.blob[:meta] + b"\x00" + st.blob[meta:], 0, 1),
                                     ("a frame region of length 0", st.blob[:meta], 0, 0),
                                     ("the last frame cut short", st.blob[:-3], st.n_frames - 1, 1)):
        want = one_shot(blob)
        assert (want[0], len(want[1]), want[3]) == (0, frames, bad), label
        for case in range(12):
            summary = _agrees(blob, cm.multi_cut(rng, len(blob)), W, f"{label}, case {case}", want)
        assert summary[0] == frames and summary[2] == bad


def test_refused_streams_next_to_a_healthy_one_and_the_layout_of_a_feed():
    st = the_file()
    wrong = b"fLaX" + st.blob[4:]
    unusable = mc.chain([(0, mc.streaminfo(min_block=0, max_block=0))]) + st.blob[-200:]
    s = HostContainer(3, W)
    models = [cm.Online(W) for _ in range(3)]
    blobs, at, got = [wrong, st.blob, unusable], [0, 0, 0], []
    rng = random.Random(19)
    while any(a < len(b) for a, b in zip(at, blobs)):
        step = [rng.choice((0, 1, 333, 700)) for _ in range(3)]
        chunks = [b[a:a + n] for b, a, n in zip(blobs, at, step)]
        at = [a + len(c) for a, c in zip(at, chunks)]
        recs, raw, first, held = s.feed(chunks)
        want = [m.feed(c) for m, c in zip(models, chunks)]
        assert want[0] == want[2] == [] and cm.tuples(recs) == cm.tuples(want[1]) and {int(r["stream"]) for r in recs} <= {1}
        assert raw == [m.summary() for m in models] and held[0] == held[2] == 0
        got += recs
    recs, raw, _, _ = s.finish()
    got += recs
    assert cm.tuples(got) == cm.tuples(cm.oneshot(st.blob)[1])
    assert raw[0] == (0, len(wrong), 1, 0) and raw[2] == (0, len(unusable), 1, 0) and raw[1] == (st.n_frames, 0, 0, 1)
    s.close()


def test_refusals():
    from flac_codec_amd import _lib

    L = _lib.lib()
    h = C.c_void_p()
    for w in (0, 15, (1 << 22) + 1):
        assert L.flacgpu_session_host_open_container(1, w, C.byref(h)) == ERR_INVALID_ARG and not h.value
    st = the_file()
    s = HostContainer(1, W)
    s.feed([st.blob[:100]])
    chunk = st.blob[100:900]
    data, lens, total = (C.c_void_p * 1)(C.cast(C.c_char_p(chunk), C.c_void_p)), (C.c_size_t * 1)(len(chunk)), C.c_uint64(0)
    recs = (_lib.FrameRecord * 16)()
    # a container's sender knows no frame boundary: a non-zero flush is refused and nothing changes
    assert L.flacgpu_session_host_feed(s.h, data, lens, (C.c_uint8 * 1)(1), recs, 16, None, None, C.byref(total)) == ERR_INVALID_ARG
    got, _, _, _ = s.feed([chunk])
    rest, _, _, _ = s.feed([st.blob[900:]])
    last, raw, _, _ = s.finish()
    assert cm.tuples(got + rest + last) == cm.tuples(cm.oneshot(st.blob)[1]) and raw[0] == (st.n_frames, 0, 0, 1)
    assert L.flacgpu_session_host_feed(s.h, data, lens, None, recs, 16, None, None, C.byref(total)) == ERR_INVALID_ARG
    s.close()
