"""flacgpu_session_host_* -- the decoder-session rule (DESIGN.md 4b "Decoder sessions") as plain host code, the device
session's counterpart -- against the rule as a Python model (_session_model.py), on the CPU: every record field, every
summary field, the held bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import _raw_frames as rf
import _session_model as sm

ERR_INVALID_ARG, ERR_BUFFER_TOO_SMALL = -1, -5   # include/flacenc_gpu.h
NEW_SYMBOLS = ("flacgpu_decoder_session_open", "flacgpu_decoder_session_feed", "flacgpu_decoder_session_feed_device",
               "flacgpu_decoder_session_finish", "flacgpu_decoder_session_pending",
               "flacgpu_decoder_session_last_feed_timing", "flacgpu_decoder_session_decoder",
               "flacgpu_decoder_session_close", "flacgpu_session_host_open", "flacgpu_session_host_feed",
               "flacgpu_session_host_finish", "flacgpu_session_host_close", "flacgpu_session_slots_host")
W = 1024   # holds every frame of the two streams (the model confirms it: raw_links_within)


class HostSession:
    def __init__(self, n_streams, w):
        from flac_codec_amd import _lib

        self.L, self._lib, self.n = _lib.lib(), _lib, n_streams
        self.h = C.c_void_p()
        assert self.L.flacgpu_session_host_open(n_streams, w, C.byref(self.h)) == 0

    def _call(self, fn, args, cap):
        from flac_codec_amd.gpu import FRAME_DTYPE

        total = C.c_uint64(0xDEAD)
        raw = (self._lib.RawStream * self.n)()
        held = (C.c_uint64 * self.n)()
        rest = (raw, C.byref(total)) if fn is self.L.flacgpu_session_host_finish else (raw, held, C.byref(total))
        if cap is None:   # the count first: a short buffer leaves the session as it was
            rc = fn(*args, None, 0, *rest)
            assert rc == (ERR_BUFFER_TOO_SMALL if total.value else 0)
            cap = total.value
        frames = np.full(cap + 1, 0xEE, dtype=np.uint8).repeat(64).view(FRAME_DTYPE)
        if cap:   # (a feed without a record was taken by the query)
            rc = fn(*args, frames.ctypes.data_as(C.POINTER(self._lib.FrameRecord)), cap, *rest)
        assert rc == 0 and (frames[cap:].view(np.uint8) == 0xEE).all()
        return ([rf.record_tuple(f) for f in frames[:total.value]],
                [(r.frames, r.skipped_bytes, r.gaps, r.uniform, r.first_frame) for r in raw], list(held))

    def feed(self, chunks, flush=None, cap=None):
        keep = [bytes(c) for c in chunks]
        data = (C.c_void_p * self.n)(*[C.cast(C.c_char_p(c), C.c_void_p) if c else None for c in keep])
        lens = (C.c_size_t * self.n)(*[len(c) for c in keep])
        fl = None if flush is None else (C.c_uint8 * self.n)(*[int(bool(f)) for f in flush])
        return self._call(self.L.flacgpu_session_host_feed, (self.h, data, lens, fl), cap)

    def finish(self):
        return self._call(self.L.flacgpu_session_host_finish, (self.h,), None)

    def close(self):
        self.L.flacgpu_session_host_close(self.h)


def _agrees(blob, cuts, flushes, w, label):
    """One stream through the host session, feed by feed against the model's feeds."""
    want_feeds, want_summary, _ = sm.online(blob, cuts, flushes, w)
    model = sm.Online(w)
    s = HostSession(1, w)
    at = 0
    for k, c in enumerate(cuts):
        recs, raw, held = s.feed([blob[at:c]], [c in flushes])
        model.feed(blob[at:c], c in flushes)
        want = sm.with_out_offsets(want_feeds[k])
        assert recs == sm.tuples(want), (label, k)
        uniform = int(len({(r["sample_rate"], r["channels"], r["bits_per_sample"]) for r in want}) == 1)
        assert raw == [model.summary() + (uniform, 0)], (label, k)
        assert held == [len(model.tail)], (label, k)
        at = c
    recs, raw, _ = s.finish()
    assert recs == sm.tuples(sm.with_out_offsets(want_feeds[-1])), label
    assert raw[0][:3] == want_summary == sm.segments(blob, flushes, w)[1], label
    s.close()


def test_every_new_symbol_is_exported():
    from flac_codec_amd import _lib

    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols(), name


@pytest.mark.parametrize("which", ["uniform", "mixed"])
def test_every_single_cut(which):
    st = rf.uniform() if which == "uniform" else rf.mixed()
    for cut in range(1, len(st.blob)):
        _agrees(st.blob, [cut, len(st.blob)], set(), W, f"{which}: cut at {cut}")


def test_seeded_multi_cuts_with_flushes():
    rng = random.Random(20261023)
    for k in range(200):
        st = rf.mixed() if k & 1 else rf.uniform()
        cuts, flushes = sm.multi_cut(rng, st)
        _agrees(st.blob, cuts, flushes, W, f"case {k}")


def test_the_W_clause_and_the_lookalike():
    st = rf.uniform()
    longest = max(len(c) for c in st.frame_bytes)
    rng = random.Random(5)
    for w in (longest, longest - 1):
        for k in range(10):
            cuts, flushes = sm.multi_cut(rng, st, flush_rate=0)
            _agrees(st.blob, cuts, flushes, w, f"W = {w}, case {k}")
    blob, _ = sm.lookalike_stream()
    for step in (1, 7, 64, 333):
        _agrees(blob, list(range(step, len(blob), step)) + [len(blob)], set(), W, f"look-alike, step {step}")


def test_every_input_of_the_raw_scan_cut_at_three_places():
    rng = random.Random(20261024)
    for label, blob in rf.all_cases():
        n = len(blob)
        cuts = sorted({rng.randint(1, n - 1) for _ in range(3)}) + [n] if n > 1 else [n] if n else []
        flushes = {cuts[1]} if len(cuts) > 2 and rng.random() < 0.3 else set()
        _agrees(blob, cuts, flushes, 1024, label)


def test_several_streams_idle_streams_and_layout_of_a_feed():
    a, b = rf.uniform(), rf.mixed()
    s = HostSession(3, W)
    ma, mb = sm.Online(W, 0), sm.Online(W, 2)
    recs, raw, held = s.feed([a.blob[:400], b"", b.blob[:900]])
    want = sm.with_out_offsets(ma.feed(a.blob[:400]) + mb.feed(b.blob[:900]))
    assert recs == sm.tuples(want) and held == [len(ma.tail), 0, len(mb.tail)]
    assert [r[4] for r in raw] == [0, ma.frames, ma.frames] and raw[1][:4] == (0, 0, 0, 0)
    recs, raw, held = s.feed([b"", b"", b.blob[900:]], [0, 1, 1])   # stream 0 idle, 1 flushed with nothing
    assert recs == sm.tuples(sm.with_out_offsets(mb.feed(b.blob[900:], True))) and held == [len(ma.tail), 0, 0]
    recs, raw, _ = s.finish()
    assert recs == sm.tuples(sm.with_out_offsets(ma.feed(b"", True)))   # the rest of stream 0 never came
    assert raw[0][:3] == ma.summary() and raw[2][:3] == mb.summary() == sm.segments(b.blob, (), W)[1]
    s.close()


def test_refusals_and_a_short_record_buffer():
    from flac_codec_amd import _lib

    L = _lib.lib()
    h = C.c_void_p()
    for w in (0, 15, (1 << 22) + 1):
        assert L.flacgpu_session_host_open(1, w, C.byref(h)) == ERR_INVALID_ARG and not h.value
    for w in (16, 1 << 22):
        assert L.flacgpu_session_host_open(1, w, C.byref(h)) == 0
        L.flacgpu_session_host_close(h)
    st = rf.uniform()
    s, model = HostSession(1, W), sm.Online(W)
    want = model.feed(st.blob[:1000])
    assert len(want) >= 2
    # a buffer one record short: refused, the count reported, and the same feed again gives what it would have given
    total, data = C.c_uint64(0), (C.c_void_p * 1)(C.cast(C.c_char_p(st.blob[:1000]), C.c_void_p))
    one = (_lib.FrameRecord * len(want))()
    rc = L.flacgpu_session_host_feed(s.h, data, (C.c_size_t * 1)(1000), None, one, len(want) - 1, None, None, C.byref(total))
    assert rc == ERR_BUFFER_TOO_SMALL and total.value == len(want) and bytes(one) == bytes(C.sizeof(one))
    recs, _, held = s.feed([st.blob[:1000]])
    assert recs == sm.tuples(sm.with_out_offsets(want)) and held == [len(model.tail)]
    s.finish()
    assert L.flacgpu_session_host_feed(s.h, data, (C.c_size_t * 1)(1000), None, one, len(want), None, None,
                                       C.byref(total)) == ERR_INVALID_ARG   # after finish
    s.close()
