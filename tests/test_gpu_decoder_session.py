"""Decoder sessions on the GPU (flacgpu_decoder_session_*; kernels/session.inc): raw frame streams fed chunk by chunk.
Expected values come from the rule as a Python model (_session_model.py), from what the hand-built frames were written
from (RawStream.pcm) and from the one-shot calls that exist without sessions (gpu.decode_frames, gpu.decode_many,
Decoder.scan_frames), never from a session.  All comparisons are exact.  Every input is well-formed memory of known
size."""
import ctypes as C
import random

import numpy as np
import pytest

import _raw_frames as rf
import _session_model as sm

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch

    torch.cuda.init()   # torch's HIP runtime first, as in decode_many


@pytest.fixture(scope="module")
def pool():
    """The distinct streams the tests cut: (RawStream, ...), and per stream {byte_offset: samples} from ONE one-shot
    gpu.decode_frames call over all of them (existing code), checked against what the frames were written from."""
    from flac_codec_amd import gpu

    streams = (rf.mixed(), rf.uniform()) + tuple(raw for raw, _ in rf.uniform_set())
    flat, frames, raw = gpu.decode_frames([s.blob for s in streams], device=0, out="host")
    samples = [dict() for _ in streams]
    for f in frames:
        assert f["status"] == 0
        at, n = int(f["out_offset"]), int(f["block_size"]) * int(f["channels"])
        samples[f["stream"]][int(f["byte_offset"])] = flat[at:at + n]
    for st, got in zip(streams, samples):
        assert sorted(got) == st.at[:-1]
        for k, pos in enumerate(st.at[:-1]):
            assert np.array_equal(got[pos], np.asarray(st.pcm[k], dtype=np.int32).reshape(-1))
    return streams, samples


def _bound(streams):
    """A max_frame_bytes for which the model confirms that the raw rule links nothing further away."""
    w = max(max(len(c) for c in s.frame_bytes) for s in streams)
    assert all(sm.raw_links_within(s.blob, w) for s in streams)
    return w


def _put(blob):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8).copy()).to(DEV)[:len(blob)]


def _at_residues(chunks, residues):
    """The chunks in ONE device tensor, chunk i at an address that is residues[i] modulo 16, the last ending with the
    tensor: (the tensor, the views)."""
    import torch

    host, index = bytearray(), []
    for b, r in zip(chunks, residues):
        host += bytes((r - len(host)) % 16 + 16)
        index.append((len(host), len(b)))
        host += b
    shard = torch.from_numpy(np.frombuffer(bytes(host) or b"\0", dtype=np.uint8).copy()).to(DEV)
    assert shard.data_ptr() % 16 == 0
    return shard, [shard[o:o + n] for o, n in index]


def _slots(parts):
    """The slot buffer of a feed whose streams have these bytes (tail + chunk): 64-byte aligned slots, at least 64 zero
    bytes behind each, 64 bytes of look-ahead; a stream without a byte has no slot."""
    out = bytearray()
    for p in parts:
        if p:
            out += p + bytes(((len(p) + 64 + 63) & ~63) - len(p))
    return bytes(out) + (bytes(64) if out else b"")


def _tuples(frames):
    return [rf.record_tuple(f) for f in frames]


def _feed_expect(models, chunks, flush):
    """The model's records of one feed over all streams, laid out as a feed lays them out."""
    recs = []
    for m, c, f in zip(models, chunks, flush):
        recs += m.feed(c or b"", f)
    return sm.tuples(sm.with_out_offsets(recs))


# ---- 1. cut independence
def test_cut_independence_of_64_streams(pool):
    from flac_codec_amd.gpu import DecoderSession

    streams, samples = pool
    W = _bound(streams)
    rng = random.Random(20261025)
    N, FEEDS = 64, 48
    which = [i % len(streams) for i in range(N)]
    plan = []   # per stream: {feed index: chunk}
    for i in range(N):
        blob = streams[which[i]].blob
        k = rng.randint(8, 40)
        cuts = set(rng.sample(range(1, len(blob)), k - 1))
        for _ in range(3):   # some 1-byte chunks
            c = rng.randint(1, len(blob) - 2)
            cuts |= {c, c + 1}
        cuts = sorted(cuts)[:FEEDS - 1]
        edges = [0] + cuts + [len(blob)]
        feeds = sorted(rng.sample(range(FEEDS), len(edges) - 1))   # idle in the feeds between
        plan.append({f: blob[a:b] for f, a, b in zip(feeds, edges, edges[1:])})
    ses = DecoderSession(N, W, device=0)
    got = [[] for _ in range(N)]
    for f in range(FEEDS + 1):
        frames, raw = ses.finish() if f == FEEDS else ses.feed([plan[i].get(f) for i in range(N)])
        flat, decoded = ses.decode_frames(out="host")
        at = 0
        for r in decoded:
            i, n = int(r["stream"]), int(r["block_size"]) * int(r["channels"])
            assert r["status"] == 0 and r["out_offset"] == at
            assert np.array_equal(flat[at:at + n], samples[which[i]][int(r["byte_offset"])]), (f, i)
            got[i].append(dict(zip(rf.RECORD_FIELDS, rf.record_tuple(r)), out_offset=0))
            at += n
        held, _ = ses.pending()
        assert max(held) <= W + 15
    assert ses.pending() == ([0] * N, sum(len(streams[w].blob) for w in which))
    for i in range(N):
        want, summary = sm.segments(streams[which[i]].blob, (), W, stream=i)
        assert sm.tuples(got[i]) == sm.tuples(want), i
        assert (raw[i].frames, raw[i].skipped_bytes, raw[i].gaps) == summary == (len(want), 0, 0), i
    ses.close()


# ---- 2. both doors, and the junction at every pair of residues
def test_both_doors_build_the_same_slots(pool):
    from flac_codec_amd.gpu import DecoderSession

    streams, _ = pool
    W = _bound(streams)
    rng = random.Random(7)
    N = 16
    blobs = [streams[i % len(streams)].blob for i in range(N)]
    host, dev = DecoderSession(N, W, device=0), DecoderSession(N, W, device=0)
    models = [sm.Online(W, i) for i in range(N)]
    at = [0] * N
    for f in range(6):
        chunks = []
        for i in range(N):
            n = 0 if (i + f) % 5 == 0 else rng.randint(1, 700)   # some streams idle
            chunks.append(blobs[i][at[i]:at[i] + n])
            at[i] += len(chunks[-1])
        flush = [rng.random() < 0.2 for _ in range(N)]
        want_slots = _slots([m.tail + c for m, c in zip(models, chunks)])
        want = _feed_expect(models, chunks, flush)
        shard, views = _at_residues(chunks, [(i + f) % 16 for i in range(N)])
        a, _ = host.feed(chunks, flush)
        b, _ = dev.feed(views, flush)
        assert _tuples(a) == _tuples(b) == want, f
        assert host.decoder.slot_bytes() == dev.decoder.slot_bytes() == want_slots, f
        assert host.pending()[0] == dev.pending()[0] == [len(m.tail) for m in models]
    host.close()
    dev.close()


def test_junction_of_tail_and_chunk_at_every_pair_of_residues():
    """256 streams: the held tail's length at every residue x the chunk's source at every residue, the tail's source
    (where the first feed left it in the other buffer) cycling.  One feed leaves the tails, the next joins them."""
    from flac_codec_amd.gpu import DecoderSession

    st = rf.build([(44100, 16, 2, n) for n in (16, 33, 17)], 20261026)
    W = _bound([st])
    N = 256
    first, second = [], []
    for i in range(N):
        junk = bytes((i * 5) % 16 + 1)          # zeros in front: the tail starts at every residue of its slot
        take = 20 + i % 16                      # the held tail: the first bytes of frame 0, every residue of its length
        first.append(junk + st.blob[:take])
        second.append(st.blob[take:])
    models = [sm.Online(W, i) for i in range(N)]
    ses = DecoderSession(N, W, device=0)
    want = _feed_expect(models, first, [False] * N)
    frames, _ = ses.feed(first)
    assert _tuples(frames) == want == []
    tails = [m.tail for m in models]
    assert [len(t) % 16 for t in tails[:16]] == [(20 + r) % 16 for r in range(16)] and ses.pending()[0] == [len(t) for t in tails]
    shard, views = _at_residues(second, [i // 16 for i in range(N)])
    want = _feed_expect(models, second, [True] * N)
    frames, raw = ses.feed(views, flush=True)
    assert ses.decoder.slot_bytes() == _slots([t + c for t, c in zip(tails, second)])
    assert _tuples(frames) == want and len(want) == 3 * N
    assert all((r.frames, r.gaps) == (3, 1) for r in raw) and ses.pending()[0] == [0] * N
    ses.close()


# ---- 3. flush
def test_flush_gives_each_frame_in_its_own_feed_and_without_it_one_feed_later(pool):
    from flac_codec_amd.gpu import DecoderSession

    streams, samples = pool
    eight = streams[2:10]   # five frames each
    W = _bound(eight)
    for flush in (True, False):
        ses = DecoderSession(8, W, device=0)
        for k in range(5):
            frames, _ = ses.feed([s.frame_bytes[k] for s in eight], flush=flush)
            flat, decoded = ses.decode_frames(out="host")
            j = k if flush else k - 1   # without flush the header behind a frame must have arrived
            assert [int(v) for v in frames["byte_offset"]] == ([s.at[j] for s in eight] if j >= 0 else [])
            for i, r in enumerate(decoded):
                a, n = int(r["out_offset"]), int(r["block_size"]) * int(r["channels"])
                assert r["status"] == 0 and np.array_equal(flat[a:a + n], samples[2 + i][eight[i].at[j]])
            assert ses.pending()[0] == ([0] * 8 if flush else [len(s.frame_bytes[k]) for s in eight])
        frames, raw = ses.finish()
        assert [int(v) for v in frames["byte_offset"]] == ([] if flush else [s.at[4] for s in eight])
        assert all((r.frames, r.skipped_bytes, r.gaps) == (5, 0, 0) for r in raw)
        ses.close()


def test_a_flush_in_the_middle_of_a_frame_loses_that_frame(pool):
    from flac_codec_amd.gpu import DecoderSession

    streams, _ = pool
    st = streams[1]
    W = _bound([st])
    cut = st.at[2] + 40   # inside frame 2
    ses = DecoderSession(1, W, device=0)
    a, _ = ses.feed([st.blob[:cut]], flush=True)
    b, raw = ses.feed([st.blob[cut:]], flush=True)
    want, summary = sm.segments(st.blob, [cut], W)
    assert _tuples(a) + _tuples(b) == sm.tuples(sm.with_out_offsets(want[:2]) + sm.with_out_offsets(want[2:]))
    assert [r["byte_offset"] for r in want] == st.at[:2] + st.at[3:-1]
    assert (raw[0].frames, raw[0].skipped_bytes, raw[0].gaps) == summary == (len(st.frame_bytes) - 1, len(st.frame_bytes[2]), 1)
    ses.close()


# ---- 4. the W clause and the pass-over
def test_a_lookalike_is_held_until_W_lies_behind_it_and_then_passed_over():
    from flac_codec_amd.gpu import DecoderSession

    blob, true_at = sm.lookalike_stream()
    W = 1024
    assert sm.raw_links_within(blob, W)
    model, ses = sm.Online(W), DecoderSession(1, W, device=0)
    got, released = [], None
    for at in range(0, len(blob), 173):
        frames, raw = ses.feed([blob[at:at + 173]])
        assert _tuples(frames) == sm.tuples(sm.with_out_offsets(model.feed(blob[at:at + 173])))
        held = ses.pending()[0][0]
        assert held == len(model.tail) <= W + 15
        assert (raw[0].frames, raw[0].skipped_bytes, raw[0].gaps) == model.summary()
        if released is None and model.base > 0:
            released = at + 173
        got += _tuples(frames)
    frames, raw = ses.finish()
    got += _tuples(frames)
    assert W + 16 <= released < W + 16 + 173          # held while L - 16 < s + W, passed over in the feed that ends it
    assert [g[0] for g in got] == [true_at + a for a in rf.uniform().at[:-1]]
    assert (raw[0].frames, raw[0].skipped_bytes, raw[0].gaps) == (len(got), true_at, 1)
    ses.close()


# ---- 5. downstream calls
def test_decode_as_and_decode_timeline_after_a_feed(pool):
    from flac_codec_amd import _lib, gpu

    streams, _ = pool
    eight = [streams[2 + k] for k in (0, 1, 3, 4, 7, 9, 11, 1)]   # at most 16 bits per sample: int16 takes them all
    assert all(bits <= 16 for s in eight for _, bits, _, _ in s.shapes)
    W = _bound(eight)
    parts = [b"".join(s.frame_bytes[:3]) for s in eight]   # the frames this feed decides, as one-shot inputs
    ses = gpu.DecoderSession(8, W, device=0)
    ses.feed([s.frame_bytes[0][:9] for s in eight])
    frames, _ = ses.feed([p[9:] for p in parts], flush=True)
    one = gpu.Decoder(0)
    for kw in (dict(dtype="float32", layout="padded"), dict(dtype="int16", layout="flat")):
        want, ws = gpu.decode_many(parts, out="host", verify_md5=False, decoder=one, raw=True, **kw)
        got, gs = ses.decode_as(out="host", **kw)
        assert np.array_equal(got, want) and [(s.rc, s.offset) for s in gs] == [(s.rc, s.offset) for s in ws]
        assert any(s.rc == 0 for s in ws) and want.size
    _, _, _, records = one.scan_frames(parts)
    assert [t[1:] for t in _tuples(frames)] == [t[1:] for t in _tuples(records)]   # byte_offset apart: 9 bytes came before

    def timeline(dec):
        fmt = _lib.OutFormat(_lib.SAMPLE_F32, _lib.LAYOUT_PADDED, 8, 0, 4400)
        plan, need, mask_need = dec.plan_timeline(fmt)
        buf, m = np.zeros(need // 4, dtype=np.float32), np.zeros(mask_need, dtype=np.uint8)
        results, tl = dec.decode_timeline(buf.ctypes.data, need, m.ctypes.data, mask_need, fmt, 0)
        return bytes(plan), bytes(results), tl.tobytes(), buf.tobytes(), m.tobytes()

    assert timeline(ses.decoder) == timeline(one)
    one.close()
    ses.close()


def test_flac_chunk_reader_gives_the_stream_readers_frames(pool):
    from flac_codec_amd.decode import FlacChunkReader, FlacStreamReader

    streams, _ = pool
    st = streams[0]   # the mixed stream: rate, channels and sample size change from frame to frame
    want = list(FlacStreamReader(st.blob, device=0))
    assert len(want) == len(st.frame_bytes)
    reader = FlacChunkReader(device=0, max_frame_bytes=_bound([st]))
    got = []
    for at in range(0, len(st.blob), 211):
        got += reader.feed(st.blob[at:at + 211])
    assert reader.pending > 0 and len(got) == len(want) - 1   # the last frame waits for a header that never comes
    got += reader.finish()
    assert got == want and (reader.skipped_bytes, reader.gaps, reader.pending) == (0, 0, 0)
    reader.close()
    reader = FlacChunkReader(device=0, max_frame_bytes=_bound([st]))
    assert [reader.feed(c, flush=True) for c in st.frame_bytes] == [[f] for f in want]   # a frame per write
    assert reader.finish() == []
    reader.close()


def test_the_example_feeds_both_ways_and_reports_identical_pcm(capsys):
    import importlib.util
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("frames2pcm_stream", os.path.join(root, "examples", "frames2pcm_stream.py"))
    mod = importlib.util.module_from_spec(spec)
    before = list(sys.path)
    try:
        spec.loader.exec_module(mod)
        assert mod.main(["frames2pcm_stream.py", "4", "5"]) == 0
    finally:
        sys.path[:] = before
    assert "identical PCM" in capsys.readouterr().out


# ---- 6. refusals
def test_refusals_leave_the_session_as_it_was(pool):
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import DecoderSession, GpuError

    streams, _ = pool
    st = streams[1]
    W = _bound([st])
    L = _lib.lib()
    h = C.c_void_p()
    for w in (15, (1 << 22) + 1):
        assert L.flacgpu_decoder_session_open(0, 1, w, 0, C.byref(h)) == INVALID_ARG and not h.value
    assert L.flacgpu_decoder_session_open(0, 1, W, 1, C.byref(h)) == INVALID_ARG and not h.value   # no flag exists
    ses, model = DecoderSession(1, W, device=0), sm.Online(W)
    a, _ = ses.feed([st.blob[:500]])
    assert _tuples(a) == sm.tuples(sm.with_out_offsets(model.feed(st.blob[:500])))
    before = ses.pending()
    with pytest.raises(GpuError):   # a scan on the session's decoder
        ses.decoder.scan_frames([st.blob])
    with pytest.raises(GpuError):
        ses.decoder.scan([st.blob])
    # a host pointer through the device door
    keep = C.c_char_p(st.blob[500:900])
    ptrs, lens = (C.c_void_p * 1)(C.cast(keep, C.c_void_p).value), (C.c_size_t * 1)(400)
    recs, raw = (_lib.DecodedStream * 1)(), (_lib.RawStream * 1)()
    nf, ne, nt = C.c_uint64(77), C.c_uint64(77), C.c_uint64(77)
    rc = L.flacgpu_decoder_session_feed_device(ses._h, ptrs, lens, None, None, recs, raw, C.byref(nf), C.byref(ne), C.byref(nt))
    assert rc == INVALID_ARG and (nf.value, ne.value, nt.value) == (77, 77, 77) and bytes(recs) == bytes(C.sizeof(recs))
    assert ses.pending() == before
    # the session's decoder is as it was too: the last feed's frames still decode, and destroy does nothing for it
    L.flacgpu_decoder_destroy(ses.decoder._h)
    flat, decoded = ses.decode_frames(out="host")
    assert _tuples(decoded) == _tuples(a) and len(a) and flat.size == sum(int(r["block_size"]) * int(r["channels"]) for r in a)
    timing = ses.last_feed_timing()
    assert sorted(timing) == ["scan_rest", "stage", "table_upload", "to_first_sync", "to_second_sync", "walk"]
    assert all(v >= 0 for v in timing.values()) and timing["to_first_sync"] > 0
    b, _ = ses.feed([st.blob[500:]])   # the next feed gives what it would have given
    assert _tuples(b) == sm.tuples(sm.with_out_offsets(model.feed(st.blob[500:])))
    ses.finish()
    with pytest.raises(GpuError):
        ses.feed([b"x"])
    with pytest.raises(GpuError):
        ses.finish()
    ses.close()


# ---- 7. a held tail that crosses a workgroup
def test_a_40_KiB_verbatim_frame_fed_in_1_KiB_pieces():
    import _flacsyn as fs
    from flac_codec_amd.gpu import DecoderSession

    rng = random.Random(20261027)
    n = 4096
    chans = [[rng.randint(-30000, 30000) for _ in range(n)] for _ in range(5)]   # 5 x 4096 x 16 bits: 40 KiB
    big = fs.write_frame(48000, 16, fs.Frame(chans, [fs.verbatim()] * 5, assignment=4, rcode=fs.RATE_CODES[48000],
                                             blocking=0, number=1), set())
    st = rf.uniform()
    blob = st.frame_bytes[0] + big + st.frame_bytes[1]
    assert 40 * 1024 <= len(big) < 41 * 1024
    W = 48 * 1024
    assert sm.raw_links_within(blob, W)
    model, ses = sm.Online(W), DecoderSession(1, W, device=0)
    got = []
    for at in range(0, len(blob), 1024):
        frames, _ = ses.feed([blob[at:at + 1024]])
        assert _tuples(frames) == sm.tuples(sm.with_out_offsets(model.feed(blob[at:at + 1024])))
        assert ses.pending()[0] == [len(model.tail)]
        if len(frames) and frames[0]["bytes"] == len(big):
            flat, decoded = ses.decode_frames(out="host")
            assert decoded[0]["status"] == 0
            assert np.array_equal(flat[:n * 5].reshape(n, 5), np.asarray(chans, dtype=np.int32).T)
        got += _tuples(frames)
    got += _tuples(ses.finish()[0])
    assert [(g[0], g[4]) for g in got] == [(0, len(st.frame_bytes[0])), (len(st.frame_bytes[0]), len(big)),
                                           (len(st.frame_bytes[0]) + len(big), len(st.frame_bytes[1]))]
    ses.close()
