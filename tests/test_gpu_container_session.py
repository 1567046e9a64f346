"""Container sessions on the GPU (flacgpu_decoder_session_open_container, _verdict; k_link_container, k_meta_feed,
the MD5 chains fed from decoded output): regular .flac files fed chunk by chunk, cut anywhere.  Every expected value
comes from the one-shot calls on the whole files (gpu.decode_many, Decoder.scan + decode_windows) or from hashlib, never
from a session.  All comparisons are exact.  Every input is well-formed memory of known size."""
import ctypes as C
import functools
import hashlib
import random

import numpy as np
import pytest

import _flacsyn as fs
from _pcm import le_bytes, synth_fast

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
DEV = "cuda:0"
INFO_FIELDS = ["sample_rate", "channels", "bits_per_sample", "min_block", "max_block", "frames", "bad_frames",
               "bad_crc16", "total_samples", "decoded_samples", "md5", "decoded_md5", "md5_status"]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch

    torch.cuda.init()   # torch's HIP runtime first, as in decode_many


def _encode(pcm, ch, bps, block, rate=48000):
    from flac_codec_amd.encode import FlacSampleWriter, Options

    w = FlacSampleWriter(None, Options.default().block_size(block), rate, bps, ch, pcm.size)
    w.write(pcm)
    w.finalize()
    data = w.getvalue()
    w.close()
    return data


def _metadata_end(blob):
    pos = 4
    while True:
        last, blen = blob[pos] & 0x80, int.from_bytes(blob[pos + 1:pos + 4], "big")
        pos += 4 + blen
        if last:
            return pos


def _with_chain(blob, blocks):
    """`blob` with the blocks [(type, payload)] behind its STREAMINFO, in place of whatever followed it."""
    end = _metadata_end(blob)
    si = bytes([blob[4] & 0x7F]) + blob[5:8 + 34]
    if not blocks:
        return b"fLaC" + bytes([si[0] | 0x80]) + si[1:] + blob[end:]
    tail = b"".join(fs.metadata_block(k, p, i + 1 == len(blocks)) for i, (k, p) in enumerate(blocks))
    return b"fLaC" + si + tail + blob[end:]


@functools.lru_cache(maxsize=1)
def sixteen():
    """16 files of differing shapes: channels 1..3; 8, 16 and 24 bits; blocks 192..1152; 6..20 frames; metadata chains of
    different lengths."""
    rng = random.Random(20261105)
    out = []
    for k in range(16):
        ch, bps, block = 1 + k % 3, (8, 16, 24)[(k // 3) % 3], (192, 576, 1152, 256, 333)[k % 5]
        frames = 6 + (k * 7) % 15
        n = block * (frames - 1) + rng.randint(1, block)
        blob = _encode(synth_fast(900 + k, ch, bps, n), ch, bps, block, rate=(16000, 44100, 48000)[k % 3])
        chain = [[], [(1, bytes(5))], [(4, b"v" * 40), (3, bytes(18 * 4)), (1, bytes(300))], [(2, b"appl" + bytes(2000))]][k % 4]
        out.append(_with_chain(blob, chain))
    return tuple(out)


def _cuts(rng, blob, pieces):
    """Ascending chunk ends: `pieces` chunks, cuts inside the marker and inside STREAMINFO and 1-byte chunks among them."""
    n = len(blob)
    cuts = {rng.randint(1, 3), rng.randint(9, 41)}
    c = rng.randint(50, n - 3)
    cuts |= {c, c + 1}
    while len(cuts) < pieces - 1:
        cuts.add(rng.randint(1, n - 1))
    return sorted(cuts)[:pieces - 1] + [n]


def _plan(rng, blobs, feeds):
    """Per stream {feed index: chunk}: every stream cut at its own places, idle in the feeds between."""
    plan = []
    for blob in blobs:
        edges = [0] + _cuts(rng, blob, rng.randint(4, min(30, feeds)))
        when = sorted(rng.sample(range(feeds), len(edges) - 1))
        plan.append({f: blob[a:b] for f, a, b in zip(when, edges, edges[1:])})
    return plan


def _bound(blobs):
    """A max_frame_bytes no smaller than any frame the one-shot scan links."""
    from flac_codec_amd.gpu import scan_stream_host

    w = 16
    for b in blobs:
        info, off, _ = scan_stream_host(b)
        ends = [int(v) for v in off[1:]] + [len(b)]
        w = max([w] + [e - int(s) for s, e in zip(off, ends)])
    return w


def _val(info, f):
    v = getattr(info, f)
    return bytes(v) if f in ("md5", "decoded_md5") else v


def _same_record(got, ref, label):
    assert got.rc == ref.rc, label
    diff = {f: (_val(got.info, f), _val(ref.info, f)) for f in INFO_FIELDS if _val(got.info, f) != _val(ref.info, f)}
    assert not diff, (label, diff)


def _at_residues(chunks, residues):
    """The chunks in ONE device tensor, chunk i at an address that is residues[i] modulo 16: the views (None: no bytes)."""
    import torch

    host, index = bytearray(), []
    for b, r in zip(chunks, residues):
        host += bytes((r - len(host)) % 16 + 16)
        index.append((len(host), len(b or b"")))
        host += b or b""
    shard = torch.from_numpy(np.frombuffer(bytes(host) or b"\0", dtype=np.uint8).copy()).to(DEV)
    assert shard.data_ptr() % 16 == 0
    return [shard[o:o + n] if n else None for o, n in index]


def _run(blobs, plan, feeds, W, door="host", decode=None, check_slots=None):
    """The session over `plan`; after every feed `decode(ses, f)` (default: decode with MD5 into device memory) gives
    (flat, streams).  Returns (per-stream samples concatenated, verdict, the session's last raw summaries)."""
    from flac_codec_amd.gpu import DecoderSession

    n = len(blobs)
    ses = DecoderSession(n, W, device=0, container=True)
    got = [[] for _ in range(n)]
    slots = []
    for f in range(feeds + 1):
        if f == feeds:
            _, raw = ses.finish()
        else:
            chunks = [plan[i].get(f) for i in range(n)]
            if door == "device":
                chunks = _at_residues(chunks, [(i + f) % 16 for i in range(n)])
            _, raw = ses.feed(chunks)
        if check_slots is not None:
            slots.append(ses.decoder.slot_bytes())
        assert max(ses.pending()[0]) <= W + 15
        out = (decode or (lambda s, k: s.decode(out="device")))(ses, f)
        if out is None:
            continue
        flat, streams = out
        for i, s in enumerate(streams):
            if s.rc == 0:
                assert s.info.md5_status == 3 and bytes(s.info.decoded_md5) == bytes(16) and s.info.frames > 0
                got[i].append(np.asarray(s.pcm.cpu() if hasattr(s.pcm, "cpu") else s.pcm).reshape(-1).copy())
            else:
                assert s.rc == INVALID_ARG and s.info.frames == 0
    assert ses.pending() == ([0] * n, sum(len(b) for b in blobs))
    verdict = ses.verdict()
    ses.close()
    if check_slots is not None:
        check_slots.append(slots)
    return [np.concatenate(g) if g else np.zeros(0, np.int32) for g in got], verdict, raw


@pytest.fixture(scope="module")
def reference():
    """decode_many of the 16 whole files, once."""
    from flac_codec_amd.gpu import decode_many

    blobs = sixteen()
    _, streams = decode_many(list(blobs), device=0, out="host")
    for s in streams:
        assert s.rc == 0 and s.info.md5_status == 1 and s.info.bad_frames == 0 and 6 <= s.info.frames <= 20
    assert {(s.info.bits_per_sample + 7) // 8 for s in streams} == {1, 2, 3} and {s.info.channels for s in streams} == {1, 2, 3}
    return blobs, streams, _bound(blobs)


# ---- 5. sixteen streams together, both doors
def test_sixteen_streams_cut_anywhere_through_both_doors(reference):
    blobs, ref, W = reference
    FEEDS = 32
    plan = _plan(random.Random(20261106), blobs, FEEDS)
    assert any(len(c) == 1 for p in plan for c in p.values()) and all(len(p) >= 4 for p in plan)
    slots = []
    for door in ("host", "device"):
        pcm, verdict, raw = _run(blobs, plan, FEEDS, W, door, check_slots=slots)
        for i, (s, v) in enumerate(zip(ref, verdict)):
            assert np.array_equal(pcm[i], np.asarray(s.pcm).reshape(-1)), (door, i)
            _same_record(v, s, (door, i))
            assert v.info.md5_status == 1 and v.out_offset == s.offset
            assert (raw[i].frames, raw[i].skipped_bytes, raw[i].gaps, raw[i].uniform) == (s.info.frames, 0, 0, 1)
    assert slots[0] == slots[1] and any(len(b) > 64 for b in slots[0])   # both doors build the same slots, feed by feed


# ---- 6. MD5 semantics
@functools.lru_cache(maxsize=1)
def four():
    out = []
    for k, (ch, bps, block) in enumerate(((1, 16, 192), (2, 24, 256), (2, 8, 333), (3, 16, 576))):
        pcm = synth_fast(950 + k, ch, bps, block * 5 + 17)
        out.append((_encode(pcm, ch, bps, block), hashlib.md5(le_bytes(pcm, bps)).digest()))
    return tuple(out)


def _set_md5(blob, md5):
    assert blob[4] & 0x7F == 0
    return blob[:26] + md5 + blob[42:]


def _four_plan(blobs, feeds=6):
    return _plan(random.Random(20261107), blobs, feeds), feeds


def test_md5_altered_zero_and_true():
    from flac_codec_amd.gpu import decode_many

    files = four()
    blobs = [_set_md5(files[0][0], bytes([files[0][1][0] ^ 1]) + files[0][1][1:]), _set_md5(files[1][0], bytes(16)),
             files[2][0], files[3][0]]
    plan, feeds = _four_plan(blobs)
    _, ref = decode_many(blobs, device=0, out="host")
    pcm, verdict, _ = _run(blobs, plan, feeds, _bound(blobs))
    assert [v.info.md5_status for v in verdict] == [0, 2, 1, 1]
    for i, (v, s) in enumerate(zip(verdict, ref)):
        _same_record(v, s, i)
        assert bytes(v.info.decoded_md5) == files[i][1]   # the true one, whatever STREAMINFO says
        assert np.array_equal(pcm[i], np.asarray(s.pcm).reshape(-1))


def test_a_feed_never_decoded_breaks_the_chains_it_had_frames_for():
    blobs = [f[0] for f in four()]
    plan, feeds = _four_plan(blobs)
    skipped_at, had = 3, []

    def decode(ses, f):
        if f == skipped_at:
            had.extend(i for i, r in enumerate(ses.records[:4]) if r.rc == 0)
            return None
        return ses.decode(out="device")

    _, verdict, _ = _run(blobs, plan, feeds, _bound(blobs), decode=decode)
    assert had and len(had) < 4, "the plan must give some streams, not all, a frame in the skipped feed"
    assert [v.info.md5_status for v in verdict] == [3 if i in had else 1 for i in range(4)]
    assert all(v.rc == 0 and v.info.frames == 6 for v in verdict)


def test_decoding_twice_hashes_once_and_no_md5_breaks_every_chain():
    from flac_codec_amd.gpu import decode_many

    blobs = [f[0] for f in four()]
    plan, feeds = _four_plan(blobs)
    _, ref = decode_many(blobs, device=0, out="host")

    def twice(ses, f):
        first = ses.decode(out="device")
        again = ses.decode(out="host")
        assert np.array_equal(first[0].cpu().numpy(), again[0])
        return again

    pcm, verdict, _ = _run(blobs, plan, feeds, _bound(blobs), decode=twice)
    for i, (v, s) in enumerate(zip(verdict, ref)):
        _same_record(v, s, i)
        assert v.info.md5_status == 1 and np.array_equal(pcm[i], np.asarray(s.pcm).reshape(-1))
    _, verdict, _ = _run(blobs, plan, feeds, _bound(blobs), decode=lambda ses, f: ses.decode(out="device", verify_md5=False))
    assert [v.info.md5_status for v in verdict] == [3] * 4 and all(bytes(v.info.decoded_md5) == bytes(16) for v in verdict)


def test_decode_as_float32_padded_feeds_the_chains_from_the_decoders_own_copy():
    from flac_codec_amd.gpu import decode_many

    blobs = [f[0] for f in four()]
    plan, feeds = _four_plan(blobs)
    batch, ref = decode_many(blobs, device=0, out="host", dtype="float32", layout="padded")
    got = [[] for _ in blobs]

    def as_float(ses, f):
        _, streams = ses.decode_as("float32", "padded", out="device", verify_md5=True)
        for i, s in enumerate(streams):
            if s.rc == 0:
                got[i].append(s.pcm.cpu().numpy().copy())
        return None

    _, verdict, _ = _run(blobs, plan, feeds, _bound(blobs), decode=as_float)
    for i, (v, s) in enumerate(zip(verdict, ref)):
        _same_record(v, s, i)
        assert v.info.md5_status == 1
        assert np.array_equal(np.concatenate(got[i], axis=1), s.pcm), i


# ---- 7. further cases
def test_lost_synchronisation_and_a_refused_stream_next_to_healthy_ones():
    from flac_codec_amd.gpu import decode_many, scan_stream_host

    files = [f[0] for f in four()]
    _, off, _ = scan_stream_host(files[1])
    at = int(off[3]) + 30   # a body byte of frame 3
    damaged = files[1][:at] + bytes([files[1][at] ^ 0xA5]) + files[1][at + 1:]
    blobs = [files[0], damaged, b"fLaX" + files[2][4:], files[3]]
    _, ref = decode_many(blobs, device=0, out="host")
    assert [s.rc for s in ref] == [0, 0, INVALID_ARG, 0] and (ref[1].info.frames, ref[1].info.bad_frames) == (3, 1)
    plan, feeds = _four_plan(blobs, 8)
    for door in ("host", "device"):
        pcm, verdict, raw = _run(blobs, plan, feeds, _bound(files), door)
        for i, (v, s) in enumerate(zip(verdict, ref)):
            _same_record(v, s, (door, i))
            if s.rc == 0:
                assert np.array_equal(pcm[i], np.asarray(s.pcm).reshape(-1)), (door, i)
        assert (raw[1].frames, raw[1].skipped_bytes, raw[1].gaps, raw[1].uniform) == (3, len(damaged) - int(off[3]), 1, 1)
        assert (raw[2].frames, raw[2].skipped_bytes, raw[2].gaps, raw[2].uniform) == (0, len(blobs[2]), 1, 0)
        assert [raw[i].skipped_bytes for i in (0, 3)] == [0, 0]


def test_a_40_kib_verbatim_frame_in_1_kib_pieces():
    from flac_codec_amd.gpu import decode_many

    rng = random.Random(3)
    n = 10000   # 2 channels x 16 bits x 10000 samples: 40 000 bytes of VERBATIM samples
    frames = [fs.Frame([[rng.randint(-32768, 32767) for _ in range(n)] for _ in range(2)], [fs.verbatim(), fs.verbatim()],
                       rcode=fs.RATE_CODES[44100], number=k) for k in range(2)]
    st = fs.write_stream(44100, 16, frames)
    assert max(len(c) for c in st.frame_bytes) > 40000
    blobs = [st.blob]
    _, ref = decode_many(blobs, device=0, out="host")
    edges = list(range(1024, len(st.blob), 1024)) + [len(st.blob)]
    plan = [{f: st.blob[a:b] for f, (a, b) in enumerate(zip([0] + edges, edges))}]
    pcm, verdict, _ = _run(blobs, plan, len(edges), _bound(blobs))
    _same_record(verdict[0], ref[0], "verbatim")
    assert verdict[0].info.md5_status == 1 and np.array_equal(pcm[0], st.pcm)


def test_a_70_000_byte_metadata_block_in_1_kib_pieces_is_never_held():
    """Through both doors: while a stream is in its metadata the session holds no byte of it (pending), however long
    the chain; the frames behind it come out as the one-shot decode gives them."""
    from flac_codec_amd.gpu import DecoderSession, decode_many

    blob = _with_chain(four()[0][0], [(2, b"appl" + bytes(range(256)) * 273 + bytes(108)), (1, bytes(9))])
    chain = _metadata_end(blob)
    assert chain > 70000
    _, ref = decode_many([blob], device=0, out="host")
    edges = list(range(1024, len(blob), 1024)) + [len(blob)]
    for door in ("host", "device"):
        ses = DecoderSession(1, _bound([blob]), device=0, container=True)
        got = []
        for a, b in zip([0] + edges, edges):
            chunk = [blob[a:b]]
            _, raw = ses.feed(_at_residues(chunk, [a // 1024 % 16]) if door == "device" else chunk)
            held, fed = ses.pending()
            assert fed == b and (held == [0] if b <= chain else held[0] <= b - chain) and raw[0].uniform == int(b >= chain)
            _, streams = ses.decode(out="host")
            got += [s.pcm.reshape(-1) for s in streams if s.rc == 0]
        ses.finish()
        got += [s.pcm.reshape(-1) for s in ses.decode(out="host")[1] if s.rc == 0]
        v = ses.verdict()[0]
        ses.close()
        _same_record(v, ref[0], door)
        assert v.info.md5_status == 1 and np.array_equal(np.concatenate(got), ref[0].pcm.reshape(-1))


def test_decode_windows_after_a_feed_is_decode_windows_after_scan_of_those_frames():
    from flac_codec_amd import gpu

    blob = four()[1][0]
    info, off, sizes = gpu.scan_stream_host(blob)
    cut = int(off[4]) + 40   # frames 0..3 are decided by the first feed (the header of frame 4 has arrived)
    ses = gpu.DecoderSession(1, _bound([blob]), device=0, container=True)
    ses.feed([blob[:cut]])
    assert ses.n_frames == 4
    part = blob[:int(off[4])]   # STREAMINFO plus those frames
    dec = gpu.Decoder(0)
    recs, _ = dec.scan([part])
    windows = [(0, 10, 300), (0, 0, 256 * 4), (0, 700, 5000)]
    want, want_res = gpu.decode_windows(dec, recs, windows, dtype="int32", out="host")
    got, got_res = gpu.decode_windows(ses.decoder, ses.records, windows, dtype="int32", out="host")
    assert [r.samples for r in want_res] == [300, 1024, 324]
    assert np.array_equal(np.asarray(got), np.asarray(want))
    assert [(r.rc, r.frames, r.samples, r.bad_frames, r.bad_crc16) for r in got_res] == \
        [(r.rc, r.frames, r.samples, r.bad_frames, r.bad_crc16) for r in want_res]
    dec.close()
    ses.close()


def test_refusals_leave_the_session_usable():
    from flac_codec_amd import _lib, gpu

    blob, digest = four()[0]
    L = _lib.lib()
    ses = gpu.DecoderSession(1, _bound([blob]), device=0, container=True)
    n = len(blob) // 2
    ses.feed([blob[:n]])
    first = ses.decode(out="host")[1][0]
    verdict = (_lib.DecodedStream * 1)()
    assert L.flacgpu_decoder_session_verdict(ses._h, verdict) == INVALID_ARG and bytes(verdict) == bytes(C.sizeof(verdict))
    with pytest.raises(gpu.GpuError):   # a container session takes no flush; nothing changes
        ses.feed([blob[n:]], flush=True)
    frames = np.zeros(8, dtype=gpu.FRAME_DTYPE)
    with pytest.raises(gpu.GpuError):   # a batch of regular streams has no frame records, as after scan
        ses.decoder.decode_frames(None, 0, 0, frames)
    assert L.flacgpu_decoder_frame_records(ses.decoder._h, None, 0) == INVALID_ARG
    ses.feed([blob[n:]])
    second = ses.decode(out="host")[1][0]
    ses.finish()
    last = ses.decode(out="host")[1][0]
    v = ses.verdict()[0]
    assert (v.rc, v.info.md5_status, bytes(v.info.decoded_md5)) == (0, 1, digest)
    assert sum(s.info.frames for s in (first, second, last) if s.rc == 0) == v.info.frames == 6
    assert L.flacgpu_decoder_session_verdict(ses._h, verdict) == INVALID_ARG and bytes(verdict) == bytes(C.sizeof(verdict))
    ses.close()
    raw = gpu.DecoderSession(1, 1024, device=0)
    assert L.flacgpu_decoder_session_verdict(raw._h, verdict) == INVALID_ARG   # a raw session has no verdict
    raw.close()


def test_file_chunk_reader_against_decode_many():
    from flac_codec_amd.decode import FlacFileChunkReader
    from flac_codec_amd.gpu import decode_many

    pcm = synth_fast(977, 2, 16, 4096 * 5 + 100)
    blob = _encode(pcm, 2, 16, 4096)
    _, ref = decode_many([blob], device=0, out="host")
    reader = FlacFileChunkReader(device=0)
    parts = [reader.feed(blob[a:a + 4096]) for a in range(0, len(blob), 4096)]
    parts.append(reader.finish())
    got = np.concatenate([p for p in parts if p.size])
    assert np.array_equal(got, ref[0].pcm) and reader.md5_ok is True and reader.rc == 0
    assert (reader.info.frames, reader.info.decoded_samples, reader.info.bad_frames) == (6, ref[0].info.decoded_samples, 0)
    reader.close()
