"""The STREAMINFO MD5 of many streams at frame sizes that are not whole MD5 blocks (tests/_md5_shapes.py): every stream of every
population through one writer per stream fed in irregular pieces (a), the batch encoder's engine pool (b) and the coalescing front
end's HASH tasks (c) -- bytes 26..42 of every file against hashlib, the three files against each other, some against the CPU
oracle; the populations that meet the lockstep branch inside a block again with shared_md5 and over a device list; every file back
through the batch decoder, whose device MD5 (k_md5_many) must give hashlib's digest too; and total lengths at every residue of the
padding.  No comparison has a tolerance, none may be left out: the last test counts them.

Before run_hash asked Md5::buffered(), leg (c) of exactly the 32 hazardous cases (_md5_shapes.hazardous_cases()) gave another
digest than hashlib's in files otherwise equal -- 1000x1x16-min, stream 1: df6277f57e90f82f122d4e406dc2c5e7 where hashlib gives
1dd585d36f3162130c680f8a07d89248 -- and every other comparison held."""
import functools
import hashlib

import numpy as np
import pytest

import _md5_shapes as ms
import _oracle as orc
from _pcm import le_bytes, synth_fast

pytestmark = pytest.mark.gpu

CASES = ms.cases()
HAZARDOUS = ms.hazardous_cases()
DONE = {}          # leg -> (stream, path) digest comparisons made


def _count(leg, n=1):
    DONE[leg] = DONE.get(leg, 0) + n


def _opts(block):
    """One Rice partition per subframe: the reference's partition search can write a frame shorter than twice its predictor order
    in a form no decoder takes (tests/_compare.py frames_the_reference_cannot_decode); with one partition it cannot, and the
    digest does not depend on it."""
    from flac_codec_amd.encode import Options

    return Options.default().block_size(block).max_partition_order(0)


def _orc_opts(block):
    return orc.options("default", block_size=block, max_partition_order=0)


@functools.lru_cache(maxsize=None)
def _pcm(si, pi):
    _, ch, bps = ms.SHAPES[si][:3]
    return [synth_fast(780000 + 1000 * si + 100 * pi + k, ch, bps, n) for k, n in enumerate(ms.lengths(si, pi))]


def _digest(pcm, bps):
    return hashlib.md5(le_bytes(pcm, bps)).digest()


def _writer_in_pieces(pcm, opts, bps, ch, seed):
    """One FlacSampleWriter fed in write() calls of 1 .. a few blocks' samples, no multiple of anything; batches of three blocks, so
    that the chain crosses partial MD5 blocks between batches as well."""
    from flac_codec_amd.encode import FlacSampleWriter

    rng = np.random.Generator(np.random.PCG64(seed))
    w = FlacSampleWriter(None, opts.batch_frames(3), ms.RATE, bps, ch, pcm.size)
    pos = 0
    while pos < pcm.size:
        kind = int(rng.integers(4))
        n = (1, int(rng.integers(2, 200)), int(rng.integers(200, 5000)), int(rng.integers(5000, 60000)))[kind]
        w.write(pcm[pos:pos + n])
        pos += n
    w.finalize()
    data = w.getvalue()
    w.close()
    return data


@functools.lru_cache(maxsize=None)
def _pool(si, pi):
    """Leg (b): the batch encoder, a writer per stream, the MD5 engine pool."""
    from flac_codec_amd.encode import BatchEncoder

    block, ch, bps = ms.SHAPES[si][:3]
    return BatchEncoder(_opts(block), threads=4).encode(_pcm(si, pi), ms.RATE, bps, ch)


def _coalesced(si, pi, shared=False):
    """Leg (c): the coalescing front end, the whole population in one batch (tests/test_md5_shape_cases.py)."""
    from flac_codec_amd.encode import BatchEncoder

    block, ch, bps = ms.SHAPES[si][:3]
    o = _opts(block).batch_frames(ms.batch_frames(ms.populations(si)[pi][1]))
    if shared:
        o = o.shared_md5(True)
    return BatchEncoder(o, threads=4, coalesce=True).encode(_pcm(si, pi), ms.RATE, bps, ch)


def _compare_files(leg, paths, pcms, bps, where):
    """paths: {name: [file per stream]}.  Every file's STREAMINFO MD5 must be hashlib's and the files of all paths equal: returns
    what is not."""
    bad = []
    names = list(paths)
    for k, pcm in enumerate(pcms):
        want = _digest(pcm, bps)
        for name in names:
            got = paths[name][k][26:42]
            _count(leg)
            if got != want:
                bad.append(f"{where} stream {k} ({pcm.size} samples) path {name}: MD5 {got.hex()}, hashlib {want.hex()}")
        first = paths[names[0]][k]
        for name in names[1:]:
            f = paths[name][k]
            if f != first:
                bad.append(f"{where} stream {k}: the file of path {name} differs from path {names[0]}'s"
                           + (" in the MD5 only" if f[:26] + f[42:] == first[:26] + first[42:] else ""))
    return bad


@pytest.mark.parametrize("si,pi", CASES, ids=[ms.case_id(si, pi) for si, pi in CASES])
def test_three_paths_give_hashlibs_digest(si, pi):
    block, ch, bps = ms.SHAPES[si][:3]
    pcms = _pcm(si, pi)
    a = [_writer_in_pieces(p, _opts(block), bps, ch, 880000 + 1000 * si + 100 * pi + k) for k, p in enumerate(pcms)]
    bad = _compare_files("sweep", {"a": a, "b": _pool(si, pi), "c": _coalesced(si, pi)}, pcms, bps, ms.case_id(si, pi))
    # the oracle's file: of the stream shorter than a block and, in the small populations, of the second stream
    for k in (1, len(pcms) - 1) if ms.populations(si)[pi][0] != "big" else (len(pcms) - 1,):
        rc, ref, _ = orc.encode_stream(_orc_opts(block), ms.RATE, bps, ch, pcms[k], total_known=True)
        _count("oracle")
        if rc != 0 or a[k] != ref:
            bad.append(f"{ms.case_id(si, pi)} stream {k}: the writer's file differs from the oracle's (rc {rc})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("si,pi", HAZARDOUS, ids=[ms.case_id(si, pi) for si, pi in HAZARDOUS])
def test_hazardous_populations_on_shared_engines_and_a_device_list(si, pi):
    from flac_codec_amd.encode import BatchEncoder

    block, ch, bps = ms.SHAPES[si][:3]
    pcms = _pcm(si, pi)
    paths = {
        "b": _pool(si, pi),
        "b-shared": BatchEncoder(_opts(block).shared_md5(True), threads=4).encode(pcms, ms.RATE, bps, ch),
        "c-shared": _coalesced(si, pi, shared=True),
        "b-devices": BatchEncoder(_opts(block), threads=4, devices=[0, 0]).encode(pcms, ms.RATE, bps, ch),
        "b-shared-devices": BatchEncoder(_opts(block).shared_md5(True), threads=4, devices=[0, 0]).encode(pcms, ms.RATE, bps, ch),
    }
    bad = _compare_files("hazardous", paths, pcms, bps, ms.case_id(si, pi))
    assert not bad, "\n".join(bad)


def test_hazardous_pairs_in_both_upload_modes():
    """The ring uploads at the stream's width where the device can widen it and int32 otherwise (then the HASH tasks read the
    stream's own byte string): at least three hazardous pairs each way, as the library says."""
    from flac_codec_amd.gpu import GpuAnalyzer

    packed = {}
    for si in sorted({si for si, _ in HAZARDOUS}):
        block, ch, bps = ms.SHAPES[si][:3]
        an = GpuAnalyzer(block, 0, 8, True, True, 2, 0.5, bps, ch, max_frames=4)
        packed[si] = an.packed_input_supported((bps + 7) // 8)
        an.close()
    at_width = [c for c in HAZARDOUS if packed[c[0]]]
    as_int32 = [c for c in HAZARDOUS if not packed[c[0]]]
    assert len(HAZARDOUS) >= 10 and len(at_width) >= 3 and len(as_int32) >= 3, (len(at_width), len(as_int32))


def _check_decoded(leg, blobs, pcms, bps_of, out, where):
    from flac_codec_amd.gpu import decode_many

    _, streams = decode_many(blobs, out=out)
    bad = []
    for k, (s, pcm) in enumerate(zip(streams, pcms)):
        bps = bps_of(k)
        want = _digest(pcm, bps)
        _count(leg)
        rec = (s.rc, s.info.bad_frames, s.info.bad_crc16, s.info.md5_status, bytes(s.info.decoded_md5))
        if rec != (0, 0, 0, 1, want):
            bad.append(f"{where} stream {k} ({pcm.size} samples, {bps} bits): rc, bad frames, bad CRC-16, MD5 status, MD5 = "
                       f"{rec[:4]} {rec[4].hex()}, hashlib {want.hex()}")
            continue
        got = s.pcm.cpu().numpy() if out == "device" else s.pcm
        if not np.array_equal(got.reshape(-1), pcm):
            bad.append(f"{where} stream {k}: decoded samples differ")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("si", range(len(ms.SHAPES)), ids=[ms.shape_id(s) for s in ms.SHAPES])
def test_round_trip_through_the_batch_decoder(si):
    """Every file of the shape in ONE decode_many call, samples to device memory, the MD5 by k_md5_many."""
    bps = ms.SHAPES[si][2]
    pops = range(len(ms.populations(si)))
    blobs = [b for pi in pops for b in _pool(si, pi)]
    pcms = [p for pi in pops for p in _pcm(si, pi)]
    _check_decoded("decode", blobs, pcms, lambda k: bps, "device", ms.shape_id(ms.SHAPES[si]))


# ---- total lengths at the edges of the MD5 padding -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _residue_streams():
    """[(bits, samples, what)] mono: 8 bits at every residue; 2, 3 and 4 bytes at 0, 55 / 56, 62 / 63 and 1 .. 4; one sample."""
    out = [(8, n, "8 bits, %d bytes = %d mod 64" % (n, n % 64)) for n in ms.residue_lengths_8bit()]
    for bits in ms.WIDTH_BITS:
        out += [(bits, n, "%d bits, %d bytes = %d mod 64" % (bits, n * ((bits + 7) // 8), t)) for t, n in ms.residue_lengths(bits)]
    out += [(bits, 1, "%d bits, one sample" % bits) for bits in ms.ONE_SAMPLE_BITS]
    return out


@functools.lru_cache(maxsize=None)
def _residue_files():
    """The residue streams' PCM and their files through the coalescing front end: one call per width, every stream a solo chain and
    a short last block (or the short block alone)."""
    from flac_codec_amd.encode import BatchEncoder

    cases = _residue_streams()
    pcms = [synth_fast(990000 + k, 1, bits, n) for k, (bits, n, _) in enumerate(cases)]
    files = [None] * len(cases)
    for bits in sorted({b for b, _, _ in cases}):
        idx = [k for k, c in enumerate(cases) if c[0] == bits]
        outs = BatchEncoder(_opts(ms.RESIDUE_BLOCK).batch_frames(64), threads=4, coalesce=True).encode(
            [pcms[k] for k in idx], ms.RATE, bits, 1)
        for k, o in zip(idx, outs):
            files[k] = o
    return pcms, files


def test_residues_writer_and_coalesced():
    cases = _residue_streams()
    assert sorted({(n * ((b + 7) // 8)) % 64 for b, n, _ in cases if b == 8 and n > 1}) == list(range(64))
    for bits, targets in ((16, {0, 56, 62, 2, 4}), (24, set(ms.RESIDUE_TARGETS)), (32, {0, 56, 4})):
        assert {t for t, _ in ms.residue_lengths(bits)} == targets
    pcms, files = _residue_files()
    bad = []
    for k, ((bits, n, what), pcm, c) in enumerate(zip(cases, pcms, files)):
        a = _writer_in_pieces(pcm, _opts(ms.RESIDUE_BLOCK), bits, 1, 991000 + k)
        want = _digest(pcm, bits)
        _count("residues", 2)
        if a[26:42] != want or c[26:42] != want or a != c:
            bad.append(f"{what}: writer {a[26:42].hex()}, coalesced {c[26:42].hex()}, hashlib {want.hex()}"
                       + ("" if a[:26] + a[42:] == c[:26] + c[42:] else "; the files differ outside the MD5"))
    rc, ref, _ = orc.encode_stream(_orc_opts(ms.RESIDUE_BLOCK), ms.RATE, 8, 1, pcms[55], total_known=True)
    assert rc == 0 and files[55] == ref
    _count("oracle")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("out", ["host", "device"])
def test_residues_through_the_batch_decoder(out):
    cases = _residue_streams()
    pcms, files = _residue_files()
    _check_decoded("residues-decode", files, pcms, lambda k: cases[k][0], out, "residues, out=" + out)


def test_residues_without_md5_report_status_3():
    from flac_codec_amd.gpu import decode_many

    pcms, files = _residue_files()
    for out in ("host", "device"):
        _, streams = decode_many(files, out=out, verify_md5=False)
        for k, (s, pcm) in enumerate(zip(streams, pcms)):
            _count("residues-nomd5")
            assert (s.rc, s.info.md5_status, bytes(s.info.decoded_md5)) == (0, 3, bytes(16)), (k, out)
            got = s.pcm.cpu().numpy() if out == "device" else s.pcm
            assert np.array_equal(got.reshape(-1), pcm), (k, out)


def test_no_comparison_was_left_out():
    """The (stream, path) comparisons the tests above made are the ones the case list defines, all of them."""
    streams = {c: len(ms.lengths(*c)) for c in CASES}
    residues = len(_residue_streams())
    assert residues == 64 + 5 + 9 + 3 + 5 + 9 + 6
    want = {
        "sweep": 3 * sum(streams.values()),
        "hazardous": 5 * sum(streams[c] for c in HAZARDOUS),
        "decode": sum(streams.values()),
        "oracle": sum(1 if ms.populations(si)[pi][0] == "big" else 2 for si, pi in CASES) + 1,
        "residues": 2 * residues,
        "residues-decode": 2 * residues,
        "residues-nomd5": 2 * residues,
    }
    assert DONE == want
