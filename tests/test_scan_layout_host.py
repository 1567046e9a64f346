"""The inputs of _scan_layout.py -- aimed at the device frame scan's blocks, workgroups, carry runs and the order of x --
proved on the CPU: the byte-level builder writes what _flacsyn's writer writes, every case's aim is recomputed from the
blobs' lengths by the layout rule, and every case's expected scan comes from the host scans (flacgpu_scan_frames_host,
flacgpu_scan_stream_host) and, up to 1 MiB, from the rules' Python models, and is the frames the builder placed.
test_gpu_scan_layout.py holds the device scan to the same on an MI355X."""
import numpy as np
import pytest

import _flacsyn as fs
import _oracle as orc
import _raw_frames as rf
import _scan_layout as sl
import _scan_model as sm
import _spec_frames as sf

MODEL_LIMIT = 1 << 20


def _fs_frame(fr):
    kw = dict(min=dict(), six=dict(bcode=6), fit=dict(bcode=7), long=dict(bcode=7, blocking=1))[fr.style]
    rcode = 13 if fr.style == "long" else fs.RATE_CODES[sl.RATE]
    return fs.Frame([fr.samples.tolist()], [fs.verbatim()], rcode=rcode, number=fr.number, **kw)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("style", ["min", "six", "fit", "long"])
def test_the_fast_builder_is_the_writer(bits, style):
    sizes = (192, 256, 4096) if style == "min" else (1, 2, 46, 192, 255, 256) if style == "six" else (1, 17, 256, 257, 1000)
    st = sl.Stream(False, bits=bits, style=style)
    for k, n in enumerate(sizes):
        plants = ((3, sl.plant(k)),) if n >= 192 and bits == 8 else ()
        fr = st.add(n, 40 + k, plants)
        assert fr.header_bytes == {"min": 6, "six": 7, "fit": 8, "long": 16}[style]
        assert len(fr.data) == fr.header_bytes + 1 + n * bits // 8 + 2
        assert fr.data == fs.write_frame(sl.RATE, bits, _fs_frame(fr), set()), (n, k)
        if not plants:
            assert 1 <= fr.samples.min() and (fr.samples.max() <= 100 if bits == 8 else fr.samples.max() < 101 << 8)
    want = fs.write_stream(sl.RATE, bits, [_fs_frame(f) for f in st.frames])
    assert st.blob == want.blob
    assert np.array_equal(st.pcm, want.pcm)
    rc, pcm, info = orc.decode_stream(st.blob)
    assert rc == 0 and info.md5_ok == 1 and np.array_equal(pcm, st.pcm)


def test_the_constants_come_from_the_sources():
    assert (sl.WG, sl.SLOT_TAIL) == (256, 64)   # what the cases' comments speak of; the aims below hold for any values
    with pytest.raises(RuntimeError):
        sl._constant("decode_many.hip", r"constexpr\s+uint32_t\s+kNoSuchConstant\s*=\s*(\d+)")


def _frames_abs(case):
    """(start, end) in the batch buffer of every frame the builder placed."""
    return [(case.layout.base[i] + f.offset, case.layout.base[i] + f.offset + len(f.data))
            for i, st in enumerate(case.streams) for f in st.frames]


def _check_aim(case, aim):
    L, kind = case.layout, aim[0]
    lens = [sl.region_len(b, case.raw) for b in case.blobs]
    assert lens == [s.size for s in case.streams]
    if kind == "every phase":
        _, i, hb = aim
        frames = case.streams[i].frames
        assert {case.frame_at(i, k) % 64 for k in range(len(frames))} == set(range(64))
        assert {f.header_bytes for f in frames} == {hb}
        assert hb == 6 or max(case.frame_at(i, k) % 64 for k in range(len(frames))) + hb > 64   # into the look-ahead
    elif kind == "header at":
        _, i, k, wg, block, byte = aim
        assert sl.where(case.frame_at(i, k)) == (wg, block, byte)
        assert case.streams[i].frames[k].header_bytes == 16
    elif kind == "slot at":
        _, i, wg, block = aim
        assert L.base[i] % 64 == 0 and sl.where(L.base[i])[:2] == (wg, block)
    elif kind == "no slot":
        assert L.base[aim[1]] is None and lens[aim[1]] == 0
        assert all(L.base[i] is not None for i in range(len(lens)) if i != aim[1])
    elif kind == "frame spans workgroups":
        _, i, k = aim
        a = case.frame_at(i, k)
        assert a // sl.WGB < (a + len(case.streams[i].frames[k].data) - 1) // sl.WGB
    elif kind == "frame covers workgroups":
        _, i, k, count = aim
        a = case.frame_at(i, k)
        assert (a + len(case.streams[i].frames[k].data) - 1) // sl.WGB - a // sl.WGB >= count
    elif kind == "region bytes":
        assert lens[aim[1]] == aim[2]
    elif kind == "region mod 64":
        assert lens[aim[1]] % 64 == aim[2]
    elif kind == "region ends with workgroup":
        end = L.base[aim[1]] + lens[aim[1]]
        assert end % sl.WGB == 0 and end // 64 < L.blocks   # the tail block is lane 0 of the next workgroup
    elif kind == "plants at":
        _, i, k, spots = aim
        fr = case.streams[i].frames[k]
        got = [case.frame_at(i, k) + at for at, _ in fr.plants]
        assert got == list(spots)
        for at, size in fr.plants:   # each is a header the scan accepts
            assert sm.parse_header(fr.data[at:at + 16])[1] == size
        blocks = [p // 64 for p in got]
        assert max(blocks.count(b) for b in blocks) >= 3 and len({p // sl.WGB for p in got}) >= 2
        edge = (min(got) // sl.WGB + 1) * sl.WGB
        assert edge - 64 <= max(p for p in got if p < edge) and edge in got   # the blocks on both sides of the boundary
    elif kind == "first candidate not at base":
        st = case.streams[aim[1]]
        assert case.raw and st.frames[0].offset > 0 and rf.parse(st.blob[:16]) is None
    elif kind == "n_wg":
        assert L.n_wg == aim[1] and L.per == -(-aim[1] // sl.WG)
        runs = -(-L.n_wg // L.per)   # lanes >= runs own empty runs
        assert (runs < sl.WG) == (aim[1] in (255, 257, 513, 770)), runs
        assert {255: 255, 256: 256, 257: 129, 512: 256, 513: 171, 768: 256, 770: 193}[aim[1]] == runs
    elif kind == "one region":
        assert len(case.streams) == 1
        _check_run_boundaries(case)
    elif kind == "slot starts in workgroups":
        got = [b // sl.WGB for b in L.base]
        assert got == list(aim[1])
        per = L.per
        place = {"first" if w % per == 0 else "last" if w % per == per - 1 else "interior" for w in got[1:]}
        assert place == ({"first"} if per == 1 else {"first", "last"} if per == 2 else {"first", "last", "interior"})
    elif kind == "frames span the run boundaries":
        _check_run_boundaries(case)
    elif kind == "region offsets":
        _, i, ks, offsets = aim
        assert [case.streams[i].frames[k].offset for k in ks] == list(offsets)
        assert [o % sl.ORDER for o in offsets] == [0, 0, 1]
    elif kind == "frame bytes":
        assert len(case.streams[aim[1]].frames[aim[2]].data) == aim[3] and aim[3] % sl.ORDER == 0
    else:
        raise AssertionError(f"unknown aim {aim}")


def _check_run_boundaries(case):
    """A frame lies across every boundary between two of k_scan_carry's runs."""
    L = case.layout
    frames = _frames_abs(case)
    starts = np.array([a for a, _ in frames])
    for r in range(1, -(-L.n_wg // L.per)):
        edge = r * L.per * sl.WGB
        k = int(np.searchsorted(starts, edge, side="left")) - 1   # the last frame that starts before the boundary
        assert k >= 0 and frames[k][0] < edge < frames[k][1], (case.name, r)


def test_the_cases_cover_the_issue():
    cases = sl.cases()
    assert len(cases) == 35 and {c.item for c in cases} == set("abcdef")
    for item in "bde":   # each shape as a raw and as a regular batch
        forms = [c.raw for c in cases if c.item == item]
        assert forms.count(True) == forms.count(False) >= 1, item
    assert sorted(c.layout.n_wg for c in cases if c.item == "c") == sorted(2 * sl.CARRY_N_WG)
    assert [(-(-n // sl.WG)) for n in sl.CARRY_N_WG] == [1, 1, 2, 2, 3, 3, 4]
    assert max(c.nbytes for c in cases) < 12.7 * 2 ** 20


@pytest.mark.parametrize("name", [c.name for c in sl.cases()])
def test_every_case_is_what_it_claims(name):
    case = sl.case(name)
    assert case.aims
    for aim in case.aims:
        _check_aim(case, aim)


def _raw_expected(case, speculative):
    """Per stream: the builder's records (stream 0, out_offset from 0, as the host scan of one input gives them) and
    summary."""
    out = []
    for st in case.streams:
        recs, at = [], 0
        for f in sl.kept_frames(st, speculative):
            recs.append((f.offset, f.number, at, 0, len(f.data), f.n, sl.RATE, 1, f.bits, 0, int(f.style == "long"), 0,
                         int(f.kept == "speculative")))
            at += f.n
        out.append((recs, sl.expected_summary(st, speculative)))
    return out


@pytest.mark.parametrize("name", [c.name for c in sl.cases()])
def test_every_case_scans_to_the_frames_the_builder_placed(name):
    from flac_codec_amd.gpu import scan_frames_host, scan_stream_host

    case = sl.case(name)
    small = case.nbytes <= MODEL_LIMIT
    if case.raw:
        for speculative in (False, True) if case.speculative or case.item == "b" else (False,):
            for st, blob, (want, summary) in zip(case.streams, case.blobs, _raw_expected(case, speculative)):
                frames, raw = scan_frames_host(blob, speculative=speculative)
                assert [rf.record_tuple(f) for f in frames] == want, speculative
                assert rf.summary_tuple(raw)[:3] == summary, speculative
                assert raw.uniform == int(len({f[8] for f in want}) == 1)
                if small:
                    model, model_summary = sf.scan(blob, speculative)
                    assert [rf.record_tuple(f) for f in model] == want, speculative
                    assert rf.summary_tuple(model_summary) == rf.summary_tuple(raw), speculative
        assert list(sl.RECORD_FIELDS) == list(rf.RECORD_FIELDS)
        return
    for st, blob in zip(case.streams, case.blobs):
        first = len(blob) - st.size
        info, offsets, sizes = scan_stream_host(blob)
        assert offsets.tolist() == [first + f.offset for f in st.frames]
        assert sizes.tolist() == [f.n for f in st.frames]
        assert (info.frames, info.bad_frames, info.decoded_samples) == (len(st.frames), 0, st.samples)
        assert (info.sample_rate, info.channels, info.bits_per_sample) == (sl.RATE, 1, st.bits)
        if small:
            assert sm.scan(blob) == (0, offsets.tolist(), sizes.tolist(), 0, st.samples)


def test_the_own_extent_cases_differ_as_they_say():
    """Item f: with its CRC-16 cut off the last frame is kept by neither rule (there is no test left that it could
    pass); with filler behind it the plain rule passes it over and the flag keeps it."""
    cut, filled = [c for c in sl.cases() if c.item == "f"]
    assert [f.kept for f in cut.streams[1].frames] == ["always", "never"]
    assert [f.kept for f in filled.streams[1].frames] == ["always", "speculative"]
    lead = sl.OWN_LEAD   # the filler in front of the first frame: skipped too
    assert sl.expected_summary(cut.streams[1], True) == sl.expected_summary(cut.streams[1], False) == (1, lead + 20009, 2)
    assert sl.expected_summary(filled.streams[1], False) == (1, lead + 20011 + 1500, 2)
    assert sl.expected_summary(filled.streams[1], True) == (2, lead + 1500, 2)
