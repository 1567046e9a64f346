"""The device frame scan (kernels/frame_scan.inc, spec_end.inc) on the inputs of _scan_layout.py, which aim at ITS
structure: a header at every byte of a block and across a workgroup's last block, slots and region ends on a workgroup's
edge, k_scan_carry with 1 to 4 workgroups per lane and empty trailing runs, offsets and lengths that are multiples of
the order of x.  test_scan_layout_host.py proves on the CPU that every case is aimed where it says and that the host
scans find the frames the builder placed; here the device scan must give the host scan's records, byte for byte, and
every frame must decode to the samples it was written from.  All comparisons are exact."""
import numpy as np
import pytest

import _raw_frames as rf
import _scan_layout as sl
from test_gpu_decode_many import _same_info, _single
from test_gpu_raw_frames import decode_frames_guarded

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
RAW = [c.name for c in sl.cases() if c.raw]
REGULAR = [c.name for c in sl.cases() if not c.raw]
_compared = {"raw": set(), "regular": set()}


@pytest.fixture(scope="module")
def dec():
    from flac_codec_amd.gpu import Decoder

    d = Decoder(0)
    yield d
    d.close()


def _scan_is_the_host_scan(dec, case, speculative=False):
    """Decoder.scan_frames of the batch: records, summaries and return codes equal to flacgpu_scan_frames_host's for every
    input (test_gpu_raw_frames.test_device_scan_equals_host_scan), and the frames the builder placed."""
    from flac_codec_amd.gpu import scan_frames_host

    recs, total, raw, frames = dec.scan_frames(case.blobs, speculative=speculative)
    at = out = 0
    for i, blob in enumerate(case.blobs):
        want, summary = scan_frames_host(blob, speculative=speculative)
        want = want.copy()
        want["stream"] = i
        want["out_offset"] += out
        got = frames[at:at + len(want)]
        assert raw[i].first_frame == at, i
        assert rf.summary_tuple(raw[i]) == rf.summary_tuple(summary), i
        assert got.tobytes() == want.tobytes(), i
        at += len(want)
        out += int((want["block_size"].astype(np.int64) * want["channels"]).sum())
        want_rc = OK if summary.uniform else UNSUPPORTED if summary.frames else INVALID_ARG
        assert recs[i].rc == want_rc, i
        assert rf.summary_tuple(raw[i])[:3] == sl.expected_summary(case.streams[i], speculative), i
    assert at == len(frames) and out == dec.raw_elements
    assert [rf.record_tuple(f) for f in frames] == sl.builder_records(case, speculative)
    return frames


def _frames_decode(dec, case, frames, speculative, dest):
    samples, out = decode_frames_guarded(dec, frames, dest)
    assert (out["status"] == 0).all()
    out["status"] = 0
    assert out.tobytes() == frames.tobytes()
    want = [f.samples for st in case.streams for f in sl.kept_frames(st, speculative)]
    assert np.array_equal(samples, np.concatenate(want))   # the records' out_offset run through the batch in this order


@pytest.mark.parametrize("name", RAW)
def test_raw_batches(dec, name):
    case = sl.case(name)
    dests = ("host", "device") if case.item in "bc" else ("host",)
    if case.item in "bf":   # item f: k_spec_end on the same batches
        spec = _scan_is_the_host_scan(dec, case, speculative=True)
        if case.item == "f":
            for dest in dests:
                _frames_decode(dec, case, spec, True, dest)
    frames = _scan_is_the_host_scan(dec, case)
    if case.item == "b":   # every frame has an end: the flag changes nothing
        assert spec.tobytes() == frames.tobytes()
    elif case.item == "f":
        own = sum(f.kept == "speculative" for st in case.streams for f in st.frames)
        assert len(spec) == len(frames) + own and int(spec["reserved"].sum()) == own
    for dest in dests:
        _frames_decode(dec, case, frames, False, dest)
    _compared["raw"].add(name)


@pytest.mark.parametrize("name", REGULAR)
def test_regular_batches(dec, name):
    from flac_codec_amd.gpu import decode_many

    case = sl.case(name)
    flat, streams = decode_many(case.blobs, out="host", verify_md5=True, decoder=dec)
    assert len(streams) == len(case.streams)
    at = 0
    for i, (st, blob, s) in enumerate(zip(case.streams, case.blobs, streams)):
        assert (s.rc, s.offset) == (OK, at), i
        assert (s.info.bad_frames, s.info.bad_crc16, s.info.md5_status) == (0, 0, 1), i
        assert (s.info.frames, s.info.decoded_samples) == (len(st.frames), st.samples), i
        assert np.array_equal(s.pcm.reshape(-1), st.pcm), i
        at += st.samples
        if case.item in "bd":
            rc, info, pcm = _single(blob)
            assert rc == OK and np.array_equal(pcm, st.pcm), i
            _same_info(s.info, info)
    assert at == flat.size
    _compared["regular"].add(name)


def test_scans_on_one_handle_do_not_depend_on_their_order(dec):
    """A batch of 257 workgroups (two to a lane of k_scan_carry, the trailing lanes empty), a small batch, the large
    one again: the grown buffers and what the first scan left in the workgroup arrays do not matter."""
    big, small = sl.case("c: many regions over 257 workgroups"), sl.case("a: block phase")
    first = _scan_is_the_host_scan(dec, big).copy()
    between = _scan_is_the_host_scan(dec, small).copy()
    again = _scan_is_the_host_scan(dec, big)
    assert first.tobytes() == again.tobytes() and len(between) == 129
    _frames_decode(dec, big, again, False, "host")


def test_nothing_was_left_out():
    """Runs last in this file: every case of _scan_layout.cases() went through its GPU test, none skipped for size."""
    assert len(_compared["raw"]) + len(_compared["regular"]) == len(sl.cases())
    assert _compared["raw"] == set(RAW) and _compared["regular"] == set(REGULAR)
