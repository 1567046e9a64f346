"""flacgpu_timeline_host -- the timeline rule for one stream's records, on the host alone -- against the Python model of
_timeline.py, and what the case set covers.  CPU only: no GPU call.

The model and the C function are compared on every case of _timeline.cases() (records from flacgpu_scan_frames_host_ex,
with and without FLACGPU_SCAN_SPECULATIVE, and from the Python scan model), on every input of _raw_frames.all_cases(),
and on record lists that no scan gives.  The cases' own expectations -- built by placement from the writer's PCM -- are
held against the model on the scanned records, so that a case whose bytes do not scan as its author meant fails here,
without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _raw_frames as rf
import _timeline as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, I16, F32, S24 = 0, 1, 2, 24
FLAT, PADDED = 0, 1


def piece():
    from flac_codec_amd.gpu import timeline_piece_bytes

    return timeline_piece_bytes()


def host(records):
    """(result tuple, [(at, flags, status)]) of flacgpu_timeline_host for a list of model dicts or a record array."""
    from flac_codec_amd import gpu

    if not isinstance(records, np.ndarray):
        rows = np.zeros(len(records), dtype=gpu.FRAME_DTYPE)
        for row, r in zip(rows, records):
            for k in rf.RECORD_FIELDS:
                row[k] = r[k]
        records = rows
    res, frames = gpu.scan_timeline_host(records)
    return tl.result_tuple(res), [(int(f["at"]), int(f["flags"]), int(f["status"])) for f in frames]


def check(records, where):
    want, frames = tl.timeline(records)
    got = host(records)
    assert got[0] == tl.result_tuple(want), where
    assert got[1] == [(at, flags, 0) for at, flags in frames], where
    return want


def test_symbols_are_exported():
    from flac_codec_amd import _lib

    _lib.lib()
    assert {"flacgpu_timeline_host", "flacgpu_timeline_piece_bytes", "flacgpu_decoder_plan_timeline",
            "flacgpu_decoder_decode_timeline"} <= _lib.exported_symbols()


def test_layouts_match_header(tmp_path):
    from flac_codec_amd import _lib

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the build needs a host C++ compiler"
    F, R = _lib.TimelineFrame, _lib.TimelineResult
    fields = [("flacgpu_timeline_frame", F), ("flacgpu_timeline_result", R)]
    exprs = [f"sizeof({name})" for name, _ in fields]
    exprs += [f"offsetof({name}, {f})" for name, t in fields for f, _ in t._fields_]
    exprs += ["(size_t)FLACGPU_TL_PLACED", "(size_t)FLACGPU_TL_DROPPED", "(size_t)FLACGPU_TL_CONCEALED",
              "(size_t)FLACGPU_TIMELINE_PIECE_BYTES"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_gpu.h"\nint main() {\n' +
                   "".join(f'    printf("%zu\\n", {e});\n' for e in exprs) + "}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cxx, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(F), C.sizeof(R)] + [getattr(t, f).offset for _, t in fields for f, _ in t._fields_]
    want += [_lib.TL_PLACED, _lib.TL_DROPPED, _lib.TL_CONCEALED, piece()]
    assert got == want
    assert got[:2] == [16, 56] and piece() % 48 == 0


@pytest.mark.parametrize("speculative", [False, True])
def test_cases_scan_as_their_authors_meant(speculative):
    """Every case: the host scan's records equal the scan model's (without `speculative`, which the model does not
    state), the C rule equals the model on them, and the model's result equals the case's own expectation with the
    concealed frames taken out (the host knows of them only after a decode)."""
    from flac_codec_amd.gpu import scan_frames_host

    for case in tl.cases(piece()):
        records = scan_frames_host(case.blob, speculative)[0]
        if not speculative:
            assert [rf.record_tuple(r) for r in records] == [rf.record_tuple(r) for r in rf.scan(case.blob)[0]], case.label
        got = check(records, case.label)
        want = dict(case.want[speculative].result, concealed=0, concealed_samples=0)
        assert tl.result_tuple(got) == tl.result_tuple(want), case.label
        if got["rc"] == tl.OK:
            assert {int(r["channels"]) for r in records} == {case.channels}, case.label
            assert {int(r["bits_per_sample"]) for r in records} == {case.bits}, case.label


def test_case_set_covers_what_the_fill_can_get_wrong():
    """Gaps begin and end at every residue modulo 16 of the byte address that each element size permits; one gap is
    longer than a piece of the fill kernel and one ends exactly on a piece boundary, in every element size or in the
    size named."""
    p = piece()
    cov = tl.coverage(tl.cases(p), p)
    for es, permitted in ((1, set(range(16))), (3, set(range(16))), (2, set(range(0, 16, 2))), (4, {0, 4, 8, 12})):
        first, last, longer, _ = cov[es]
        assert first == permitted and last == permitted, (es, sorted(first), sorted(last))
        assert longer, es
    assert cov[4][3] and cov[2][3]
    gaps = {n for c in tl.cases(p) for _, n in c.want[False].gap_runs()}
    assert {1, 5, 4097} <= gaps
    sizes = {pc.shape[1] for c in tl.cases(p) for _, pc in c.want[False].pieces}
    assert {16, 17, 33, 192, 4096} <= sizes
    shapes = {(c.bits, c.channels) for c in tl.cases(p) if c.want[False].rc == tl.OK}
    assert {b for b, _ in shapes} == {8, 12, 16, 24, 32} and {ch for _, ch in shapes} == {1, 2, 3}
    Cp, T = tl.layout(tl.cases(p))
    assert Cp == 3 and T % 16 == 0


def test_rule_on_every_raw_frame_input():
    """_raw_frames.all_cases(): 2253 inputs, most of them a damaged stream of frames of different formats -- the
    refusals -- and the uniform one."""
    from flac_codec_amd.gpu import scan_frames_host

    cases = rf.all_cases()
    assert len(cases) == 2253
    seen = set()
    for label, blob in cases:
        for speculative in (False, True):
            seen.add(check(scan_frames_host(blob, speculative)[0], label)["rc"])
    assert seen == {tl.OK, tl.INVALID_ARG, tl.UNSUPPORTED}


def test_rule_on_records_no_scan_gives():
    seen = set()
    for k, records in enumerate(tl.random_records(20261019, 3000)):
        want = check(records, k)
        seen.add((want["rc"], want["dropped"] > 0, want["gaps"] > 0))
    assert {(tl.OK, True, True), (tl.OK, False, False), (tl.UNSUPPORTED, False, False)} <= seen
    top = dict(tl.random_records(1, 1)[0][0], number=(1 << 36) - 1, block_size=65535, blocking=0)
    want = check([top], "the largest position")
    assert want["first_sample"] == ((1 << 36) - 1) * 65535


def test_refusals_are_named():
    from flac_codec_amd import _lib

    reasons = set()
    for case in tl.cases(piece()):
        if case.want[False].rc == tl.OK:
            continue
        got = host(rf.scan(case.blob)[0])
        assert got[0][0] == case.want[False].rc, case.label
        reasons.add(_lib.lib().flacgpu_last_error().decode())
    assert len(reasons) == 5 and all(r.startswith("flacgpu_timeline_host: ") for r in reasons), reasons


def test_refusals_that_need_no_handle():
    from flac_codec_amd import _lib

    L = _lib.lib()
    fmt = _lib.OutFormat(F32, PADDED, 2, 0, 192)
    res = (_lib.TimelineResult * 1)()
    need, mask = C.c_uint64(7), C.c_uint64(7)
    assert L.flacgpu_decoder_plan_timeline(None, C.byref(fmt), res, C.byref(need), C.byref(mask)) == tl.INVALID_ARG
    assert L.flacgpu_decoder_decode_timeline(None, None, 0, None, 0, C.byref(fmt), 0, res, None, 0) == tl.INVALID_ARG
    rec = (_lib.FrameRecord * 2)()
    frames = (_lib.TimelineFrame * 2)()
    assert L.flacgpu_timeline_host(rec, 2, frames, 2, None) == tl.INVALID_ARG
    assert L.flacgpu_timeline_host(None, 2, frames, 2, res) == tl.INVALID_ARG
    frames[0].at = frames[1].at = 99
    assert L.flacgpu_timeline_host(rec, 2, frames, 1, res) == -5   # FLACGPU_ERR_BUFFER_TOO_SMALL
    assert (frames[0].at, frames[1].at) == (99, 99), "a refused call wrote"
    assert L.flacgpu_timeline_host(rec, 2, None, 0, res) == tl.OK   # the counts alone
    assert L.flacgpu_timeline_host(None, 0, None, 0, res) == tl.OK and res[0].rc == tl.INVALID_ARG
