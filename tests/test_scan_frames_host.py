"""flacgpu_scan_frames_host -- the frame scan of raw frame streams (bare frames, no fLaC marker, no STREAMINFO; DESIGN.md
4b "Raw frame streams") that the batch decoder's device scan is specified against -- on the CPU: against what the
hand-built frames were written from, and against the rule as a Python model (_raw_frames.py) on cut, flipped and
look-alike input."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import _raw_frames as rf

ERR_INVALID_ARG, ERR_BUFFER_TOO_SMALL = -1, -5   # include/flacenc_gpu.h
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacenc_gpu.h")


def _scan(blob, cap=None):
    """(rc, records as tuples, summary tuple, n_frames) of one flacgpu_scan_frames_host call with `cap` records (None:
    as many as the count query reports)."""
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import FRAME_DTYPE

    L = _lib.lib()
    blob = bytes(blob)
    n, raw = C.c_uint32(0xDEAD), _lib.RawStream()
    if cap is None:
        rc = L.flacgpu_scan_frames_host(blob, len(blob), None, 0, C.byref(n), C.byref(raw))
        assert rc == 0
        cap = n.value
    frames = np.full(cap + 1, 0xEE, dtype=np.uint8).repeat(64).view(FRAME_DTYPE)
    rc = L.flacgpu_scan_frames_host(blob, len(blob), frames.ctypes.data_as(C.POINTER(_lib.FrameRecord)), cap,
                                    C.byref(n), C.byref(raw))
    assert (frames[cap:].view(np.uint8) == 0xEE).all(), "a write past the capacity"
    assert rc == 0 or (frames.view(np.uint8) == 0xEE).all(), "a refused call wrote"
    recs = [rf.record_tuple(f) for f in frames[:n.value]] if rc == 0 else []
    return rc, recs, rf.summary_tuple(raw), n.value


def _model(blob):
    frames, summary = rf.scan(blob)
    return [rf.record_tuple(f) for f in frames], rf.summary_tuple(summary)


def _agrees(blob, label):
    rc, recs, summary, n = _scan(blob)
    want, want_summary = _model(blob)
    assert rc == 0 and n == len(want), label
    assert recs == want, label
    assert summary == want_summary, label
    return recs, summary


def _kept(st, recs):
    """The true frames of `st` among `recs` (by start and length), and whether every record is one."""
    true = {(st.at[k], len(c)): k for k, c in enumerate(st.frame_bytes)}
    kept = [true.get((r[0], r[4])) for r in recs]
    return {k for k in kept if k is not None}, None not in kept


def test_exports_and_struct_layouts():
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import FRAME_DTYPE

    for name in ("flacgpu_scan_frames_host", "flacgpu_decoder_scan_frames", "flacgpu_decoder_frame_records",
                 "flacgpu_decoder_decode_frames"):
        assert name in _lib.exported_symbols(), name
    assert C.sizeof(_lib.FrameRecord) == 64 and C.sizeof(_lib.RawStream) == 32 and FRAME_DTYPE.itemsize == 64
    text = open(HEADER).read()
    for struct, cls in (("flacgpu_frame_record", _lib.FrameRecord), ("flacgpu_raw_stream", _lib.RawStream)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = []
        for ctype, names in re.findall(r"(uint64_t|uint32_t)\s+([^;]+);", body):
            declared += [(name.strip(), 8 if ctype == "uint64_t" else 4) for name in names.split(",")]
        assert declared == [(name, C.sizeof(ct)) for name, ct in cls._fields_], struct
        at = 0
        for name, size in declared:   # no padding: every field follows the one before
            assert getattr(cls, name).offset == at, (struct, name)
            at += size
    assert [n for n, _ in _lib.FrameRecord._fields_] == list(rf.RECORD_FIELDS) == list(FRAME_DTYPE.names)


def test_mixed_stream_gives_every_field():
    st = rf.mixed()
    assert [s for s in st.shapes] == list(rf.SHAPES) * 2
    assert set(st.assignments) >= {8, 9, 10} and (192000, 32, 2, 16) == st.shapes[5] and st.assignments[5] == 10
    rc, recs, summary, n = _scan(st.blob)
    assert rc == 0 and n == 12
    assert recs == [rf.record_tuple(r) for r in rf.expected_records(st)]
    assert summary == (12, 0, 0, 0)   # frames, skipped_bytes, gaps, uniform
    assert (recs, summary) == _model(st.blob)


def test_one_shape_repeated_is_uniform():
    st = rf.uniform()
    rc, recs, summary, n = _scan(st.blob)
    assert rc == 0 and recs == [rf.record_tuple(r) for r in rf.expected_records(st)]
    assert summary == (len(st.frame_bytes), 0, 0, 1)


def test_head_cuts_lose_frame_0_only():
    st = rf.mixed()
    cuts = rf.head_cuts(st)
    assert len(cuts) == len(st.frame_bytes[0])
    for k, blob in enumerate(cuts, start=1):
        recs, summary = _agrees(blob, f"head cut {k}")
        assert [(r[0] + k, r[4]) for r in recs] == [(st.at[j], len(st.frame_bytes[j])) for j in range(1, 12)], k
        gaps = 0 if k == len(st.frame_bytes[0]) else 1   # the whole of frame 0 cut: nothing is left to skip
        assert summary == (11, len(st.frame_bytes[0]) - k, gaps, 0), k


def test_tail_cuts():
    st = rf.mixed()
    hb = rf.header_bytes(st, 11)
    whole_header = 0
    for left, blob in rf.tail_cuts(st):
        recs, summary = _agrees(blob, f"tail cut, {left} bytes left")
        kept, all_true = _kept(st, recs)
        assert all_true, left
        if left >= hb:   # the last frame's header is whole: it ends frame 10, and only the last frame is lost
            whole_header += 1
            assert kept == set(range(11)), left
        else:
            assert kept <= set(range(11)), left
    assert whole_header == len(st.frame_bytes[11]) - hb


def test_one_flipped_byte_at_every_position():
    st = rf.mixed()
    own = body = 0
    cases = rf.flips(st)
    assert len(cases) == len(st.blob) > 1000
    for pos, blob in cases:
        recs, _ = _agrees(blob, f"flip at {pos}")
        kept, all_true = _kept(st, recs)
        assert all_true, f"flip at {pos}: a kept frame that is no frame"
        j = rf.frame_of(st, pos)
        lost = set(range(12)) - kept
        if pos - st.at[j] >= rf.header_bytes(st, j):   # a body or CRC-16 byte: the frame's own loss
            body += 1
            assert lost == {j}, f"flip at {pos}"
        else:   # a header byte costs the frame in front too (frame 0 has none); a flipped number still parses
            assert lost <= {j - 1, j}, f"flip at {pos}"
        own += lost == {j}
    assert body == len(st.blob) - sum(rf.header_bytes(st, k) for k in range(12))
    assert own >= 0.95 * len(cases)   # not vacuous: nearly every flip costs exactly its own frame


def test_non_subset_frames_are_not_kept():
    """A frame whose header leaves the rate or the sample size to a STREAMINFO is no candidate and is never a record of
    its own.  By the rule its predecessor then ends at the next candidate the CRC-16 fits -- and a whole frame appended
    to a whole frame leaves the CRC-16 fitting (the CRC of a frame with its own CRC is 0) -- so the predecessor's record
    runs over the odd frame's bytes: kept by the scan, and marked as not parsing by decode_frames
    (test_gpu_raw_frames.py), because its subframes end before its bytes do."""
    st = rf.mixed()
    for label, blob in rf.non_subset_cases():
        recs, summary = _agrees(blob, label)
        extra = len(blob) - len(st.blob)
        assert st.at[3] not in [r[0] for r in recs], label   # where the odd frame starts
        want = [(st.at[k] + (extra if k > 2 else 0), len(st.frame_bytes[k]) + (extra if k == 2 else 0)) for k in range(12)]
        assert [(r[0], r[4]) for r in recs] == want, label
        assert summary == (12, 0, 0, 0), label


def test_look_alike_regions():
    kept = 0
    for label, blob in rf.lookalike_cases():
        recs, _ = _agrees(blob, label)
        kept += len(recs)
    assert kept > 0   # "headers that link by CRC-16" do link


def test_empty_input_small_capacity_and_null_arguments():
    from flac_codec_amd import _lib

    L = _lib.lib()
    st = rf.mixed()
    n, raw = C.c_uint32(7), _lib.RawStream()
    assert L.flacgpu_scan_frames_host(b"", 0, None, 0, C.byref(n), C.byref(raw)) == 0
    assert L.flacgpu_scan_frames_host(None, 0, None, 0, C.byref(n), C.byref(raw)) == 0
    assert n.value == 0 and rf.summary_tuple(raw) == (0, 0, 0, 0)
    rc, recs, _, n_frames = _scan(st.blob, cap=11)
    assert rc == ERR_BUFFER_TOO_SMALL and n_frames == 12
    rc, recs, _, n_frames = _scan(st.blob, cap=40)   # more room than frames
    assert rc == 0 and len(recs) == 12
    assert L.flacgpu_scan_frames_host(None, 10, None, 0, C.byref(n), C.byref(raw)) == ERR_INVALID_ARG
    assert L.flacgpu_scan_frames_host(st.blob, len(st.blob), None, 0, None, C.byref(raw)) == ERR_INVALID_ARG
    assert L.flacgpu_scan_frames_host(st.blob, len(st.blob), None, 0, C.byref(n), None) == ERR_INVALID_ARG
