"""flacgpu_scan_stream_host -- the metadata parse and frame scan that flacgpu_decode_stream starts with and that the batch
decoder's device scan is specified against -- on the CPU: against the true frame boundaries of the
hand-built matrix, against the rule written as a Python model on damaged input (_scan_model.py), and its refusals."""
import ctypes as C

import numpy as np
import pytest

import _flacsyn as fs
import _foreign_matrix as fm
import _scan_model as model

ERR_INVALID_ARG, ERR_BUFFER_TOO_SMALL = -1, -5   # include/flacenc_gpu.h


def _scan(blob, cap=None):
    """(rc, StreamInfo, offsets, sizes, n_frames) of one flacgpu_scan_stream_host call with arrays of `cap` entries
    (None: as many as the count query reports)."""
    from flac_codec_amd import _lib

    L = _lib.lib()
    blob = bytes(blob)
    info, n = _lib.StreamInfo(), C.c_uint32(0xDEAD)
    if cap is None:
        rc = L.flacgpu_scan_stream_host(blob, len(blob), C.byref(info), None, None, 0, C.byref(n))
        if rc:
            return rc, info, [], [], n.value
        cap = n.value
    off, sizes = np.full(cap + 1, 2 ** 64 - 1, np.uint64), np.full(cap + 1, 2 ** 32 - 1, np.uint32)
    rc = L.flacgpu_scan_stream_host(blob, len(blob), C.byref(info), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    sizes.ctypes.data_as(C.POINTER(C.c_uint32)), cap, C.byref(n))
    assert off[cap] == 2 ** 64 - 1 and sizes[cap] == 2 ** 32 - 1, "a write past the capacity"
    assert rc == 0 or ((off == 2 ** 64 - 1).all() and (sizes == 2 ** 32 - 1).all()), "a refused call wrote"
    return rc, info, off[:n.value].tolist() if rc == 0 else [], sizes[:n.value].tolist() if rc == 0 else [], n.value


def _streaminfo(info):
    return {f: bytes(info.md5) if f == "md5" else getattr(info, f) for f in model.STREAMINFO_FIELDS}


def _all_zero(info):
    return bytes(info) == bytes(C.sizeof(info))


def test_export_is_declared_and_bound():
    from flac_codec_amd import _lib

    assert "flacgpu_scan_stream_host" in _lib.exported_symbols()


def test_undamaged_streams_scan_to_their_true_frames():
    cases = list(fm.valid_cases()) + [st for _, st in fm.invalid_cases()]   # a malformed SUBFRAME does not disturb the scan
    assert len(cases) == 143
    for st in cases:
        rc, info, off, sizes, n = _scan(st.blob)
        want, at = [], len(st.blob) - sum(len(c) for c in st.frame_bytes)
        for c in st.frame_bytes:
            want.append(at)
            at += len(c)
        assert rc == 0 and n == len(st.frame_bytes), st.name
        assert off == want, st.name
        assert sizes == st.frame_sizes, st.name
        assert (info.frames, info.bad_frames, info.decoded_samples) == (n, 0, sum(st.frame_sizes)), st.name
        assert (info.sample_rate, info.channels, info.bits_per_sample) == (st.rate, st.channels, st.bps), st.name
        # STREAMINFO is the writer's first block: its block sizes at bytes 8..12, total at 21..26, MD5 at 26..42
        assert info.min_block == int.from_bytes(st.blob[8:10], "big"), st.name
        assert info.max_block == int.from_bytes(st.blob[10:12], "big"), st.name
        unknown_total = st.name in ("total-samples-unknown", "all-unknown")
        assert info.total_samples == (0 if unknown_total else sum(st.frame_sizes)), st.name
        stored = {1: st.digest, 2: bytes(16), 0: bytes([st.digest[0] ^ 1]) + st.digest[1:]}[st.md5_status]
        assert bytes(info.md5) == stored, st.name
        assert (info.bad_crc16, info.md5_status, bytes(info.decoded_md5)) == (0, 0, bytes(16)), st.name
        assert model.scan(st.blob) == (0, want, st.frame_sizes, 0, sum(st.frame_sizes)), st.name   # the model agrees


def test_damaged_streams_scan_as_the_rule_says():
    cases = model.damaged_cases()
    assert 250 <= len(cases) <= 350
    kinds = set()
    for label, blob in cases:
        rc, info, off, sizes, n = _scan(blob)
        want_rc, want_off, want_sizes, want_bad, want_samples = model.scan(blob)
        assert rc == want_rc, label
        assert (off, sizes) == (want_off, want_sizes), label
        assert (n, info.frames, info.bad_frames, info.decoded_samples) == \
            (len(want_off), len(want_off), want_bad, want_samples), label
        md = model.metadata(blob)
        if md:
            assert _streaminfo(info) == md[2], label
        kinds.add((rc, bool(n), want_bad))
    # refused, empty and clean, nothing kept, clean, some frames kept before the loss
    assert kinds == {(ERR_INVALID_ARG, False, 0), (0, False, 0), (0, False, 1), (0, True, 0), (0, True, 1)}


def _with_streaminfo(st, **fields):
    """st's stream with STREAMINFO fields overwritten: max_block (16 bits at byte 10), channels - 1 | bps - 1 (8 bits
    from bit 4 of byte 20)."""
    b = bytearray(st.blob)
    if "max_block" in fields:
        b[10:12] = fields["max_block"].to_bytes(2, "big")
    if "channels" in fields:
        v = int.from_bytes(b[20:22], "big") & ~0x0FF0 | (fields["channels"] - 1) << 9 | (fields["bps"] - 1) << 4
        b[20:22] = v.to_bytes(2, "big")
    return bytes(b)


def test_refusals():
    st = next(s for s in fm.valid_cases() if s.name == "metadata-all-blocks")
    first = len(st.blob) - sum(len(c) for c in st.frame_bytes)
    si = st.blob[4:42]   # STREAMINFO with its block header, not the last block
    for label, blob, zero in (
            ("len < 42", st.blob[:41], True),
            ("no marker", b"fLaX" + st.blob[4:], True),
            ("no STREAMINFO", b"fLaC" + fs.metadata_block(1, bytes(60), last=True) + st.blob[first:], True),
            ("STREAMINFO of 33 bytes", b"fLaC" + fs.metadata_block(0, st.blob[8:41], last=True) + st.blob[first:], True),
            ("max_block 0", _with_streaminfo(st, max_block=0), False),
            ("block list past the end", st.blob[:first - 1], False),
            ("block header past the end", b"fLaC" + si + bytes(2), False),
            ("no last block", b"fLaC" + si + fs.metadata_block(1, bytes(10)), False)):
        rc, info, off, sizes, n = _scan(blob)
        assert (rc, n) == (ERR_INVALID_ARG, 0), label
        assert model.scan(blob)[0] == ERR_INVALID_ARG, label
        assert (info.frames, info.bad_frames, info.decoded_samples, info.bad_crc16, info.md5_status) == (0,) * 5, label
        if zero:
            assert _all_zero(info), label
        else:   # the STREAMINFO fields are filled as soon as the block is seen
            want = dict(model.metadata(st.blob)[2], **({"max_block": 0} if label == "max_block 0" else {}))
            assert _streaminfo(info) == want, label
    # channels and bits per sample are 3 and 5 bits plus one: 8 and 32 are their largest values, and are accepted
    rc, info, _, _, _ = _scan(_with_streaminfo(st, channels=8, bps=32))
    assert rc == 0 and (info.channels, info.bits_per_sample) == (8, 32)


def test_count_query_capacity_and_null_arguments():
    from flac_codec_amd import _lib

    L = _lib.lib()
    st = next(s for s in fm.valid_cases() if s.name == "rice-k")
    nf = len(st.frame_bytes)
    assert nf == 15
    rc, info, off, sizes, n = _scan(st.blob, cap=nf + 3)   # more room than needed
    assert (rc, n, len(off), sizes) == (0, nf, nf, st.frame_sizes)
    for cap in (0, 1, nf - 1):   # too small: the count and `info`, nothing in the arrays (checked by _scan's sentinels)
        rc, info, _, _, n = _scan(st.blob, cap=cap)
        assert (rc, n, info.frames, info.decoded_samples) == (ERR_BUFFER_TOO_SMALL, nf, nf, sum(st.frame_sizes)), cap
        assert L.flacgpu_last_error() == b"output buffer too small"
    # one array alone
    info, n, only = _lib.StreamInfo(), C.c_uint32(0), np.zeros(nf, np.uint32)
    rc = L.flacgpu_scan_stream_host(st.blob, len(st.blob), C.byref(info), None, only.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    nf, C.byref(n))
    assert rc == 0 and only.tolist() == st.frame_sizes
    # NULL data, info or count
    assert L.flacgpu_scan_stream_host(None, 100, C.byref(info), None, None, 0, C.byref(n)) == ERR_INVALID_ARG
    assert L.flacgpu_scan_stream_host(st.blob, len(st.blob), None, None, None, 0, C.byref(n)) == ERR_INVALID_ARG
    assert L.flacgpu_scan_stream_host(st.blob, len(st.blob), C.byref(info), None, None, 0, None) == ERR_INVALID_ARG


def test_python_wrapper():
    from flac_codec_amd.gpu import GpuError, scan_stream_host

    st = next(s for s in fm.valid_cases() if s.name == "stereo-16")
    info, off, sizes = scan_stream_host(st.blob)
    assert info.frames == len(off) == len(sizes) == st.n_frames and sizes.tolist() == st.frame_sizes
    assert off[0] == len(st.blob) - sum(len(c) for c in st.frame_bytes)
    with pytest.raises(GpuError, match="no fLaC marker"):
        scan_stream_host(b"RIFF" + st.blob[4:])
