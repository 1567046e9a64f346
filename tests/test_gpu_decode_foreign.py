"""The FLAC decoders on hand-built streams this project's encoder never writes (_foreign_matrix.py, written by
_flacsyn.py; the PCM is the correct answer by construction, and test_flacsyn_oracle.py holds the writer to the CPU
oracle): one decode_many batch to host memory, the same streams in another order to device memory, and
flacgpu_decode_stream per stream must all give the PCM, its MD5 and a clean record.  Malformed subframes must be
counted as bad frames, identically by both decoders, without a write outside the output.

Without the 33-bit path of decode.inc (the parent's subframe decoder) the cases that fail here are frames of
"stereo-32", the 32-bit left/side, side/right and mid/side stream.  The parent's device code compiled for the host and
run over every frame of the matrix fails on 12 of that stream's 33 frames and on nothing else: all 11 mid/side frames
(10 decode to other samples, so wrong PCM and md5_status 0; the FIXED order 4 one is refused as a bad frame) and the
left/side frame with an order 32 LPC side channel (refused).  The other left/side and side/right frames pass there
because left - side and side + right are right modulo 2^32 and the 33-bit read happens to find its bits."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import _foreign_matrix as fm
from _pcm import le_bytes as _le_bytes

pytestmark = pytest.mark.gpu

INFO_FIELDS = ["sample_rate", "channels", "bits_per_sample", "min_block", "max_block", "frames", "bad_frames",
               "bad_crc16", "total_samples", "decoded_samples", "md5", "decoded_md5", "md5_status"]


def _single(blob):
    """flacgpu_decode_stream on one stream: (rc, StreamInfo, interleaved samples)."""
    from flac_codec_amd import _lib

    L = _lib.lib()
    info = _lib.StreamInfo()
    blob = bytes(blob)
    rc = L.flacgpu_decode_stream(blob, len(blob), -1, None, 0, C.byref(info))
    if rc or info.frames == 0:
        return rc, info, np.zeros(0, np.int32)
    out = np.empty(info.decoded_samples * info.channels, dtype=np.int32)
    rc = L.flacgpu_decode_stream(blob, len(blob), -1, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size,
                                 C.byref(info))
    return rc, info, out


def _val(info, f):
    v = getattr(info, f)
    return bytes(v) if f in ("md5", "decoded_md5") else v


def _check(st, rc, info, samples, how):
    """Everything the issue requires of one valid stream's result."""
    tag = f"{st.name} ({how})"
    assert rc == 0, tag
    assert (info.bad_frames, info.bad_crc16) == (0, 0), tag
    assert info.frames == st.n_frames, tag
    assert np.array_equal(np.asarray(samples).reshape(-1), st.pcm), tag
    digest = hashlib.md5(_le_bytes(st.pcm, st.bps)).digest()
    assert digest == st.digest and bytes(info.decoded_md5) == digest, tag
    assert info.md5_status == st.md5_status, tag


def test_valid_matrix_in_one_batch_to_host():
    from flac_codec_amd.gpu import decode_many

    cases = fm.valid_cases()
    flat, streams = decode_many([s.blob for s in cases], out="host")
    assert len(streams) == len(cases)
    for st, s in zip(cases, streams):
        _check(st, s.rc, s.info, s.pcm, "decode_many, host")
    assert flat.size == sum(s.pcm.size for s in cases)


def test_valid_matrix_permuted_to_device():
    """Another fixed order: the lanes of a wave get other neighbours; per stream the result is the same."""
    from flac_codec_amd.gpu import decode_many

    cases = fm.valid_cases()
    order = np.random.default_rng(4321).permutation(len(cases))
    assert not np.array_equal(order, np.arange(len(cases)))
    _, streams = decode_many([cases[i].blob for i in order], out="device")
    for i, s in zip(order, streams):
        _check(cases[i], s.rc, s.info, s.pcm.cpu().numpy(), "decode_many, permuted, device")


def test_valid_matrix_stream_by_stream():
    for st in fm.valid_cases():
        rc, info, out = _single(st.blob)
        _check(st, rc, info, out, "flacgpu_decode_stream")


def test_invalid_subframes_are_refused_without_a_stray_write():
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    bad = fm.invalid_cases()
    good = [s for s in fm.valid_cases() if s.name in ("lpc8", "stereo-32", "channels-3", "wasted-16")]
    assert len(good) == 4
    batch, kinds = [], []
    for k, (reason, st) in enumerate(bad):   # valid streams between the malformed ones
        batch.append(st)
        kinds.append(reason)
        if k % 3 == 0:
            batch.append(good[(k // 3) % 4])
            kinds.append(None)
    singles = [_single(st.blob) for st in batch]
    dec = Decoder(0)
    try:
        recs, total = dec.scan([st.blob for st in batch])
        guard, sentinel = 64, -0x5A5A5A5B
        buf = torch.full((guard + total + guard,), sentinel, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        dec.decode(buf.data_ptr() + 4 * guard, total, _lib.DECODE_OUT_DEVICE, recs)
        got = buf.cpu().numpy()
    finally:
        dec.close()
    assert (got[:guard] == sentinel).all() and (got[guard + total:] == sentinel).all()
    for st, reason, rec, (rc, sinfo, sout) in zip(batch, kinds, recs, singles):
        assert rec.rc == rc == 0, st.name
        diff = {f: (_val(rec.info, f), _val(sinfo, f)) for f in INFO_FIELDS
                if _val(rec.info, f) != _val(sinfo, f) and not (reason and f in ("decoded_md5", "md5_status"))}
        assert not diff, (st.name, diff)   # (the samples of a frame that does not decode are undefined: so is the MD5)
        mine = got[guard + rec.out_offset:guard + rec.out_offset + rec.info.decoded_samples * rec.info.channels]
        if reason is None:   # untouched by its neighbours
            _check(st, rec.rc, rec.info, mine, "between malformed streams")
        else:
            assert rec.info.frames == 3 and rec.info.bad_frames == 1 and rec.info.bad_crc16 == 0, reason
            assert rec.info.md5_status == 0, reason
            # the valid frames around the malformed one decode
            n_bad = st.pcm.size - 2 * 192
            assert np.array_equal(mine[:192], st.pcm[:192]) and np.array_equal(mine[192 + n_bad:], st.pcm[192 + n_bad:])
            assert np.array_equal(sout[:192], st.pcm[:192]) and np.array_equal(sout[192 + n_bad:], st.pcm[192 + n_bad:])


def test_three_scans_agree_on_the_matrix_and_on_damaged_streams():
    """flacgpu_scan_stream_host (no device), flacgpu_decoder_scan's records before any decode (metadata on the host, frames
    found on the device) and flacgpu_decode_stream give the same rc, frames, decoded_samples, scan-time bad_frames and
    STREAMINFO fields, for the matrix and for the damaged streams of test_stream_scan.py.  flacgpu_decode_stream adds the
    frames that do not decode to bad_frames: there are none where every frame the scan kept is a valid frame of the matrix
    byte for byte, and elsewhere at most as many as the other frames kept."""
    import _scan_model as model
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    L = _lib.lib()
    blobs = [(st.name, st.blob) for st in fm.valid_cases()] + [(r, st.blob) for r, st in fm.invalid_cases()] + \
        list(model.damaged_cases())
    pristine = {c for st in fm.valid_cases() for c in st.frame_bytes}
    dec = Decoder(0)
    try:
        recs, _ = dec.scan([b for _, b in blobs])
    finally:
        dec.close()
    scan_fields = ["frames", "decoded_samples", "bad_frames"] + model.STREAMINFO_FIELDS
    for (label, blob), rec in zip(blobs, recs):
        info, n = _lib.StreamInfo(), C.c_uint32(0)
        rc = L.flacgpu_scan_stream_host(blob, len(blob), C.byref(info), None, None, 0, C.byref(n))
        off = np.zeros(n.value, np.uint64)
        assert rc == L.flacgpu_scan_stream_host(blob, len(blob), C.byref(info), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                None, n.value, C.byref(n)), label
        host = {f: _val(info, f) for f in scan_fields}
        assert (rec.rc, {f: _val(rec.info, f) for f in scan_fields}) == (rc, host), label
        src, sinfo, _ = _single(blob)
        single = {f: _val(sinfo, f) for f in scan_fields}
        ends = off.tolist()[1:] + [len(blob) if not info.bad_frames else None]   # (lost sync: the last end is not reported)
        other = sum(1 for a, b in zip(off.tolist(), ends)
                    if (blob[a:b] not in pristine if b else not any(blob.startswith(c, a) for c in pristine)))
        extra = single.pop("bad_frames") - host.pop("bad_frames")
        assert (src, single) == (rc, host) and 0 <= extra <= other, label
