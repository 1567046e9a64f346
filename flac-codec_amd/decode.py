"""Verification of FLAC files on the GPU, the counterpart of the reference's `decode::verify` (decode.rs:1282-1310):
every frame must be found and parse with a correct CRC-16, and the MD5 of the decoded samples is compared with
STREAMINFO's.  Many files go through one batch (gpu.decode_many)."""
import enum
import os

from . import gpu


class Verified(enum.Enum):
    MD5_MATCH = "md5_match"
    MD5_MISMATCH = "md5_mismatch"
    NO_MD5 = "no_md5"


class DecodeError(Exception):
    """A stream that is not FLAC, has no usable STREAMINFO, or holds a frame that could not be found or decoded."""


def _result(rec):
    if rec.rc != 0:
        return DecodeError("not a FLAC stream or no usable STREAMINFO (rc %d)" % rec.rc)
    info = rec.info
    if info.bad_frames or info.bad_crc16:
        return DecodeError("%d bad frame(s), %d CRC-16 mismatch(es) after %d good frame(s)"
                           % (info.bad_frames, info.bad_crc16, info.frames))
    return {1: Verified.MD5_MATCH, 0: Verified.MD5_MISMATCH, 2: Verified.NO_MD5}[info.md5_status]


def verify_many(paths, device=-1):
    """One result per path, in order: a Verified, or the DecodeError / OSError of that file (returned, not raised, so
    that one bad file does not hide the others).  The readable files are verified in one GPU batch."""
    blobs, results = [], []
    for p in paths:
        try:
            with open(os.fspath(p), "rb") as f:
                blobs.append(f.read())
            results.append(None)
        except OSError as e:
            results.append(e)
    _, recs = gpu.decode_many(blobs, device=device, out="device", verify_md5=True)
    it = iter(recs)
    return [r if r is not None else _result(next(it)) for r in results]


def verify(path, device=-1):
    """Verified.MD5_MATCH / MD5_MISMATCH / NO_MD5; raises DecodeError (or OSError) for a file that does not decode."""
    r = verify_many([path], device=device)[0]
    if isinstance(r, Exception):
        raise r
    return r
