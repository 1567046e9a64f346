"""Verification of FLAC files on the GPU, the counterpart of the reference's `decode::verify` (decode.rs:1282-1310):
every frame must be found and parse with a correct CRC-16, and the MD5 of the decoded samples is compared with
STREAMINFO's.  Many files go through one batch (gpu.decode_many).  FlacStreamReader / FrameBuf are the counterpart of
`decode::FlacStreamReader` (decode.rs:1099-1268): the reader of what encode.FlacStreamWriter writes."""
import enum
import os

import numpy as np

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
    that one bad file does not hide the others).  The readable files are verified in one GPU batch.  An entry may also
    be a stream that already lies in device memory (a 1-D uint8 CUDA tensor, gpu.Decoder.scan): then every entry must
    be one, and none is read from disk."""
    blobs, results = [], []
    for p in paths:
        if gpu.is_device_blob(p):
            blobs.append(p)
            results.append(None)
            continue
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


class FrameBuf:
    """One decoded frame of a raw frame stream (decode.rs:1099 FrameBuf): `samples` is interleaved int32
    [block_size * channels], with the parameters its own header gave."""
    __slots__ = ("samples", "sample_rate", "channels", "bits_per_sample")

    def __init__(self, samples, sample_rate, channels, bits_per_sample):
        self.samples = np.asarray(samples, dtype=np.int32)
        self.sample_rate, self.channels, self.bits_per_sample = int(sample_rate), int(channels), int(bits_per_sample)

    def __eq__(self, other):
        return (isinstance(other, FrameBuf) and np.array_equal(self.samples, other.samples) and
                (self.sample_rate, self.channels, self.bits_per_sample) ==
                (other.sample_rate, other.channels, other.bits_per_sample))

    def __repr__(self):
        return "FrameBuf(%d samples, %d Hz, %d channel(s), %d bits)" % (
            self.samples.size, self.sample_rate, self.channels, self.bits_per_sample)


class FlacStreamReader:
    """Reads the frames of a raw frame stream -- what encode.FlacStreamWriter writes: bare subset frames, no fLaC marker,
    no STREAMINFO -- one FrameBuf per read() (decode.rs:1142 FlacStreamReader).  The whole input is decoded in one GPU
    batch on first use.  Frames are found by the rule of DESIGN.md "Raw frame streams": bytes that belong to no whole
    frame are skipped, where the reference reports an error at the point of damage.  speculative=True ends a frame that
    no header ends by its own bits (FLACGPU_SCAN_SPECULATIVE): as the reference does, a frame is then decoded from its
    own bits and kept when the header behind it is damaged or cut off."""

    def __init__(self, data, device=-1, speculative=False):
        self._data = data.read() if hasattr(data, "read") else bytes(data)
        self._device = device
        self._speculative = speculative
        self._frames = None
        self._next = 0

    def _decode(self):
        if self._frames is None:
            self._pcm, self._frames, raw = gpu.decode_frames([self._data], device=self._device, out="host",
                                                              speculative=self._speculative)
            self._skipped_bytes, self._gaps = int(raw[0].skipped_bytes), int(raw[0].gaps)
            self._data = None

    @property
    def skipped_bytes(self):
        """Bytes of the input that belong to no whole frame (decodes the input on first use)."""
        self._decode()
        return self._skipped_bytes

    @property
    def gaps(self):
        """Maximal runs of skipped bytes: leading, between frames, trailing (decodes the input on first use)."""
        self._decode()
        return self._gaps

    def read(self):
        """The next FrameBuf.  Raises DecodeError for a frame that was found but does not decode (the read after that
        goes on with the next frame) and EOFError behind the last frame (decode.rs:1195)."""
        self._decode()
        if self._next >= len(self._frames):
            raise EOFError("no more frames")
        f = self._frames[self._next]
        self._next += 1
        if f["status"]:
            raise DecodeError("the frame at byte %d %s" % (f["byte_offset"], " and ".join(
                w for bit, w in ((1, "does not parse"), (2, "has a wrong CRC-16")) if f["status"] & bit)))
        at, count = int(f["out_offset"]), int(f["block_size"]) * int(f["channels"])
        return FrameBuf(self._pcm[at:at + count], f["sample_rate"], f["channels"], f["bits_per_sample"])

    def __iter__(self):
        return self

    def __next__(self):
        try:
            return self.read()
        except EOFError:
            raise StopIteration from None


class FlacChunkReader:
    """One raw frame stream that arrives in pieces cut anywhere -- a socket, a file read piece by piece, the writes of a
    stream writer --, over gpu.DecoderSession (DESIGN.md 4b "Decoder sessions").  feed(data) returns the frames the bytes
    so far decide, a list of FrameBuf: without flush a frame comes out once the header behind it has arrived;
    flush=True says that the bytes so far end on a frame boundary and decides everything.  finish() returns what is
    left.  No frame may be longer than max_frame_bytes (16 .. 2^22).  A frame that was found but does not decode raises
    DecodeError; the frames of that feed are lost with it."""

    def __init__(self, device=-1, max_frame_bytes=1 << 20):
        self._session = gpu.DecoderSession(1, max_frame_bytes, device)
        self.skipped_bytes = self.gaps = 0   # so far: bytes in no whole frame, and their maximal runs

    def _frames(self, raw):
        self.skipped_bytes, self.gaps = int(raw[0].skipped_bytes), int(raw[0].gaps)
        pcm, frames = self._session.decode_frames(out="host")
        out = []
        for f in frames:
            if f["status"]:
                raise DecodeError("the frame at byte %d %s" % (f["byte_offset"], " and ".join(
                    w for bit, w in ((1, "does not parse"), (2, "has a wrong CRC-16")) if f["status"] & bit)))
            at, count = int(f["out_offset"]), int(f["block_size"]) * int(f["channels"])
            out.append(FrameBuf(pcm[at:at + count], f["sample_rate"], f["channels"], f["bits_per_sample"]))
        return out

    def feed(self, data, flush=False):
        return self._frames(self._session.feed([data], flush)[1])

    def finish(self):
        return self._frames(self._session.finish()[1])

    @property
    def pending(self):
        """Bytes fed and not decided yet."""
        return self._session.pending()[0][0]

    def close(self):
        self._session.close()


class FlacFileChunkReader:
    """One regular .flac file that arrives in pieces cut anywhere -- inside the marker, the metadata or a frame --, over
    a container gpu.DecoderSession (DESIGN.md 4b "Container sessions").  feed(data) returns the PCM the bytes so far
    decide, an int32 array [samples, channels] (no row while the metadata is under way; a frame comes out once the header
    behind it has arrived); finish() returns the last samples and settles `info` and `md5_ok`, what `flac -t` would say.
    No frame may be longer than max_frame_bytes (16 .. 2^22).  Once the stream loses synchronisation nothing more is
    decoded (info.bad_frames is 1 after finish)."""

    def __init__(self, device=-1, max_frame_bytes=1 << 20):
        self._session = gpu.DecoderSession(1, max_frame_bytes, device, container=True)
        self.info = None      # the file's StreamInfo: STREAMINFO's fields once the first frame is out, all of it after finish
        self.md5_ok = None    # after finish: True / False, None when STREAMINFO holds no MD5 or the file is refused
        self.rc = None        # after finish: 0, or what the one-shot decode returns for a file it refuses

    def _pcm(self):
        _, streams = self._session.decode(out="host", verify_md5=True)
        s = streams[0]
        if s.rc:
            return np.zeros((0, self.info.channels if self.info else 0), dtype=np.int32)
        if self.info is None:
            self.info = s.info
        return s.pcm.copy()

    def feed(self, data):
        self._session.feed([data])
        return self._pcm()

    def finish(self):
        self._session.finish()
        pcm = self._pcm()
        v = self._session.verdict()[0]
        self.rc, self.info = v.rc, v.info
        self.md5_ok = {0: False, 1: True}.get(v.info.md5_status) if v.rc == 0 else None
        return pcm

    @property
    def pending(self):
        """Bytes fed and not decided yet."""
        return self._session.pending()[0][0]

    def close(self):
        self._session.close()
