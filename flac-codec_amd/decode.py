"""Verification of FLAC files on the GPU, the counterpart of the reference's `decode::verify` (decode.rs:1282-1310):
every frame must be found and parse with a correct CRC-16, and the MD5 of the decoded samples is compared with
STREAMINFO's.  Many files go through one batch (gpu.decode_many).  FlacStreamReader / FrameBuf are the counterpart of
`decode::FlacStreamReader` (decode.rs:1099-1268): the reader of what encode.FlacStreamWriter writes.  FrameIterator, Frame
and the subframe and residual classes are the counterpart of `stream::FrameIterator` (stream.rs:1621-3079): the frames of
a file as they are coded, analysed in one GPU batch (gpu.analyze_many)."""
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


# ---- frame analysis: the reference's FrameIterator / Frame / Subframe / Residuals / ResidualPartition ------------------
class FrameHeader:
    """A frame's header (stream.rs FrameHeader).  channel_assignment is "INDEPENDENT", "LEFT_SIDE", "SIDE_RIGHT" or
    "MID_SIDE"; frame_number is the coded number: a frame number, or with blocking_strategy a sample number."""
    __slots__ = ("blocking_strategy", "block_size", "sample_rate", "channel_assignment", "channels", "bits_per_sample",
                 "frame_number")

    def __repr__(self):
        return "FrameHeader(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


class Standard:
    """A Rice-coded residual partition."""
    __slots__ = ("rice", "residuals")

    def __init__(self, rice, residuals):
        self.rice, self.residuals = rice, residuals


class Escaped:
    """A partition whose residuals are stored as plain signed values of escape_size bits."""
    __slots__ = ("escape_size", "residuals")

    def __init__(self, escape_size, residuals):
        self.escape_size, self.residuals = escape_size, residuals


class ConstantPartition:
    """An escaped partition of 0 bits per residual: partition_len zeros (ResidualPartition::Constant)."""
    __slots__ = ("partition_len",)

    def __init__(self, partition_len):
        self.partition_len = partition_len

    @property
    def residuals(self):
        return np.zeros(self.partition_len, dtype=np.int64)


class Residuals:
    """The residual section of a FIXED or LPC subframe: `partitions` is a list of Standard, Escaped and
    ConstantPartition.  A subframe of more than 64 partitions (`clipped`) lists the first 64."""
    __slots__ = ("_method", "_order", "partitions", "clipped")

    def __init__(self, method, order, partitions, clipped):
        self._method, self._order, self.partitions, self.clipped = method, order, partitions, clipped

    def coding_method(self):
        return "RICE2" if self._method else "RICE"

    def partition_order(self):
        return self._order


class Subframe:
    """Base of Constant, Verbatim, Fixed and Lpc; wasted_bps is common to all."""
    __slots__ = ("wasted_bps", "wide")
    name = ""

    def subframe_type(self):
        return self.name


class Constant(Subframe):
    __slots__ = ("block_size", "sample")
    name = "CONSTANT"


class Verbatim(Subframe):
    __slots__ = ("samples",)
    name = "VERBATIM"


class Fixed(Subframe):
    __slots__ = ("order", "warm_up", "residuals")
    name = "FIXED"


class Lpc(Subframe):
    __slots__ = ("order", "warm_up", "precision", "shift", "coefficients", "residuals")
    name = "LPC"


class Frame:
    """One frame as it is coded (stream.rs Frame): `header` and one subframe per channel.  Nothing is decoded: the
    subframes hold warm-up samples, predictor and residuals as the bit stream states them, after wasted-bit removal.
    `bits` is the frame's length, `status` the analysis' (bit 0: the frame does not parse -- subframes is then empty
    --, bit 1: its CRC-16 is wrong)."""
    __slots__ = ("header", "subframes", "bits", "status")


_RATES = (0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000)
_ASSIGNMENTS = {8: "LEFT_SIDE", 9: "SIDE_RIGHT", 10: "MID_SIDE"}


def _subframe(rec, row, n):
    """rec: a SUBFRAME_DTYPE record, row: its n row elements (exact integers)."""
    kind = int(rec["type"])
    s = (Constant, Verbatim, Fixed, Lpc)[kind]()
    s.wasted_bps = int(rec["wasted"])
    s.wide = bool(int(rec["reserved"][0]) & 1)
    if kind == 0:
        s.block_size, s.sample = n, int(row[0])
        return s
    if kind == 1:
        s.samples = row[:n]
        return s
    order = s.order = int(rec["order"])
    s.warm_up = row[:order]
    if kind == 3:
        s.precision, s.shift = int(rec["precision"]), int(rec["shift"])
        s.coefficients = [int(c) for c in rec["coeffs"][:order]]
    parts, at, plen = [], order, int(rec["part_len"])
    listed = min(int(rec["n_partitions"]), 64)
    for p in range(listed):
        count = plen - order if p == 0 else plen
        if int(rec["rice"][p]) != 0xFF:
            parts.append(Standard(int(rec["rice"][p]), row[at:at + count]))
        elif int(rec["escape_bits"][p]):
            parts.append(Escaped(int(rec["escape_bits"][p]), row[at:at + count]))
        else:
            parts.append(ConstantPartition(count))
        at += count
    s.residuals = Residuals(int(rec["coding_method"]), int(rec["partition_order"]), parts, bool(int(rec["reserved"][0]) & 2))
    return s


class FrameIterator:
    """Iterates over the frames of a FLAC file as they are coded, yielding (Frame, offset) with `offset` the frame's
    first byte in `data` -- the reference's stream::FrameIterator, with every frame of the file analysed in one GPU
    batch on first use (gpu.analyze_many).  data: the bytes of a .flac file, or with raw=True of a raw frame stream.
    A frame that holds a subframe wider than 32 bits (the side channel of 32-bit stereo) is parsed again on the host
    (gpu.analyze_frame_host), so that its values are exact."""

    def __init__(self, data, raw=False, device=-1):
        self._data = data.read() if hasattr(data, "read") else bytes(data)
        self._raw, self._device = raw, device
        self._frames = None

    def _analyse(self):
        data = self._data
        if self._raw:
            records, _ = gpu.scan_frames_host(data)
            offsets = [int(x) for x in records["byte_offset"]]
            rate0 = bps0 = 0
        else:
            info, offs, _ = gpu.scan_stream_host(data)
            offsets = [int(x) for x in offs]
            rate0, bps0 = int(info.sample_rate), int(info.bits_per_sample)
        an = gpu.analyze_many([data], raw=self._raw, rows=True, out="host", device=self._device)
        if an.frames.size != len(offsets):
            raise DecodeError("the device scan found %d frames, the host scan %d" % (an.frames.size, len(offsets)))
        out = []
        for f, at in enumerate(offsets):
            fa, subs = an.frames[f], an.subframes_of(f)
            n, hb, status = int(fa["block_size"]), int(fa["header_bytes"]), int(fa["status"])
            length = hb + (int(fa["plan"]["body_bits"]) + 7) // 8 + 2
            rows = [an.row(f, c) for c in range(len(subs))]
            if not status & 1 and any(int(s["reserved"][0]) & 1 for s in subs):
                fa, subs, rows = gpu.analyze_frame_host(data[at:at + length], bps0)
            h = FrameHeader()
            b = data[at:at + hb]
            h.blocking_strategy = bool(b[1] & 1)
            h.block_size = n
            rcode, code = b[2] & 15, int(fa["assignment_code"])
            tail = b[hb - 1 - (1 if rcode == 12 else 2 if rcode in (13, 14) else 0):hb - 1]
            h.sample_rate = (rate0 if rcode == 0 else _RATES[rcode] if rcode < 12 else
                             int.from_bytes(tail, "big") * {12: 1000, 13: 1, 14: 10}[rcode])
            h.channel_assignment = _ASSIGNMENTS.get(code, "INDEPENDENT")
            h.channels = int(fa["plan"]["channels"])
            h.bits_per_sample = (0, 8, 12, 0, 16, 20, 24, 32)[(b[3] >> 1) & 7] or bps0
            ones = 8 - (b[4] ^ 0xFF).bit_length()
            h.frame_number = b[4] & (0x7F >> ones)
            for i in range(1, ones):
                h.frame_number = h.frame_number << 6 | (b[4 + i] & 0x3F)
            fr = Frame()
            fr.header, fr.status = h, int(fa["status"])
            fr.bits = 8 * length if not status & 1 else 0
            fr.subframes = [] if status & 1 else [_subframe(s, rows[c], n) for c, s in enumerate(subs)]
            out.append((fr, at))
        self._frames = out

    def __iter__(self):
        if self._frames is None:
            self._analyse()
        return iter(self._frames)
