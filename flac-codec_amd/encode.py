"""Python mirror of the reference's `flac_codec::encode` module surface
(/root/reference/src/encode.rs): `Options`, `Window`, `FlacSampleWriter`, `FlacByteWriter`,
`FlacChannelWriter`, `FlacStreamWriter` -- same names, argument meaning and error behaviour,
so the parity tests read like the reference's own tests (tests/format.rs).

All work is done by libflacenc_amd.so (C ABI in include/flacenc_stream.h, gfx950 kernels
behind include/flacenc_gpu.h).  There is no CPU fallback.
"""
import ctypes as C
import threading
import io
import os

import numpy as np

from . import _lib


# --------------------------------------------------------------------------------------
# errors: the reference's `Error` (src/lib.rs:59-193) and `OptionsError` (encode.rs:1676-1698)
# --------------------------------------------------------------------------------------
class Error(Exception):
    """flac_codec::Error"""
    code = None


class OptionsError(Exception):
    """flac_codec::encode::OptionsError"""
    code = None


def _mk(name, base, code):
    cls = type(name, (base,), {"code": code})
    return cls


InvalidBlockSize = _mk("InvalidBlockSize", OptionsError, -101)
InvalidLpcOrder = _mk("InvalidLpcOrder", OptionsError, -102)
InvalidMaxPartitions = _mk("InvalidMaxPartitions", OptionsError, -103)
ExcessivePadding = _mk("ExcessivePadding", OptionsError, -104)
InvalidBitsPerSample = _mk("InvalidBitsPerSample", Error, -110)
InvalidSampleRate = _mk("InvalidSampleRate", Error, -111)
ExcessiveChannels = _mk("ExcessiveChannels", Error, -112)
SamplesNotDivisibleByChannels = _mk("SamplesNotDivisibleByChannels", Error, -113)
InvalidTotalSamples = _mk("InvalidTotalSamples", Error, -114)
InvalidTotalBytes = _mk("InvalidTotalBytes", Error, -115)
ExcessiveTotalSamples = _mk("ExcessiveTotalSamples", Error, -116)
SampleCountMismatch = _mk("SampleCountMismatch", Error, -117)
NoSamples = _mk("NoSamples", Error, -118)
ExcessiveFrameNumber = _mk("ExcessiveFrameNumber", Error, -119)
ChannelCountMismatch = _mk("ChannelCountMismatch", Error, -120)
ChannelLengthMismatch = _mk("ChannelLengthMismatch", Error, -121)
NonSubsetSampleRate = _mk("NonSubsetSampleRate", Error, -122)
NonSubsetBitsPerSample = _mk("NonSubsetBitsPerSample", Error, -123)
Io = _mk("Io", Error, -130)
InvalidArgument = _mk("InvalidArgument", Error, -140)
Finalized = _mk("Finalized", Error, -141)
GpuError = _mk("GpuError", Error, -150)
Unsupported = _mk("Unsupported", Error, -151)

_BY_CODE = {c.code: c for c in list(globals().values())
            if isinstance(c, type) and issubclass(c, (Error, OptionsError)) and c.code is not None}


def _check(rc):
    if rc == 0:
        return
    msg = _stream_lib().flacenc_last_error().decode(errors="replace")
    raise _BY_CODE.get(rc, Error)(f"{_BY_CODE.get(rc, Error).__name__} ({rc}) {msg}".strip())


# --------------------------------------------------------------------------------------
# C structs of include/flacenc_stream.h
# --------------------------------------------------------------------------------------
class _COptions(C.Structure):
    _fields_ = [
        ("block_size", C.c_uint32),
        ("max_partition_order", C.c_uint32),
        ("max_lpc_order", C.c_uint32),
        ("mid_side", C.c_uint8),
        ("exhaustive_channel_correlation", C.c_uint8),
        ("window_kind", C.c_uint8),
        ("reserved0", C.c_uint8),
        ("window_param", C.c_float),
        ("padding", C.c_int64),
        ("seektable_mode", C.c_int32),
        ("seektable_value", C.c_uint32),
        ("batch_frames", C.c_uint32),
        ("device", C.c_int32),
        ("pack_threads", C.c_uint32),
        ("host_pack", C.c_uint32),
        ("vendor_string", C.c_char_p),
        ("comment_fields", C.POINTER(C.c_char_p)),
        ("n_comment_fields", C.c_uint32),
        ("pipeline_depth", C.c_uint32),
        ("shared_md5", C.c_uint32),
    ]


_WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)
_SEEK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)


class _CSink(C.Structure):
    _fields_ = [("write", _WRITE_FN), ("seek", _SEEK_FN), ("user", C.c_void_p), ("start", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [
        ("frames", C.c_uint64),
        ("samples_per_channel", C.c_uint64),
        ("bytes_written", C.c_uint64),
        ("min_frame_size", C.c_uint32),
        ("max_frame_size", C.c_uint32),
        ("md5", C.c_uint8 * 16),
        ("gpu_ms", C.c_double),
        ("pack_ms", C.c_double),
        ("md5_ms", C.c_double),
    ]


class _CJob(C.Structure):
    _fields_ = [
        ("samples", C.POINTER(C.c_int32)),
        ("count", C.c_size_t),
        ("sample_rate", C.c_uint32),
        ("bits_per_sample", C.c_uint32),
        ("channels", C.c_uint32),
        ("reserved", C.c_uint32),
        ("out", C.c_void_p),
        ("out_cap", C.c_size_t),
        ("out_len", C.c_size_t),
        ("status", C.c_int32),
        ("reserved1", C.c_int32),
        ("elapsed_ms", C.c_double),
        ("pack_ms", C.c_double),
        ("gpu_ms", C.c_double),
        ("md5_ms", C.c_double),
        ("start_ms", C.c_double),
    ]


_bound = False
_bind_lock = threading.Lock()


def _stream_lib():
    """The library with the stream-writer entry points bound (once, under a lock: a thread must
    never call through a function whose restype is still the default int)."""
    global _bound
    L = _lib.lib()
    if _bound:
        return L
    with _bind_lock:
        if _bound:
            return L
        vp, ip = C.c_void_p, C.POINTER(C.c_int32)
        po = C.POINTER(_COptions)
        ps = C.POINTER(_CSink)
        for n in ("flacenc_options_default", "flacenc_options_fast", "flacenc_options_best"):
            getattr(L, n).argtypes = [po]
            getattr(L, n).restype = None
        L.flacenc_options_validate.argtypes = [po]
        L.flacenc_sample_writer_new.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                                C.c_uint64, ps, C.POINTER(vp)]
        L.flacenc_byte_writer_new.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                              C.c_uint64, C.c_int, ps, C.POINTER(vp)]
        L.flacenc_channel_writer_new.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                                 C.c_uint64, ps, C.POINTER(vp)]
        L.flacenc_write_samples.argtypes = [vp, ip, C.c_size_t]
        L.flacenc_write_bytes.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.flacenc_write_channels.argtypes = [vp, C.POINTER(ip), C.c_uint32, C.c_size_t]
        L.flacenc_finalize.argtypes = [vp]
        L.flacenc_writer_free.argtypes = [vp]
        L.flacenc_writer_free.restype = None
        L.flacenc_writer_data.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.flacenc_writer_data.restype = C.POINTER(C.c_uint8)
        L.flacenc_writer_stats.argtypes = [vp, C.POINTER(Stats)]
        L.flacenc_stream_writer_new.argtypes = [po, ps, C.POINTER(vp)]
        L.flacenc_stream_writer_write.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, ip, C.c_size_t]
        L.flacenc_stream_writer_data.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.flacenc_stream_writer_data.restype = C.POINTER(C.c_uint8)
        L.flacenc_stream_writer_free.argtypes = [vp]
        L.flacenc_stream_writer_free.restype = None
        L.flacenc_last_error.restype = C.c_char_p
        L.flacenc_encode_many.argtypes = [po, C.POINTER(_CJob), C.c_size_t, C.c_uint32]
        L.flacenc_encode_many_devices.argtypes = [po, C.POINTER(_CJob), C.c_size_t, C.c_uint32, C.POINTER(C.c_int),
                                                  C.c_uint32]
        L.flacenc_encode_many_coalesced.argtypes = [po, C.POINTER(_CJob), C.c_size_t, C.c_uint32]
        pf = C.POINTER(_lib.OutFormat)
        L.flacenc_device_batch_plan.argtypes = [po, pf, C.c_uint32, C.c_uint32, C.POINTER(_lib.DeviceJob), C.c_size_t,
                                                C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.flacenc_encode_many_device.argtypes = [po, vp, pf, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.POINTER(_lib.DeviceJob), C.c_size_t, C.c_uint32, vp]
        L.flacenc_device_out_plan.argtypes = [po, pf, C.c_uint32, C.c_uint32, C.POINTER(_lib.DeviceOutJob), C.c_size_t,
                                              C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.flacenc_encode_many_device_out.argtypes = [po, vp, pf, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.POINTER(_lib.DeviceOutJob), C.c_size_t, vp, C.c_size_t, C.c_uint32, vp]
        L.flacenc_device_session_plan.argtypes = [po, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint64, C.c_uint32,
                                                  C.POINTER(C.c_size_t)]
        L.flacenc_device_session_open.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_size_t,
                                                  C.c_uint64, C.c_uint32, C.POINTER(vp)]
        L.flacenc_device_session_open_ex.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                                     C.POINTER(C.c_uint8), C.c_size_t, C.c_uint64, C.c_uint32, C.POINTER(vp)]
        L.flacenc_device_session_header_len.argtypes = [vp, C.c_size_t]
        L.flacenc_device_session_header_len.restype = C.c_size_t
        L.flacenc_device_session_write.argtypes = [vp, vp, pf, C.POINTER(_lib.SessionChunk), vp]
        L.flacenc_device_session_finalize.argtypes = [vp, C.POINTER(_lib.SessionFinal)]
        L.flacenc_device_session_close.argtypes = [vp]
        L.flacenc_device_session_close.restype = None
        L.flacenc_device_stream_writer_plan.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32,
                                                        C.POINTER(C.c_size_t)]
        L.flacenc_device_stream_writer_open.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32,
                                                        C.POINTER(C.c_uint64), C.POINTER(vp)]
        L.flacenc_device_stream_writer_write.argtypes = [vp, vp, pf, C.POINTER(_lib.SessionChunk), vp]
        L.flacenc_device_stream_writer_frame_number.argtypes = [vp, C.c_size_t]
        L.flacenc_device_stream_writer_frame_number.restype = C.c_uint64
        L.flacenc_device_stream_writer_close.argtypes = [vp]
        L.flacenc_device_stream_writer_close.restype = None
        L.flacenc_stream_header_unknown_total.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64,
                                                          C.POINTER(C.c_uint32), C.c_uint32, vp, C.c_size_t,
                                                          C.POINTER(C.c_size_t)]
        L.flacenc_release_pools.argtypes = []
        L.flacenc_release_pools.restype = None
        L.flacenc_device_tail_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.flacenc_device_tail_stats.restype = None
        L.flacgpu_place_runs_host.argtypes = [C.POINTER(_lib.PlaceRun), C.c_uint32]
        L.flacgpu_place_workgroup.restype = C.c_uint32
        L.flacenc_ingest_sample.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]
        L.flacenc_ingest_sample.restype = C.c_int32
        L.flacenc_worst_case_bytes.restype = C.c_size_t
        L.flacenc_worst_case_bytes.argtypes = [po, C.c_uint32, C.c_uint32, C.c_uint64]
        _bound = True
    return L


# --------------------------------------------------------------------------------------
# Window (encode.rs:1711-1720) and Options (encode.rs:1361-1672)
# --------------------------------------------------------------------------------------
class Window:
    """The method to use for windowing the input signal (encode.rs:1713)."""

    def __init__(self, kind, param=0.0):
        self.kind, self.param = kind, float(param)

    Rectangle = None
    Hann = None

    @staticmethod
    def Tukey(p):
        return Window(2, p)

    def __repr__(self):
        return {0: "Rectangle", 1: "Hann"}.get(self.kind, f"Tukey({self.param})")


Window.Rectangle = Window(0)
Window.Hann = Window(1)


class Options:
    """FLAC encoding options (encode.rs:1363).  Builder methods return `self` and raise the
    `OptionsError` the reference's builder returns."""

    def __init__(self, preset="default"):
        self._c = _COptions()
        getattr(_stream_lib(), "flacenc_options_" + preset)(C.byref(self._c))
        self._clobber = False
        self._vendor = None      # VORBIS_COMMENT vendor string (None = reference default)
        self._fields = None      # list of "NAME=value" strings, None = no block

    # presets, encode.rs:1376-1408, 1635-1657
    @classmethod
    def default(cls):
        return cls("default")

    @classmethod
    def fast(cls):
        return cls("fast")

    @classmethod
    def best(cls):
        return cls("best")

    def block_size(self, block_size):  # encode.rs:1418
        if block_size < 16 or block_size > 65535:
            raise InvalidBlockSize("block size must be >= 16")
        self._c.block_size = block_size
        return self

    def max_lpc_order(self, max_lpc_order):  # encode.rs:1430; None = no LPC subframes
        if max_lpc_order is None:
            self._c.max_lpc_order = 0
        else:
            if not 0 < max_lpc_order <= 32:
                raise InvalidLpcOrder("maximum LPC order must be <= 32")
            self._c.max_lpc_order = max_lpc_order
        return self

    def max_partition_order(self, max_partition_order):  # encode.rs:1447
        if not 0 <= max_partition_order <= 15:
            raise InvalidMaxPartitions("max partition order must be <= 15")
        self._c.max_partition_order = max_partition_order
        return self

    def mid_side(self, mid_side):  # encode.rs:1460
        self._c.mid_side = int(bool(mid_side))
        return self

    def window(self, window):  # encode.rs:1465
        self._c.window_kind, self._c.window_param = window.kind, window.param
        return self

    def fast_channel_correlation(self, fast):  # encode.rs:1472
        self._c.exhaustive_channel_correlation = int(not fast)
        return self

    def padding(self, size):  # encode.rs:1486
        if size < 0 or size >= (1 << 24):
            raise ExcessivePadding("padding size is too large for block")
        self._c.padding = size
        return self

    def no_padding(self):  # encode.rs:1505
        self._c.padding = 0
        return self

    def tag(self, field, value):  # encode.rs:1513: adds NAME=value, creating the block if needed
        if "=" in field:
            raise ValueError("field must not contain '='")  # the reference panics (metadata/mod.rs:2357)
        if self._fields is None:
            self._fields = []
        self._fields.append(f"{field}={value}")
        return self

    def comment(self, fields, vendor_string=None):  # encode.rs:1525: replaces the whole block
        self._fields = list(fields)
        self._vendor = vendor_string
        return self

    def _c_options(self):
        """The C struct with the VORBIS_COMMENT pointers filled in (kept alive on self)."""
        if self._fields is None:
            self._c.vendor_string, self._c.n_comment_fields = None, 0
            self._c.comment_fields = None
        else:
            self._keep = (C.c_char_p * max(len(self._fields), 1))(*[f.encode() for f in self._fields])
            self._c.comment_fields = self._keep
            self._c.n_comment_fields = len(self._fields)
            self._c.vendor_string = (self._vendor or "flac-codec 1.3.2").encode()
        return self._c

    def seektable_seconds(self, seconds):  # encode.rs:1568
        self._c.seektable_mode, self._c.seektable_value = (1, seconds & 0xFF) if seconds else (0, 0)
        return self

    def seektable_frames(self, frames):  # encode.rs:1579
        self._c.seektable_mode, self._c.seektable_value = (2, frames) if frames else (0, 0)
        return self

    def no_seektable(self):  # encode.rs:1585
        self._c.seektable_mode = 0
        return self

    def overwrite(self):  # encode.rs:1627
        self._clobber = True
        return self

    # execution knobs without a reference counterpart
    def batch_frames(self, n):
        self._c.batch_frames = n
        return self

    def device(self, ordinal):
        self._c.device = ordinal
        return self

    def pack_threads(self, n):
        self._c.pack_threads = n
        return self

    def pipeline_depth(self, n):
        """Batches in flight per writer (each on its own context / HIP stream / pinned staging)."""
        self._c.pipeline_depth = n
        return self

    def shared_md5(self, on=True):
        """Hash this stream on the shared multi-stream MD5 engines (many concurrent writers)."""
        self._c.shared_md5 = int(bool(on))
        return self

    def host_pack(self, on=True):
        """Keep Rice bit-packing + CRC on the host (default: assembled on the GPU)."""
        self._c.host_pack = int(bool(on))
        return self

    def _open(self, path):  # Options::create, encode.rs:1660-1671
        return open(path, "wb" if self._clobber else "xb")


# --------------------------------------------------------------------------------------
# writers
# --------------------------------------------------------------------------------------
class _Writer:
    def __init__(self, writer):
        self._h = C.c_void_p(None)
        self._py = writer
        self._sink = None
        self._closed = False
        if writer is not None:
            start = writer.tell()

            def _w(_user, data, n):
                try:
                    writer.write(C.string_at(data, n))
                    return 0
                except Exception:
                    return 1

            def _s(_user, off):
                try:
                    writer.seek(off)
                    return 0
                except Exception:
                    return 1

            self._cb = (_WRITE_FN(_w), _SEEK_FN(_s))  # keep alive
            self._sink = _CSink(self._cb[0], self._cb[1], None, start)

    def _sink_ptr(self):
        return C.byref(self._sink) if self._sink is not None else None

    def finalize(self):
        """Finalizes the stream (encode.rs:624): last partial block, SEEKTABLE, STREAMINFO."""
        _check(_stream_lib().flacenc_finalize(self._h))

    def getvalue(self):
        """Bytes of the stream when no writer object was given (memory sink)."""
        n = C.c_size_t(0)
        p = _stream_lib().flacenc_writer_data(self._h, C.byref(n))
        return C.string_at(p, n.value) if p else b""

    def stats(self):
        s = Stats()
        _check(_stream_lib().flacenc_writer_stats(self._h, C.byref(s)))
        return s

    def close(self):
        """Drop: finalize silently and free (encode.rs:399-405)."""
        if self._h:
            _stream_lib().flacenc_writer_free(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _total(total):
    return (0, 0) if total is None else (1, int(total))


class FlacSampleWriter(_Writer):
    """A FLAC writer which accepts samples as signed integers (encode.rs:461)."""

    def __init__(self, writer, options, sample_rate, bits_per_sample, channels, total_samples=None):
        super().__init__(writer)
        ht, tv = _total(total_samples)
        _check(_stream_lib().flacenc_sample_writer_new(
            C.byref(options._c_options()), sample_rate, bits_per_sample, channels, ht, tv, self._sink_ptr(),
            C.byref(self._h)))

    @classmethod
    def new_cdda(cls, writer, options, total_samples=None):  # encode.rs:535
        return cls(writer, options, 44100, 16, 2, total_samples)

    @classmethod
    def create(cls, path, options, sample_rate, bits_per_sample, channels, total_samples=None):
        return cls(options._open(path), options, sample_rate, bits_per_sample, channels, total_samples)

    def write(self, samples):
        """Interleaved samples, any count (encode.rs:558)."""
        s = np.ascontiguousarray(samples, dtype=np.int32)
        _check(_stream_lib().flacenc_write_samples(self._h, s.ctypes.data_as(C.POINTER(C.c_int32)), s.size))


class FlacByteWriter(_Writer, io.RawIOBase):
    """A FLAC writer which accepts samples as bytes (encode.rs:105); `endian` is "little"
    or "big" (the reference's `Endianness` type parameter)."""

    def __init__(self, writer, options, sample_rate, bits_per_sample, channels, total_bytes=None,
                 endian="little"):
        _Writer.__init__(self, writer)
        ht, tv = _total(total_bytes)
        _check(_stream_lib().flacenc_byte_writer_new(
            C.byref(options._c_options()), sample_rate, bits_per_sample, channels, ht, tv,
            int(endian == "big"), self._sink_ptr(), C.byref(self._h)))

    @classmethod
    def endian(cls, writer, endianness, options, sample_rate, bits_per_sample, channels,
               total_bytes=None):  # encode.rs:205
        return cls(writer, options, sample_rate, bits_per_sample, channels, total_bytes, endianness)

    @classmethod
    def new_cdda(cls, writer, options, total_bytes=None):
        return cls(writer, options, 44100, 16, 2, total_bytes)

    @classmethod
    def create(cls, path, options, sample_rate, bits_per_sample, channels, total_bytes=None,
               endian="little"):
        return cls(options._open(path), options, sample_rate, bits_per_sample, channels, total_bytes, endian)

    def write(self, data):  # io::Write::write, encode.rs:359: the whole buffer is consumed
        b = bytes(data)
        _check(_stream_lib().flacenc_write_bytes(self._h, b, len(b)))
        return len(b)

    def writable(self):
        return True

    def close(self):
        _Writer.close(self)


class FlacChannelWriter(_Writer):
    """A FLAC writer which accepts samples as channels of signed integers (encode.rs:735)."""

    def __init__(self, writer, options, sample_rate, bits_per_sample, channels, total_samples=None):
        super().__init__(writer)
        self._channels = channels
        ht, tv = _total(total_samples)
        _check(_stream_lib().flacenc_channel_writer_new(
            C.byref(options._c_options()), sample_rate, bits_per_sample, channels, ht, tv, self._sink_ptr(),
            C.byref(self._h)))

    @classmethod
    def new_cdda(cls, writer, options, total_samples=None):
        return cls(writer, options, 44100, 16, 2, total_samples)

    def write(self, channels):
        """`channels`: one sequence of samples per channel, all of one length (encode.rs:832)."""
        chans = [np.ascontiguousarray(c, dtype=np.int32) for c in channels]
        if len(chans) != self._channels:  # encode.rs:856-859
            raise ChannelCountMismatch("ChannelCountMismatch")
        if any(c.size != chans[0].size for c in chans):  # encode.rs:849-855
            raise ChannelLengthMismatch("ChannelLengthMismatch")
        ptrs = (C.POINTER(C.c_int32) * len(chans))(*[c.ctypes.data_as(C.POINTER(C.c_int32)) for c in chans])
        _check(_stream_lib().flacenc_write_channels(self._h, ptrs, len(chans), chans[0].size))


class FlacStreamWriter:
    """A FLAC writer which outputs header-less subset frames, one per `write` call
    (encode.rs:1050)."""

    def __init__(self, writer, options):
        self._h = C.c_void_p(None)
        self._py = writer
        self._sink = None
        if writer is not None:
            def _w(_user, data, n):
                try:
                    writer.write(C.string_at(data, n))
                    return 0
                except Exception:
                    return 1

            self._cb = (_WRITE_FN(_w), _SEEK_FN(lambda _u, _o: 1))
            self._sink = _CSink(self._cb[0], self._cb[1], None, 0)
        _check(_stream_lib().flacenc_stream_writer_new(
            C.byref(options._c_options()), C.byref(self._sink) if self._sink is not None else None,
            C.byref(self._h)))

    def write(self, sample_rate, channels, bits_per_sample, samples):  # encode.rs:1142
        s = np.ascontiguousarray(samples, dtype=np.int32)
        _check(_stream_lib().flacenc_stream_writer_write(
            self._h, sample_rate, channels, bits_per_sample, s.ctypes.data_as(C.POINTER(C.c_int32)), s.size))

    def write_cdda(self, samples):  # encode.rs:1270
        self.write(44100, 2, 16, samples)

    def getvalue(self):
        n = C.c_size_t(0)
        p = _stream_lib().flacenc_stream_writer_data(self._h, C.byref(n))
        return C.string_at(p, n.value) if p else b""

    def close(self):
        if self._h:
            _stream_lib().flacenc_stream_writer_free(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchEncoder:
    """Many independent streams at once (flacenc_encode_many): the C++ front end keeps `threads` host
    workers busy, each running FlacSampleWriter::new / write / finalize (encode.rs:487, 558, 624) for
    one stream at a time; output buffers are allocated once and reused by later calls."""

    def __init__(self, options, threads=0, devices=None, coalesce=False):
        """devices: None (the options' device), "all" (every visible device) or a list of HIP ordinals -- stream i is
        encoded whole on devices[i mod len] (flacenc_encode_many_devices).  coalesce: streams of one shape share analysis
        batches (flacenc_encode_many_coalesced: many SMALL streams)."""
        self._opts, self._threads, self._devices, self._coalesce = options, threads, devices, coalesce
        self._bufs = []
        self._shard = None   # encode_device(out="device"): the reused device buffer of the files

    def prepare(self, streams, sample_rate, bits_per_sample, channels):
        """The job array of a call (what a C caller would hold): arrays pinned in a handle, output buffers sized for the
        worst case.  run(handle) then is the C entry point alone."""
        L = _stream_lib()
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in streams]
        jobs = (_CJob * len(arrs))()
        co = self._opts._c_options()
        L.flacenc_worst_case_bytes.restype = C.c_size_t
        L.flacenc_worst_case_bytes.argtypes = [C.POINTER(_COptions), C.c_uint32, C.c_uint32, C.c_uint64]
        for i, a in enumerate(arrs):
            # every frame VERBATIM with its headers + a seek point per frame + the metadata: never too small
            cap = int(L.flacenc_worst_case_bytes(C.byref(co), bits_per_sample, channels, a.size // max(1, channels)))
            if i >= len(self._bufs):
                self._bufs.append(np.empty(cap, dtype=np.uint8))
            elif self._bufs[i].size < cap:
                self._bufs[i] = np.empty(cap, dtype=np.uint8)
            j = jobs[i]
            j.samples = a.ctypes.data_as(C.POINTER(C.c_int32))
            j.count = a.size
            j.sample_rate, j.bits_per_sample, j.channels = sample_rate, bits_per_sample, channels
            j.out = self._bufs[i].ctypes.data
            j.out_cap = self._bufs[i].size
        return (jobs, arrs, co)

    def run(self, handle):
        """One call of flacenc_encode_many / _coalesced / _devices on a prepared job array."""
        L = _stream_lib()
        jobs, arrs, co = handle
        if self._coalesce:
            _check(L.flacenc_encode_many_coalesced(C.byref(co), jobs, len(arrs), self._threads))
        elif self._devices is None:
            _check(L.flacenc_encode_many(C.byref(co), jobs, len(arrs), self._threads))
        elif self._devices == "all":
            _check(L.flacenc_encode_many_devices(C.byref(co), jobs, len(arrs), self._threads, None, 0xFFFFFFFF))
        else:
            devs = (C.c_int * len(self._devices))(*self._devices)
            _check(L.flacenc_encode_many_devices(C.byref(co), jobs, len(arrs), self._threads, devs, len(self._devices)))

    def results(self, handle, copy=True):
        jobs, arrs, _ = handle
        self.last_jobs = [{k: getattr(jobs[i], k) for k in ("elapsed_ms", "pack_ms", "gpu_ms", "md5_ms", "start_ms")}
                          for i in range(len(arrs))]
        views = [self._bufs[i][: jobs[i].out_len] for i in range(len(arrs))]
        return [v.tobytes() for v in views] if copy else views

    def encode(self, streams, sample_rate, bits_per_sample, channels, copy=True):
        """streams: list of interleaved int32 arrays.  Returns the .flac bytes of every stream (or
        memoryviews into the reused output buffers with copy=False)."""
        h = self.prepare(streams, sample_rate, bits_per_sample, channels)
        self.run(h)
        return self.results(h, copy)

    @staticmethod
    def _device_batch(tensor, lengths, dtype, offsets, channels):
        """What an encode_device call's tensor holds: (streams, offsets, lengths, channels, format)."""
        if dtype not in (None, "int24"):
            raise ValueError("dtype must be None (the tensor's own: int16, int32 or float32) or 'int24'")
        if not tensor.is_contiguous() or not tensor.is_cuda:
            raise ValueError("tensor must be a contiguous tensor on the GPU")
        if dtype == "int24":
            if str(tensor.dtype) != "torch.uint8" or tensor.dim() < 2 or tensor.shape[-1] != 3:
                raise ValueError("dtype='int24' takes a uint8 tensor with a trailing axis of 3")
            code, shape = _lib.SAMPLE_S24, tuple(int(v) for v in tensor.shape[:-1])
        else:
            code = {"torch.int32": _lib.SAMPLE_I32, "torch.int16": _lib.SAMPLE_I16,
                    "torch.float32": _lib.SAMPLE_F32}.get(str(tensor.dtype))
            if code is None:
                raise ValueError("tensor must be int16, int32 or float32, or uint8 [..., 3] with dtype='int24'")
            shape = tuple(int(v) for v in tensor.shape)
        if offsets is None:
            if len(shape) != 3:
                raise ValueError("a padded batch is [B, C, T] ([B, C, T, 3] for dtype='int24')")
            n, channels, padded = shape
            lengths = [padded] * n if lengths is None else [int(v) for v in lengths]
            offsets = [0] * n
            fmt = _lib.OutFormat(code, _lib.LAYOUT_PADDED, channels, 0, padded)
        else:
            if len(shape) != 1 or lengths is None or not channels:
                raise ValueError("a flat batch is [elements] ([elements, 3] for dtype='int24') with offsets, lengths "
                                 "and channels")
            offsets, lengths, channels = [int(v) for v in offsets], [int(v) for v in lengths], int(channels)
            n = len(offsets)
            if any(o < 0 or o + s * channels > shape[0] for o, s in zip(offsets, lengths)):
                raise ValueError("a stream reaches past the tensor")
            fmt = _lib.OutFormat(code, _lib.LAYOUT_FLAT, 0, 0, 0)
        if len(lengths) != n:
            raise ValueError("one length per stream")
        return n, offsets, lengths, channels, fmt

    def prepare_device(self, tensor, lengths, bits_per_sample, dtype=None, offsets=None, channels=None):
        """The job array of an encode_device call: a [B, C, T] tensor is a PADDED batch of B streams of C channels,
        stream i of lengths[i] (default T) samples; with `offsets` the tensor is FLAT, stream i interleaved from element
        offsets[i].  dtype="int24": uint8 with a trailing axis of 3.  Output buffers sized for the worst case and reused
        by later calls."""
        L = _stream_lib()
        n, offsets, lengths, channels, fmt = self._device_batch(tensor, lengths, dtype, offsets, channels)
        jobs = (_lib.DeviceJob * max(n, 1))()
        co = self._opts._c_options()
        for i, samples in enumerate(lengths):
            jobs[i].in_offset = offsets[i]
            cap = int(L.flacenc_worst_case_bytes(C.byref(co), bits_per_sample, max(channels, 1), samples))
            if i >= len(self._bufs):
                self._bufs.append(np.empty(cap, dtype=np.uint8))
            elif self._bufs[i].size < cap:
                self._bufs[i] = np.empty(cap, dtype=np.uint8)
            jobs[i].samples = samples
            jobs[i].out = self._bufs[i].ctypes.data
            jobs[i].out_cap = self._bufs[i].size
        return (jobs, n, co, fmt, channels)

    def run_device(self, handle, tensor, sample_rate, bits_per_sample, verify_md5=True, stream=None):
        """One call of flacenc_encode_many_device on a prepared job array; returns its return code (0, or the first
        failing job's status -- every job's own status, out_len, altered and md5 are in the array)."""
        import torch

        L = _stream_lib()
        jobs, n, co, fmt, channels = handle
        if stream is None:
            stream = torch.cuda.current_stream(tensor.device).cuda_stream
        if co.device < 0:
            co.device = tensor.device.index
        return L.flacenc_encode_many_device(C.byref(co), tensor.data_ptr() if tensor.numel() else None, C.byref(fmt),
                                            sample_rate, bits_per_sample, channels, jobs, n,
                                            0 if verify_md5 else _lib.DEVICE_NO_MD5, stream or None)

    def prepare_device_out(self, tensor, lengths, bits_per_sample, dtype=None, offsets=None, channels=None, shard=None,
                           slots=None):
        """The job array of an encode_device(out="device") call (the tensor as in prepare_device) and the device buffer
        the files go to.  Without `slots`: a torch.uint8 shard of this encoder's on the tensor's device, reused by later
        calls, with one slot of flacenc_worst_case_bytes per stream, one behind another.  slots=[(offset, cap), ...]
        with shard= (a contiguous 1-D uint8 tensor on the tensor's device): the caller's buffer and slots."""
        import torch

        L = _stream_lib()
        n, offsets, lengths, channels, fmt = self._device_batch(tensor, lengths, dtype, offsets, channels)
        co = self._opts._c_options()
        if slots is None:
            if shard is not None:
                raise ValueError("shard= goes with slots=")
            slots, total = [], 0
            for samples in lengths:
                cap = int(L.flacenc_worst_case_bytes(C.byref(co), bits_per_sample, max(channels, 1), samples))
                slots.append((total, cap))
                total += cap
            if self._shard is None or self._shard.device != tensor.device or self._shard.numel() < total:
                self._shard = torch.empty(max(total, 1), dtype=torch.uint8, device=tensor.device)
            shard = self._shard
        else:
            if (shard is None or not shard.is_cuda or shard.device != tensor.device or shard.dtype != torch.uint8
                    or shard.dim() != 1 or not shard.is_contiguous()):
                raise ValueError("slots= takes shard=, a contiguous 1-D uint8 tensor on the tensor's device")
            slots = [(int(o), int(c)) for o, c in slots]
            if len(slots) != n or any(o < 0 or c < 0 for o, c in slots):
                raise ValueError("one (offset, cap) slot per stream")
        jobs = (_lib.DeviceOutJob * max(n, 1))()
        for i in range(n):
            jobs[i].in_offset, jobs[i].samples = offsets[i], lengths[i]
            jobs[i].out_offset, jobs[i].out_cap = slots[i]
        return (jobs, n, co, fmt, channels, shard)

    def run_device_out(self, handle, tensor, sample_rate, bits_per_sample, verify_md5=True, stream=None):
        """One call of flacenc_encode_many_device_out on a prepared job array; returns its return code, as run_device."""
        import torch

        L = _stream_lib()
        jobs, n, co, fmt, channels, shard = handle
        if stream is None:
            stream = torch.cuda.current_stream(tensor.device).cuda_stream
        if co.device < 0:
            co.device = tensor.device.index
        return L.flacenc_encode_many_device_out(C.byref(co), tensor.data_ptr() if tensor.numel() else None, C.byref(fmt),
                                                sample_rate, bits_per_sample, channels, jobs, n, shard.data_ptr(),
                                                shard.numel(), 0 if verify_md5 else _lib.DEVICE_NO_MD5, stream or None)

    def encode_device(self, tensor, lengths=None, sample_rate=44100, bits_per_sample=16, verify_md5=True, copy=True,
                      dtype=None, offsets=None, channels=None, out="host", shard=None, slots=None):
        """A batch of streams held on the GPU -> .flac bytes, the samples never visiting the host
        (flacenc_encode_many_device).  tensor: contiguous [B, C, T] torch tensor on the GPU, int16 (x >> (16 - bps)),
        int32 (clamped to bps bits) or float32 (x * 2^(bps - 1), rounded to nearest even, clamped; NaN -> 0); with
        dtype="int24" a uint8 tensor [B, C, T, 3] of packed little-endian 24-bit elements (sign-extended, then
        x >> (24 - bps); bps <= 24).  lengths: samples of every stream (default T; what lies behind is never read).
        offsets (with lengths and channels): the tensor is flat instead -- [elements], or [elements, 3] for "int24" --
        and stream i is [lengths[i]][channels] interleaved from element offsets[i]; what lies between is never read.
        Runs behind the work queued on the tensor's current torch stream and returns when the files are complete.  verify_md5=False leaves STREAMINFO's MD5 zero
        ("unknown") and skips the hash kernel.  self.last_altered: per stream, the elements that were clamped, NaN or
        (int16, int24) lost non-zero low bits; self.last_md5: the digests; self.last_status: every stream's status.
        out="device" (flacenc_encode_many_device_out): the files stay on the GPU, in one uint8 shard tensor of this
        encoder's that later calls reuse (so the views of one call are valid until the next) -- one worst-case slot per
        stream, one behind another -- and the call returns the list of 1-D views shard[o : o + out_len], which
        Decoder.scan and decode_many take as they are; only frame sizes, digests and headers cross the link.
        slots=[(offset, cap), ...] with shard= puts the files into the caller's own uint8 tensor instead: no byte
        outside [offset, offset + out_len) of a stream is written."""
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device'")
        if out == "host":
            if shard is not None or slots is not None:
                raise ValueError("shard= and slots= go with out='device'")
            h = self.prepare_device(tensor, lengths, bits_per_sample, dtype, offsets, channels)
            rc = self.run_device(h, tensor, sample_rate, bits_per_sample, verify_md5)
        else:
            h = self.prepare_device_out(tensor, lengths, bits_per_sample, dtype, offsets, channels, shard, slots)
            rc = self.run_device_out(h, tensor, sample_rate, bits_per_sample, verify_md5)
        jobs, n = h[0], h[1]
        self.last_altered = [int(jobs[i].altered) for i in range(n)]
        self.last_status = [int(jobs[i].status) for i in range(n)]
        self.last_md5 = [bytes(jobs[i].md5) for i in range(n)]
        _check(rc)
        if out == "device":
            return [h[5][int(jobs[i].out_offset): int(jobs[i].out_offset) + int(jobs[i].out_len)] for i in range(n)]
        views = [self._bufs[i][: jobs[i].out_len] for i in range(n)]
        return [v.tobytes() for v in views] if copy else views

    def open_device_session(self, totals, sample_rate, bits_per_sample, channels, max_chunk, verify_md5=True, keep=True,
                            device=None, n_streams=None):
        """A DeviceSession: the streams of encode_device taken chunk by chunk (flacenc_device_session_*).  totals:
        every stream's length per channel, declared now -- None for a stream whose length is not known yet
        (FlacSampleWriter::new with None: its header has no placeholder SEEKTABLE, finalize fills in the total); with
        totals=None, n_streams=k opens k such streams.  max_chunk: the most samples per channel one write brings for
        one stream.  device: the HIP ordinal (default: the options', else the current one)."""
        if totals is None:
            if n_streams is None:
                raise ValueError("totals=None takes n_streams")
            totals = [None] * int(n_streams)
        elif n_streams is not None and int(n_streams) != len(totals):
            raise ValueError("n_streams differs from len(totals)")
        return DeviceSession(self._opts, totals, sample_rate, bits_per_sample, channels, max_chunk, verify_md5, keep, device)

    def open_device_stream_writer(self, n_streams, sample_rate, bits_per_sample, channels, max_block, first_numbers=None,
                                  device=None):
        """A DeviceStreamWriter: n_streams streams of one shape on the GPU -> raw subset frames, one per stream and
        write (flacenc_device_stream_writer_*).  max_block: the most samples per channel one write brings for one
        stream, at most 65535.  first_numbers: every stream's first frame number (default 0)."""
        return DeviceStreamWriter(self._opts, n_streams, sample_rate, bits_per_sample, channels, max_block, first_numbers,
                                  device)


class DeviceSession:
    """n streams of one shape, produced on the GPU piece by piece, -> .flac files (flacenc_device_session_*): write()
    takes the next chunk of every stream in the tensor forms encode_device takes and returns the frames that chunk
    completes; finalize() returns the files -- byte for byte what encode_device gives for the concatenated samples.
    A total of None: the stream's length is not known yet, and its file is FlacSampleWriter's with total_samples=None.
    A context manager: leaving the block closes the session."""

    def __init__(self, options, totals, sample_rate, bits_per_sample, channels, max_chunk, verify_md5=True, keep=True,
                 device=None):
        L = _stream_lib()
        self._co = options._c_options()
        if device is not None:
            self._co.device = int(device)
        self._totals = [None if t is None else int(t) for t in totals]
        self._n, self._bps, self._channels, self._keep = len(self._totals), bits_per_sample, channels, keep
        self._block = int(self._co.block_size)
        self._pending = [0] * self._n   # samples carried towards the next block, as the library counts them
        self._parts = [[] for _ in range(self._n)]
        self._bufs = []
        self._h = C.c_void_p()
        arr = (C.c_uint64 * max(self._n, 1))(*[t or 0 for t in self._totals])
        flags = 0 if verify_md5 else _lib.DEVICE_NO_MD5
        if any(t is None for t in self._totals):
            known = (C.c_uint8 * max(self._n, 1))(*[int(t is not None) for t in self._totals])
            _check(L.flacenc_device_session_open_ex(C.byref(self._co), sample_rate, bits_per_sample, channels, arr, known,
                                                    self._n, int(max_chunk), flags, C.byref(self._h)))
        else:
            _check(L.flacenc_device_session_open(C.byref(self._co), sample_rate, bits_per_sample, channels, arr, self._n,
                                                 int(max_chunk), flags, C.byref(self._h)))
        self.last_status = [0] * self._n
        self.last_altered = [0] * self._n
        self.last_md5 = [bytes(16)] * self._n

    def header_len(self, i):
        return int(_stream_lib().flacenc_device_session_header_len(self._h, i))

    def write(self, tensor, lengths=None, dtype=None, offsets=None):
        """The next chunk of every stream (lengths[i] samples of stream i, 0 allowed; the tensor as in encode_device)
        -> list[bytes]: the frames this write completes, per stream.  Runs behind the tensor's current torch stream and
        returns when the tensor may be reused.  self.last_status / self.last_altered: this write's (a stream whose
        status is not 0 is dead -- its later chunks are ignored -- and the others go on; finalize() raises for it)."""
        import torch

        L = _stream_lib()
        n, offsets, lengths, channels, fmt = BatchEncoder._device_batch(tensor, lengths, dtype, offsets, self._channels)
        if n != self._n or channels != self._channels:
            raise ValueError("one chunk per stream of the session, of the session's channel count")
        chunks = (_lib.SessionChunk * max(n, 1))()
        for i in range(n):
            blocks = (self._pending[i] + lengths[i]) // self._block
            cap = int(L.flacenc_worst_case_bytes(C.byref(self._co), self._bps, channels, blocks * self._block)) if blocks else 0
            if i >= len(self._bufs):
                self._bufs.append(np.empty(max(cap, 1), dtype=np.uint8))
            elif self._bufs[i].size < cap:
                self._bufs[i] = np.empty(cap, dtype=np.uint8)
            chunks[i].in_offset, chunks[i].samples = offsets[i], lengths[i]
            chunks[i].out, chunks[i].out_cap = self._bufs[i].ctypes.data, self._bufs[i].size
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        rc = L.flacenc_device_session_write(self._h, tensor.data_ptr() if tensor.numel() else None, C.byref(fmt), chunks,
                                            stream or None)
        _check(rc)   # refused as a whole: no chunk field was written and the session is as it was
        self.last_status = [int(chunks[i].status) for i in range(n)]
        self.last_altered = [int(chunks[i].altered) for i in range(n)]
        out = []
        for i in range(n):
            if not self.last_status[i]:
                self._pending[i] = (self._pending[i] + lengths[i]) % self._block
            out.append(self._bufs[i][: chunks[i].out_len].tobytes())
            if self._keep:
                self._parts[i].append(out[-1])
        return out

    def finalize(self):
        """-> list[bytes], the whole files (keep=True), or (headers, tails) for a session opened with keep=False.
        self.last_status, self.last_altered (summed over the writes) and self.last_md5 as for encode_device."""
        L = _stream_lib()
        n = self._n
        finals = (_lib.SessionFinal * max(n, 1))()
        tail_cap = int(L.flacenc_worst_case_bytes(C.byref(self._co), self._bps, self._channels, self._block))
        bufs = []
        for i in range(n):
            hb = np.empty(max(self.header_len(i), 1), dtype=np.uint8)
            tb = np.empty(tail_cap, dtype=np.uint8)
            bufs.append((hb, tb))
            finals[i].header, finals[i].header_cap = hb.ctypes.data, hb.size
            finals[i].tail, finals[i].tail_cap = tb.ctypes.data, tb.size
        rc = L.flacenc_device_session_finalize(self._h, finals)
        self.last_status = [int(finals[i].status) for i in range(n)]
        self.last_altered = [int(finals[i].altered) for i in range(n)]
        self.last_md5 = [bytes(finals[i].md5) for i in range(n)]
        _check(rc)
        headers = [bufs[i][0][: finals[i].header_len].tobytes() for i in range(n)]
        tails = [bufs[i][1][: finals[i].tail_len].tobytes() for i in range(n)]
        if not self._keep:
            return headers, tails
        return [headers[i] + b"".join(self._parts[i]) + tails[i] for i in range(n)]

    def close(self):
        if self._h:
            _stream_lib().flacenc_device_session_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceStreamWriter:
    """n streams of one shape, produced on the GPU piece by piece, -> raw subset FLAC frames without metadata
    (flacenc_device_stream_writer_*; FlacStreamWriter for a batch in device memory): write() takes up to max_block
    samples of every stream in the tensor forms encode_device takes and returns ONE frame per stream that brought
    samples, numbered with that stream's own count -- what decode_frames, decode_timeline and FlacStreamReader read.
    A context manager: leaving the block closes the writer."""

    def __init__(self, options, n_streams, sample_rate, bits_per_sample, channels, max_block, first_numbers=None,
                 device=None):
        L = _stream_lib()
        self._co = options._c_options()
        if device is not None:
            self._co.device = int(device)
        self._n, self._bps, self._channels, self._max_block = int(n_streams), bits_per_sample, channels, int(max_block)
        self._bufs = []
        self._h = C.c_void_p()
        first = None
        if first_numbers is not None:
            if len(first_numbers) != self._n:
                raise ValueError("one first frame number per stream")
            first = (C.c_uint64 * max(self._n, 1))(*[int(v) for v in first_numbers])
        _check(L.flacenc_device_stream_writer_open(C.byref(self._co), sample_rate, bits_per_sample, channels, self._n,
                                                   self._max_block, first, C.byref(self._h)))
        self.last_status = [0] * self._n
        self.last_altered = [0] * self._n

    @property
    def frame_numbers(self):
        """Every stream's next frame number."""
        L = _stream_lib()
        return [int(L.flacenc_device_stream_writer_frame_number(self._h, i)) for i in range(self._n)]

    def write(self, tensor, lengths, dtype=None, offsets=None):
        """lengths[i] samples of stream i (0: none this time; at most max_block; the tensor as in encode_device) ->
        list[bytes]: every stream's frame, b"" for a stream without samples.  Runs behind the tensor's current torch
        stream and returns when the tensor may be reused.  A write the library refuses as a whole raises and changes
        nothing.  self.last_status / self.last_altered: this write's, per stream (a stream whose status is not 0 got
        no frame number and may be written again)."""
        import torch

        L = _stream_lib()
        n, offsets, lengths, channels, fmt = BatchEncoder._device_batch(tensor, lengths, dtype, offsets, self._channels)
        if n != self._n or channels != self._channels:
            raise ValueError("one chunk per stream of the writer, of the writer's channel count")
        chunks = (_lib.SessionChunk * max(n, 1))()
        for i in range(n):
            # a frame at its largest: header <= 16 bytes, CRC-16, every subframe VERBATIM at bps + 1 bits with a header
            # byte and a wasted-bits escape
            cap = 18 + 2 * channels + (lengths[i] * channels * (self._bps + 1) + 7) // 8 if lengths[i] > 0 else 0
            if i >= len(self._bufs):
                self._bufs.append(np.empty(max(cap, 1), dtype=np.uint8))
            elif self._bufs[i].size < cap:
                self._bufs[i] = np.empty(cap, dtype=np.uint8)
            chunks[i].in_offset, chunks[i].samples = offsets[i], lengths[i]
            chunks[i].out, chunks[i].out_cap = self._bufs[i].ctypes.data, self._bufs[i].size
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        rc = L.flacenc_device_stream_writer_write(self._h, tensor.data_ptr() if tensor.numel() else None, C.byref(fmt),
                                                  chunks, stream or None)
        _check(rc)   # refused as a whole: no chunk field was written and no number advanced
        self.last_status = [int(chunks[i].status) for i in range(n)]
        self.last_altered = [int(chunks[i].altered) for i in range(n)]
        return [self._bufs[i][: chunks[i].out_len].tobytes() for i in range(n)]

    def close(self):
        if self._h:
            _stream_lib().flacenc_device_stream_writer_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
