"""ctypes loader for libflacenc_amd.so (the C-ABI shared library of this package).

The library holds the hand-written gfx950 kernels; there is NO CPU fallback: if it is
missing or fails to load, importing anything that needs it raises.
"""
import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# FLACENC_AMD_LIBRARY: another build of the same library (the sanitizer builds of csrc/Makefile `sanitize`)
LIB_PATH = os.environ.get("FLACENC_AMD_LIBRARY") or os.path.join(_HERE, "libflacenc_amd.so")

MAX_CHANNELS = 8
MAX_LPC_ORDER = 32
MAX_PARTITIONS = 64
N_KERNELS = 12
DECODE_OUT_DEVICE = 1   # flacgpu_decoder_decode flags (include/flacenc_gpu.h)
DECODE_NO_MD5 = 2
SAMPLE_I32, SAMPLE_I16, SAMPLE_F32 = 0, 1, 2   # flacgpu_out_format.dtype
SAMPLE_S24 = 24   # packed 3-byte little-endian elements
LAYOUT_FLAT, LAYOUT_PADDED = 0, 1              # flacgpu_out_format.layout
SCAN_SPECULATIVE = 1    # flacgpu_*_scan_frames*_ex flags: end a frame that no header ends by its own bits
FRAME_SPECULATIVE = 1   # FrameRecord.reserved bit 0: the frame was ended that way
TL_PLACED, TL_DROPPED, TL_CONCEALED = 1, 2, 4   # TimelineFrame.flags (FLACGPU_TL_*)


class GpuOptions(C.Structure):
    """flacgpu_options (include/flacenc_gpu.h)."""
    _fields_ = [
        ("block_size", C.c_uint32),
        ("max_partition_order", C.c_uint32),
        ("max_lpc_order", C.c_uint32),
        ("mid_side", C.c_uint8),
        ("exhaustive_channel_correlation", C.c_uint8),
        ("window_kind", C.c_uint8),
        ("reserved", C.c_uint8),
        ("window_param", C.c_float),
    ]


class SubframePlan(C.Structure):
    """flacgpu_subframe_plan."""
    _fields_ = [
        ("type", C.c_uint8),
        ("wasted", C.c_uint8),
        ("bps", C.c_uint8),
        ("order", C.c_uint8),
        ("precision", C.c_uint8),
        ("shift", C.c_uint8),
        ("coding_method", C.c_uint8),
        ("partition_order", C.c_uint8),
        ("source", C.c_uint8),
        ("reserved", C.c_uint8 * 3),
        ("n_partitions", C.c_uint32),
        ("part_len", C.c_uint32),
        ("bits", C.c_uint32),
        ("coeffs", C.c_int32 * MAX_LPC_ORDER),
        ("rice", C.c_uint8 * MAX_PARTITIONS),
        ("escape_bits", C.c_uint8 * MAX_PARTITIONS),
    ]


class FramePlan(C.Structure):
    """flacgpu_frame_plan."""
    _fields_ = [
        ("assignment", C.c_uint8),
        ("channels", C.c_uint8),
        ("block_size", C.c_uint16),
        ("body_bits", C.c_uint32),
    ]


class VerifyResult(C.Structure):
    """flacgpu_verify_result."""
    _fields_ = [
        ("frames", C.c_uint32),
        ("bad_structure", C.c_uint32),
        ("bad_crc16", C.c_uint32),
        ("frames_pcm_differs", C.c_uint32),
        ("samples_differ", C.c_uint32),
        ("compared_pcm", C.c_uint32),
    ]


class StreamInfo(C.Structure):
    """flacgpu_stream_info."""
    _fields_ = [
        ("sample_rate", C.c_uint32), ("channels", C.c_uint32), ("bits_per_sample", C.c_uint32),
        ("min_block", C.c_uint32), ("max_block", C.c_uint32),
        ("frames", C.c_uint32), ("bad_frames", C.c_uint32), ("bad_crc16", C.c_uint32),
        ("total_samples", C.c_uint64), ("decoded_samples", C.c_uint64),
        ("md5", C.c_uint8 * 16), ("decoded_md5", C.c_uint8 * 16),
        ("md5_status", C.c_uint32), ("reserved", C.c_uint32),
    ]


class DecodedStream(C.Structure):
    """flacgpu_decoded_stream: one stream's record of the batch decoder."""
    _fields_ = [("rc", C.c_int32), ("reserved", C.c_uint32), ("out_offset", C.c_uint64), ("info", StreamInfo)]


class OutFormat(C.Structure):
    """flacgpu_out_format: element type and layout of flacgpu_decoder_decode_as's output."""
    _fields_ = [("dtype", C.c_uint32), ("layout", C.c_uint32), ("channels_padded", C.c_uint32),
                ("reserved", C.c_uint32), ("samples_padded", C.c_uint64)]


class DeviceJob(C.Structure):
    """flacenc_device_job: one stream of flacenc_encode_many_device (include/flacenc_stream.h); the tensor's format is
    an OutFormat (flacenc_tensor_format is flacgpu_out_format)."""
    _fields_ = [("in_offset", C.c_uint64), ("samples", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_size_t),
                ("out_len", C.c_size_t), ("status", C.c_int32), ("altered", C.c_uint32), ("md5", C.c_uint8 * 16)]


class DeviceOutJob(C.Structure):
    """flacenc_device_out_job: one stream of flacenc_encode_many_device_out; its file goes to bytes
    [out_offset, out_offset + out_cap) of the call's device buffer."""
    _fields_ = [("in_offset", C.c_uint64), ("samples", C.c_uint64), ("out_offset", C.c_uint64), ("out_cap", C.c_uint64),
                ("out_len", C.c_uint64), ("status", C.c_int32), ("altered", C.c_uint32), ("md5", C.c_uint8 * 16)]


class PlaceRun(C.Structure):
    """flacgpu_place_run: one byte run of flacgpu_place_frames / flacgpu_place_runs_host."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("n", C.c_uint64)]


DEVICE_NO_MD5 = 1   # FLACENC_DEVICE_NO_MD5


class SessionChunk(C.Structure):
    """flacenc_session_chunk: one stream's part of a flacenc_device_session_write call, or of a
    flacenc_device_stream_writer_write call (out then receives the stream's one raw frame)."""
    _fields_ = [("in_offset", C.c_uint64), ("samples", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_size_t),
                ("out_len", C.c_size_t), ("status", C.c_int32), ("altered", C.c_uint32)]


class SessionFinal(C.Structure):
    """flacenc_session_final: one stream's header, short last frame, status, altered count and MD5 at finalize."""
    _fields_ = [("header", C.c_void_p), ("header_cap", C.c_size_t), ("header_len", C.c_size_t), ("tail", C.c_void_p),
                ("tail_cap", C.c_size_t), ("tail_len", C.c_size_t), ("status", C.c_int32), ("altered", C.c_uint32),
                ("md5", C.c_uint8 * 16)]


class Md5Piece(C.Structure):
    """flacgpu_md5_piece: `count` int32 samples from element `off`, appended to chain `chain` (flacgpu_md5_chains_update)."""
    _fields_ = [("chain", C.c_uint32), ("reserved", C.c_uint32), ("off", C.c_uint64), ("count", C.c_uint64)]


class Md5State(C.Structure):
    """flacgpu_md5_state: one resumable MD5 chain in host memory (flacgpu_md5_init_host / feed_host / final_host)."""
    _fields_ = [("h", C.c_uint32 * 4), ("len", C.c_uint64), ("buf", C.c_uint8 * 64)]


class Window(C.Structure):
    """flacgpu_window: samples [start, start + length) per channel of one scanned stream."""
    _fields_ = [("stream", C.c_uint32), ("reserved", C.c_uint32), ("start", C.c_uint64), ("length", C.c_uint64)]


class WindowResult(C.Structure):
    """flacgpu_window_result: one window's record of flacgpu_decoder_decode_windows."""
    _fields_ = [("rc", C.c_int32), ("frames", C.c_uint32), ("bad_frames", C.c_uint32), ("bad_crc16", C.c_uint32),
                ("samples", C.c_uint64)]


class FrameRecord(C.Structure):
    """flacgpu_frame_record: one kept frame of a raw frame stream (64 bytes)."""
    _fields_ = [("byte_offset", C.c_uint64), ("number", C.c_uint64), ("out_offset", C.c_uint64),
                ("stream", C.c_uint32), ("bytes", C.c_uint32), ("block_size", C.c_uint32), ("sample_rate", C.c_uint32),
                ("channels", C.c_uint32), ("bits_per_sample", C.c_uint32), ("assignment", C.c_uint32),
                ("blocking", C.c_uint32), ("status", C.c_uint32), ("reserved", C.c_uint32)]


class FrameAnalysis(C.Structure):
    """flacgpu_frame_analysis: one frame of flacgpu_decoder_analyze (40 bytes)."""
    _fields_ = [("row_offset", C.c_uint64), ("first_subframe", C.c_uint64), ("block_size", C.c_uint32),
                ("header_bytes", C.c_uint32), ("status", C.c_uint32), ("assignment_code", C.c_uint32),
                ("plan", FramePlan)]


AN_WIDE, AN_PARTS_CLIPPED = 1, 2   # flacgpu_subframe_plan.reserved[0] of an analysed subframe


class RawStream(C.Structure):
    """flacgpu_raw_stream: one input's summary of a raw frame scan (32 bytes)."""
    _fields_ = [("first_frame", C.c_uint64), ("skipped_bytes", C.c_uint64), ("frames", C.c_uint32),
                ("gaps", C.c_uint32), ("uniform", C.c_uint32), ("reserved", C.c_uint32)]


class SessionTiming(C.Structure):
    """flacgpu_session_timing: where the host's time went in a decoder session's last feed, in milliseconds."""
    _fields_ = [(name, C.c_double) for name in ("stage_ms", "to_first_sync_ms", "to_second_sync_ms", "scan_rest_ms",
                                                "walk_ms", "table_upload_ms")]


class MetaFeedState(C.Structure):
    """flacgpu_meta_feed: the resumable metadata walk's state, 104 bytes whatever the chain's length."""
    _fields_ = [("words", C.c_uint64 * 13)]


class SessionSlotSrc(C.Structure):
    """flacgpu_session_slot_src: one slot's held tail and new chunk, for flacgpu_session_slots_host."""
    _fields_ = [("tail", C.c_void_p), ("tail_len", C.c_uint64), ("chunk", C.c_void_p), ("chunk_len", C.c_uint64)]


class TimelineFrame(C.Structure):
    """flacgpu_timeline_frame: one record's place on its stream's timeline (16 bytes)."""
    _fields_ = [("at", C.c_uint64), ("flags", C.c_uint32), ("status", C.c_uint32)]


class TimelineResult(C.Structure):
    """flacgpu_timeline_result: one stream's timeline (56 bytes)."""
    _fields_ = [("rc", C.c_int32), ("placed", C.c_uint32), ("dropped", C.c_uint32), ("concealed", C.c_uint32),
                ("gaps", C.c_uint32), ("reserved", C.c_uint32), ("first_sample", C.c_uint64),
                ("timeline_samples", C.c_uint64), ("gap_samples", C.c_uint64), ("concealed_samples", C.c_uint64)]


class ShardCounters(C.Structure):
    """flacgpu_shard_counters: the four integers that cross shards of a stream (include/flacenc_gpu.h)."""
    _fields_ = [("frames", C.c_uint64), ("bytes", C.c_uint64), ("min_frame", C.c_uint64), ("max_frame", C.c_uint64)]

    def as_list(self):
        return [int(self.frames), int(self.bytes), int(self.min_frame), int(self.max_frame)]


class Segment(C.Structure):
    """flacgpu_segment: a run of whole blocks of one stream inside a batch of several (include/flacenc_gpu.h)."""
    _fields_ = [("pcm", C.c_void_p), ("n_frames", C.c_uint32), ("reserved", C.c_uint32), ("first_frame_number", C.c_uint64)]


class RaggedFrame(C.Structure):
    """flacgpu_ragged_frame: one frame of any length 1 .. block_size in a ragged batch (include/flacenc_gpu.h)."""
    _fields_ = [("pcm", C.c_void_p), ("samples", C.c_uint32), ("reserved", C.c_uint32), ("frame_number", C.c_uint64)]


class GpuStats(C.Structure):
    _fields_ = [
        ("frames", C.c_uint32),
        ("lpc_failed", C.c_uint32),
        ("order_ties", C.c_uint32),
        ("log2_edge", C.c_uint32),
        ("order_ties_resolved", C.c_uint32),
        ("fir_recheck", C.c_uint32),
        ("fir_rechecked", C.c_uint32),
        ("fixed_decided", C.c_uint32),
        ("fixed_refetched", C.c_uint32),
    ]


class LpcParams(C.Structure):
    """K4's record per (frame, candidate) (csrc/kernels/types.h LpcParams; flacgpu_device_buffer 7).  status: 0 ok,
    1 InsufficientLpcSamples / no candidate, 2 NoBestLpcOrder, 3 ZeroLpCoefficients, 4 LpNegativeShiftError."""
    _fields_ = [("status", C.c_int32), ("order", C.c_uint8), ("precision", C.c_uint8), ("shift", C.c_uint8),
                ("est8", C.c_uint8), ("qlp", C.c_int32 * 32)]


_lib = None


class LibraryMissing(RuntimeError):
    pass


_load_lock = threading.Lock()


def lib():
    """Load libflacenc_amd.so.  Fails loudly when the HIP extension is not built.  Thread-safe:
    writers are used from many threads, and a half-bound library (default `int` return types
    truncate pointers) must never be visible."""
    global _lib
    if _lib is not None:
        return _lib
    with _load_lock:
        if _lib is None:
            _lib = _load()
    return _lib


def _load():
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    ip = C.POINTER(C.c_int32)
    L.flacgpu_create.argtypes = [C.POINTER(GpuOptions), C.c_uint32, C.c_uint32, C.c_int,
                                 C.c_uint32, C.POINTER(vp)]
    L.flacgpu_destroy.argtypes = [vp]
    L.flacgpu_destroy.restype = None
    L.flacgpu_last_error.restype = C.c_char_p
    L.flacgpu_analyze.argtypes = [vp, ip, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(FramePlan),
                                  C.POINTER(SubframePlan), ip]
    L.flacgpu_analyze_device.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, vp]
    L.flacgpu_fetch.argtypes = [vp, C.POINTER(FramePlan), C.POINTER(SubframePlan), ip]
    L.flacgpu_get_stats.argtypes = [vp, C.POINTER(GpuStats)]
    L.flacgpu_resolve.argtypes = [vp]
    L.flacgpu_device_buffer.argtypes = [vp, C.c_int]
    L.flacgpu_device_buffer.restype = vp
    # test hooks (not in the public header): K4 alone on rows of autocorrelations, and its host restatement on one row
    u32p = C.POINTER(C.c_uint32)
    L.flacgpu_test_lpc_rows.argtypes = [vp, C.POINTER(C.c_double), C.c_uint32, u32p, u32p, C.c_uint32, vp, u32p, u32p]
    L.flacenc_lpc_host_row.argtypes = [C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.flacenc_lpc_host_row.restype = None
    L.flacgpu_set_timing.argtypes = [vp, C.c_int]
    L.flacgpu_get_kernel_ms.argtypes = [vp, C.POINTER(C.c_float * N_KERNELS)]
    L.flacgpu_pack_device.argtypes = [vp, C.c_uint64, C.c_uint32, vp]
    L.flacgpu_set_tuning.argtypes = [vp, C.c_int, C.c_int]
    L.flacgpu_encode_device.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, vp]
    L.flacgpu_fetch_frames.argtypes = [vp, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]
    L.flacgpu_encode_frames.argtypes = [vp, ip, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64,
                                        C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]
    L.flacenc_pack_frames.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                      C.c_uint32, C.c_void_p, C.c_void_p, ip, C.c_uint32,
                                      C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.flacgpu_decode_stream.argtypes = [C.c_char_p, C.c_size_t, C.c_int, ip, C.c_size_t, C.POINTER(StreamInfo)]
    L.flacgpu_scan_stream_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(StreamInfo), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]
    L.flacgpu_decoder_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.flacgpu_decoder_destroy.argtypes = [vp]
    L.flacgpu_decoder_destroy.restype = None
    L.flacgpu_decoder_scan.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32,
                                       C.POINTER(DecodedStream), C.POINTER(C.c_uint64)]
    L.flacgpu_decoder_decode.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.POINTER(DecodedStream)]
    L.flacgpu_decoder_plan_output.argtypes = [C.POINTER(OutFormat), C.POINTER(DecodedStream), C.c_uint32,
                                              C.POINTER(C.c_uint64)]
    L.flacgpu_decoder_decode_as.argtypes = [vp, vp, C.c_size_t, C.POINTER(OutFormat), C.c_uint32,
                                            C.POINTER(DecodedStream)]
    L.flacgpu_decoder_plan_windows.argtypes = [C.POINTER(OutFormat), C.POINTER(DecodedStream), C.c_uint32,
                                               C.POINTER(Window), C.c_uint32, C.POINTER(C.c_uint64)]
    L.flacgpu_decoder_decode_windows.argtypes = [vp, vp, C.c_size_t, C.POINTER(OutFormat), C.c_uint32,
                                                 C.POINTER(Window), C.c_uint32, C.POINTER(WindowResult)]
    L.flacgpu_window_frames.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.c_uint64,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.flacgpu_scan_frames_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(FrameRecord), C.c_size_t,
                                           C.POINTER(C.c_uint32), C.POINTER(RawStream)]
    L.flacgpu_decoder_scan_frames.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32,
                                              C.POINTER(DecodedStream), C.POINTER(RawStream), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.flacgpu_scan_frames_host_ex.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(FrameRecord), C.c_size_t,
                                              C.POINTER(C.c_uint32), C.POINTER(RawStream)]
    L.flacgpu_decoder_scan_frames_ex.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32, C.c_uint32,
                                                 C.POINTER(DecodedStream), C.POINTER(RawStream), C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.flacgpu_decoder_scan_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32, vp,
                                              C.POINTER(DecodedStream), C.POINTER(C.c_uint64)]
    L.flacgpu_decoder_scan_frames_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_uint32,
                                                     C.c_uint32, vp, C.POINTER(DecodedStream), C.POINTER(RawStream),
                                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.flacgpu_decoder_slot_bytes.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_uint64)]
    L.flacgpu_meta_walk_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(StreamInfo), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint64)]
    u8p, szp, q = C.POINTER(C.c_uint8), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)
    feed_out = [C.POINTER(DecodedStream), C.POINTER(RawStream), q, q, q]
    L.flacgpu_decoder_session_open.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.flacgpu_decoder_session_feed.argtypes = [vp, C.POINTER(C.c_void_p), szp, u8p] + feed_out
    L.flacgpu_decoder_session_feed_device.argtypes = [vp, C.POINTER(C.c_void_p), szp, u8p, vp] + feed_out
    L.flacgpu_decoder_session_finish.argtypes = [vp] + feed_out
    L.flacgpu_decoder_session_pending.argtypes = [vp, q, q]
    L.flacgpu_decoder_session_last_feed_timing.argtypes = [vp, C.POINTER(SessionTiming)]
    L.flacgpu_decoder_session_decoder.argtypes = [vp]
    L.flacgpu_decoder_session_decoder.restype = vp
    L.flacgpu_decoder_session_close.argtypes = [vp]
    L.flacgpu_decoder_session_close.restype = None
    L.flacgpu_session_host_open.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.flacgpu_session_host_feed.argtypes = [vp, C.POINTER(C.c_void_p), szp, u8p, C.POINTER(FrameRecord), C.c_size_t,
                                            C.POINTER(RawStream), q, q]
    L.flacgpu_session_host_finish.argtypes = [vp, C.POINTER(FrameRecord), C.c_size_t, C.POINTER(RawStream), q]
    L.flacgpu_session_host_close.argtypes = [vp]
    L.flacgpu_session_host_close.restype = None
    L.flacgpu_session_slots_host.argtypes = [C.POINTER(SessionSlotSrc), C.c_uint32, vp, C.c_size_t, q]
    L.flacgpu_decoder_session_open_container.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.flacgpu_decoder_session_verdict.argtypes = [vp, C.POINTER(DecodedStream)]
    L.flacgpu_session_host_open_container.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.flacgpu_meta_feed_init_host.argtypes = [C.POINTER(MetaFeedState)]
    L.flacgpu_meta_feed_init_host.restype = None
    L.flacgpu_meta_feed_host.argtypes = [C.POINTER(MetaFeedState), C.c_char_p, C.c_size_t, szp]
    L.flacgpu_meta_feed_result_host.argtypes = [C.POINTER(MetaFeedState), C.c_uint64, C.POINTER(StreamInfo),
                                                C.POINTER(C.c_uint32), q]
    L.flacgpu_decoder_frame_records.argtypes = [vp, C.POINTER(FrameRecord), C.c_size_t]
    L.flacgpu_decoder_decode_frames.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.POINTER(FrameRecord), C.c_size_t]
    L.flacgpu_analyze_frame_host.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(FrameAnalysis),
                                             C.POINTER(SubframePlan), vp, C.c_size_t]
    L.flacgpu_decoder_plan_analysis.argtypes = [vp, q, q, q]
    L.flacgpu_decoder_analyze.argtypes = [vp, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    L.flacgpu_timeline_host.argtypes = [C.POINTER(FrameRecord), C.c_size_t, C.POINTER(TimelineFrame), C.c_size_t,
                                        C.POINTER(TimelineResult)]
    L.flacgpu_timeline_piece_bytes.argtypes = []
    L.flacgpu_timeline_piece_bytes.restype = C.c_uint32
    L.flacgpu_decoder_plan_timeline.argtypes = [vp, C.POINTER(OutFormat), C.POINTER(TimelineResult),
                                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.flacgpu_decoder_decode_timeline.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(OutFormat), C.c_uint32,
                                                  C.POINTER(TimelineResult), C.POINTER(TimelineFrame), C.c_size_t]
    L.flacgpu_pack_plans.argtypes = [vp, ip, C.c_uint32, C.c_uint32, C.POINTER(FramePlan), C.POINTER(SubframePlan),
                                     C.c_uint64, C.c_uint32]
    L.flacgpu_host_alloc.argtypes = [C.c_size_t]
    L.flacgpu_host_alloc.restype = vp
    L.flacgpu_host_free.argtypes = [vp]
    L.flacgpu_host_free.restype = None
    L.flacgpu_current_device.argtypes = []
    L.flacgpu_packed_input_supported.argtypes = [vp, C.c_uint32]
    L.flacgpu_encode_packed_async.argtypes = [vp, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                              C.c_uint32]
    L.flacgpu_frames_ready.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
    L.flacgpu_fetch_frames_async.argtypes = [vp, C.c_void_p, C.c_size_t]
    L.flacgpu_wait.argtypes = [vp]
    L.flacgpu_verify_device.argtypes = [vp, C.c_uint32, C.c_uint64, C.POINTER(VerifyResult),
                                        C.POINTER(C.c_float)]
    L.flacgpu_fetch_decoded.argtypes = [vp, ip]
    L.flacgpu_experiment_mfma_autocorr.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32),
                                                   C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    L.flacgpu_kernel_name.argtypes = [C.c_int]
    L.flacgpu_kernel_name.restype = C.c_char_p
    L.flacgpu_packed_cap.argtypes = [vp]
    L.flacgpu_packed_cap.restype = C.c_size_t
    L.flacgpu_pipeline_create.argtypes = [C.POINTER(GpuOptions), C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                          C.POINTER(vp)]
    L.flacgpu_pipeline_destroy.argtypes = [vp]
    L.flacgpu_pipeline_destroy.restype = None
    L.flacgpu_pipeline_submit.argtypes = [vp, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]
    L.flacgpu_pipeline_retire.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_uint64)),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.flacgpu_pipeline_in_flight.argtypes = [vp]
    L.flacgpu_pipeline_in_flight.restype = C.c_uint32
    L.flacgpu_pipeline_depth.argtypes = [vp]
    L.flacgpu_pipeline_depth.restype = C.c_uint32
    L.flacgpu_link_probe.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.flacgpu_encode_segments_device.argtypes = [vp, C.POINTER(Segment), C.c_uint32, C.c_uint32, vp]
    L.flacgpu_encode_segments.argtypes = [vp, C.POINTER(Segment), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.flacgpu_encode_segments_packed_async_host.argtypes = [vp, C.c_void_p, C.c_uint32, C.POINTER(Segment), C.c_uint32,
                                                            C.c_uint32, C.c_void_p, C.c_size_t]
    L.flacgpu_encode_ragged_device.argtypes = [vp, C.POINTER(RaggedFrame), C.c_uint32, C.c_uint32, vp]
    u32p = C.POINTER(C.c_uint32)
    L.flacgpu_ragged_plan.argtypes = [C.POINTER(GpuOptions), u32p, C.c_uint32, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
    L.flacgpu_ragged_pool_uploads.argtypes = [vp]
    L.flacgpu_ragged_pool_uploads.restype = C.c_uint64
    sc = C.POINTER(ShardCounters)
    u64p = C.POINTER(C.c_uint64)
    L.flacgpu_merge_counters.argtypes = [sc, C.c_uint32, sc, u64p]
    L.flacgpu_shard_range.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p]
    L.flacgpu_shard_range.restype = None
    L.flacgpu_device_count.argtypes = []
    L.flacgpu_multi_create.argtypes = [C.POINTER(GpuOptions), C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.flacgpu_multi_destroy.argtypes = [vp]
    L.flacgpu_multi_destroy.restype = None
    L.flacgpu_multi_shards.argtypes = [vp]
    L.flacgpu_multi_shards.restype = C.c_uint32
    L.flacgpu_multi_device_of.argtypes = [vp, C.c_uint32]
    L.flacgpu_multi_host_copy_stats.argtypes = [vp, u64p, u64p, C.POINTER(C.c_uint32)]
    L.flacgpu_device_numa_info.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.flacgpu_multi_encode.argtypes = [vp, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32,
                                       C.c_void_p, C.c_size_t, u64p, u64p, sc, sc]
    L.flacgpu_multi_encode_device.argtypes = [vp, C.c_uint32, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]
    L.flacgpu_multi_wait.argtypes = [vp]
    L.flacgpu_multi_counters.argtypes = [vp, sc, sc]
    L.flacgpu_multi_last_context.argtypes = [vp, C.c_uint32]
    L.flacgpu_multi_last_context.restype = vp
    L.flacgpu_rccl_available.argtypes = []
    L.flacgpu_rccl_allgather_counters.argtypes = [vp, vp, sc, sc, C.c_uint32, C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_uint32)]
    L.flacgpu_md5_chains_create.argtypes = [C.c_int, C.c_uint32, C.POINTER(vp)]
    L.flacgpu_md5_chains_destroy.argtypes = [vp]
    L.flacgpu_md5_chains_destroy.restype = None
    L.flacgpu_md5_chains_update.argtypes = [vp, vp, C.POINTER(Md5Piece), C.c_uint32, C.c_uint32, vp]
    L.flacgpu_md5_chains_final.argtypes = [vp, C.c_void_p]
    L.flacgpu_md5_stage_bytes.argtypes = []
    L.flacgpu_md5_stage_bytes.restype = C.c_uint32
    L.flacgpu_md5_init_host.argtypes = [C.POINTER(Md5State)]
    L.flacgpu_md5_init_host.restype = None
    L.flacgpu_md5_feed_host.argtypes = [C.POINTER(Md5State), C.c_void_p, C.c_uint64, C.c_uint32]
    L.flacgpu_md5_final_host.argtypes = [C.POINTER(Md5State), C.c_void_p]
    L.flacgpu_build_id.argtypes = []
    L.flacgpu_build_id.restype = C.c_char_p
    return L


def build_id():
    """flacgpu_build_id() of the loaded library (hash of the sources it was built from)."""
    return lib().flacgpu_build_id().decode()


def source_build_id():
    """The same hash computed from the sources in the tree (None when they are not there): differs from build_id()
    when the library is stale."""
    import hashlib

    src = os.path.join(_HERE, "csrc")
    files = []
    for sub, pat in (("", ".hip"), ("host", ""), ("kernels", "")):
        d = os.path.join(src, sub)
        if not os.path.isdir(d):
            return None
        files += [os.path.join(sub, f) for f in os.listdir(d)
                  if f.endswith(pat) and os.path.isfile(os.path.join(d, f))]
    files.append("Makefile")
    h = hashlib.sha256()
    for f in sorted(files):      # make's $(sort): byte order
        h.update(open(os.path.join(src, f), "rb").read())
    return h.hexdigest()[:16]


def exported_symbols():
    """Names of the dynamic symbols the shared library exports (for the ABI test)."""
    import subprocess

    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}
