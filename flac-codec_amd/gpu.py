"""Thin Python handle on the analysis C ABI (include/flacenc_gpu.h).

`GpuAnalyzer` replaces the analysis half of the reference's `encode_frame`
(/root/reference/src/encode.rs:2259-2406) for a batch of frames.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FramePlan, GpuOptions, GpuStats, SubframePlan

LAYOUT_INTERLEAVED, LAYOUT_PLANAR = 0, 1

# _lib.LpcParams as a numpy record (GpuAnalyzer.lpc_params, test_lpc_rows)
LPC_DTYPE = np.dtype([("status", "<i4"), ("order", "u1"), ("precision", "u1"), ("shift", "u1"), ("est8", "u1"),
                      ("qlp", "<i4", (32,))])
assert LPC_DTYPE.itemsize == C.sizeof(_lib.LpcParams)


class GpuError(RuntimeError):
    def __init__(self, code, where):
        msg = _lib.lib().flacgpu_last_error().decode(errors="replace")
        super().__init__(f"{where}: flacgpu error {code}: {msg}")
        self.code = code


class GpuAnalyzer:
    def __init__(self, block_size, max_partition_order, max_lpc_order, mid_side, exhaustive,
                 window_kind, window_param, bits_per_sample, channels, max_frames, device=-1):
        L = _lib.lib()
        o = GpuOptions(block_size, max_partition_order, max_lpc_order or 0, int(bool(mid_side)),
                       int(bool(exhaustive)), window_kind, 0, window_param)
        self._h = C.c_void_p(None)
        self.block_size, self.channels, self.max_frames = block_size, channels, max_frames
        self.bits_per_sample = bits_per_sample
        self.last_frames = 0   # frames of the batch submitted last (sizes the offsets arrays)
        rc = L.flacgpu_create(C.byref(o), bits_per_sample, channels, device, max_frames,
                              C.byref(self._h))
        if rc:
            raise GpuError(rc, "flacgpu_create")

    def close(self):
        if self._h:
            _lib.lib().flacgpu_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _alloc(self, n_frames):
        plans = (FramePlan * n_frames)()
        subs = (SubframePlan * (n_frames * self.channels))()
        res = np.empty((n_frames, self.channels, self.block_size), dtype=np.int32)
        return plans, subs, res

    def analyze(self, pcm, n_frames, last_frame_len, layout=LAYOUT_INTERLEAVED):
        """pcm: host int32 array.  Returns (frame plans, subframe plans, residuals)."""
        self.last_frames = n_frames
        pcm = np.ascontiguousarray(pcm, dtype=np.int32)
        plans, subs, res = self._alloc(n_frames)
        rc = _lib.lib().flacgpu_analyze(
            self._h, pcm.ctypes.data_as(C.POINTER(C.c_int32)), layout, n_frames, last_frame_len,
            plans, subs, res.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc:
            raise GpuError(rc, "flacgpu_analyze")
        return plans, subs, res

    def analyze_device(self, device_ptr, n_frames, last_frame_len, layout=LAYOUT_INTERLEAVED,
                       stream=None):
        self.last_frames = n_frames
        rc = _lib.lib().flacgpu_analyze_device(self._h, C.c_void_p(device_ptr), layout, n_frames,
                                               last_frame_len, C.c_void_p(stream or 0))
        if rc:
            raise GpuError(rc, "flacgpu_analyze_device")

    def fetch(self, n_frames, want_residuals=True):
        plans, subs, res = self._alloc(n_frames)
        rc = _lib.lib().flacgpu_fetch(
            self._h, plans, subs,
            res.ctypes.data_as(C.POINTER(C.c_int32)) if want_residuals else None)
        if rc:
            raise GpuError(rc, "flacgpu_fetch")
        return plans, subs, res

    TUNE_TWO_RANGES, TUNE_LAG_SPLIT, TUNE_BLOCKING_WAIT, TUNE_COPY_INPUT, TUNE_CHUNK_MSAMPLES = 1, 2, 3, 4, 5

    def set_tuning(self, key, value):
        rc = _lib.lib().flacgpu_set_tuning(self._h, key, value)
        if rc:
            raise GpuError(rc, "flacgpu_set_tuning")

    def set_two_ranges(self, on):
        """Cut big batches of 4096-sample frames into two frame ranges on two HIP streams
        (FLACGPU_TUNE_TWO_RANGES); off by default."""
        self.set_tuning(self.TUNE_TWO_RANGES, 1 if on else 0)

    def encode_device(self, device_ptr, n_frames, last_frame_len, first_frame_number, sample_rate,
                      layout=LAYOUT_INTERLEAVED, stream=None):
        """analyze_device + pack_device in one call (see set_two_ranges)."""
        self.last_frames = n_frames
        rc = _lib.lib().flacgpu_encode_device(self._h, C.c_void_p(device_ptr), layout, n_frames,
                                              last_frame_len, first_frame_number, sample_rate,
                                              C.c_void_p(stream or 0))
        if rc:
            raise GpuError(rc, "flacgpu_encode_device")

    def encode_segments(self, segments, sample_rate):
        """segments: [(host int32 array of whole blocks, first_frame_number), ...] of streams of this context's shape, encoded
        as ONE batch (flacgpu_encode_segments).  Returns (bytes, offsets[total_frames + 1]): frames in segment order."""
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a, _ in segments]
        per = self.block_size * self.channels
        segs = (_lib.Segment * len(arrs))()
        total = 0
        for i, (a, (_, first)) in enumerate(zip(arrs, segments)):
            assert a.size % per == 0 and a.size
            segs[i].pcm, segs[i].n_frames, segs[i].first_frame_number = a.ctypes.data, a.size // per, first
            total += a.size // per
        self.last_frames = total
        off = (C.c_uint64 * (total + 1))()
        tot = C.c_uint64(0)
        cap = total * (per * 4 + 64) + 256
        buf = np.empty(cap, dtype=np.uint8)
        rc = _lib.lib().flacgpu_encode_segments(self._h, segs, len(arrs), sample_rate, C.c_void_p(buf.ctypes.data), cap, off,
                                                C.byref(tot))
        if rc:
            raise GpuError(rc, "flacgpu_encode_segments")
        return buf[: tot.value].tobytes(), [int(v) for v in off]

    def encode_segments_device(self, segments, sample_rate, stream=None):
        """segments: [(device pointer, n_frames, first_frame_number), ...]; asynchronous (fetch_frames() for the result)."""
        segs = (_lib.Segment * len(segments))()
        total = 0
        for i, (ptr, n, first) in enumerate(segments):
            segs[i].pcm, segs[i].n_frames, segs[i].first_frame_number = ptr, n, first
            total += n
        self.last_frames = total
        rc = _lib.lib().flacgpu_encode_segments_device(self._h, segs, len(segments), sample_rate, C.c_void_p(stream or 0))
        if rc:
            raise GpuError(rc, "flacgpu_encode_segments_device")

    def encode_ragged_device(self, frames, sample_rate, stream=None):
        """frames: [(device pointer, samples, frame_number), ...] -- frames of any length 1 .. block_size, of any streams of
        this context's shape, encoded as ONE batch (flacgpu_encode_ragged_device); asynchronous (fetch_frames() for the
        result).  Every frame's bytes are those of a one-frame encode_device call."""
        tab = (_lib.RaggedFrame * max(len(frames), 1))()
        for i, (ptr, n, number) in enumerate(frames):
            tab[i].pcm, tab[i].samples, tab[i].reserved, tab[i].frame_number = ptr, n, 0, number
        rc = _lib.lib().flacgpu_encode_ragged_device(self._h, tab, len(frames), sample_rate, C.c_void_p(stream or 0))
        if rc:
            raise GpuError(rc, "flacgpu_encode_ragged_device")
        self.last_frames = len(frames)

    def ragged_pool_uploads(self):
        """How often this context has uploaded its ragged window pool (a batch whose lengths are all in the pool uploads none)."""
        return int(_lib.lib().flacgpu_ragged_pool_uploads(self._h))

    def pack_plans(self, pcm, n_frames, last_frame_len, plans, subframes, first_frame_number, sample_rate):
        """flacgpu_pack_plans: device-side frame assembly of caller-supplied decisions.  Returns (bytes, offsets)."""
        a = np.ascontiguousarray(pcm, dtype=np.int32)
        rc = _lib.lib().flacgpu_pack_plans(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), n_frames, last_frame_len, plans,
                                           subframes, first_frame_number, sample_rate)
        if rc:
            raise GpuError(rc, "flacgpu_pack_plans")
        self.last_frames = n_frames
        return self.fetch_frames(n_frames)

    def pack_device(self, first_frame_number, sample_rate, stream=None):
        """Device-side frame assembly of the last analysed batch (bytes stay in HBM)."""
        rc = _lib.lib().flacgpu_pack_device(self._h, first_frame_number, sample_rate,
                                            C.c_void_p(stream or 0))
        if rc:
            raise GpuError(rc, "flacgpu_pack_device")

    def fetch_frames(self, n_frames=None):
        """Returns (bytes, offsets[n_frames+1]) of the frames packed on the device."""
        held = self.last_frames or n_frames
        if n_frames is not None and held != n_frames:
            raise ValueError(f"the context holds a batch of {held} frames, not {n_frames}")
        n_frames = held
        off = (C.c_uint64 * (n_frames + 1))()
        total = C.c_uint64(0)
        L = _lib.lib()
        rc = L.flacgpu_fetch_frames(self._h, None, 0, off, C.byref(total))
        if rc not in (0, -5):
            raise GpuError(rc, "flacgpu_fetch_frames")
        buf = np.empty(total.value, dtype=np.uint8)
        rc = L.flacgpu_fetch_frames(self._h, buf.ctypes.data, buf.size, off, C.byref(total))
        if rc:
            raise GpuError(rc, "flacgpu_fetch_frames")
        return buf.tobytes(), list(off)

    def encode_frames(self, pcm, n_frames, last_frame_len, first_frame_number, sample_rate,
                      layout=LAYOUT_INTERLEAVED):
        """analyze + pack + fetch on host PCM; returns (bytes, offsets)."""
        self.last_frames = n_frames
        pcm = np.ascontiguousarray(pcm, dtype=np.int32)
        cap = pcm.size * 4 + n_frames * 128 + 1024
        buf = np.empty(cap, dtype=np.uint8)
        off = (C.c_uint64 * (n_frames + 1))()
        total = C.c_uint64(0)
        rc = _lib.lib().flacgpu_encode_frames(
            self._h, pcm.ctypes.data_as(C.POINTER(C.c_int32)), layout, n_frames, last_frame_len,
            first_frame_number, sample_rate, buf.ctypes.data, cap, off, C.byref(total))
        if rc:
            raise GpuError(rc, "flacgpu_encode_frames")
        return buf[: total.value].tobytes(), list(off)

    def encode_frames_pinned(self, pcm, n_frames, last_frame_len, first_frame_number, sample_rate, repeat=1,
                             layout=LAYOUT_INTERLEAVED):
        """flacgpu_encode_frames with BOTH host buffers in pinned memory (flacgpu_host_alloc), which is what a caller
        that cares about the PCIe leg hands over: the copies run at the link's rate instead of through the runtime's
        staging of pageable memory.  `repeat` calls back to back; returns (bytes, offsets, seconds per call)."""
        import time

        self.last_frames = n_frames
        L = _lib.lib()
        pcm = np.ascontiguousarray(pcm, dtype=np.int32)
        cap = pcm.size * 4 + n_frames * 128 + 1024
        hin = L.flacgpu_host_alloc(pcm.nbytes + 64)
        hout = L.flacgpu_host_alloc(cap)
        if not hin or not hout:
            if hin:
                L.flacgpu_host_free(hin)
            if hout:
                L.flacgpu_host_free(hout)
            raise MemoryError("flacgpu_host_alloc")
        try:
            C.memmove(hin, pcm.ctypes.data, pcm.nbytes)
            off = (C.c_uint64 * (n_frames + 1))()
            total = C.c_uint64(0)
            times = []
            for _ in range(repeat):
                t = time.perf_counter()
                rc = L.flacgpu_encode_frames(self._h, C.cast(hin, C.POINTER(C.c_int32)), layout, n_frames, last_frame_len,
                                             first_frame_number, sample_rate, hout, cap, off, C.byref(total))
                times.append(time.perf_counter() - t)
                if rc:
                    raise GpuError(rc, "flacgpu_encode_frames")
            return C.string_at(hout, total.value), list(off), times
        finally:
            L.flacgpu_host_free(hin)
            L.flacgpu_host_free(hout)

    def encode_packed(self, pcm_le, bytes_per_sample, n_frames, last_frame_len, first_frame_number,
                      sample_rate, pinned=True):
        """The asynchronous host path in one go (flacgpu_encode_packed_async -> frames_ready ->
        fetch_frames_async -> wait): pcm_le = interleaved little-endian samples of bytes_per_sample
        bytes (uint8 array).  Returns (bytes, offsets)."""
        self.last_frames = n_frames
        L = _lib.lib()
        src = np.ascontiguousarray(pcm_le, dtype=np.uint8)
        hin = hout = None
        try:
            if pinned:
                hin = L.flacgpu_host_alloc(src.size + 64)
                C.memmove(hin, src.ctypes.data, src.size)
            rc = L.flacgpu_encode_packed_async(self._h, hin if pinned else src.ctypes.data, bytes_per_sample,
                                               n_frames, last_frame_len, first_frame_number, sample_rate)
            if rc:
                raise GpuError(rc, "flacgpu_encode_packed_async")
            offp = C.POINTER(C.c_uint64)()
            total = C.c_uint64(0)
            rc = L.flacgpu_frames_ready(self._h, C.byref(offp), C.byref(total))
            if rc:
                raise GpuError(rc, "flacgpu_frames_ready")
            off = [offp[i] for i in range(n_frames + 1)]
            if pinned:
                hout = L.flacgpu_host_alloc(total.value + 64)
                dst = hout
            else:
                buf = np.empty(total.value + 64, dtype=np.uint8)
                dst = buf.ctypes.data
            rc = L.flacgpu_fetch_frames_async(self._h, dst, total.value + 64)
            if rc:
                raise GpuError(rc, "flacgpu_fetch_frames_async")
            rc = L.flacgpu_wait(self._h)
            if rc:
                raise GpuError(rc, "flacgpu_wait")
            data = C.string_at(dst, total.value)
            return data, off
        finally:
            if hin:
                L.flacgpu_host_free(hin)
            if hout:
                L.flacgpu_host_free(hout)

    def encode_segments_packed(self, pcm_le, bytes_per_sample, segments, sample_rate):
        """flacgpu_encode_segments_packed_async_host in one go: pcm_le = the segments' whole blocks back to back (uint8 array of
        little-endian samples of bytes_per_sample bytes, or int32 samples viewed as bytes when bytes_per_sample == 4);
        segments = [(n_frames, first_frame_number), ...].  Pinned buffers both ways.  Returns (bytes, offsets)."""
        L = _lib.lib()
        src = np.ascontiguousarray(pcm_le).view(np.uint8).reshape(-1)
        n_frames = sum(n for n, _ in segments)
        self.last_frames = n_frames
        segs = (_lib.Segment * len(segments))()
        for i, (n, first) in enumerate(segments):
            segs[i].pcm = None
            segs[i].n_frames = n
            segs[i].first_frame_number = first
        cap = L.flacgpu_packed_cap(self._h)
        hin = L.flacgpu_host_alloc(src.size + 64)
        hout = L.flacgpu_host_alloc(cap)
        try:
            C.memmove(hin, src.ctypes.data, src.size)
            rc = L.flacgpu_encode_segments_packed_async_host(self._h, hin, bytes_per_sample, segs, len(segments), sample_rate,
                                                             hout, cap)
            if rc:
                raise GpuError(rc, "flacgpu_encode_segments_packed_async_host")
            offp = C.POINTER(C.c_uint64)()
            total = C.c_uint64(0)
            rc = L.flacgpu_frames_ready(self._h, C.byref(offp), C.byref(total))
            if rc:
                raise GpuError(rc, "flacgpu_frames_ready")
            off = [offp[i] for i in range(n_frames + 1)]
            rc = L.flacgpu_fetch_frames_async(self._h, hout, cap)
            if rc:
                raise GpuError(rc, "flacgpu_fetch_frames_async")
            rc = L.flacgpu_wait(self._h)
            if rc:
                raise GpuError(rc, "flacgpu_wait")
            return C.string_at(hout, total.value), off
        finally:
            L.flacgpu_host_free(hin)
            L.flacgpu_host_free(hout)

    def packed_input_supported(self, bytes_per_sample):
        return bool(_lib.lib().flacgpu_packed_input_supported(self._h, bytes_per_sample))

    def verify_device(self, sample_rate, first_frame_number=0):
        """Decode the frames packed last on the GPU, check CRC-16 and compare with the analysed
        PCM.  Returns (VerifyResult, kernel_ms)."""
        res = _lib.VerifyResult()
        ms = C.c_float(0)
        rc = _lib.lib().flacgpu_verify_device(self._h, sample_rate, first_frame_number,
                                              C.byref(res), C.byref(ms))
        if rc:
            raise GpuError(rc, "flacgpu_verify_device")
        return res, ms.value

    def fetch_decoded(self, n_frames, last_frame_len):
        n = ((n_frames - 1) * self.block_size + last_frame_len) * self.channels
        out = np.empty(n, dtype=np.int32)
        rc = _lib.lib().flacgpu_fetch_decoded(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc:
            raise GpuError(rc, "flacgpu_fetch_decoded")
        return out

    def device_buffer(self, which):
        return _lib.lib().flacgpu_device_buffer(self._h, which)

    def candidates_per_frame(self):
        """Candidate slots per frame: L, R, M, S for stereo below 32 bits, else one per channel."""
        return 4 if self.channels == 2 and self.bits_per_sample < 32 else self.channels

    def lpc_params(self):
        """K4's records of the last analysis (flacgpu_device_buffer 7: after the host's re-decision of order ties), one
        per (frame, candidate), as a structured array of LPC_DTYPE.  The fields behind a non-zero status are stale."""
        out = np.zeros(self.last_frames * self.candidates_per_frame(), dtype=LPC_DTYPE)
        src = self.device_buffer(7)
        if not src:
            raise GpuError(-1, "flacgpu_device_buffer(7)")
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = hip.hipMemcpy(out.ctypes.data, src, out.nbytes, 2)   # hipMemcpyDeviceToHost
        if rc:
            raise RuntimeError(f"hipMemcpy of the LPC records: HIP error {rc}")
        return out

    def test_lpc_rows(self, ac, n, bps):
        """flacgpu_test_lpc_rows (a test hook): K4 alone, through the product's launcher for this context's max_lpc_order,
        on rows of f64 autocorrelations ([rows][lags], lags 0 .. max_lpc_order in front, at most 36) with a length and an
        effective bps per row.  Returns (records as K4 left them, LPC_DTYPE; the rows K4 listed as order ties;
        [lpc_failed, order_ties, log2_edge] of the launch)."""
        ac = np.ascontiguousarray(ac, dtype=np.float64)
        rows, ld = ac.shape
        n = np.ascontiguousarray(n, dtype=np.uint32)
        bps = np.ascontiguousarray(bps, dtype=np.uint32)
        assert n.shape == (rows,) and bps.shape == (rows,)
        out = np.zeros(rows, dtype=LPC_DTYPE)
        ties = np.zeros(rows, dtype=np.uint32)
        counters = np.zeros(3, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        rc = _lib.lib().flacgpu_test_lpc_rows(self._h, ac.ctypes.data_as(C.POINTER(C.c_double)), ld, n.ctypes.data_as(u32p),
                                              bps.ctypes.data_as(u32p), rows, out.ctypes.data, ties.ctypes.data_as(u32p),
                                              counters.ctypes.data_as(u32p))
        if rc:
            raise GpuError(rc, "flacgpu_test_lpc_rows")
        return out, sorted(int(v) for v in ties[:min(int(counters[1]), rows)]), [int(v) for v in counters]

    def experiment_mfma_autocorr(self):
        """EXPERIMENT (not on the product path): f64-MFMA autocorrelation of the last batch.
        Returns dict(ms, compared, params_differ, max_rel_err)."""
        ms, cmp_, diff, err = C.c_float(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0)
        rc = _lib.lib().flacgpu_experiment_mfma_autocorr(self._h, C.byref(ms), C.byref(cmp_),
                                                         C.byref(diff), C.byref(err))
        if rc:
            raise GpuError(rc, "flacgpu_experiment_mfma_autocorr")
        return {"ms": ms.value, "compared": cmp_.value, "params_differ": diff.value,
                "max_rel_err": err.value}

    def stats(self):
        s = GpuStats()
        rc = _lib.lib().flacgpu_get_stats(self._h, C.byref(s))
        if rc:
            raise GpuError(rc, "flacgpu_get_stats")
        return s

    def handed_subframes(self):
        """(handed, subframes, enabled) of the last batch: subframes whose residual the candidate kernel handed to the frame
        kernel (flacgpu_handed_subframes)"""
        L = _lib.lib()
        h, n, e = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        L.flacgpu_handed_subframes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        rc = L.flacgpu_handed_subframes(self._h, C.byref(h), C.byref(n), C.byref(e))
        if rc:
            raise GpuError(rc, "flacgpu_handed_subframes")
        return h.value, n.value, bool(e.value)

    def set_timing(self, on=True):
        _lib.lib().flacgpu_set_timing(self._h, int(on))

    def kernel_ms(self):
        arr = (C.c_float * _lib.N_KERNELS)()
        _lib.lib().flacgpu_get_kernel_ms(self._h, C.byref(arr))
        L = _lib.lib()
        return {L.flacgpu_kernel_name(i).decode(): float(arr[i]) for i in range(_lib.N_KERNELS)
                if arr[i] > 0}


def decode_stream(data, device=-1, want_pcm=True):
    """Stand-alone GPU decode + verify of a whole FLAC stream (flacgpu_decode_stream): returns
    (interleaved int32 PCM or None, StreamInfo)."""
    L = _lib.lib()
    info = _lib.StreamInfo()
    data = bytes(data)
    rc = L.flacgpu_decode_stream(data, len(data), device, None, 0, C.byref(info))   # sizes + verification
    if rc:
        raise GpuError(rc, "flacgpu_decode_stream")
    if not want_pcm:
        return None, info
    out = np.empty(info.decoded_samples * info.channels, dtype=np.int32)
    rc = L.flacgpu_decode_stream(data, len(data), device, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size,
                                 C.byref(info))
    if rc:
        raise GpuError(rc, "flacgpu_decode_stream")
    return out, info


def scan_stream_host(data):
    """flacgpu_scan_stream_host: the metadata parse and frame scan flacgpu_decode_stream starts with, on the host alone
    (no GPU needed).  Returns (StreamInfo, frame start offsets, block sizes)."""
    L = _lib.lib()
    info = _lib.StreamInfo()
    data = bytes(data)
    n = C.c_uint32(0)
    rc = L.flacgpu_scan_stream_host(data, len(data), C.byref(info), None, None, 0, C.byref(n))   # the count
    if rc:
        raise GpuError(rc, "flacgpu_scan_stream_host")
    offsets, sizes = np.empty(n.value, dtype=np.uint64), np.empty(n.value, dtype=np.uint32)
    rc = L.flacgpu_scan_stream_host(data, len(data), C.byref(info), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    sizes.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n))
    if rc:
        raise GpuError(rc, "flacgpu_scan_stream_host")
    return info, offsets, sizes


FRAME_DTYPE = np.dtype([(name, np.dtype(ct).str) for name, ct in _lib.FrameRecord._fields_])   # flacgpu_frame_record


def scan_frames_host(data, speculative=False):
    """flacgpu_scan_frames_host_ex: the kept frames of a raw frame stream (bare frames, no fLaC marker, no STREAMINFO) by
    the rule of DESIGN.md "Raw frame streams", on the host alone (no GPU needed).  Returns (frames, RawStream): a
    structured array of FRAME_DTYPE records and the summary.  speculative=True (FLACGPU_SCAN_SPECULATIVE): a frame that
    no header ends is ended by its own bits, and its record has _lib.FRAME_SPECULATIVE in `reserved`."""
    L = _lib.lib()
    data = bytes(data)
    flags = _lib.SCAN_SPECULATIVE if speculative else 0
    n, raw = C.c_uint32(0), _lib.RawStream()
    rc = L.flacgpu_scan_frames_host_ex(data, len(data), flags, None, 0, C.byref(n), C.byref(raw))   # the count
    if rc:
        raise GpuError(rc, "flacgpu_scan_frames_host_ex")
    frames = np.zeros(n.value, dtype=FRAME_DTYPE)
    rc = L.flacgpu_scan_frames_host_ex(data, len(data), flags, frames.ctypes.data_as(C.POINTER(_lib.FrameRecord)),
                                       n.value, C.byref(n), C.byref(raw))
    if rc:
        raise GpuError(rc, "flacgpu_scan_frames_host_ex")
    return frames, raw


# flacgpu_frame_analysis / flacgpu_subframe_plan as flacgpu_decoder_analyze fills them
ANALYSIS_FRAME_DTYPE = np.dtype(_lib.FrameAnalysis)
SUBFRAME_DTYPE = np.dtype(_lib.SubframePlan)


def analyze_frame_host(frame, streaminfo_bps=0, rows=True):
    """flacgpu_analyze_frame_host: what one frame (header .. CRC-16, as a scan gives it) is made of, on the host alone
    (no GPU needed).  Returns (analysis, subframes, rows64): an ANALYSIS_FRAME_DTYPE record, a SUBFRAME_DTYPE array of
    the frame's channels, and -- rows=True -- an int64 array [channels, roundup4(block_size)] (None otherwise, and for
    a frame whose header does not parse).  analysis["status"] bit 0: the frame does not parse; the subframe records
    and rows are then unspecified."""
    frame = bytes(frame)
    fa = np.zeros(1, dtype=ANALYSIS_FRAME_DTYPE)
    subs = np.zeros(8, dtype=SUBFRAME_DTYPE)
    L = _lib.lib()

    def call(buf):
        rc = L.flacgpu_analyze_frame_host(frame, len(frame), streaminfo_bps,
                                          fa.ctypes.data_as(C.POINTER(_lib.FrameAnalysis)),
                                          subs.ctypes.data_as(C.POINTER(_lib.SubframePlan)),
                                          buf.ctypes.data if buf is not None and buf.size else None,
                                          buf.size if buf is not None else 0)
        if rc:
            raise GpuError(rc, "flacgpu_analyze_frame_host")

    call(None)   # the records alone: they say how large the rows are
    ch, n = int(fa[0]["plan"]["channels"]), int(fa[0]["block_size"])
    rows64 = None
    if rows and ch and n:
        rows64 = np.zeros((ch, (n + 3) & ~3), dtype=np.int64)
        call(rows64)
    return fa[0], subs[:ch], rows64


class FrameAnalysis:
    """What analyze_many / Decoder.analyze return: `frames` (ANALYSIS_FRAME_DTYPE) and `subframes` (SUBFRAME_DTYPE) are
    numpy structured arrays mirroring flacgpu_frame_analysis and flacgpu_subframe_plan; `rows` is flat int32 -- a numpy
    array, a CUDA tensor for out="device", None for the records-only pass."""
    __slots__ = ("frames", "subframes", "rows")

    def __init__(self, frames, subframes, rows):
        self.frames, self.subframes, self.rows = frames, subframes, rows

    def subframes_of(self, f):
        """The subframe records of frame f, one per channel."""
        at = int(self.frames[f]["first_subframe"])
        return self.subframes[at:at + int(self.frames[f]["plan"]["channels"])]

    def row(self, f, c):
        """The block_size elements of channel c's row of frame f (a CONSTANT row is defined at [0] alone)."""
        n = int(self.frames[f]["block_size"])
        at = int(self.frames[f]["row_offset"]) + c * ((n + 3) & ~3)
        return self.rows[at:at + n]


TIMELINE_FRAME_DTYPE = np.dtype([(name, np.dtype(ct).str) for name, ct in _lib.TimelineFrame._fields_])


def timeline_piece_bytes():
    """flacgpu_timeline_piece_bytes: the most bytes one workgroup of the timeline's fill kernel writes."""
    return int(_lib.lib().flacgpu_timeline_piece_bytes())


def scan_timeline_host(records):
    """flacgpu_timeline_host: the timeline rule (include/flacenc_gpu.h "raw frame streams on a timeline") for the records
    of one stream -- a FRAME_DTYPE array as scan_frames_host returns it -- on the host alone (no GPU needed).  Returns
    (TimelineResult, frames): `frames` is a TIMELINE_FRAME_DTYPE array, one entry per record (at, flags, status)."""
    records = np.ascontiguousarray(records, dtype=FRAME_DTYPE)
    frames = np.zeros(records.size, dtype=TIMELINE_FRAME_DTYPE)
    result = _lib.TimelineResult()
    rc = _lib.lib().flacgpu_timeline_host(records.ctypes.data_as(C.POINTER(_lib.FrameRecord)), records.size,
                                          frames.ctypes.data_as(C.POINTER(_lib.TimelineFrame)), frames.size,
                                          C.byref(result))
    if rc:
        raise GpuError(rc, "flacgpu_timeline_host")
    return result, frames


def is_device_blob(b):
    """True for a torch tensor (a stream handed over in device memory), without importing torch for bytes."""
    return hasattr(b, "data_ptr") and hasattr(b, "is_cuda")


class DecodedStream:
    """One stream of a decode_many batch: rc (what flacgpu_decode_stream returns for it), info (StreamInfo), offset
    (first element in the flat output) and pcm (a [samples, channels] view of the flat output, or the
    [channels, samples] view batch[i, :channels, :decoded_samples] of a padded batch; None when rc != 0)."""
    __slots__ = ("rc", "info", "offset", "pcm")

    def __init__(self, rc, info, offset, pcm):
        self.rc, self.info, self.offset, self.pcm = rc, info, offset, pcm


class Decoder:
    """flacgpu_decoder: a batch decoder handle that keeps its device buffers and pinned staging between calls.
    Not thread-safe."""

    def __init__(self, device=-1):
        self._h = None
        L = _lib.lib()
        h = C.c_void_p()
        rc = L.flacgpu_decoder_create(device, C.byref(h))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_create")
        self._h = h
        self.device = device
        self.device_index = device if device >= 0 else L.flacgpu_current_device()   # -1: the creator's current device
        self.n_raw_streams = self.n_raw_frames = 0   # of the last scan_frames

    def close(self):
        if self._h:
            _lib.lib().flacgpu_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _sources(self, blobs, stream):
        """The pointer and length arrays of a scan's inputs: (ptrs, lens, n, keep, stream).  `stream` is None for host
        bytes, else the hipStream_t (an integer, 0: the legacy default stream) the device scan is ordered after."""
        blobs = list(blobs)
        on_device = [is_device_blob(b) for b in blobs]
        if any(on_device) and not all(on_device):
            raise ValueError("a batch is all device tensors or all host bytes, not a mix")
        n = len(blobs)
        ptrs = (C.c_void_p * max(n, 1))()
        lens = (C.c_size_t * max(n, 1))()
        if n and on_device[0]:
            import torch

            dev = self.device_index
            for i, b in enumerate(blobs):
                if not b.is_cuda or b.device.index != dev:
                    raise ValueError(f"blob {i} lies on {b.device}, the decoder on cuda:{dev}")
                if b.dtype != torch.uint8 or b.dim() != 1 or not b.is_contiguous():
                    raise ValueError(f"blob {i} must be a contiguous 1-D torch.uint8 tensor")
                ptrs[i] = b.data_ptr() if b.numel() else None
                lens[i] = b.numel()
            if stream is None:
                stream = torch.cuda.current_stream(dev)
            return ptrs, lens, n, blobs, int(getattr(stream, "cuda_stream", stream) or 0)
        if stream is not None:
            raise ValueError("stream goes with device tensors")
        keep = []   # the bytes objects' own buffers, no copy; alive until the scan has uploaded them
        for i, b in enumerate(blobs):
            b = b if isinstance(b, bytes) else bytes(b)
            cp = C.c_char_p(b)
            keep.append(cp)
            ptrs[i] = C.cast(cp, C.c_void_p).value
            lens[i] = len(b)
        return ptrs, lens, n, keep, None

    def scan(self, blobs, stream=None):
        """flacgpu_decoder_scan: returns (records, total int32 samples).  `blobs` are bytes, or -- all of them -- 1-D
        contiguous torch.uint8 tensors on the decoder's device (views into one shard tensor, say), which are scanned
        where they lie (flacgpu_decoder_scan_device), ordered after `stream` (default: torch's current stream on that
        device).  The tensors may be freed or overwritten once the call returns."""
        L = _lib.lib()
        ptrs, lens, n, keep, st = self._sources(blobs, stream)
        recs = (_lib.DecodedStream * max(n, 1))()
        total = C.c_uint64(0)
        if st is None:
            rc, who = L.flacgpu_decoder_scan(self._h, ptrs, lens, n, recs, C.byref(total)), "flacgpu_decoder_scan"
        else:
            rc = L.flacgpu_decoder_scan_device(self._h, ptrs, lens, n, C.c_void_p(st), recs, C.byref(total))
            who = "flacgpu_decoder_scan_device"
        del keep
        if rc:
            raise GpuError(rc, who)
        return recs, total.value

    def scan_frames(self, blobs, speculative=False, stream=None):
        """flacgpu_decoder_scan_frames_ex: a batch of raw frame streams (bare frames, no metadata; a byte range of a
        file).  Returns (records, total int32 samples of the uniform streams, raw, frames): `records` serve decode,
        decode_as and decode_windows as scan's do, `raw` is the _lib.RawStream array, `frames` the structured array
        (FRAME_DTYPE) of every kept frame of the batch, whose last out_offset + block_size * channels is the element
        count decode_frames writes.  speculative=True (FLACGPU_SCAN_SPECULATIVE): a frame that no header ends is ended
        by its own bits, and its record has _lib.FRAME_SPECULATIVE in `reserved`.  Device tensors and `stream` as for
        scan (flacgpu_decoder_scan_frames_device)."""
        L = _lib.lib()
        ptrs, lens, n, keep, st = self._sources(blobs, stream)
        recs = (_lib.DecodedStream * max(n, 1))()
        raw = (_lib.RawStream * max(n, 1))()
        n_frames, elements, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        flags = _lib.SCAN_SPECULATIVE if speculative else 0
        if st is None:
            rc = L.flacgpu_decoder_scan_frames_ex(self._h, ptrs, lens, n, flags, recs, raw, C.byref(n_frames),
                                                  C.byref(elements), C.byref(total))
            who = "flacgpu_decoder_scan_frames_ex"
        else:
            rc = L.flacgpu_decoder_scan_frames_device(self._h, ptrs, lens, n, flags, C.c_void_p(st), recs, raw,
                                                      C.byref(n_frames), C.byref(elements), C.byref(total))
            who = "flacgpu_decoder_scan_frames_device"
        del keep
        if rc:
            raise GpuError(rc, who)
        frames = np.zeros(n_frames.value, dtype=FRAME_DTYPE)
        rc = L.flacgpu_decoder_frame_records(self._h, frames.ctypes.data_as(C.POINTER(_lib.FrameRecord)), frames.size)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_frame_records")
        self.raw_elements = elements.value
        self.n_raw_streams, self.n_raw_frames = n, int(n_frames.value)
        return recs, total.value, raw, frames

    def slot_bytes(self):
        """flacgpu_decoder_slot_bytes: the decoder's slot buffer as the last scan left it (every frame region at a
        64-byte boundary, zero tails, 64 bytes of look-ahead), as bytes.  For tests: host and device scans of the same
        bytes build the same buffer."""
        L = _lib.lib()
        need = C.c_uint64(0)
        rc = L.flacgpu_decoder_slot_bytes(self._h, None, 0, C.byref(need))
        if rc and rc != -5:
            raise GpuError(rc, "flacgpu_decoder_slot_bytes")
        buf = np.empty(need.value, dtype=np.uint8)
        rc = L.flacgpu_decoder_slot_bytes(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(need))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_slot_bytes")
        return buf.tobytes()

    def decode_frames(self, out_ptr, out_cap, flags, frames):
        """flacgpu_decoder_decode_frames: every kept frame of the raw scan into the int32 buffer at out_ptr (device or
        host address); `frames` (the structured array scan_frames returned, or one of its size) gets the records with
        status filled."""
        rc = _lib.lib().flacgpu_decoder_decode_frames(self._h, out_ptr, out_cap, flags,
                                                      frames.ctypes.data_as(C.POINTER(_lib.FrameRecord)), frames.size)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_decode_frames")
        return frames

    def plan_analysis(self):
        """flacgpu_decoder_plan_analysis for the handle's scanned batch: (frames, subframe records, int32 row elements)."""
        nf, ns, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().flacgpu_decoder_plan_analysis(self._h, C.byref(nf), C.byref(ns), C.byref(nr))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_plan_analysis")
        return nf.value, ns.value, nr.value

    def analyze(self, rows=False, out="host"):
        """flacgpu_decoder_analyze of the handle's scanned batch (any scan, or a session's feed): a FrameAnalysis.
        rows=False is the records-only pass (no sample is stored, .rows is None).  out="device" has the kernel write
        into torch tensors on the decoder's device: the rows stay there as an int32 CUDA tensor, the records come back
        as numpy arrays either way."""
        if out not in ("device", "host"):
            raise ValueError("out must be 'device' or 'host'")
        nf, ns, nr = self.plan_analysis()
        L = _lib.lib()
        if out == "device":
            import torch

            dev = f"cuda:{self.device_index}"
            t_frames = torch.empty(nf * ANALYSIS_FRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            t_subs = torch.empty(ns * SUBFRAME_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            t_rows = torch.empty(nr, dtype=torch.int32, device=dev) if rows else None
            torch.cuda.synchronize(self.device_index)
            rc = L.flacgpu_decoder_analyze(self._h, _lib.DECODE_OUT_DEVICE, t_frames.data_ptr() if nf else None, nf,
                                           t_subs.data_ptr() if ns else None, ns,
                                           t_rows.data_ptr() if rows and nr else None, nr if rows else 0)
            if rc:
                raise GpuError(rc, "flacgpu_decoder_analyze")
            frames = t_frames.cpu().numpy().view(ANALYSIS_FRAME_DTYPE)
            subs = t_subs.cpu().numpy().view(SUBFRAME_DTYPE)
            return FrameAnalysis(frames, subs, t_rows)
        frames = np.zeros(nf, dtype=ANALYSIS_FRAME_DTYPE)
        subs = np.zeros(ns, dtype=SUBFRAME_DTYPE)
        # one element more than none, so that rows=True never passes the NULL that selects the records-only pass
        r = np.zeros(max(nr, 1), dtype=np.int32) if rows else None
        rc = L.flacgpu_decoder_analyze(self._h, 0, frames.ctypes.data if nf else None, nf,
                                       subs.ctypes.data if ns else None, ns, r.ctypes.data if rows else None,
                                       r.size if rows else 0)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_analyze")
        return FrameAnalysis(frames, subs, r[:nr] if rows else None)

    def plan_timeline(self, fmt, check=True):
        """flacgpu_decoder_plan_timeline for the handle's last raw scan: (results, out_bytes, mask_bytes), `results` the
        _lib.TimelineResult array of the scan's streams.  check=False returns (results, None, None) for a format the
        call refuses instead of raising: the results are filled either way, and pad_to is sized from them."""
        results = (_lib.TimelineResult * max(self.n_raw_streams, 1))()
        need, mask = C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().flacgpu_decoder_plan_timeline(self._h, C.byref(fmt), results, C.byref(need), C.byref(mask))
        if rc and check:
            raise GpuError(rc, "flacgpu_decoder_plan_timeline")
        return (results, None, None) if rc else (results, need.value, mask.value)

    def decode_timeline(self, out_ptr, out_cap_bytes, mask_ptr, mask_cap_bytes, fmt, flags, frames=None):
        """flacgpu_decoder_decode_timeline of the last raw scan into the buffers at out_ptr and mask_ptr (both device or
        both host addresses; mask_ptr may be None).  Returns (results, frames): the _lib.TimelineResult array and a
        TIMELINE_FRAME_DTYPE array with one entry per record of the scan."""
        results = (_lib.TimelineResult * max(self.n_raw_streams, 1))()
        if frames is None:
            frames = np.zeros(self.n_raw_frames, dtype=TIMELINE_FRAME_DTYPE)
        rc = _lib.lib().flacgpu_decoder_decode_timeline(self._h, out_ptr, out_cap_bytes, mask_ptr, mask_cap_bytes,
                                                        C.byref(fmt), flags, results,
                                                        frames.ctypes.data_as(C.POINTER(_lib.TimelineFrame)), frames.size)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_decode_timeline")
        return results, frames

    def decode(self, out_ptr, out_cap, flags, recs):
        """flacgpu_decoder_decode into the int32 buffer at out_ptr (device or host address)."""
        rc = _lib.lib().flacgpu_decoder_decode(self._h, out_ptr, out_cap, flags, recs)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_decode")
        return recs

    @staticmethod
    def plan_output(fmt, recs, n):
        """flacgpu_decoder_plan_output: the bytes the output of `fmt` takes for the first n scanned records."""
        need = C.c_uint64(0)
        rc = _lib.lib().flacgpu_decoder_plan_output(C.byref(fmt), recs, n, C.byref(need))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_plan_output")
        return need.value

    def decode_as(self, out_ptr, out_cap_bytes, fmt, flags, recs):
        """flacgpu_decoder_decode_as into the buffer at out_ptr (device or host address) in the format `fmt`
        (_lib.OutFormat)."""
        rc = _lib.lib().flacgpu_decoder_decode_as(self._h, out_ptr, out_cap_bytes, C.byref(fmt), flags, recs)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_decode_as")
        return recs

    @staticmethod
    def plan_windows(fmt, recs, n, windows):
        """flacgpu_decoder_plan_windows: the bytes the windows (a _lib.Window array) take in `fmt` for the first n
        scanned records."""
        need = C.c_uint64(0)
        rc = _lib.lib().flacgpu_decoder_plan_windows(C.byref(fmt), recs, n, windows, len(windows), C.byref(need))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_plan_windows")
        return need.value

    def decode_windows(self, out_ptr, out_cap_bytes, fmt, flags, windows):
        """flacgpu_decoder_decode_windows of the scanned batch into the buffer at out_ptr (device or host address):
        `windows` is a _lib.Window array, `fmt` a PADDED _lib.OutFormat.  Returns the _lib.WindowResult array."""
        n = len(windows)
        results = (_lib.WindowResult * max(n, 1))()
        rc = _lib.lib().flacgpu_decoder_decode_windows(self._h, out_ptr, out_cap_bytes, C.byref(fmt), flags, windows, n,
                                                       results)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_decode_windows")
        return results


class _SessionDecoder(Decoder):
    """The decoder a DecoderSession owns: every decode call of Decoder works on it; the session destroys it."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device
        self.device_index = device if device >= 0 else _lib.lib().flacgpu_current_device()
        self.n_raw_streams = self.n_raw_frames = self.raw_elements = 0

    def close(self):
        self._h = None


class DecoderSession:
    """flacgpu_decoder_session: `n_streams` raw frame streams fed chunk by chunk, the chunks cut anywhere (DESIGN.md 4b
    "Decoder sessions").  No frame is longer than `max_frame_bytes` (16 .. 2^22).  The bytes that cannot be judged yet
    stay in device memory between feeds.  `decoder` is the session's own Decoder: after a feed every decode call works on
    it, over that feed's frames.  Not thread-safe.

    container=True opens a CONTAINER session (DESIGN.md 4b "Container sessions"): the streams are regular .flac files --
    marker, metadata chain, frames -- whose metadata is walked across feeds and whose frames are decided by the regular
    rule with STREAMINFO's values.  After a feed the decoder stands as Decoder.scan leaves it (decode, decode_as and
    decode_windows work; feed and finish return no frame records); the first decode of a feed with MD5 hashes its samples
    into the session's chains, and verdict() gives every stream's record as the one-shot decode gives it.  flush is not
    taken."""

    def __init__(self, n_streams, max_frame_bytes, device=-1, container=False):
        self._h = None
        L = _lib.lib()
        h = C.c_void_p()
        self.container = bool(container)
        if container:
            rc = L.flacgpu_decoder_session_open_container(device, n_streams, max_frame_bytes, C.byref(h))
        else:
            rc = L.flacgpu_decoder_session_open(device, n_streams, max_frame_bytes, 0, C.byref(h))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_session_open_container" if container else "flacgpu_decoder_session_open")
        self._h = h
        self.n_streams = n_streams
        self.decoder = _SessionDecoder(C.c_void_p(L.flacgpu_decoder_session_decoder(h)), device)
        self.records = (_lib.DecodedStream * max(n_streams, 1))()   # of the last feed: for decode / decode_as
        self.frames = np.zeros(0, dtype=FRAME_DTYPE)

    def close(self):
        if self._h:
            self.decoder.close()
            _lib.lib().flacgpu_decoder_session_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _done(self, rc, who, n_frames, elements, total):
        if rc:
            raise GpuError(rc, who)
        dec = self.decoder
        self.n_frames, self.total = int(n_frames.value), int(total.value)   # of this feed: frames; decode's int32 samples
        if self.container:   # a batch of regular streams: no frame records
            return self.frames, list(self._raw)[:self.n_streams]
        frames = np.zeros(n_frames.value, dtype=FRAME_DTYPE)
        rc = _lib.lib().flacgpu_decoder_frame_records(dec._h, frames.ctypes.data_as(C.POINTER(_lib.FrameRecord)), frames.size)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_frame_records")
        dec.raw_elements = elements.value
        dec.n_raw_streams, dec.n_raw_frames = self.n_streams, int(n_frames.value)
        self.frames = frames
        return frames, list(self._raw)[:self.n_streams]

    def feed(self, chunks, flush=False, stream=None):
        """One chunk per stream -- bytes-like, or all of them 1-D torch.uint8 tensors on the session's device (ordered
        after `stream` as Decoder.scan's are); None or an empty chunk: no bytes for that stream.  flush: True, False or
        one bool per stream ("what I have fed this stream ends on a frame boundary: decide everything now").  Returns
        (frames, raw): the records (FRAME_DTYPE) of the frames decided by this feed, byte_offset counting from each
        stream's first byte, and the streams' _lib.RawStream summaries (frames, skipped_bytes and gaps cumulative)."""
        chunks = list(chunks)
        if len(chunks) != self.n_streams:
            raise ValueError(f"{len(chunks)} chunks for a session of {self.n_streams} streams")
        if any(is_device_blob(b) for b in chunks if b is not None):
            import torch

            empty = torch.empty(0, dtype=torch.uint8, device=f"cuda:{self.decoder.device_index}")
            chunks = [empty if b is None else b for b in chunks]
        else:
            chunks = [b"" if b is None else b for b in chunks]
        ptrs, lens, n, keep, st = self.decoder._sources(chunks, stream)
        flags = [bool(flush)] * n if isinstance(flush, (bool, int)) else [bool(f) for f in flush]
        if len(flags) != n:
            raise ValueError("flush is one bool, or one per stream")
        fl = (C.c_uint8 * max(n, 1))(*[int(f) for f in flags])
        self._raw = (_lib.RawStream * max(n, 1))()
        n_frames, elements, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L = _lib.lib()
        if st is None:
            rc = L.flacgpu_decoder_session_feed(self._h, ptrs, lens, fl, self.records, self._raw, C.byref(n_frames),
                                                C.byref(elements), C.byref(total))
            who = "flacgpu_decoder_session_feed"
        else:
            rc = L.flacgpu_decoder_session_feed_device(self._h, ptrs, lens, fl, C.c_void_p(st), self.records, self._raw,
                                                       C.byref(n_frames), C.byref(elements), C.byref(total))
            who = "flacgpu_decoder_session_feed_device"
        del keep
        return self._done(rc, who, n_frames, elements, total)

    def finish(self):
        """Flushes every stream: (frames, raw) as feed; raw is then every whole stream's summary.  No feed may follow."""
        self._raw = (_lib.RawStream * max(self.n_streams, 1))()
        n_frames, elements, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = _lib.lib().flacgpu_decoder_session_finish(self._h, self.records, self._raw, C.byref(n_frames),
                                                       C.byref(elements), C.byref(total))
        return self._done(rc, "flacgpu_decoder_session_finish", n_frames, elements, total)

    def decode(self, out="device", verify_md5=True):
        """flacgpu_decoder_decode of the last feed's batch: (flat int32, streams) as decode_many gives them -- the
        streams with a frame decided in this feed, back to back.  In a container session the first call after a feed with
        verify_md5=True is the one that hashes the feed's samples into the session's MD5 chains."""
        if out not in ("device", "host"):
            raise ValueError("out must be 'device' or 'host'")
        dec, total = self.decoder, self.total
        flags = 0 if verify_md5 else _lib.DECODE_NO_MD5
        recs = (_lib.DecodedStream * max(self.n_streams, 1))()
        if out == "device":
            import torch

            flat = torch.empty(total, dtype=torch.int32, device=f"cuda:{dec.device_index}")
            torch.cuda.synchronize(dec.device_index)
            dec.decode(flat.data_ptr() if total else None, total, flags | _lib.DECODE_OUT_DEVICE, recs)
        else:
            flat = np.empty(total, dtype=np.int32)
            dec.decode(flat.ctypes.data if total else None, total, flags, recs)
        streams = []
        for i in range(self.n_streams):
            r = recs[i]
            info = _lib.StreamInfo()
            C.memmove(C.byref(info), C.byref(r.info), C.sizeof(info))
            pcm = None
            if r.rc == 0:
                ch = max(info.channels, 1)
                pcm = flat[r.out_offset:r.out_offset + info.decoded_samples * ch].reshape(-1, ch)
            streams.append(DecodedStream(r.rc, info, r.out_offset, pcm))
        return flat, streams

    def verdict(self):
        """flacgpu_decoder_session_verdict, once, after finish and the decode that follows it: the list of every
        stream's _lib.DecodedStream as the one-shot scan + decode of the whole file gives it (rc, STREAMINFO, frames,
        decoded_samples, bad_frames, bad_crc16, decoded_md5, md5_status; 3: a feed's frames were never hashed)."""
        out = (_lib.DecodedStream * max(self.n_streams, 1))()
        rc = _lib.lib().flacgpu_decoder_session_verdict(self._h, out)
        if rc:
            raise GpuError(rc, "flacgpu_decoder_session_verdict")
        return list(out)[:self.n_streams]

    def pending(self):
        """(held bytes per stream, bytes fed to the session so far)."""
        held, fed = (C.c_uint64 * max(self.n_streams, 1))(), C.c_uint64(0)
        rc = _lib.lib().flacgpu_decoder_session_pending(self._h, held, C.byref(fed))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_session_pending")
        return [int(v) for v in held[:self.n_streams]], int(fed.value)

    def decode_frames(self, out="device"):
        """The samples of the last feed's frames: (flat int32, frames) as gpu.decode_frames gives them -- frame f is
        flat[out_offset : out_offset + block_size * channels] as [block_size, channels], status filled."""
        if out not in ("device", "host"):
            raise ValueError("out must be 'device' or 'host'")
        frames = self.frames.copy()
        return _decode_scanned_frames(self.decoder, frames, out), frames

    def last_feed_timing(self):
        """flacgpu_decoder_session_last_feed_timing: where the host's time went in the last feed or finish, a dict of
        milliseconds (stage, to_first_sync, to_second_sync, scan_rest, walk, table_upload)."""
        t = _lib.SessionTiming()
        rc = _lib.lib().flacgpu_decoder_session_last_feed_timing(self._h, C.byref(t))
        if rc:
            raise GpuError(rc, "flacgpu_decoder_session_last_feed_timing")
        return {name[:-3]: float(getattr(t, name)) for name, _ in t._fields_}

    def decode_as(self, dtype="float32", layout="padded", pad_to=None, pad_channels=None, out="device", verify_md5=False):
        """The last feed's frames per stream, as decode_many(raw=True) gives a batch: (flat or [B, C, T] batch, streams).
        A stream without a frame in this feed, or whose frames of this feed differ, is absent (rc != 0)."""
        if dtype not in _DTYPES or layout not in ("flat", "padded") or out not in ("device", "host"):
            raise ValueError("dtype, layout and out as for decode_many")
        return _decode_many_as(self.decoder, self.records, self.n_streams, out, 0 if verify_md5 else _lib.DECODE_NO_MD5,
                               dtype, layout, pad_to, pad_channels)


def window_frames(frame_sizes, start, length):
    """flacgpu_window_frames: (first, count, skip) of the frames of a stream with these block sizes that samples
    [start, start + length) touch.  Needs no GPU."""
    sizes = np.ascontiguousarray(frame_sizes, dtype=np.uint32)
    first, count, skip = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = _lib.lib().flacgpu_window_frames(sizes.ctypes.data_as(C.POINTER(C.c_uint32)), sizes.size, start, length,
                                          C.byref(first), C.byref(count), C.byref(skip))
    if rc:
        raise GpuError(rc, "flacgpu_window_frames")
    return first.value, count.value, skip.value


def ragged_plan(samples, block_size, max_partition_order):
    """flacgpu_ragged_plan: the checks of a ragged batch (GpuAnalyzer.encode_ragged_device) and the layout of its window
    pool, for frames of these lengths under these options.  Returns (window_of[n_frames], distinct lengths in
    first-appearance order, pool_doubles); raises GpuError for a batch the encoder would refuse.  Needs no GPU."""
    lens = np.ascontiguousarray(samples, dtype=np.uint32)
    n = int(lens.size)
    o = GpuOptions(block_size, max_partition_order, 0, 0, 0, 0, 0, 0.0)
    u32p = C.POINTER(C.c_uint32)
    window_of, distinct = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    nd, pool = C.c_uint32(0), C.c_uint64(0)
    rc = _lib.lib().flacgpu_ragged_plan(C.byref(o), lens.ctypes.data_as(u32p) if n else None, n, window_of.ctypes.data_as(u32p),
                                        distinct.ctypes.data_as(u32p), C.byref(nd), C.byref(pool))
    if rc:
        raise GpuError(rc, "flacgpu_ragged_plan")
    return [int(v) for v in window_of[:n]], [int(v) for v in distinct[:nd.value]], int(pool.value)


def window_array(windows):
    """A _lib.Window array from (stream, start, length) tuples or an [N, 3] integer array."""
    rows = [tuple(int(v) for v in w) for w in windows]
    if any(len(r) != 3 for r in rows):
        raise ValueError("a window is (stream, start, length)")
    return (_lib.Window * len(rows))(*[_lib.Window(s, 0, a, n) for s, a, n in rows])


_DTYPES = {"int32": _lib.SAMPLE_I32, "int16": _lib.SAMPLE_I16, "float32": _lib.SAMPLE_F32, "int24": _lib.SAMPLE_S24}


def _element_array(dtype, shape):
    """(array dtype name, shape) of an output of `shape` elements: "int24" has no array dtype, its elements are a
    trailing axis of 3 uint8 (little-endian)."""
    return ("uint8", tuple(shape) + (3,)) if dtype == "int24" else (dtype, tuple(shape))


def _decode_many_as(dec, recs, n, out, flags, dtype, layout, pad_to, pad_channels):
    """decode_many's other formats: (flat or [B, C, T] batch, streams)."""
    fmt = _lib.OutFormat(_DTYPES[dtype], _lib.LAYOUT_FLAT, 0, 0, 0)
    ok = [recs[i] for i in range(n) if recs[i].rc == 0]
    if layout == "padded":
        fmt.layout = _lib.LAYOUT_PADDED
        fmt.samples_padded = pad_to or max([r.info.decoded_samples for r in ok], default=0)
        fmt.channels_padded = pad_channels or max([r.info.channels for r in ok], default=0)
        shape = (n, fmt.channels_padded, fmt.samples_padded)
    else:
        shape = (sum(r.info.decoded_samples * r.info.channels for r in ok),)
    need = Decoder.plan_output(fmt, recs, n)   # refuses before anything is allocated
    array_dtype, shape = _element_array(dtype, shape)
    if out == "device":
        import torch

        dev = dec.device if dec.device >= 0 else torch.cuda.current_device()
        buf = torch.empty(shape, dtype=getattr(torch, array_dtype), device=f"cuda:{dev}")
        torch.cuda.synchronize(dev)
        dec.decode_as(buf.data_ptr() if need else None, need, fmt, flags | _lib.DECODE_OUT_DEVICE, recs)
    else:
        buf = np.empty(shape, dtype=array_dtype)
        dec.decode_as(buf.ctypes.data if need else None, need, fmt, flags, recs)
    streams = []
    for i in range(n):
        r = recs[i]
        info = _lib.StreamInfo()
        C.memmove(C.byref(info), C.byref(r.info), C.sizeof(info))
        pcm = None
        if r.rc == 0 and layout == "padded":
            pcm = buf[i, :info.channels, :info.decoded_samples]
        elif r.rc == 0:
            ch = max(info.channels, 1)
            pcm = buf[r.out_offset:r.out_offset + info.decoded_samples * ch].reshape((-1, ch) + tuple(shape[1:]))
        streams.append(DecodedStream(r.rc, info, r.out_offset, pcm))
    return buf, streams


def _decode_scanned_frames(dec, frames, out):
    """flacgpu_decoder_decode_frames of the raw batch `dec` holds (a scan_frames, or a session's feed) into a new flat
    int32 buffer -- a torch tensor on the decoder's device for out="device", a numpy array for "host"; `frames` (the
    batch's records) gets the status filled."""
    total = dec.raw_elements
    if out == "device":
        import torch

        dev = dec.device if dec.device >= 0 else torch.cuda.current_device()
        flat = torch.empty(total, dtype=torch.int32, device=f"cuda:{dev}")
        torch.cuda.synchronize(dev)
        dec.decode_frames(flat.data_ptr() if total else None, total, _lib.DECODE_OUT_DEVICE, frames)
    else:
        flat = np.empty(total, dtype=np.int32)
        dec.decode_frames(flat.ctypes.data if total else None, total, 0, frames)
    return flat


def decode_frames(blobs, device=-1, out="device", decoder=None, speculative=False):
    """Decode every whole frame of a batch of raw frame streams (bare FLAC frames without metadata, as FlacStreamWriter
    writes them, or a byte range cut out of a file) in one GPU call: flacgpu_decoder_scan_frames +
    flacgpu_decoder_decode_frames.  The frames' sample rate, channels and sample size may differ from one to the next.

    Returns (samples, frames, raw): `samples` is flat int32 -- a torch tensor on the GPU for out="device", a numpy array
    for out="host" --, frame f being samples[out_offset : out_offset + block_size * channels] as [block_size, channels];
    `frames` is a numpy structured array of the records (FRAME_DTYPE; status != 0: the frame did not decode and its
    samples are undefined), ordered by input, then position; raw[i] is the _lib.RawStream summary of input i.
    speculative=True scans with FLACGPU_SCAN_SPECULATIVE (Decoder.scan_frames)."""
    if out not in ("device", "host"):
        raise ValueError("out must be 'device' or 'host'")
    if out == "device":
        import torch

        torch.cuda.init()   # torch's HIP runtime first, as in decode_many
    own = decoder is None
    dec = Decoder(device) if own else decoder
    try:
        _, _, raw, frames = dec.scan_frames(blobs, speculative)
        flat = _decode_scanned_frames(dec, frames, out)
    finally:
        if own:
            dec.close()
    return flat, frames, list(raw)[:len(blobs)]


def analyze_many(blobs, raw=False, speculative=False, rows=False, out="host", decoder=None, device=-1):
    """What every frame of a batch of FLAC streams is made of, in one GPU call (flacgpu_decoder_scan or, raw=True,
    flacgpu_decoder_scan_frames_ex, then flacgpu_decoder_analyze): subframe types, orders, wasted bits, predictors, Rice
    methods, partition orders and parameters, exact bit lengths and -- rows=True -- the residual rows as they are coded.
    The counterpart of the reference's FrameIterator for a whole batch; nothing is decoded.

    Returns a FrameAnalysis: .frames / .subframes are numpy structured arrays mirroring flacgpu_frame_analysis and
    flacgpu_subframe_plan, .rows flat int32 (numpy, or a CUDA tensor for out="device"; None with rows=False),
    .subframes_of(f) and .row(f, c) pick a frame's records and rows.  Frames come in the scan's order: by input, then
    position.  speculative=True (with raw=True alone) scans with FLACGPU_SCAN_SPECULATIVE."""
    if speculative and not raw:
        raise ValueError("speculative goes with raw=True")
    if out == "device":
        import torch

        torch.cuda.init()   # torch's HIP runtime first, as in decode_many
    own = decoder is None
    dec = Decoder(device) if own else decoder
    try:
        if raw:
            dec.scan_frames(blobs, speculative)
        else:
            dec.scan(blobs)
        return dec.analyze(rows=rows, out=out)
    finally:
        if own:
            dec.close()


def decode_many(blobs, device=-1, out="device", verify_md5=True, decoder=None, dtype="int32", layout="flat",
                pad_to=None, pad_channels=None, raw=False, speculative=False):
    """Decode many FLAC streams in one GPU call (flacgpu_decoder_scan + flacgpu_decoder_decode).

    Returns (flat, streams): `flat` holds every stream's interleaved int32 samples one after another -- a torch tensor
    on the GPU for out="device", a numpy array for out="host" -- and `streams` is a list of DecodedStream.  Every record
    equals what flacgpu_decode_stream gives for that stream alone (a stream without frames is hashed as the empty
    input: md5_status 1 / 2 instead of 0).  verify_md5=False skips the MD5 (md5_status 3).

    dtype "int16" (sample << (16 - bps); every stream must have bps <= 16), "int24" (sample << (24 - bps) as 3
    little-endian bytes, bps <= 24: uint8 with a trailing axis of 3 -- flat [total_elements, 3] with pcm views
    [samples, channels, 3], padded [B, C, T, 3] -- which is a WAV data chunk as it stands) or "float32"
    (sample * 2^-(bps - 1)) converts in the same kernel pass (flacgpu_decoder_decode_as).  layout="padded" returns
    (batch, streams): `batch` is [B, C, T], planar and zero-padded, with T = pad_to or the longest stream and C = pad_channels or the most channels;
    streams[i].pcm is the view batch[i, :channels, :decoded_samples], and the lengths vector a padded batch goes with
    is [s.info.decoded_samples for s in streams].  A stream with rc != 0 is a row of zeros.

    raw=True takes the inputs as raw frame streams (no fLaC marker, no STREAMINFO; flacgpu_decoder_scan_frames): a stream
    whose whole frames share one sample rate, channel count and sample size decodes as a regular one (md5_status 2:
    there is no MD5 to compare with), one whose frames differ has rc -2 (decode_frames serves it), one without a whole
    frame rc -1.  With decoder= the scan stays on the handle for a following decode_windows.  speculative=True (with
    raw=True alone) scans with FLACGPU_SCAN_SPECULATIVE: a frame whose successor's header is damaged or cut off is kept."""
    if out not in ("device", "host"):
        raise ValueError("out must be 'device' or 'host'")
    if dtype not in _DTYPES or layout not in ("flat", "padded"):
        raise ValueError("dtype must be 'int32', 'int16', 'int24' or 'float32' and layout 'flat' or 'padded'")
    if layout == "flat" and (pad_to is not None or pad_channels is not None):
        raise ValueError("pad_to and pad_channels go with layout='padded'")
    if speculative and not raw:
        raise ValueError("speculative goes with raw=True")
    if out == "device":
        import torch

        torch.cuda.init()   # torch's HIP runtime first: initialised after the library's first HIP call it sees no GPU
    own = decoder is None
    dec = Decoder(device) if own else decoder
    try:
        recs, total = dec.scan_frames(blobs, speculative)[:2] if raw else dec.scan(blobs)
        flags = 0 if verify_md5 else _lib.DECODE_NO_MD5
        if (dtype, layout) != ("int32", "flat"):
            return _decode_many_as(dec, recs, len(blobs), out, flags, dtype, layout, pad_to, pad_channels)
        if out == "device":
            import torch

            dev = dec.device if dec.device >= 0 else torch.cuda.current_device()
            flat = torch.empty(total, dtype=torch.int32, device=f"cuda:{dev}")
            torch.cuda.synchronize(dev)
            dec.decode(flat.data_ptr() if total else None, total, flags | _lib.DECODE_OUT_DEVICE, recs)
        else:
            flat = np.empty(total, dtype=np.int32)
            dec.decode(flat.ctypes.data if total else None, total, flags, recs)
    finally:
        if own:
            dec.close()
    streams = []
    for i in range(len(blobs)):
        r = recs[i]
        info = _lib.StreamInfo()
        C.memmove(C.byref(info), C.byref(r.info), C.sizeof(info))
        pcm = None
        if r.rc == 0:
            ch = max(info.channels, 1)
            pcm = flat[r.out_offset:r.out_offset + info.decoded_samples * ch].reshape(-1, ch)
        streams.append(DecodedStream(r.rc, info, r.out_offset, pcm))
    return flat, streams


def decode_timeline(blobs, dtype="float32", pad_to=None, pad_channels=None, out="device", speculative=False, mask=True,
                    decoder=None, device=-1):
    """Decode a batch of raw frame streams (a lossy transport's frames, a byte range of a file) onto their timelines:
    every whole frame is put where its coded frame or sample number says it belongs, and what is lost -- a gap between
    two frames, a frame that does not decode -- is zero (flacgpu_decoder_scan_frames_ex + flacgpu_decoder_decode_timeline).

    Returns (batch, mask, results, frames): `batch` is [B, C, T], planar and zero-padded, in `dtype` as for decode_many
    ("int24": uint8 [B, C, T, 3]) -- a torch tensor on the GPU for out="device", a numpy array for out="host" -- with
    T = pad_to or the longest timeline and C = pad_channels or the most channels; `mask` is uint8 [B, T], 1 where a
    decoded sample stands (None with mask=False); results[i] is the _lib.TimelineResult of stream i (rc != 0: the stream
    has no timeline and is a row of zeros; first_sample: the position of batch[i, :, 0] in the stream); `frames` is a
    TIMELINE_FRAME_DTYPE array beside the scan's records (Decoder.scan_frames(...)[3])."""
    if out not in ("device", "host"):
        raise ValueError("out must be 'device' or 'host'")
    if dtype not in _DTYPES:
        raise ValueError("dtype must be 'int32', 'int16', 'int24' or 'float32'")
    if out == "device":
        import torch

        torch.cuda.init()   # torch's HIP runtime first, as in decode_many
    own = decoder is None
    dec = Decoder(device) if own else decoder
    try:
        _, _, raw, records = dec.scan_frames(blobs, speculative)
        n = len(blobs)
        fmt = _lib.OutFormat(_DTYPES[dtype], _lib.LAYOUT_PADDED, pad_channels or 0, 0, pad_to or 0)
        if pad_to is None or pad_channels is None:   # the batch's own maxima, from the plan
            plan = dec.plan_timeline(fmt, check=False)[0]
            ok = [i for i in range(n) if plan[i].rc == 0]
            if pad_to is None:
                fmt.samples_padded = max([plan[i].timeline_samples for i in ok], default=0)
            if pad_channels is None:
                fmt.channels_padded = max([int(records["channels"][raw[i].first_frame]) for i in ok], default=0)
        _, need, mask_need = dec.plan_timeline(fmt)   # refuses before anything is allocated
        array_dtype, shape = _element_array(dtype, (n, fmt.channels_padded, fmt.samples_padded))
        mshape = (n, fmt.samples_padded)
        if out == "device":
            dev = dec.device if dec.device >= 0 else torch.cuda.current_device()
            buf = torch.empty(shape, dtype=getattr(torch, array_dtype), device=f"cuda:{dev}")
            m = torch.empty(mshape, dtype=torch.uint8, device=f"cuda:{dev}") if mask else None
            torch.cuda.synchronize(dev)
            results, frames = dec.decode_timeline(buf.data_ptr() if need else None, need,
                                                  m.data_ptr() if mask and mask_need else None, mask_need if mask else 0,
                                                  fmt, _lib.DECODE_OUT_DEVICE)
        else:
            buf = np.empty(shape, dtype=array_dtype)
            m = np.empty(mshape, dtype=np.uint8) if mask else None
            results, frames = dec.decode_timeline(buf.ctypes.data if need else None, need,
                                                  m.ctypes.data if mask and mask_need else None, mask_need if mask else 0,
                                                  fmt, 0)
    finally:
        if own:
            dec.close()
    return buf, m, list(results)[:n], frames


def decode_windows(decoder, recs, windows, dtype="float32", out="device", pad_to=None, pad_channels=None):
    """Sample windows (random crops) of the batch that `decoder` has scanned (`recs`: what Decoder.scan returned):
    only the frames a window touches are decoded, and only the windows are written (flacgpu_decoder_decode_windows).

    `windows` is a sequence of (stream, start, length) tuples or an [N, 3] integer array.  Returns (batch, results):
    `batch` is [N, C, T], planar and zero-padded -- a torch tensor on the GPU for out="device", a numpy array for
    out="host" -- with T = pad_to or the longest window and C = pad_channels or the most channels of a named stream;
    results[i] is the _lib.WindowResult of window i (rc, frames, bad_frames, bad_crc16, samples: the valid samples of
    batch[i], fewer than the window's length where it reaches past the stream's end).  dtype as for decode_many
    ("int24": uint8 [N, C, T, 3])."""
    if out not in ("device", "host"):
        raise ValueError("out must be 'device' or 'host'")
    if dtype not in _DTYPES:
        raise ValueError("dtype must be 'int32', 'int16', 'int24' or 'float32'")
    wins = window_array(windows)
    n = len(recs)
    named = [recs[w.stream] for w in wins if w.stream < n and recs[w.stream].rc == 0]
    fmt = _lib.OutFormat(_DTYPES[dtype], _lib.LAYOUT_PADDED, 0, 0, 0)
    fmt.samples_padded = pad_to or max([w.length for w in wins], default=0)
    fmt.channels_padded = pad_channels or max([r.info.channels for r in named], default=0)
    shape = (len(wins), fmt.channels_padded, fmt.samples_padded)
    need = Decoder.plan_windows(fmt, recs, n, wins)   # refuses before anything is allocated
    array_dtype, shape = _element_array(dtype, shape)
    if out == "device":
        import torch

        dev = decoder.device if decoder.device >= 0 else torch.cuda.current_device()
        buf = torch.empty(shape, dtype=getattr(torch, array_dtype), device=f"cuda:{dev}")
        torch.cuda.synchronize(dev)
        results = decoder.decode_windows(buf.data_ptr() if need else None, need, fmt, _lib.DECODE_OUT_DEVICE, wins)
    else:
        buf = np.empty(shape, dtype=array_dtype)
        results = decoder.decode_windows(buf.ctypes.data if need else None, need, fmt, 0, wins)
    return buf, list(results)[:len(wins)]


def host_pack_frames(sample_rate, bits_per_sample, channels, first_frame_number, n_frames,
                     row_stride, plans, subs, rows, threads=1):
    """Host bit-packing of an analysed batch (flacenc_pack_frames); returns (bytes, offsets)."""
    L = _lib.lib()
    off = (C.c_uint64 * (n_frames + 1))()
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    args = (sample_rate, bits_per_sample, channels, first_frame_number, n_frames, row_stride,
            C.cast(plans, C.c_void_p), C.cast(subs, C.c_void_p),
            rows.ctypes.data_as(C.POINTER(C.c_int32)), threads)
    rc = L.flacenc_pack_frames(*args, None, 0, off)
    if rc not in (0, -140):
        raise RuntimeError(f"flacenc_pack_frames: {rc}")
    buf = np.empty(off[n_frames], dtype=np.uint8)
    rc = L.flacenc_pack_frames(*args, buf.ctypes.data, buf.size, off)
    if rc:
        raise RuntimeError(f"flacenc_pack_frames: {rc}")
    return buf.tobytes(), list(off)


class PinnedBuffer:
    """Pinned host memory from flacgpu_host_alloc, viewed as a numpy uint8 array (`.array`)."""

    def __init__(self, nbytes):
        self._p = _lib.lib().flacgpu_host_alloc(nbytes)
        if not self._p:
            raise MemoryError("flacgpu_host_alloc")
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    @property
    def address(self):
        return self._p

    def close(self):
        if self._p:
            self.array = None
            _lib.lib().flacgpu_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """flacgpu_pipeline_* (include/flacenc_gpu.h): `depth` encoder contexts taking consecutive batches in rotation --
    upload of batch n, kernels of n - 1 and the frames of n - 2 in flight together.  PCM comes from PINNED buffers
    (PinnedBuffer) and must stay untouched until its batch has been retired."""

    def __init__(self, block_size, max_partition_order, max_lpc_order, mid_side, exhaustive, window_kind, window_param,
                 bits_per_sample, channels, max_frames, depth=4, device=-1):
        L = _lib.lib()
        o = GpuOptions(block_size, max_partition_order, max_lpc_order or 0, int(bool(mid_side)),
                       int(bool(exhaustive)), window_kind, 0, window_param)
        self._h = C.c_void_p(None)
        rc = L.flacgpu_pipeline_create(C.byref(o), bits_per_sample, channels, device, max_frames, depth, C.byref(self._h))
        if rc:
            raise GpuError(rc, "flacgpu_pipeline_create")
        self.depth = depth

    def in_flight(self):
        return _lib.lib().flacgpu_pipeline_in_flight(self._h)

    def submit(self, pinned_address, bytes_per_sample, n_frames, last_frame_len, first_frame_number, sample_rate):
        """Returns False (nothing queued) when every slot holds a batch: retire() first."""
        rc = _lib.lib().flacgpu_pipeline_submit(self._h, C.c_void_p(pinned_address), bytes_per_sample, n_frames,
                                                last_frame_len, first_frame_number, sample_rate)
        if rc == -6:
            return False
        if rc:
            raise GpuError(rc, "flacgpu_pipeline_submit")
        return True

    def retire(self, copy=True):
        """The oldest batch in flight: (frame bytes, offsets[n_frames + 1]); with copy=False a (address, total,
        offsets pointer, n_frames) tuple valid until the next submit."""
        frames = C.c_void_p(None)
        off = C.POINTER(C.c_uint64)()
        n = C.c_uint32(0)
        total = C.c_uint64(0)
        rc = _lib.lib().flacgpu_pipeline_retire(self._h, C.byref(frames), C.byref(off), C.byref(n), C.byref(total))
        if rc:
            raise GpuError(rc, "flacgpu_pipeline_retire")
        if not copy:
            return frames.value, total.value, off, n.value
        return C.string_at(frames.value, total.value), [off[i] for i in range(n.value + 1)]

    def close(self):
        if self._h:
            _lib.lib().flacgpu_pipeline_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_counters_c(per_shard):
    """flacgpu_merge_counters on [[frames, bytes, min_frame, max_frame], ...]: (merged record, shard byte offsets)."""
    n = len(per_shard)
    arr = (_lib.ShardCounters * n)(*[_lib.ShardCounters(*[int(v) for v in c]) for c in per_shard])
    merged = _lib.ShardCounters()
    offs = (C.c_uint64 * n)()
    rc = _lib.lib().flacgpu_merge_counters(arr, n, C.byref(merged), offs)
    if rc:
        raise GpuError(rc, "flacgpu_merge_counters")
    return merged.as_list(), [int(v) for v in offs]


def shard_range_c(total_frames, shards, shard):
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    _lib.lib().flacgpu_shard_range(total_frames, shards, shard, C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


class MultiDevice:
    """flacgpu_multi_* (include/flacenc_gpu.h "several GPUs"): one process, one shard per listed device, batches of
    contiguous frames of one stream dealt to the shards in turn, the four-integer records merged on the host.  `devices=None`: every visible device;
    an ordinal may be listed more than once (a 1-GPU box then exercises the whole multi-shard path)."""

    def __init__(self, block_size, max_partition_order, max_lpc_order, mid_side, exhaustive, window_kind, window_param,
                 bits_per_sample, channels, max_frames, devices=None, depth=2):
        L = _lib.lib()
        o = GpuOptions(block_size, max_partition_order, max_lpc_order or 0, int(bool(mid_side)),
                       int(bool(exhaustive)), window_kind, 0, window_param)
        self._h = C.c_void_p(None)
        devs = (C.c_int * len(devices))(*devices) if devices else None
        rc = L.flacgpu_multi_create(C.byref(o), bits_per_sample, channels, devs, len(devices) if devices else 0,
                                    max_frames, depth, C.byref(self._h))
        if rc:
            raise GpuError(rc, "flacgpu_multi_create")
        self.shards = L.flacgpu_multi_shards(self._h)
        self.devices = [L.flacgpu_multi_device_of(self._h, k) for k in range(self.shards)]
        self.block_size, self.channels, self.bits_per_sample = block_size, channels, bits_per_sample

    def encode(self, pcm, n_frames, last_frame_len, first_frame_number, sample_rate, bytes_per_sample=4):
        """Host PCM of one stream's run of blocks (int32 array, or a uint8 array of packed little-endian samples) ->
        (frame bytes, offsets[n_frames + 1], per-shard records, merged record)."""
        L = _lib.lib()
        pcm = np.ascontiguousarray(pcm, dtype=np.int32 if bytes_per_sample == 4 else np.uint8)
        off = (C.c_uint64 * (n_frames + 1))()
        total = C.c_uint64(0)
        per = (_lib.ShardCounters * self.shards)()
        merged = _lib.ShardCounters()
        args = (self._h, C.c_void_p(pcm.ctypes.data), bytes_per_sample, n_frames, last_frame_len, first_frame_number,
                sample_rate)
        cap = n_frames * (self.block_size * self.channels * ((self.bits_per_sample + 7) // 8 + 1) + 64)
        buf = np.empty(cap, dtype=np.uint8)
        rc = L.flacgpu_multi_encode(*args, C.c_void_p(buf.ctypes.data), cap, off, C.byref(total), per, C.byref(merged))
        if rc:
            raise GpuError(rc, "flacgpu_multi_encode")
        return (buf[: total.value].tobytes(), [int(v) for v in off], [c.as_list() for c in per], merged.as_list())

    def encode_raw(self, address, n_frames, last_frame_len, first_frame_number, sample_rate, bytes_per_sample=4):
        """flacgpu_multi_encode on a caller-held (pinned) buffer, frames into a reused output array: the timed form."""
        L = _lib.lib()
        cap = n_frames * (self.block_size * self.channels * ((self.bits_per_sample + 7) // 8 + 1) + 64)
        if getattr(self, "_out", None) is None or self._out.size < cap:
            self._out = np.empty(cap, dtype=np.uint8)
            self._out[:] = 0      # touched: page faults are not the encoder's
        total = C.c_uint64(0)
        rc = L.flacgpu_multi_encode(self._h, C.c_void_p(address), bytes_per_sample, n_frames, last_frame_len, first_frame_number,
                                    sample_rate, C.c_void_p(self._out.ctypes.data), cap, None, C.byref(total), None, None)
        if rc:
            raise GpuError(rc, "flacgpu_multi_encode")
        return total.value

    def host_copy_stats(self):
        """(bytes handed out in `out`, bytes the host copied to put them there, shard threads bound near their GPU)"""
        a, b, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        rc = _lib.lib().flacgpu_multi_host_copy_stats(self._h, C.byref(a), C.byref(b), C.byref(n))
        if rc:
            raise GpuError(rc, "flacgpu_multi_host_copy_stats")
        return a.value, b.value, n.value

    @staticmethod
    def numa_info(device):
        """(NUMA node of the device's PCI function or -1, its local CPU list as sysfs spells it or '')"""
        node = C.c_int(-1)
        buf = C.create_string_buffer(1024)
        rc = _lib.lib().flacgpu_device_numa_info(device, C.byref(node), buf, 1024)
        if rc:
            raise GpuError(rc, "flacgpu_device_numa_info")
        return node.value, buf.value.decode()

    def encode_device(self, shard, device_ptr, n_frames, last_frame_len, first_frame_number, sample_rate,
                      layout=LAYOUT_INTERLEAVED):
        rc = _lib.lib().flacgpu_multi_encode_device(self._h, shard, C.c_void_p(device_ptr), layout, n_frames,
                                                    last_frame_len, first_frame_number, sample_rate)
        if rc:
            raise GpuError(rc, "flacgpu_multi_encode_device")

    def wait(self):
        rc = _lib.lib().flacgpu_multi_wait(self._h)
        if rc:
            raise GpuError(rc, "flacgpu_multi_wait")

    def counters(self):
        per = (_lib.ShardCounters * self.shards)()
        merged = _lib.ShardCounters()
        rc = _lib.lib().flacgpu_multi_counters(self._h, per, C.byref(merged))
        if rc:
            raise GpuError(rc, "flacgpu_multi_counters")
        return [c.as_list() for c in per], merged.as_list()

    def fetch_last(self, shard, n_frames):
        """Frame bytes and offsets of shard `shard`'s last resident batch."""
        h = _lib.lib().flacgpu_multi_last_context(self._h, shard)
        off = (C.c_uint64 * (n_frames + 1))()
        total = C.c_uint64(0)
        rc = _lib.lib().flacgpu_fetch_frames(C.c_void_p(h), None, 0, off, C.byref(total))
        if rc not in (0, -5):
            raise GpuError(rc, "flacgpu_fetch_frames")
        buf = np.empty(total.value, dtype=np.uint8)
        rc = _lib.lib().flacgpu_fetch_frames(C.c_void_p(h), C.c_void_p(buf.ctypes.data), buf.size, off, C.byref(total))
        if rc:
            raise GpuError(rc, "flacgpu_fetch_frames")
        return buf.tobytes(), [int(v) for v in off]

    def close(self):
        if self._h:
            _lib.lib().flacgpu_multi_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_allgather_counters(nccl_comm, local, cap_ranks=64, stream=None):
    """flacgpu_rccl_allgather_counters: every rank's [frames, bytes, min_frame, max_frame] over the caller's RCCL
    communicator (an ncclComm_t as an integer / c_void_p); returns (records in rank order, this rank)."""
    mine = _lib.ShardCounters(*[int(v) for v in local])
    out = (_lib.ShardCounters * cap_ranks)()
    n, me = C.c_uint32(0), C.c_uint32(0)
    rc = _lib.lib().flacgpu_rccl_allgather_counters(C.c_void_p(nccl_comm), C.c_void_p(stream or 0), C.byref(mine), out,
                                                    cap_ranks, C.byref(n), C.byref(me))
    if rc:
        raise GpuError(rc, "flacgpu_rccl_allgather_counters")
    return [out[i].as_list() for i in range(n.value)], int(me.value)
