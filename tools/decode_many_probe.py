#!/usr/bin/env python3
"""Wall times of the batch decoder (flacgpu_decoder_scan + flacgpu_decoder_decode) on three workloads, against a loop
over flacgpu_decode_stream and the oracle's CPU decoder on one core; writes profiles/r07_decode_many.json.

    python tools/decode_many_probe.py [--workloads clips,tracks,hour] [--out FILE] [--reps 3]
    python tools/decode_many_probe.py --merge-stats kernel_stats.csv --out FILE   (adds one rocprofv3 --stats run)
    python tools/decode_many_probe.py --formats [--out profiles/r09_decode_formats.json] [--reps 9]
    python tools/decode_many_probe.py --formats --label parent --package-root DIR   (DIR: a built checkout of the
                                             parent commit; the default int32 path only, into the same file)
    python tools/decode_many_probe.py --formats --kernels-only   (one warm call per leg, for rocprofv3)
    python tools/decode_many_probe.py --formats --s24 [--out profiles/r12_s24.json] [--reps 15] [--shrink 4]
    python tools/decode_many_probe.py --windows [--workloads tracks,clips] [--out profiles/r10_decode_windows.json]
                                             [--reps 15] [--kernels-only]
    python tools/decode_many_probe.py --raw --label this_1 [--out profiles/r13_raw_frames.json] [--reps 15]
    python tools/decode_many_probe.py --raw --label parent --package-root DIR   (the regular leg only)
    python tools/decode_many_probe.py --raw --label this_2          (in this order: this build, parent, this build)
    python tools/decode_many_probe.py --raw --kernels-only          (one warm call per leg, for rocprofv3)
    python tools/decode_many_probe.py --raw --speculative --label this_1 [--out profiles/r14_speculative.json]
    python tools/decode_many_probe.py --raw --speculative --label parent --package-root DIR   (both flag-off legs)
    python tools/decode_many_probe.py --raw --speculative --label this_2
    python tools/decode_many_probe.py --raw --speculative --kernels-only

    python tools/decode_many_probe.py --timeline --label this_1 [--out profiles/r16_timeline.json] [--reps 15]
    python tools/decode_many_probe.py --timeline --label parent --package-root DIR   (the decode_as leg only)
    python tools/decode_many_probe.py --timeline --label this_2
    python tools/decode_many_probe.py --timeline --kernels-only
    python tools/decode_many_probe.py --raw|--timeline --label parent --package-root DIR --parent-all-legs   (a parent that
                                             has every leg of the mode: each is then held to the parent's own spread of it)
    python tools/decode_many_probe.py --analyze [--out profiles/r25_frame_analysis.json] [--reps 15]
    python tools/decode_many_probe.py --analyze --kernels-only      (a warm call and three more per leg, for rocprofv3)
    python tools/decode_many_probe.py --session [--out profiles/r22_decoder_session.json] [--reps 15]
    python tools/decode_many_probe.py --session --container [--out profiles/r24_container_session.json] [--reps 15]
                                             [--workloads clips,hour] [--hour-seconds N]   (container sessions: whole
                                             .flac files in pieces, MD5 across feeds; see container_session's docstring)

--timeline (flacgpu_decoder_decode_timeline): on the clips with the metadata stripped, float32, device output, handle
warm, the wall time of scan_frames + decode_as (padded; the parent's call for such a batch) and of scan_frames +
decode_timeline with the mask, undamaged and with one frame in 50 removed by a fixed seed.  The undamaged timeline is
held to the parent's own min-max spread of its decode_as leg; the damaged leg has no parent and is reported as it is.

--raw (flacgpu_decoder_scan_frames): on the clips, device output, no MD5, handle warm, the wall time of (regular) scan +
decode of the files as they are and (raw) scan_frames + decode of the same files with the fLaC marker and metadata
removed; both must give the same PCM, and its SHA-256 must be the same under every label.  Every leg reads the shader
clock before and after.  The parent's build runs the regular leg alone; once this_1, parent and this_2 are in the file,
`verdict` holds the parent's min-max spread (the allowance) and whether each of this build's medians lies inside it.

--raw --speculative (FLACGPU_SCAN_SPECULATIVE): the same two legs -- the parent's build, which has the raw scan, runs
both, and the verdict holds each flag-off leg of this build to the parent's spread of the same leg; they are timed
first, before the process has done anything the parent's does not -- and behind them a third, the raw leg with
speculative=True, whose PCM must be the same again.  The record names the candidates without a link, which k_spec_end
walks, as this probe's own model of K_r2's rule counts them on the host (clean input: the rare false candidates and the
last frame's look-alikes); the device's link array is not read.  A fourth leg gives the walk something to do: the same
clips with byte 0 of every second frame zeroed, under the flag, which must keep exactly the other frames -- all by their
own bits but a stream's last.  (In the --kernels-only run k_spec_end's shortest calls are the clean input's and its
longest the damaged one's.)

--formats (flacgpu_decoder_decode_as): on the clips, device output, no MD5, handle warm, the wall time of one
scan + decode call into (a) what a caller of flacgpu_decoder_decode does -- interleaved int32, then torch ops to the
same [B, 1, T] float32 (or int16) padded tensor -- and (b) decode_many(dtype=, layout="padded") in one call; and the
default int32 path itself, whose figure the parent's build repeats on the same box (the regression guard: the margin is
the spread over --reps that this probe sees).

--formats --s24 (FLACGPU_SAMPLE_S24, dtype="int24"): on 1024 clips of 10 s, 48 kHz stereo 24-bit (divided by
--shrink), no MD5, handle warm.  Host output: (a) decode_many(dtype="int32", out="host") and the numpy pack to 3 bytes
that a WAV writer then needs, against (b) one decode_many(dtype="int24", out="host"); both must give the same bytes.
Device output: the int32 call against the int24 call, with the bytes each holds.

--device-input (flacgpu_decoder_scan_device): the clips and the tracks in one batch, the scan alone, handle warm, median
and min to max of 15 runs, the shader clock read before and after each leg: (a) the bytes in host memory through
flacgpu_decoder_scan; (b) the same bytes resident in device memory through flacgpu_decoder_scan_device; (c) for bytes
born on the device, a download into pinned memory plus the host scan, to set against (b); and a plain device-to-device
copy of the same byte count (torch's copy_, a hipMemcpyAsync), the yardstick for the gather kernel, whose own time a
`rocprofv3 --kernel-trace --stats` run of `--device-input --kernels-only` gives (--merge-stats puts it into the
record as kernel_stats and gather_effective_gbps).  --label this_1 / parent (with --package-root, leg (a) alone) / this_2 in
that order add the guard on the host door: profiles/r15_device_input.json.

--session (flacgpu_decoder_session_*; DESIGN.md 4b "Decoder sessions"), median and min to max of 15, the shader clock
read before and after each leg.  Per-feed latency: the device stream writer's workload -- 64 mono 16 kHz streams, one
frame of 80 ms per stream per feed, the frames written by a device stream writer beforehand -- as feed + decode_frames
into device memory, with flush=True (each frame out in its own feed) and without (one feed later); the feed and the
decode are also timed apart, and the feed call's own division (flacgpu_decoder_session_last_feed_timing: staging, the
scan up to each of its two synchronisations, the host walk, the frame table's upload) is recorded beside them.
Throughput: the clips, metadata stripped, fed in 1, 4, 16 and 64 pieces (a feed and a decode_frames per piece, then
finish) against one-shot scan_frames + decode_frames in the same process, identical PCM asserted by SHA-256 over the
frames in stream order: profiles/r22_decoder_session.json.

--windows (flacgpu_decoder_decode_windows): on a resident scan (scanned once, outside the timed part), device output,
no MD5, handle warm, the wall time of one round of random crops -- one crop of 5 s (tracks) or 1 s (clips) per stream
at seeded random positions -- as (a) what a caller without windows does: decode_as float32 PADDED of the whole batch,
then torch slicing into [B, C, T]; and (b) decode_windows.  Each leg runs in its own decoder and reports the peak
device memory it adds on top of the resident scan (hipMemGetInfo through torch, so the library's buffers count).  (a)
needs the whole batch's padded output beside the scan; when that does not fit, both legs take the largest prefix of the
batch that does, and the record says so.

Workloads (default options of FlacSampleWriter; a few distinct streams repeated to the batch size -- the decoder
does not see that they repeat):
    clips   1024 clips of 10 s, 16 kHz mono 16-bit
    tracks  256 tracks of 3 min, 44.1 kHz stereo 16-bit
    hour    one stream of 1 h, 48 kHz stereo 24-bit
"new" wall time: host bytes (a list of Python bytes) to interleaved int32 in HBM (a torch tensor), the handle warm
(buffers already grown), median of --reps.  "loop": flacgpu_decode_stream per stream into host memory (its only
output).  "oracle": orc_decode_stream on one core over the first streams until --oracle-seconds have passed, scaled
to the workload by decoded samples."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = {   # name: (streams, distinct, seconds, rate, channels, bps)
    "clips": (1024, 16, 10, 16000, 1, 16),
    "clips24": (1024, 16, 10, 48000, 2, 24),
    "tracks": (256, 4, 180, 44100, 2, 16),
    "hour": (1, 1, 3600, 48000, 2, 24),
}
COPY_TBPS = 6.3   # measured device copy rate


def make_blobs(name):
    from _pcm import synth_fast
    from flac_codec_amd.encode import FlacSampleWriter, Options

    n, distinct, secs, rate, ch, bps = WORKLOADS[name]
    uniq = []
    for k in range(distinct):
        pcm = synth_fast(900 + k, ch, bps, secs * rate)
        w = FlacSampleWriter(None, Options.default(), rate, bps, ch, pcm.size)
        w.write(pcm)
        w.finalize()
        uniq.append(w.getvalue())
        w.close()
        del pcm
    return [uniq[i % distinct] for i in range(n)]


def time_new(blobs, reps, md5):
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    dec = Decoder(0)
    flags = _lib.DECODE_OUT_DEVICE | (0 if md5 else _lib.DECODE_NO_MD5)
    recs, total = dec.scan(blobs)
    out = torch.empty(total, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dec.decode(out.data_ptr(), total, flags, recs)   # warm: buffers grown, code loaded
    times, scan_t = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        recs, total = dec.scan(blobs)
        t1 = time.perf_counter()
        dec.decode(out.data_ptr(), total, flags, recs)
        t2 = time.perf_counter()
        times.append(t2 - t0)
        scan_t.append(t1 - t0)
    bad = sum(1 for r in recs if r.rc or r.info.bad_frames or r.info.bad_crc16 or (md5 and r.info.md5_status != 1))
    dec.close()
    del out
    return float(np.median(times)), float(np.median(scan_t)), int(total), bad


def time_loop(blobs):
    from flac_codec_amd import _lib

    L = _lib.lib()
    info = _lib.StreamInfo()
    buf = None
    t0 = time.perf_counter()
    for b in blobs:
        rc = L.flacgpu_decode_stream(b, len(b), 0, None, 0, C.byref(info))
        need = info.decoded_samples * info.channels
        if buf is None or buf.size < need:
            buf = np.empty(need, np.int32)
        rc |= L.flacgpu_decode_stream(b, len(b), 0, buf.ctypes.data_as(C.POINTER(C.c_int32)), buf.size, C.byref(info))
        assert rc == 0 and info.md5_status == 1
    return time.perf_counter() - t0


def time_loop_single_call(blobs):
    """one flacgpu_decode_stream call per stream (the size known beforehand), the loop's lower bound"""
    from flac_codec_amd import _lib

    L = _lib.lib()
    info = _lib.StreamInfo()
    sizes = []
    for b in blobs[:1]:
        L.flacgpu_decode_stream(b, len(b), 0, None, 0, C.byref(info))
        sizes.append(info.decoded_samples * info.channels)
    buf = np.empty(max(sizes) * 2, np.int32)
    t0 = time.perf_counter()
    for b in blobs:
        rc = L.flacgpu_decode_stream(b, len(b), 0, buf.ctypes.data_as(C.POINTER(C.c_int32)), buf.size, C.byref(info))
        assert rc == 0
    return time.perf_counter() - t0


def time_oracle(blobs, budget):
    import _oracle as orc

    t0 = time.perf_counter()
    done, samples = 0, 0
    for b in blobs:
        rc, out, _ = orc.decode_stream(b)
        assert rc == 0
        done += 1
        samples += out.size
        if time.perf_counter() - t0 > budget:
            break
    return time.perf_counter() - t0, done, samples


def _sclk_mhz():
    """The shader clock now (MHz), read only; None when rocm-smi does not answer."""
    import re
    import subprocess

    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
    except (OSError, subprocess.SubprocessError):
        return None
    m = re.search(r"sclk clock level.*?\((\d+)Mhz\)", out)
    return int(m.group(1)) if m else None


def parent_only(args):
    """True when this run times only the legs that the parent of the pull request a mode was written for had."""
    return args.label == "parent" and not args.parent_all_legs


def _spread(times):
    t = sorted(times)
    return {"median_s": float(np.median(t)), "min_s": t[0], "max_s": t[-1], "reps": len(t)}


def formats(args):
    """The --formats leg (see the module docstring)."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, decode_many

    blobs = make_blobs("clips")
    new_abi = hasattr(_lib, "OutFormat")
    dec = Decoder(0)
    scale = {"float32": 2.0 ** -15, "int16": None}

    def legacy(dtype):   # (a): the parent's only output, then a second pass over HBM in torch
        flat, streams = decode_many(blobs, out="device", verify_md5=False, decoder=dec)
        T = max(s.info.decoded_samples for s in streams)
        batch = torch.zeros((len(streams), 1, T), dtype=getattr(torch, dtype), device=flat.device)
        for i, s in enumerate(streams):   # mono: [samples, 1] -> [1, samples]
            row = s.pcm.T
            batch[i, :, :row.shape[1]] = row.to(torch.float32) * scale[dtype] if scale[dtype] else row.to(torch.int16)
        return batch

    def legacy_equal_lengths(dtype):   # (a) at its best: every clip as long as the others, one reshape
        flat, streams = decode_many(blobs, out="device", verify_md5=False, decoder=dec)
        v = flat.view(len(streams), 1, -1)
        return v.to(torch.float32) * scale[dtype] if scale[dtype] else v.to(torch.int16)

    def fused(dtype):    # (b)
        return decode_many(blobs, out="device", verify_md5=False, decoder=dec, dtype=dtype, layout="padded")[0]

    def default():
        return decode_many(blobs, out="device", verify_md5=False, decoder=dec)[0]

    legs = {"int32_flat_default": default}
    if new_abi and args.label != "parent":
        for dt in ("float32", "int16"):
            legs[f"a_int32_then_torch_{dt}"] = (lambda dt=dt: legacy(dt))
            legs[f"a_equal_lengths_reshape_{dt}"] = (lambda dt=dt: legacy_equal_lengths(dt))
            legs[f"b_decode_as_padded_{dt}"] = (lambda dt=dt: fused(dt))
    if args.kernels_only:
        for fn in legs.values():
            fn()
            fn()
        torch.cuda.synchronize()
        dec.close()
        return
    res = {"tool": "tools/decode_many_probe.py --formats", "workload": "clips: 1024 x 10 s, 16 kHz mono 16-bit",
           "device_output": True, "md5": False, "runs": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    rec = {"build_id": _lib.build_id(), "sclk_mhz_before": _sclk_mhz(), "legs": {}}
    if new_abi and args.label != "parent":   # (a) and (b) give the same tensor
        for dt in ("float32", "int16"):
            assert torch.equal(legacy(dt), fused(dt)) and torch.equal(legacy_equal_lengths(dt), fused(dt))
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()   # warm: buffers grown, code loaded
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        rec["legs"][name] = dict(_spread(times), output_bytes=int(out.numel() * out.element_size()))
        del out
    rec["sclk_mhz_after"] = _sclk_mhz()
    res["runs"][args.label] = rec
    dec.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({args.label: rec}, indent=1), flush=True)


def s24(args):
    """The --formats --s24 leg (see the module docstring)."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, decode_many

    blobs = make_blobs("clips24")
    blobs = blobs[:max(1, len(blobs) // args.shrink)]
    dec = Decoder(0)

    def a_host():   # the int32 download, then the pack on the CPU
        flat, _ = decode_many(blobs, out="host", verify_md5=False, decoder=dec)
        return np.ascontiguousarray(flat.view(np.uint8).reshape(-1, 4)[:, :3])

    def a_host_call_only():
        return decode_many(blobs, out="host", verify_md5=False, decoder=dec)[0]

    def b_host():
        return decode_many(blobs, out="host", verify_md5=False, decoder=dec, dtype="int24")[0]

    def dev(dtype):
        return decode_many(blobs, out="device", verify_md5=False, decoder=dec, dtype=dtype)[0]

    legs = {"host_a_int32_then_numpy_pack": a_host, "host_a_int32_call_alone": a_host_call_only,
            "host_b_int24": b_host, "device_int32": lambda: dev("int32"), "device_int24": lambda: dev("int24")}
    if args.kernels_only:
        for fn in legs.values():
            fn()
            fn()
        torch.cuda.synchronize()
        dec.close()
        return
    assert np.array_equal(a_host(), b_host())
    assert np.array_equal(dev("int24").cpu().numpy(), b_host())
    n = len(blobs)
    rec = {"tool": "tools/decode_many_probe.py --formats --s24", "build_id": _lib.build_id(),
           "workload": f"{n} clips x 10 s, 48 kHz stereo 24-bit", "md5": False, "legs": {}}
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()   # warm: buffers grown, code loaded
        sclk_before = _sclk_mhz()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        rec["legs"][name] = dict(_spread(times), sclk_mhz_before=sclk_before, sclk_mhz_after=_sclk_mhz(),
                                 output_bytes=int(out.nbytes if isinstance(out, np.ndarray) else
                                                  out.numel() * out.element_size()))
        del out
    dec.close()
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res["decoder"] = rec
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(rec, indent=1), flush=True)


def _gf_mul(a, b):   # a * b modulo the CRC-16 polynomial, over GF(2)
    r = 0
    for i in range(15, -1, -1):
        r = ((r << 1) ^ 0x8005) & 0xFFFF if r & 0x8000 else (r << 1) & 0xFFFF
        if (b >> i) & 1:
            r ^= a
    return r


def _gf_xpow(e):     # x^e
    r, sq = 1, 2
    while e:
        if e & 1:
            r = _gf_mul(r, sq)
        sq, e = _gf_mul(sq, sq), e >> 1
    return r


def unlinked_candidates(blob):
    """The candidates of the raw scan of `blob` that K_r2 (k_link_raw) leaves without a link -- those k_spec_end walks --
    by the scan's identity: frame [s, q) has a right CRC-16 exactly when A(q) == A(s), A(k) = P(k) x^(-8 k)."""
    import _oracle as orc
    import _raw_frames as rf

    heads = rf.candidates(blob)
    order = sorted(heads)
    A, P, at = {}, 0, 0
    for q in order + [len(blob)]:
        P = _gf_mul(P, _gf_xpow(8 * (q - at) % 32767)) ^ orc.crc16(blob[at:q])
        A[q], at = _gf_mul(P, _gf_xpow(-8 * q % 32767)), q
    none = 0
    for i, s in enumerate(order):
        lo = s + heads[s]["header_bytes"] + 2 + heads[s]["channels"]
        linked = any(q >= lo and A[q] == A[s] for q in order[i + 1:]) or (len(blob) - s >= 2 and A[len(blob)] == A[s])
        none += not linked
    return none, len(order)


def raw_frames(args):
    """The --raw leg (see the module docstring)."""
    import hashlib

    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, decode_many, scan_stream_host

    blobs = make_blobs("clips")
    has_raw = hasattr(Decoder, "scan_frames") and (args.speculative or not parent_only(args))
    has_spec = args.speculative and not parent_only(args)
    dec = Decoder(0)
    legs = {"regular_scan_decode": lambda: decode_many(blobs, out="device", verify_md5=False, decoder=dec)[0]}
    if has_raw:
        bare = [b[int(scan_stream_host(b)[1][0]):] for b in blobs]   # from the first frame on
        legs["raw_scan_frames_decode"] = lambda: decode_many(bare, out="device", verify_md5=False, decoder=dec,
                                                             raw=True)[0]
    spec_legs = {}
    if has_spec:
        spec_legs["raw_scan_frames_decode_speculative"] = lambda: decode_many(
            bare, out="device", verify_md5=False, decoder=dec, raw=True, speculative=True)[0]
        spec_legs["raw_damaged_scan_frames_decode_speculative"] = lambda: decode_many(
            damaged_batch(), out="device", verify_md5=False, decoder=dec, raw=True, speculative=True)[0]
    made = {}

    def damaged_batch():   # built on first use: behind the flag-off legs' timing
        if not made:
            cache, pairs = {}, []
            for b, whole in zip(bare, blobs):
                if b not in cache:
                    offsets = scan_stream_host(whole)[1]
                    d = bytearray(b)
                    for off in offsets[1::2]:
                        d[int(off) - int(offsets[0])] = 0
                    cache[b] = (bytes(d), len(offsets) - len(offsets) // 2)
                pairs.append(cache[b])
            made["blobs"], made["undamaged"] = [d for d, _ in pairs], sum(n for _, n in pairs)
        return made["blobs"]

    if args.kernels_only:
        for fn in list(legs.values()) + list(spec_legs.values()):
            fn()
            fn()
        torch.cuda.synchronize()
        dec.close()
        return
    res = {"tool": "tools/decode_many_probe.py --raw" + (" --speculative" if args.speculative else ""),
           "workload": "clips: 1024 x 10 s, 16 kHz mono 16-bit", "device_output": True, "md5": False, "order": [], "runs": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    pcm = legs["regular_scan_decode"]()
    rec = {"build_id": _lib.build_id(), "pcm_sha256": hashlib.sha256(pcm.cpu().numpy().tobytes()).hexdigest(),
           "legs": {}}
    if has_raw:
        assert torch.equal(pcm, legs["raw_scan_frames_decode"]())   # identical PCM
    for other in res["runs"].values():
        assert other["pcm_sha256"] == rec["pcm_sha256"]             # and under every label

    def timed(legs):
        for name, fn in legs.items():
            fn()
            torch.cuda.synchronize()   # warm: buffers grown, code loaded
            sclk_before = _sclk_mhz()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            rec["legs"][name] = dict(_spread(times), sclk_mhz_before=sclk_before, sclk_mhz_after=_sclk_mhz())
            del out

    # The flag-off legs first, in a process that has done nothing the parent's has not: no speculative scan, no damaged
    # batch, no spec_len.  Everything of the flag comes behind them.
    timed(legs)
    if has_spec:
        assert torch.equal(pcm, spec_legs["raw_scan_frames_decode_speculative"]())
        damaged = damaged_batch()
        counts = {}
        for b in set(bare) | set(damaged):   # the batch repeats a few distinct streams
            counts[b] = unlinked_candidates(b)
        # counted by this probe's model of K_r2's rule (unlinked_candidates), not read from the device's link array
        rec["candidates"] = sum(counts[b][1] for b in bare)
        rec["candidates_without_link_by_the_probes_model"] = sum(counts[b][0] for b in bare)
        _, streams = decode_many(damaged, out="device", verify_md5=False, decoder=dec, raw=True, speculative=True)
        assert sum(s.info.frames for s in streams) == made["undamaged"] and all(s.rc == 0 for s in streams)
        _, streams = decode_many(damaged, out="device", verify_md5=False, decoder=dec, raw=True)
        rec["damaged"] = {"frames_kept_with_the_flag": made["undamaged"],
                          "frames_kept_without_it": int(sum(s.info.frames for s in streams)),
                          "candidates": sum(counts[b][1] for b in damaged),
                          "candidates_without_link_by_the_probes_model": sum(counts[b][0] for b in damaged)}
        timed(spec_legs)
    del pcm
    dec.close()
    res["runs"][args.label] = rec
    res["order"].append(args.label)
    runs = res["runs"]
    if all(k in runs for k in ("this_1", "parent", "this_2")):
        allow = runs["parent"]["legs"]["regular_scan_decode"]
        inside = lambda leg, allow: allow["min_s"] <= leg["median_s"] <= allow["max_s"]   # noqa: E731
        res["verdict"] = {"allowance_parent_min_s": allow["min_s"], "allowance_parent_max_s": allow["max_s"],
                          "parent_median_s": allow["median_s"]}
        for label in ("this_1", "this_2"):
            for name, leg in runs[label]["legs"].items():
                if name.endswith("_speculative") and name not in runs["parent"]["legs"]:   # no leg of the parent's
                    continue
                # a leg the parent ran is held to the parent's spread of that leg; else (r13) to the regular leg's
                ref = runs["parent"]["legs"].get(name, allow)
                res["verdict"][f"{label}.{name}"] = {"median_s": leg["median_s"], "inside_parent_spread": inside(leg, ref),
                                                     "parent_min_s": ref["min_s"], "parent_max_s": ref["max_s"],
                                                     "over_parent_median": leg["median_s"] / ref["median_s"]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({args.label: rec, "verdict": res.get("verdict")}, indent=1), flush=True)


def analyze(args):
    """The --analyze leg: frame analysis (flacgpu_decoder_analyze; DESIGN.md 4b "Frame analysis") against decode_frames on
    ONE raw scan of the 1024 clips, handle warm, device output, one process: the records-only pass, the pass with rows,
    and decode_frames, each call alone (the scan is not timed), median and min to max of --reps runs, the shader clock
    before and after each leg: profiles/r25_frame_analysis.json.  No test asserts a time; the yardstick is decode_frames
    in the same process.  --kernels-only: a warm call and three more per leg, for rocprofv3 --kernel-trace --stats."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import ANALYSIS_FRAME_DTYPE, SUBFRAME_DTYPE, Decoder, scan_stream_host

    blobs = make_blobs("clips")
    bare = [b[int(scan_stream_host(b)[1][0]):] for b in blobs]   # from the first frame on
    dec = Decoder(0)
    _, _, _, frames = dec.scan_frames(bare)
    nf, ns, nr = dec.plan_analysis()
    L = _lib.lib()
    t_frames = torch.empty(nf * ANALYSIS_FRAME_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    t_subs = torch.empty(ns * SUBFRAME_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    t_rows = torch.empty(nr, dtype=torch.int32, device="cuda:0")
    t_pcm = torch.empty(dec.raw_elements, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def analysis(rows):
        rc = L.flacgpu_decoder_analyze(dec._h, _lib.DECODE_OUT_DEVICE, t_frames.data_ptr(), nf, t_subs.data_ptr(), ns,
                                       t_rows.data_ptr() if rows else None, nr if rows else 0)
        assert rc == 0, rc

    legs = {"analyze_records_only": lambda: analysis(False), "analyze_with_rows": lambda: analysis(True),
            "decode_frames": lambda: dec.decode_frames(t_pcm.data_ptr(), dec.raw_elements, _lib.DECODE_OUT_DEVICE,
                                                       frames.copy())}
    if args.kernels_only:
        for fn in legs.values():
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        dec.close()
        return
    res = {"tool": "tools/decode_many_probe.py --analyze", "workload": "clips: 1024 x 10 s, 16 kHz mono 16-bit",
           "device_output": True, "one_scan": "scan_frames, not timed", "build_id": _lib.build_id(), "frames": int(nf),
           "subframes": int(ns), "row_elements": int(nr), "reps": args.reps, "legs": {}}
    if os.path.exists(args.out):   # keep a kernel_stats record merged earlier
        with open(args.out) as f:
            res["kernel_stats"] = json.load(f).get("kernel_stats", {})
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()   # warm: buffers grown, tables uploaded, code loaded
        sclk_before = _sclk_mhz()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res["legs"][name] = dict(_spread(times), sclk_mhz_before=sclk_before, sclk_mhz_after=_sclk_mhz())
    status = t_frames.cpu().numpy().view(ANALYSIS_FRAME_DTYPE)["status"]
    res["frames_with_status"] = int((status != 0).sum())
    ref = res["legs"]["decode_frames"]["median_s"]
    res["over_decode_frames_median"] = {k: v["median_s"] / ref for k, v in res["legs"].items()}
    dec.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


def session(args):
    """The --session leg (see the module docstring)."""
    import hashlib

    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.encode import BatchEncoder, Options
    from flac_codec_amd.gpu import Decoder, DecoderSession, decode_frames, scan_stream_host

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from stream2flac import one_second

    res = {"tool": "tools/decode_many_probe.py --session", "build_id": _lib.build_id(), "reps": args.reps}

    def leg(times):
        return dict(_spread(times))

    # ---- per-feed latency: the device stream writer's workload, 64 mono 16 kHz streams, one 80 ms frame per stream
    n_streams, rate, packet, steps = 64, 16000, 1280, args.reps + 3
    frames = [[] for _ in range(n_streams)]
    with BatchEncoder(Options.default()).open_device_stream_writer(n_streams, rate, 16, 1, max_block=packet) as writer:
        for step in range(steps):
            chunk = one_second(torch, step, n_streams, 1, packet, rate, "cuda")
            for k, frame in enumerate(writer.write(chunk, [packet] * n_streams)):
                frames[k].append(frame)
    bound = max(len(f) for per in frames for f in per)
    res["latency"] = {"workload": "64 streams, 16 kHz mono 16-bit, one frame of 80 ms (1280 samples) per stream per feed",
                      "bytes_per_feed": sum(len(per[0]) for per in frames), "max_frame_bytes": bound,
                      "stream_writer_write_ms_r21": 0.47, "legs": {}}
    for name, flush in (("flush", True), ("no_flush", False)):
        ses = DecoderSession(n_streams, bound, device=0)
        out = torch.empty(n_streams * packet, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        feed_t, decode_t, both_t, got, inside = [], [], [], 0, {}
        sclk_before = None
        for step in range(steps):
            if step == 3:
                sclk_before = _sclk_mhz()   # three feeds warm: buffers grown, code loaded
            chunks = [per[step] for per in frames]
            t0 = time.perf_counter()
            recs, _ = ses.feed(chunks, flush)
            t1 = time.perf_counter()
            ses.decoder.decode_frames(out.data_ptr() if len(recs) else None, out.numel() if len(recs) else 0,
                                      _lib.DECODE_OUT_DEVICE, recs)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert len(recs) == (n_streams if flush or step else 0) and not recs["status"].any()
            got += len(recs)
            if step >= 3:
                for key, v in ses.last_feed_timing().items():   # the C call's own clock reads, milliseconds
                    inside.setdefault(key, []).append(v * 1e-3)
                feed_t.append(t1 - t0)
                decode_t.append(t2 - t1)
                both_t.append(t2 - t0)
        res["latency"]["legs"][name] = {"feed_plus_decode_frames": leg(both_t), "feed": leg(feed_t),
                                        "decode_frames": leg(decode_t),
                                        "inside_the_feed_call": {key: leg(v) for key, v in inside.items()},
                                        "sclk_mhz_before": sclk_before,
                                        "sclk_mhz_after": _sclk_mhz(), "frames": got}
        ses.close()

    # ---- throughput: the clips, metadata stripped, whole and in pieces
    blobs = make_blobs("clips")
    bare = [b[int(scan_stream_host(b)[1][0]):] for b in blobs]
    del blobs
    dec = Decoder(0)

    def one_shot():
        return decode_frames(bare, out="device", decoder=dec)

    flat, recs, _ = one_shot()
    bound = int(recs["bytes"].max())
    order = np.lexsort((recs["byte_offset"], recs["stream"]))
    host = flat.cpu().numpy()
    sha = hashlib.sha256()
    for r in recs[order]:
        sha.update(host[int(r["out_offset"]):int(r["out_offset"]) + int(r["block_size"]) * int(r["channels"])].tobytes())
    res["throughput"] = {"workload": "clips: 1024 x 10 s, 16 kHz mono 16-bit, metadata stripped",
                         "bytes": sum(len(b) for b in bare), "frames": int(len(recs)), "max_frame_bytes": bound,
                         "pcm_sha256": sha.hexdigest(), "legs": {}}
    total = int(flat.numel())
    del flat, host
    sclk = _sclk_mhz()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        one_shot()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res["throughput"]["legs"]["one_shot_scan_frames_decode_frames"] = dict(leg(times), sclk_mhz_before=sclk,
                                                                           sclk_mhz_after=_sclk_mhz())
    dec.close()
    out = torch.empty(total, dtype=torch.int32, device="cuda:0")
    for pieces in (1, 4, 16, 64):
        cut = [[b[len(b) * p // pieces:len(b) * (p + 1) // pieces] for p in range(pieces)] for b in bare]

        def run(check):
            ses = DecoderSession(len(bare), bound, device=0)
            parts = []
            for p in range(pieces + 1):
                recs, _ = ses.finish() if p == pieces else ses.feed([c[p] for c in cut])
                n = ses.decoder.raw_elements
                ses.decoder.decode_frames(out.data_ptr() if n else None, n, _lib.DECODE_OUT_DEVICE, recs)
                if check:
                    parts.append((recs, out[:n].cpu().numpy()))
            torch.cuda.synchronize()
            ses.close()
            return parts

        parts = run(True)   # warm, and the PCM: every frame once, in stream order
        keys = np.concatenate([np.stack([r["stream"].astype(np.int64), r["byte_offset"].astype(np.int64), np.full(len(r), i, np.int64),
                                         np.arange(len(r), dtype=np.int64)], 1)
                               for i, (r, _) in enumerate(parts)])
        sha = hashlib.sha256()
        for _, _, i, k in keys[np.lexsort((keys[:, 1], keys[:, 0]))]:
            r = parts[i][0][k]
            assert not r["status"]
            sha.update(parts[i][1][int(r["out_offset"]):int(r["out_offset"]) + int(r["block_size"]) * int(r["channels"])].tobytes())
        assert sha.hexdigest() == res["throughput"]["pcm_sha256"] and len(keys) == res["throughput"]["frames"]
        del parts
        sclk = _sclk_mhz()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run(False)
            times.append(time.perf_counter() - t0)
        res["throughput"]["legs"][f"session_{pieces}_pieces"] = dict(leg(times), sclk_mhz_before=sclk,
                                                                     sclk_mhz_after=_sclk_mhz(), identical_pcm=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


def container_session(args):
    """The --session --container leg: container sessions (DESIGN.md 4b "Container sessions"), whole .flac files fed in
    pieces with the MD5 taken across feeds.  (a) per-feed latency: 64 mono 16 kHz files, one 80 ms frame a feed, feed +
    decode with MD5, beside a raw session over the same frames (feed + decode_frames) in the same process.  (b)
    throughput: the workloads of --workloads (default clips,hour; --hour-seconds shortens the one-hour stream) in 1, 16
    and 64 pieces with MD5 against one-shot scan + decode with and without MD5; the SHA-256 of the PCM in stream order
    and the digests must be identical.  Median and min-max of --reps, sclk before and after each leg."""
    import hashlib

    import torch

    from _pcm import synth_fast
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import FlacSampleWriter, Options
    from flac_codec_amd.gpu import Decoder, DecoderSession, scan_stream_host

    res = {"tool": "tools/decode_many_probe.py --session --container", "build_id": _lib.build_id(), "reps": args.reps}

    def leg(times, before):
        return dict(_spread(times), sclk_mhz_before=before, sclk_mhz_after=_sclk_mhz())

    # ---- (a) per-feed latency
    n_streams, rate, packet, steps = 64, 16000, 1280, args.reps + 3
    files = []
    for k in range(16):
        pcm = synth_fast(1200 + k, 1, 16, packet * (steps + 1))
        w = FlacSampleWriter(None, Options.default().block_size(packet), rate, 16, 1, pcm.size)
        w.write(pcm)
        w.finalize()
        files.append(w.getvalue())
        w.close()
    cuts = []   # per distinct file: chunk k ends behind frame k (the first holds the metadata too)
    for b in files:
        off = [int(v) for v in scan_stream_host(b)[1]]
        cuts.append(([0] + off[1:steps + 1], off[1:steps + 2], off[0]))
    bound = max(e - s for c in cuts for s, e in zip([c[2]] + c[1][:-1], c[1]))
    res["latency"] = {"workload": "64 files, 16 kHz mono 16-bit, one frame of 80 ms (1280 samples) per file per feed",
                      "max_frame_bytes": bound, "legs": {}}
    for name in ("container_feed_decode_md5", "raw_feed_decode_frames"):
        container = name.startswith("container")
        ses = DecoderSession(n_streams, bound, device=0, container=container)
        out = torch.empty(n_streams * packet, dtype=torch.int32, device="cuda:0")
        recs = (_lib.DecodedStream * n_streams)()
        torch.cuda.synchronize()
        feed_t, decode_t, both_t, before, frames = [], [], [], None, 0
        for step in range(steps):
            if step == 3:
                before = _sclk_mhz()   # three feeds warm: buffers grown, code loaded
            chunks = []
            for i in range(n_streams):
                starts, ends, first = cuts[i % 16]
                a = starts[step] if container or step else first   # the raw session gets the frames alone
                chunks.append(files[i % 16][a:ends[step]])
            t0 = time.perf_counter()
            fr, _ = ses.feed(chunks)
            t1 = time.perf_counter()
            if container:
                ses.decoder.decode(out.data_ptr() if ses.total else None, ses.total, _lib.DECODE_OUT_DEVICE, recs)
                frames += ses.n_frames
            else:
                ses.decoder.decode_frames(out.data_ptr() if len(fr) else None, out.numel() if len(fr) else 0,
                                          _lib.DECODE_OUT_DEVICE, fr)
                frames += len(fr)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if step >= 3:
                feed_t.append(t1 - t0)
                decode_t.append(t2 - t1)
                both_t.append(t2 - t0)
        assert frames == n_streams * (steps - 1), frames   # without flush a frame comes out one feed late
        res["latency"]["legs"][name] = {"feed_plus_decode": leg(both_t, before), "feed": dict(_spread(feed_t)),
                                        "decode": dict(_spread(decode_t)), "frames": frames}
        ses.close()   # (the files' last frame was never fed: no verdict is asked for)

    # ---- (b) throughput
    res["throughput"] = {}
    for wname in args.workloads.split(","):
        if wname == "hour" and args.hour_seconds:
            WORKLOADS["hour"] = (1, 1, args.hour_seconds, 48000, 2, 24)
        blobs = make_blobs(wname)
        n = len(blobs)
        dec = Decoder(0)
        legs = {}
        one = {}
        for md5 in (False, True):
            flags = _lib.DECODE_OUT_DEVICE | (0 if md5 else _lib.DECODE_NO_MD5)
            recs, total = dec.scan(blobs)
            out = torch.empty(total, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            dec.decode(out.data_ptr(), total, flags, recs)   # warm
            before, times = _sclk_mhz(), []
            for _ in range(args.reps if not (md5 and wname == "hour") else min(args.reps, 3)):
                t0 = time.perf_counter()
                recs, total = dec.scan(blobs)
                dec.decode(out.data_ptr(), total, flags, recs)
                times.append(time.perf_counter() - t0)
            legs["one_shot_scan_decode" + ("_md5" if md5 else "_no_md5")] = leg(times, before)
            if md5:
                host = out.cpu().numpy()
                sha = hashlib.sha256()
                for r in recs[:n]:
                    sha.update(host[r.out_offset:r.out_offset + r.info.decoded_samples * r.info.channels].tobytes())
                one = {"pcm_sha256": sha.hexdigest(), "digests": [bytes(r.info.decoded_md5).hex() for r in recs[:n]],
                       "frames": [r.info.frames for r in recs[:n]]}
                assert all(r.rc == 0 and r.info.md5_status == 1 for r in recs[:n])
                del host
        dec.close()
        bound = max(int(np.diff(np.append(scan_stream_host(b)[1], len(b)).astype(np.int64)).max()) for b in set(blobs))
        for pieces in (1, 16, 64):
            cut = [[b[len(b) * p // pieces:len(b) * (p + 1) // pieces] for p in range(pieces)] for b in blobs]

            def run(check):
                ses = DecoderSession(n, bound, device=0, container=True)
                recs = (_lib.DecodedStream * n)()
                parts = [[] for _ in range(n)]
                for p in range(pieces + 1):
                    ses.finish() if p == pieces else ses.feed([c[p] for c in cut])
                    ses.decoder.decode(out.data_ptr() if ses.total else None, ses.total, _lib.DECODE_OUT_DEVICE, recs)
                    if check and ses.total:
                        host = out[:ses.total].cpu().numpy()
                        for i in range(n):
                            if recs[i].rc == 0:
                                a = recs[i].out_offset
                                parts[i].append(host[a:a + recs[i].info.decoded_samples * recs[i].info.channels].copy())
                verdict = ses.verdict()
                ses.close()
                return parts, verdict

            parts, verdict = run(True)   # warm, and the PCM and the digests against the one-shot's
            sha = hashlib.sha256()
            for per in parts:
                for a in per:
                    sha.update(a.tobytes())
            assert sha.hexdigest() == one["pcm_sha256"], "the session's PCM differs from the one-shot's"
            assert [bytes(v.info.decoded_md5).hex() for v in verdict] == one["digests"]
            assert all(v.rc == 0 and v.info.md5_status == 1 for v in verdict) and [v.info.frames for v in verdict] == one["frames"]
            del parts
            before, times = _sclk_mhz(), []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                run(False)
                times.append(time.perf_counter() - t0)
            legs[f"container_session_{pieces}_pieces_md5"] = dict(leg(times, before), identical_pcm_and_digests=True)
        n_s, _, secs, rate_w, ch, bps = WORKLOADS[wname]
        res["throughput"][wname] = {"workload": f"{n_s} x {secs} s, {rate_w} Hz, {ch} ch, {bps} bit", "streams": n,
                                    "bytes": sum(len(b) for b in blobs), "frames": sum(one["frames"]),
                                    "max_frame_bytes": bound, "pcm_sha256": one["pcm_sha256"], "legs": legs}
        del blobs, out
        with open(args.out, "w") as f:   # after every workload: a later one may run out of time
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


def timeline(args):
    """The --timeline leg (see the module docstring)."""
    import hashlib
    import random

    import torch

    from flac_codec_amd import _lib, gpu
    from flac_codec_amd.gpu import Decoder, decode_many, scan_frames_host, scan_stream_host

    blobs = make_blobs("clips")
    bare = [b[int(scan_stream_host(b)[1][0]):] for b in blobs]   # from the first frame on
    has_tl = hasattr(gpu, "decode_timeline") and not parent_only(args)
    dec = Decoder(0)
    legs = {"raw_scan_frames_decode_as": lambda: decode_many(bare, out="device", verify_md5=False, decoder=dec, raw=True,
                                                             dtype="float32", layout="padded")[0]}
    tl_legs = {}
    made = {}

    def damaged_batch():   # one frame in 50 removed, by a fixed seed; built behind the legs the parent has too
        if not made:
            rng, cache = random.Random(20261019), {}
            for b in bare:
                if b not in cache:
                    recs = scan_frames_host(b)[0]
                    lost = {k for k in range(len(recs)) if rng.randrange(50) == 0} or {len(recs) // 2}
                    cache[b] = (b"".join(b[int(r["byte_offset"]):int(r["byte_offset"]) + int(r["bytes"])]
                                         for k, r in enumerate(recs) if k not in lost), len(recs), len(lost))
            made["blobs"] = [cache[b][0] for b in bare]
            made["frames"] = sum(cache[b][1] for b in bare)
            made["lost"] = sum(cache[b][2] for b in bare)
        return made["blobs"]

    if has_tl:
        tl_legs["timeline_undamaged"] = lambda: gpu.decode_timeline(bare, decoder=dec)[:2]
        tl_legs["timeline_one_frame_in_50_lost"] = lambda: gpu.decode_timeline(damaged_batch(), decoder=dec)[:2]
    if args.kernels_only:
        for fn in list(legs.values()) + list(tl_legs.values()):
            fn()
            fn()
        torch.cuda.synchronize()
        dec.close()
        return
    res = {"tool": "tools/decode_many_probe.py --timeline", "workload": "clips: 1024 x 10 s, 16 kHz mono 16-bit, metadata "
           "stripped", "device_output": True, "dtype": "float32", "mask": True, "order": [], "runs": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    pcm = legs["raw_scan_frames_decode_as"]()
    rec = {"build_id": _lib.build_id(), "pcm_sha256": hashlib.sha256(pcm.cpu().numpy().tobytes()).hexdigest(), "legs": {}}
    for other in res["runs"].values():
        assert other["pcm_sha256"] == rec["pcm_sha256"]   # the same samples under every label

    def timed(legs):
        for name, fn in legs.items():
            fn()
            torch.cuda.synchronize()   # warm: buffers grown, code loaded
            sclk_before = _sclk_mhz()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            rec["legs"][name] = dict(_spread(times), sclk_mhz_before=sclk_before, sclk_mhz_after=_sclk_mhz())
            del out

    timed(legs)   # first, in a process that has done nothing the parent's has not
    if has_tl:
        batch, mask, results, _ = gpu.decode_timeline(bare, decoder=dec)
        assert torch.equal(batch, pcm) and all(r.rc == 0 and r.gaps == 0 for r in results)   # identical samples
        assert int(mask.sum()) == sum(r.timeline_samples for r in results)
        damaged = damaged_batch()
        batch, mask, results, frames = gpu.decode_timeline(damaged, decoder=dec)
        assert all(r.rc == 0 for r in results) and len(frames) == made["frames"] - made["lost"]
        rec["damaged"] = {"frames": made["frames"], "frames_removed": made["lost"],
                          "gaps": int(sum(r.gaps for r in results)), "gap_samples": int(sum(r.gap_samples for r in results)),
                          "timeline_samples": int(sum(r.timeline_samples for r in results)),
                          "mask_ones": int(mask.sum())}
        del batch, mask
        timed(tl_legs)
    del pcm
    dec.close()
    res["runs"][args.label] = rec
    res["order"].append(args.label)
    runs = res["runs"]
    if all(k in runs for k in ("this_1", "parent", "this_2")):
        allow = runs["parent"]["legs"]["raw_scan_frames_decode_as"]
        res["verdict"] = {"allowance_parent_min_s": allow["min_s"], "allowance_parent_max_s": allow["max_s"],
                          "parent_median_s": allow["median_s"]}
        for label in ("this_1", "this_2"):
            for name, leg in runs[label]["legs"].items():
                # a leg the parent ran is held to the parent's spread of that leg; else (r16) the undamaged timeline to
                # the decode_as leg's, and the damaged one, which has no parent, to nothing
                ref = runs["parent"]["legs"].get(name, allow if name == "timeline_undamaged" else None)
                if ref is None:
                    continue
                res["verdict"][f"{label}.{name}"] = {
                    "median_s": leg["median_s"], "inside_parent_spread": ref["min_s"] <= leg["median_s"] <= ref["max_s"],
                    "parent_min_s": ref["min_s"], "parent_max_s": ref["max_s"],
                    "over_parent_median": leg["median_s"] / ref["median_s"]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({args.label: rec, "verdict": res.get("verdict")}, indent=1), flush=True)


def device_input(args):
    """The --device-input leg (see the module docstring)."""
    import hashlib

    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    L = _lib.lib()
    has_door = hasattr(L, "flacgpu_decoder_scan_device") and args.label != "parent"
    blobs = make_blobs("clips") + make_blobs("tracks")
    n = len(blobs)
    data = b"".join(blobs)
    offs = np.cumsum([0] + [len(b) for b in blobs])
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    recs, total = (_lib.DecodedStream * n)(), C.c_uint64(0)
    shard = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    down = torch.empty(len(data), dtype=torch.uint8).pin_memory()   # (c): where the download lands
    host = np.frombuffer(data, dtype=np.uint8)
    hptrs = (C.c_void_p * n)(*[host.ctypes.data + int(o) for o in offs[:-1]])
    pptrs = (C.c_void_p * n)(*[down.data_ptr() + int(o) for o in offs[:-1]])
    dptrs = (C.c_void_p * n)(*[shard.data_ptr() + int(o) for o in offs[:-1]])
    copy = torch.empty_like(shard)
    dec = Decoder(0)

    def host_scan(ptrs=hptrs):
        assert L.flacgpu_decoder_scan(dec._h, ptrs, lens, n, recs, C.byref(total)) == 0

    def device_scan():
        assert L.flacgpu_decoder_scan_device(dec._h, dptrs, lens, n, None, recs, C.byref(total)) == 0

    def download_then_host_scan():
        down.copy_(shard)   # D2H into pinned memory, synchronous
        host_scan(pptrs)

    def plain_d2d():
        copy.copy_(shard)

    if args.kernels_only:   # for rocprofv3 --kernel-trace --stats: a warm call, then three traced ones per door
        for _ in range(4):
            device_scan()
            host_scan()
        dec.close()
        return
    legs = {"a_host_bytes_host_scan": host_scan}
    if has_door:
        legs.update({"b_device_bytes_device_scan": device_scan, "c_device_bytes_download_host_scan": download_then_host_scan,
                     "plain_d2d_copy_of_the_bytes": plain_d2d})
    res = {"tool": "tools/decode_many_probe.py --device-input", "workload": "clips (1024 x 10 s, 16 kHz mono 16-bit) + "
           "tracks (256 x 3 min, 44.1 kHz stereo 16-bit) in one batch, the scan alone, handle warm",
           "streams": n, "compressed_bytes": len(data), "order": [], "runs": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    host_scan()
    rec = {"build_id": _lib.build_id(), "records_sha256": hashlib.sha256(bytes(recs)).hexdigest(), "legs": {}}
    for other in res["runs"].values():
        assert other["records_sha256"] == rec["records_sha256"]   # the same scan under every label
    if has_door:
        device_scan()
        assert hashlib.sha256(bytes(recs)).hexdigest() == rec["records_sha256"]   # and through the device door
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()   # warm: buffers grown, code loaded
        sclk_before = _sclk_mhz()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        rec["legs"][name] = dict(_spread(times), sclk_mhz_before=sclk_before, sclk_mhz_after=_sclk_mhz())
    if has_door:
        d2d = rec["legs"]["plain_d2d_copy_of_the_bytes"]["median_s"]
        rec["plain_d2d_gbps"] = len(data) / d2d / 1e9
    dec.close()
    res["runs"][args.label] = rec
    res["order"].append(args.label)
    runs = res["runs"]
    if all(k in runs for k in ("this_1", "parent", "this_2")):   # the host door must cost what it cost
        allow = runs["parent"]["legs"]["a_host_bytes_host_scan"]
        res["host_door_guard"] = {"parent_median_s": allow["median_s"], "parent_min_s": allow["min_s"],
                                  "parent_max_s": allow["max_s"]}
        for label in ("this_1", "this_2"):
            leg = runs[label]["legs"]["a_host_bytes_host_scan"]
            res["host_door_guard"][label] = {"median_s": leg["median_s"],
                                             "inside_parent_spread": allow["min_s"] <= leg["median_s"] <= allow["max_s"],
                                             "over_parent_median": leg["median_s"] / allow["median_s"]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({args.label: rec, "host_door_guard": res.get("host_door_guard")}, indent=1), flush=True)


def windows(args):
    """The --windows leg (see the module docstring)."""
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder, decode_windows, window_array

    res = {"tool": "tools/decode_many_probe.py --windows", "device_output": True, "md5": False, "workloads": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    crop_s = {"tracks": 5, "clips": 1}

    def used():   # device memory in use, whoever allocated it
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    for name in args.workloads.split(","):
        n, _, secs, rate, ch, bps = WORKLOADS[name]
        blobs = make_blobs(name)
        T = crop_s[name] * rate
        free = torch.cuda.mem_get_info(0)[0]
        # (a) holds the padded float32 batch beside the scan (and its scratch, as large again)
        fit = min(n, int(free * 0.8 // (3 * 4 * ch * secs * rate + len(blobs[0]))))
        blobs = blobs[:fit]
        rng = np.random.default_rng(10)
        rounds = [[(i, int(rng.integers(0, secs * rate - T + 1)), T) for i in range(fit)]
                  for _ in range(args.reps + 1)]
        rec = {"streams": fit, "of": n, "prefix_because_full_output_does_not_fit": fit < n, "crop_samples": T,
               "channels": ch, "build_id": _lib.build_id(), "sclk_mhz_before": _sclk_mhz(), "legs": {}}

        def leg_a(dec, recs, wins):
            fmt = _lib.OutFormat(_lib.SAMPLE_F32, _lib.LAYOUT_PADDED, ch, 0, secs * rate)
            full = torch.empty((fit, ch, secs * rate), dtype=torch.float32, device="cuda:0")
            dec.decode_as(full.data_ptr(), full.numel() * 4, fmt, _lib.DECODE_OUT_DEVICE | _lib.DECODE_NO_MD5, recs)
            idx = torch.tensor([w[1] for w in wins], device="cuda:0")[:, None] + torch.arange(T, device="cuda:0")
            return torch.gather(full, 2, idx[:, None, :].expand(fit, ch, T))

        def leg_b(dec, recs, wins):
            return decode_windows(dec, recs, wins, dtype="float32", out="device")[0]

        outs = {}
        for leg, fn in (("a_decode_as_padded_then_slice", leg_a), ("b_decode_windows", leg_b)):
            base = used()
            dec = Decoder(0)
            recs, _ = dec.scan(blobs)
            resident = used()
            out = fn(dec, recs, rounds[0])   # warm: buffers grown, code loaded
            outs[leg] = out.clone()
            del out
            torch.cuda.empty_cache()
            if args.kernels_only:
                fn(dec, recs, rounds[1])
                torch.cuda.synchronize()
                dec.close()
                continue
            times, peak = [], 0
            for wins in rounds[1:]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(dec, recs, wins)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                peak = max(peak, used())
                del out
                torch.cuda.empty_cache()
            rec["legs"][leg] = dict(_spread(times), resident_scan_bytes=int(resident - base),
                                    peak_bytes_over_resident_scan=int(peak - resident))
            dec.close()
            del dec
        assert torch.equal(outs["a_decode_as_padded_then_slice"], outs["b_decode_windows"])   # the same crops
        rec["sclk_mhz_after"] = _sclk_mhz()
        res["workloads"][name] = rec
        print(json.dumps({name: rec}, indent=1), flush=True)
        del blobs, outs
    if not args.kernels_only:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def run(args):
    res = {"tool": "tools/decode_many_probe.py", "copy_rate_TBps": COPY_TBPS, "workloads": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for name in args.workloads.split(","):
        t0 = time.perf_counter()
        blobs = make_blobs(name)
        n, _, secs, rate, ch, bps = WORKLOADS[name]
        rec = {"streams": n, "seconds_each": secs, "rate": rate, "channels": ch, "bps": bps,
               "flac_bytes": int(sum(len(b) for b in blobs)), "encode_s": time.perf_counter() - t0}
        w_md5, scan_md5, total, bad = time_new(blobs, args.reps, True)
        w_nomd5, scan_nomd5, _, bad2 = time_new(blobs, args.reps, False)
        rec.update({"samples_interleaved": total, "new_md5_s": w_md5, "new_no_md5_s": w_nomd5,
                    "new_scan_s": scan_md5, "streams_not_clean": bad + bad2})
        rec["loop_decode_stream_s"] = time_loop(blobs)
        rec["loop_single_call_s"] = time_loop_single_call(blobs)
        ot, odone, osamp = time_oracle(blobs, args.oracle_seconds)
        rec["oracle_one_core"] = {"streams_decoded": odone, "seconds": ot, "samples": osamp,
                                  "scaled_to_workload_s": ot * total / max(osamp, 1)}
        rec["speedup_vs_loop_md5"] = rec["loop_decode_stream_s"] / w_md5
        res["workloads"][name] = rec
        print(json.dumps({name: rec}), flush=True)
        del blobs
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def merge_stats(args):
    """kernel_stats.csv of one rocprofv3 --kernel-trace --stats run (of --workloads, --reps 1) into the record"""
    import csv

    with open(args.out) as f:
        res = json.load(f)
    rows = {}
    with open(args.merge_stats) as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                               "avg_ms": float(r["AverageNs"]) / 1e6}
    mine = {k: v for k, v in rows.items() if any(s in k for s in ("k_scan_", "k_link", "k_decode_many", "k_frame_crc",
                                                                   "k_finish_many", "k_md5_many", "k_finish_as",
                                                                   "k_pad_rows", "k_finish_window", "k_spec_end",
                                                                   "k_fill_runs", "k_gather_slots", "k_meta_walk",
                                                                   "k_cand_heads", "k_analyze_many"))}   # (k_scan_ and k_link cover the raw kernels)
    res.setdefault("kernel_stats", {})[args.stats_label] = mine
    gather = [v for k, v in mine.items() if "k_gather_slots" in k]
    if gather and "compressed_bytes" in res:   # --device-input: the gather against the plain copy
        res["gather_effective_gbps"] = res["compressed_bytes"] / (gather[0]["avg_ms"] * 1e-3) / 1e9
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(mine, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="clips,tracks,hour")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, help="timed runs per leg (default 3; --device-input: 15)")
    ap.add_argument("--device-input", action="store_true",
                    help="the device-resident input leg: profiles/r15_device_input.json")
    ap.add_argument("--formats", action="store_true", help="the output-format leg: profiles/r09_decode_formats.json")
    ap.add_argument("--windows", action="store_true", help="the random-crop leg: profiles/r10_decode_windows.json")
    ap.add_argument("--s24", action="store_true", help="with --formats: the packed 24-bit leg, profiles/r12_s24.json")
    ap.add_argument("--raw", action="store_true", help="the raw frame stream leg: profiles/r13_raw_frames.json")
    ap.add_argument("--speculative", action="store_true",
                    help="with --raw: add the FLACGPU_SCAN_SPECULATIVE leg, profiles/r14_speculative.json")
    ap.add_argument("--timeline", action="store_true", help="the timeline leg: profiles/r16_timeline.json")
    ap.add_argument("--analyze", action="store_true", help="the frame analysis leg: profiles/r25_frame_analysis.json")
    ap.add_argument("--session", action="store_true", help="the decoder session leg: profiles/r22_decoder_session.json")
    ap.add_argument("--container", action="store_true",
                    help="with --session: the container session leg, profiles/r24_container_session.json")
    ap.add_argument("--hour-seconds", type=int, default=0,
                    help="--session --container: the length of the 'hour' stream in seconds (0: the whole hour)")
    ap.add_argument("--shrink", type=int, default=1, help="--s24: divide the clip count")
    ap.add_argument("--label", default="this", help="--formats: the run's name in the file (parent: the default int32 "
                    "leg only; any other name: every leg)")
    ap.add_argument("--parent-all-legs", action="store_true",
                    help="--raw, --timeline: with --label parent, time every leg of the mode (a parent that has them all); "
                    "the verdict then holds each leg to the parent's spread of the same leg")
    ap.add_argument("--package-root", help="--formats: measure the flac_codec_amd of this checkout, not of this one")
    ap.add_argument("--oracle-seconds", type=float, default=20.0)
    ap.add_argument("--merge-stats")
    ap.add_argument("--stats-label", default="run")
    ap.add_argument("--kernels-only", action="store_true", help="one warm decode per workload (for rocprofv3)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 15 if args.device_input or args.session or args.analyze else 3
    if not args.out:
        args.out = os.path.join(ROOT, "profiles", "r15_device_input.json" if args.device_input else
                                "r16_timeline.json" if args.timeline else
                                "r25_frame_analysis.json" if args.analyze else
                                "r24_container_session.json" if args.session and args.container else
                                "r22_decoder_session.json" if args.session else
                                "r14_speculative.json" if args.raw and args.speculative else
                                "r13_raw_frames.json" if args.raw else
                                "r10_decode_windows.json" if args.windows else
                                "r12_s24.json" if args.s24 else
                                "r09_decode_formats.json" if args.formats else "r07_decode_many.json")
    if args.windows and args.workloads == "clips,tracks,hour":
        args.workloads = "tracks,clips"
    if args.merge_stats:
        return merge_stats(args)
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    import torch

    torch.cuda.init()   # before the library's first HIP call (else torch sees no GPU)
    if args.device_input:
        return device_input(args)
    if args.timeline:
        return timeline(args)
    if args.analyze:
        return analyze(args)
    if args.session and args.container:
        if args.workloads == "clips,tracks,hour":
            args.workloads = "clips,hour"
        return container_session(args)
    if args.session:
        return session(args)
    if args.raw:
        return raw_frames(args)
    if args.formats and args.s24:
        return s24(args)
    if args.formats:
        return formats(args)
    if args.windows:
        return windows(args)
    if args.kernels_only:
        for name in args.workloads.split(","):   # (the hour's MD5 alone runs > 1 min: left to the timed run)
            blobs = make_blobs(name)
            time_new(blobs, 1, name != "hour")
        return
    run(args)


if __name__ == "__main__":
    main()
