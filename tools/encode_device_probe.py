#!/usr/bin/env python3
"""What BatchEncoder.encode_device saves a caller who holds a float32 [B, C, T] batch on the GPU.

Workloads (the r07 shapes): 1024 clips of 10 s, 16 kHz mono 16-bit; 256 tracks of 3 min, 44.1 kHz stereo 16-bit.
  leg (a)  what such a caller did before: tensor.cpu(), numpy quantise + interleave, BatchEncoder(coalesce=True).encode
  leg (b)  encode_device, with and without the MD5
Handle warm, median and min-max of --repeats (15) runs, sclk read before and after; both legs must give identical
files.  Writes profiles/r11_encode_device.json.  --kernels: one encode_device call per workload and nothing else, for a
`rocprofv3 --kernel-trace --stats -- python tools/encode_device_probe.py --kernels` run of its own (the per-kernel split:
k_ingest, k_md5_many and the one-frame tail calls).

--int24: the packed 24-bit leg instead, on 1024 clips of 10 s, 48 kHz stereo 24-bit held as [B, C, T, 3] uint8 (divided
by --shrink): (a) the caller widens the bytes to int32 in torch and calls encode_device on that, (b)
encode_device(dtype="int24"); identical files asserted.  Merged into profiles/r12_s24.json under "encoder".

--out-device: what encode_device(out="device") saves a caller who wants the FILES on the GPU, on the two workloads above:
(a) encode_device to host buffers followed by the upload of the files into one device tensor -- what such a caller does
without it -- and (b) encode_device(out="device"); identical bytes asserted, handle warm, median and min-max of --repeats,
sclk before and after each leg.  Every workload's record also holds "host_output", encode_device to host buffers alone: the
figure to compare between builds.  Writes profiles/r18_device_out.json.  With --kernels: one encode_device(out="device")
call per workload and nothing else (k_place_runs' share, under rocprofv3 as above).
--session: what a DeviceSession (flacenc_device_session_*) costs beside the one-shot call, on the two workloads above:
(a) encode_device on the whole tensor, with and without the MD5 -- the yardstick, and the figure to compare between builds
-- and (b) a session fed the same tensor in 1 s chunks (views of it made contiguous outside the timed region), with and
without the MD5; identical files asserted, handle warm, median and min-max of --repeats, sclk before and after each leg.
Writes profiles/r19_session.json.  --one-shot-only (with --session): leg (a) alone, merged into the record under
"one_shot_of" / --label; with --root DIR the package of another checkout (the parent commit) is measured by the same code.
With --kernels: per workload one one-shot call and one session, then ONE stream of 3 min stereo through both, and nothing
else -- k_md5_chain beside k_md5_many on the same staged samples, under rocprofv3 as above.
--host-only (with --out-device): the "host_output" leg alone, merged into the record under "host_output_of" / --label; with
--root DIR the package of another checkout built beside this one (the parent commit) is measured by the same code.
--session --unknown-total: the session legs (--session-only is implied) and beside them the same session opened WITHOUT the
streams' totals (flacenc_device_session_open_ex), with and without the MD5; the two sessions' files must hold the same
bytes from the first frame on.  Writes profiles/r21_unknown_length.json under "session".
--stream-writer: a DeviceStreamWriter (flacenc_device_stream_writer_*) on 64 streams of 16-bit mono at 24 kHz, 1920 samples
(80 ms) a write, 50 writes: median and min-max of ONE write over the 50 (the first, which creates the contexts, apart),
sclk before and after; the frames of the first run go back through gpu.decode_frames and are compared.  Merged into
profiles/r21_unknown_length.json under "stream_writer"."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = {
    "clips_1024x10s_16k_mono": dict(n=1024, samples=160000, channels=1, rate=16000),
    "tracks_256x3min_44k1_stereo": dict(n=256, samples=3 * 60 * 44100, channels=2, rate=44100),
}


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        return {k: v.get("sclk clock speed:") for k, v in json.loads(out).items() if isinstance(v, dict)}
    except Exception as e:   # the figure is context, not a result
        return {"error": str(e)}


def make_batch(w, shrink):
    import torch
    from _pcm import synth_fast

    n, T, ch = max(1, w["n"] // shrink), w["samples"], w["channels"]
    base = synth_fast(11, ch, 16, T + 4096).reshape(-1, ch).T.astype(np.float32) / 32768.0   # [ch, T + 4096]
    host = np.stack([base[:, (37 * i) % 4096:(37 * i) % 4096 + T] for i in range(n)])
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


def leg_a(enc, t):
    x = t.cpu().numpy()
    q = np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int32)
    streams = [np.ascontiguousarray(q[i].T).reshape(-1) for i in range(q.shape[0])]
    return enc.encode(streams, enc_rate, 16, x.shape[1])


def int24_leg(a):
    import torch
    from _pcm import synth_fast
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import BatchEncoder, Options

    n, T, ch, rate = max(1, 1024 // a.shrink), 480000, 2, 48000
    base = synth_fast(12, ch, 24, T + 4096).reshape(-1, ch).T   # [ch, T + 4096] int32 of 24 bits
    host = np.stack([base[:, (37 * i) % 4096:(37 * i) % 4096 + T] for i in range(n)])
    packed = np.ascontiguousarray(np.ascontiguousarray(host, dtype="<i4").view(np.uint8).reshape(n, ch, T, 4)[..., :3])
    t = torch.from_numpy(packed).cuda()
    del host, packed
    enc = BatchEncoder(Options.default())

    def widen_then_encode(copy=False):
        x = t.to(torch.int32)
        x = (x[..., 0] | x[..., 1] << 8 | x[..., 2] << 16) << 8 >> 8   # sign-extended
        return enc.encode_device(x.contiguous(), None, sample_rate=rate, bits_per_sample=24, copy=copy)

    def direct(copy=False):
        return enc.encode_device(t, None, sample_rate=rate, bits_per_sample=24, copy=copy, dtype="int24")

    if a.kernels:
        direct()
        return
    assert widen_then_encode(True) == direct(True), "the two legs differ"
    r = {"tool": "tools/encode_device_probe.py --int24", "build_id": _lib.build_id(),
         "workload": f"{n} clips x 10 s, 48 kHz stereo 24-bit", "samples": n * ch * T, "tensor_bytes_int24": t.numel(),
         "tensor_bytes_int32": 4 * n * ch * T}
    for k, fn in (("a_torch_widen_then_encode_device_int32", widen_then_encode), ("b_encode_device_int24", direct)):
        before = sclk()   # around every leg: a clock change between the legs shows
        r[k] = dict(timed(fn, a.repeats), sclk_before=before, sclk_after=sclk())
    for k in ("a_torch_widen_then_encode_device_int32", "b_encode_device_int24"):
        r[k]["gsamples_per_s"] = r["samples"] / r[k]["median_ms"] / 1e6
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["encoder"] = r
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(r, indent=1))


def out_device_leg(a):
    import torch
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import BatchEncoder, Options

    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if not a.host_only:
        res = {"tool": "tools/encode_device_probe.py --out-device", "build_id": _lib.build_id(), "shrink": a.shrink,
               "workloads": {}, "host_output_of": res.get("host_output_of", {})}
    for name, w in WORKLOADS.items():
        if a.only and name != a.only:
            continue
        t = make_batch(w, a.shrink)
        enc = BatchEncoder(Options.default())
        kw = dict(sample_rate=w["rate"], bits_per_sample=16)

        def host_output():
            return enc.encode_device(t, None, copy=False, **kw)

        def host_then_upload():
            return torch.from_numpy(np.concatenate(host_output())).cuda()

        def device_output():
            return enc.encode_device(t, None, out="device", **kw)

        if a.kernels:
            device_output()
            continue
        legs = [("host_output", host_output)]
        if not a.host_only:
            assert torch.equal(host_then_upload(), torch.cat(device_output())), f"{name}: the two legs differ"
            legs += [("a_encode_device_then_upload", host_then_upload), ("b_encode_device_out_device", device_output)]
        r = {"streams": t.shape[0], "samples": t.numel(), "file_bytes": int(sum(v.size for v in host_output()))}
        for k, fn in legs:
            before = sclk()   # around every leg: a clock change between the legs shows
            r[k] = dict(timed(fn, a.repeats), sclk_before=before, sclk_after=sclk())
            r[k]["gsamples_per_s"] = r["samples"] / r[k]["median_ms"] / 1e6
        if a.host_only:
            res.setdefault("host_output_of", {}).setdefault(a.label, {"build_id": _lib.build_id()})[name] = r["host_output"]
        else:
            res["workloads"][name] = r
        print(name, json.dumps(r))
        del t
        torch.cuda.empty_cache()
    if a.kernels:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


def session_leg(a):
    import torch
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import BatchEncoder, Options

    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if not a.one_shot_only:
        res = {"tool": "tools/encode_device_probe.py --session", "build_id": _lib.build_id(), "shrink": a.shrink,
               "workloads": {}, "one_shot_of": res.get("one_shot_of", {})}
    shapes = dict(WORKLOADS)
    if a.kernels:
        shapes["one_track_3min_44k1_stereo"] = dict(n=1, samples=3 * 60 * 44100, channels=2, rate=44100)
    for name, w in shapes.items():
        if a.only and name != a.only:
            continue
        t = make_batch(w, 1 if w["n"] == 1 else a.shrink)
        enc = BatchEncoder(Options.default())
        n, ch, T, rate = t.shape[0], t.shape[1], t.shape[2], w["rate"]

        def one_shot(md5=True):
            return enc.encode_device(t, None, sample_rate=rate, bits_per_sample=16, verify_md5=md5, copy=False)

        def session(md5=True, known=True):
            with enc.open_device_session([T if known else None] * n, rate, 16, ch, max_chunk=rate, verify_md5=md5) as ses:
                for piece in chunks:
                    ses.write(piece)
                return ses.finalize()

        if a.kernels:
            chunks = [t[:, :, at:at + rate].contiguous() for at in range(0, T, rate)]
            one_shot()
            session()
            del t, chunks
            torch.cuda.empty_cache()
            continue
        legs = [] if a.session_only else [("a_one_shot", one_shot), ("a_one_shot_no_md5", lambda: one_shot(False))]
        if not a.one_shot_only:
            chunks = [t[:, :, at:at + rate].contiguous() for at in range(0, T, rate)]   # (a second copy of the batch)
            if not a.session_only:
                assert [bytes(v) for v in one_shot()] == session(), f"{name}: the two legs differ"
                assert [bytes(v) for v in one_shot(False)] == session(False), f"{name}: the two legs differ without MD5"
            legs += [("b_session_1s_chunks", session), ("b_session_1s_chunks_no_md5", lambda: session(False))]
            if a.unknown_total:
                for md5 in (True, False):   # another header, the same bytes from the first frame on
                    for f, g in zip(session(md5), session(md5, False)):
                        assert f[first_frame(f):] == g[first_frame(g):] and len(f) > len(g), f"{name}: the frames differ"
                legs += [("c_session_unknown_total", lambda: session(True, False)),
                         ("c_session_unknown_total_no_md5", lambda: session(False, False))]
        # (FLACGPU_NO_RAGGED=1 in the environment: the short last blocks one one-frame call each, as before r20 -- the A/B leg)
        r = {"streams": n, "samples": t.numel(), "writes": (T + rate - 1) // rate, "samples_per_stream": T,
             "no_ragged": bool(os.environ.get("FLACGPU_NO_RAGGED"))}
        for k, fn in legs:
            before = sclk()   # around every leg: a clock change between the legs shows
            r[k] = dict(timed(fn, a.repeats), sclk_before=before, sclk_after=sclk())
            r[k]["gsamples_per_s"] = r["samples"] / r[k]["median_ms"] / 1e6
        if a.one_shot_only:
            res.setdefault("one_shot_of", {}).setdefault(a.label, {"build_id": _lib.build_id()})[name] = {
                k: r[k] for k in ("a_one_shot", "a_one_shot_no_md5")}
        else:
            res["workloads"][name] = r
        print(name, json.dumps(r))
        del t
        chunks = None
        torch.cuda.empty_cache()
    if a.kernels:
        return
    if a.unknown_total:   # one record for both of r21's legs
        whole = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                whole = json.load(f)
        res["tool"] += " --unknown-total"
        res.pop("one_shot_of", None)
        whole["session"] = res
        res = whole
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


def stream_writer_leg(a):
    import torch
    from flac_codec_amd import _lib, gpu
    from flac_codec_amd.encode import BatchEncoder, Options

    n, rate, packet, writes = max(1, 64 // a.shrink), 24000, 1920, 50
    t = make_batch(dict(n=n, samples=packet * writes, channels=1, rate=rate), 1)
    chunks = [t[:, :, at:at + packet].contiguous() for at in range(0, packet * writes, packet)]
    enc = BatchEncoder(Options.default())
    runs = []   # [run][write] ms
    before = sclk()
    for run in range(a.repeats + 1):
        frames, ts = [[] for _ in range(n)], []
        with enc.open_device_stream_writer(n, rate, 16, 1, max_block=packet) as w:
            for piece in chunks:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = w.write(piece, [packet] * n)
                ts.append((time.perf_counter() - t0) * 1e3)
                for k in range(n):
                    frames[k].append(out[k])
            assert w.frame_numbers == [writes] * n
        if run == 0:   # (warm: contexts, pinned buffers, staging) the frames decode back to what went in
            flat, records, raw = gpu.decode_frames([b"".join(f) for f in frames], out="host")
            assert all(r.frames == writes and r.skipped_bytes == 0 for r in raw) and not records["status"].any()
            want = torch.clamp(torch.round(t.double() * 32768.0), -32768, 32767).to(torch.int32)[:, 0, :].cpu().numpy()
            assert np.array_equal(flat.reshape(n, packet * writes), want), "the decoded frames differ from the tensor"
            file_bytes = sum(len(f) for per in frames for f in per)
            continue
        runs.append(ts)
    after = sclk()
    if a.kernels:
        return
    every = [v for ts in runs for v in ts[1:]]   # (a run's first write takes the contexts from the pool)
    r = {"tool": "tools/encode_device_probe.py --stream-writer", "build_id": _lib.build_id(),
         "workload": f"{n} streams, 16-bit mono {rate} Hz, {packet} samples a write, {writes} writes", "streams": n,
         "samples_per_write": n * packet, "frame_bytes_per_run": file_bytes, "runs": len(runs),
         "no_ragged": bool(os.environ.get("FLACGPU_NO_RAGGED")),
         "per_write_ms": {"median": statistics.median(every), "min": min(every), "max": max(every), "writes": len(every)},
         "first_write_of_a_run_ms": {"median": statistics.median(ts[0] for ts in runs), "min": min(ts[0] for ts in runs),
                                     "max": max(ts[0] for ts in runs)},
         "per_run_ms": {"median": statistics.median(sum(ts) for ts in runs), "min": min(sum(ts) for ts in runs),
                        "max": max(sum(ts) for ts in runs)},
         "sclk_before": before, "sclk_after": after}
    r["realtime_factor"] = packet / rate * 1e3 / r["per_write_ms"]["median"]   # 80 ms of audio per stream and write
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["stream_writer_no_ragged" if r["no_ragged"] else "stream_writer"] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(r, indent=1))


def first_frame(data):
    """where a .flac file's first frame starts: behind the last metadata block"""
    pos = 4
    while True:
        last, size = data[pos] & 0x80, int.from_bytes(data[pos + 1:pos + 4], "big")
        pos += 4 + size
        if last:
            return pos


def timed(fn, repeats):
    import torch

    fn()   # warm: contexts, pinned buffers, staging
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": repeats}


def main():
    global enc_rate
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="divide the stream counts (a quick look)")
    ap.add_argument("--only", default=None, help="one workload's name")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--int24", action="store_true", help="the packed 24-bit leg: profiles/r12_s24.json")
    ap.add_argument("--out-device", action="store_true", help="files left on the GPU: profiles/r18_device_out.json")
    ap.add_argument("--host-only", action="store_true", help="with --out-device: the host-output leg alone")
    ap.add_argument("--session", action="store_true", help="a session fed 1 s chunks: profiles/r19_session.json")
    ap.add_argument("--one-shot-only", action="store_true", help="with --session: the one-shot legs alone")
    ap.add_argument("--session-only", action="store_true",
                    help="with --session: the session legs alone (no one-shot legs, no comparison of the files): repeated A/B runs")
    ap.add_argument("--unknown-total", action="store_true",
                    help="with --session: the same session without declared totals beside it: profiles/r21_unknown_length.json")
    ap.add_argument("--stream-writer", action="store_true", help="a DeviceStreamWriter's write: profiles/r21_unknown_length.json")
    ap.add_argument("--label", default="this_build", help="with --host-only / --one-shot-only: the record's name")
    ap.add_argument("--no-tail", action="store_true",
                    help="cut every stream to whole 4096-sample blocks (clips: 159 744 samples): the call without its tail phase")
    ap.add_argument("--root", default=None, help="measure the package of another checkout")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.unknown_total:
        a.session_only = True
    a.out = a.out or os.path.join(ROOT, "profiles", "r21_unknown_length.json" if a.unknown_total or a.stream_writer else
                                  "r12_s24.json" if a.int24 else
                                  "r18_device_out.json" if a.out_device else
                                  "r19_session.json" if a.session else "r11_encode_device.json")
    if a.no_tail:
        for w in WORKLOADS.values():
            w["samples"] -= w["samples"] % 4096
    if a.root:   # (the package is imported below, never before this line)
        sys.path.insert(0, os.path.abspath(a.root))
    import torch

    torch.cuda.init()
    if a.int24:
        return int24_leg(a)
    if a.out_device:
        return out_device_leg(a)
    if a.stream_writer:
        return stream_writer_leg(a)
    if a.session:
        return session_leg(a)
    from flac_codec_amd import _lib
    from flac_codec_amd.encode import BatchEncoder, Options

    result = {"build_id": _lib.lib().flacgpu_build_id().decode() if hasattr(_lib.lib(), "flacgpu_build_id") else None,
              "sclk_before": sclk(), "workloads": {}}
    result["shrink"] = a.shrink
    for name, w in WORKLOADS.items():
        if a.only and name != a.only:
            continue
        t = make_batch(w, a.shrink)
        enc_rate = w["rate"]
        dev = BatchEncoder(Options.default())
        if a.kernels:
            dev.encode_device(t, None, sample_rate=w["rate"], bits_per_sample=16)
            continue
        host = BatchEncoder(Options.default(), coalesce=True)
        files_a = leg_a(host, t)
        files_b = dev.encode_device(t, None, sample_rate=w["rate"], bits_per_sample=16)
        assert files_a == files_b, f"{name}: the two legs differ"
        samples = t.numel()
        r = {"streams": t.shape[0], "samples": samples,
             "a_cpu_numpy_coalesced": timed(lambda: leg_a(host, t), a.repeats),
             "b_encode_device": timed(lambda: dev.encode_device(t, None, sample_rate=w["rate"], bits_per_sample=16, copy=False), a.repeats),
             "b_encode_device_no_md5": timed(lambda: dev.encode_device(t, None, sample_rate=w["rate"], bits_per_sample=16, verify_md5=False, copy=False), a.repeats)}
        for k in ("a_cpu_numpy_coalesced", "b_encode_device", "b_encode_device_no_md5"):
            r[k]["gsamples_per_s"] = samples / r[k]["median_ms"] / 1e6
        result["workloads"][name] = r
        print(name, json.dumps(r))
        del t
        torch.cuda.empty_cache()
    if a.kernels:
        return
    result["sclk_after"] = sclk()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
