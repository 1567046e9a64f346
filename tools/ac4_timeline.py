#!/usr/bin/env python3
"""Where a lag-group wave of k_autocorr4 spends a tile (a library built with -DAC4_TIMELINE=1):
    tools/build_variant.sh tl "-DAC4_TIMELINE=1"            (add -DAC4_FETCH_DEPTH=1 for the one-set schedule)
    FLACENC_AMD_LIBRARY=<the tl.so that script lists> python3 tools/ac4_timeline.py [--contexts 1|3] [--out x.json]
Stamps (100 MHz, low words) per wave and tile: 0 top, 1 the staged loads of tile t + 1 have arrived (the tile's first sixteen
LDS reads are awaited with them), 2 tile t + 1 converted and the next loads requested, 3 / 4 the two f64 blocks done,
5 past the barrier.  --contexts 1: the kernel alone (one context, its kernels back to back: nothing else on the chip
while k_autocorr4 runs); --contexts 3: the headline step, three contexts in rotation, other contexts' kernels beside it.
The records of a wave are those of the LAST launch that wrote them; every figure is a difference inside one record."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402

WAVES, TILES, WORDS = 512 * 4, 128, 8
PHASES = [("0-1 wait: staged loads (+ first LDS reads)", 0, 1), ("1-2 convert tile t+1, request ahead", 1, 2),
          ("2-3 f64 block 0", 2, 3), ("3-4 LDS reads + f64 block 1", 3, 4), ("4-5 barrier", 4, 5), ("0-5 tile", 0, 5)]


def summarise(rec, sel, res, label):
    """rec: [waves, tiles, 8] uint32; sel: boolean mask over tiles"""
    r = rec[:, sel, :]
    # a record is two 16-byte stores: with several contexts in flight two launches may each have written one half of it.
    # Such a record shows as a phase of (nearly) 2^32 ticks or of more than a millisecond, and is left out
    d = (r[:, :, 1:6] - r[:, :, 0:5]).astype(np.uint32)
    ok = (r[:, :, 7] == 1) & (d < 100000).all(axis=2)
    out = {"records": int(ok.sum()), "records_torn_between_launches": int(ok.size - ok.sum())}
    print(f"-- {label}: {out['records']} records")
    for name, a, b in PHASES:
        d = ((r[:, :, b] - r[:, :, a]).astype(np.uint32)[ok]).astype(np.float64) * 0.01   # us (wraps cancel in uint32)
        if d.size == 0:
            continue
        q = {"mean": float(d.mean()), "p50": float(np.median(d)), "p90": float(np.percentile(d, 90)),
             "p99": float(np.percentile(d, 99)), "max": float(d.max())}
        print(f"{name:44s} mean {q['mean']:6.3f}  p50 {q['p50']:6.3f}  p90 {q['p90']:6.3f}  p99 {q['p99']:6.3f}  max {q['max']:7.3f} us")
        out[name] = q
    res[label] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=1, choices=(1, 3))
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--frames", type=int, default=bench.FRAMES)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from flac_codec_amd import _lib

    L = _lib.lib()
    try:
        fn = L.flacgpu_ac4_timeline
    except AttributeError:
        sys.exit("this library has no timeline: build it with -DAC4_TIMELINE=1")
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    w = bench.Workload(torch, a.config, a.frames, 0, a.contexts, 0, 0)
    w.only_first = a.contexts == 1
    w.prewarm(200)
    assert fn(None, 0, 1) == WAVES * TILES * WORDS * 4
    for _ in range(a.steps):
        w.step()
    torch.cuda.synchronize()
    buf = np.zeros(WAVES * TILES * WORDS, dtype=np.uint32)
    assert fn(buf.ctypes.data, buf.nbytes, 0) == buf.nbytes
    rec = buf.reshape(WAVES, TILES, WORDS)
    assert (rec[:, :, 7] == 1).all() and (rec[:, :, 6] == np.arange(TILES)[None, :]).all(), "not every wave and tile left a record"
    res = {"contexts": a.contexts, "config": a.config, "frames": a.frames, "build_id": _lib.build_id(),
           "unit": "us; stamps are s_memrealtime, 10 ns"}
    t = np.arange(TILES)
    summarise(rec, t == 0, res, "the first tile (every wave's cold requests at once)")
    summarise(rec, t >= 1, res, "all tiles but the first")
    summarise(rec, (t >= 40) & (t < 88), res, "tiles 40..87 (flat window: one v_fma_f64 per term)")
    summarise(rec, ((t >= 4) & (t < 28)) | ((t >= 100) & (t < 124)), res, "tiles 4..27 and 100..123 (taper: multiply and add)")
    # the wave that is late at its wait: share of tiles whose wait exceeds 0.1 / 0.3 us, and the time a wave spends there in all
    wait = (rec[:, 1:, 1] - rec[:, 1:, 0]).astype(np.uint32).astype(np.float64) * 0.01
    span = (rec[:, -1, 5] - rec[:, 0, 0]).astype(np.uint32).astype(np.float64) * 0.01
    whole = span < 1000.0            # first and last record of the same launch
    wait, span = wait[whole], span[whole]
    res["waves_with_a_whole_span"] = int(whole.sum())
    res["wait_share_over_0.1us"] = float((wait > 0.1).mean())
    res["wait_share_over_0.3us"] = float((wait > 0.3).mean())
    res["wave_wait_sum_us"] = {"mean": float(wait.sum(axis=1).mean()), "max": float(wait.sum(axis=1).max())}
    res["wave_span_us"] = {"mean": float(span.mean()), "max": float(span.max())}
    print(f"waits over 0.1 us: {res['wait_share_over_0.1us']:.3f} of the tiles, over 0.3 us: {res['wait_share_over_0.3us']:.3f}; "
          f"per wave {res['wave_wait_sum_us']['mean']:.1f} us of waiting in a span of {res['wave_span_us']['mean']:.1f} us "
          f"(slowest wave {res['wave_span_us']['max']:.1f})")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
