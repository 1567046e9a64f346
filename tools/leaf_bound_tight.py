#!/usr/bin/env python3
"""How many candidates could skip the FIXED half's partition tree and exact count (Params::defer_fixed) under a TIGHTER lower
bound of the FIXED size -- measured on the CPU, before anything is built on the device.

For the first FRAMES of the bench's distinct frames (config 3; `--signal ar2` and `--signal hi`, bench.make_pcm) and each of a
frame's four candidates (left, right, mid, side), this prints the share for which `bound > exact LPC bits` holds, i.e. for
which the kernel's rule `lpc_bits < fixed_lb` would decide encode.rs:2929-2934 for LPC without the exact FIXED size -- for the
present bound (the leaf sums alone; to be held against the device's fixed_count_skipped), for the tight one with ONE exact
quotient sum per leaf, and for the form the kernel evaluates (exact at the rule's parameter and the one below it;
tests/_leaf_bound_tight.py).  A candidate only DEFERS where K4's size estimate of the LPC candidate plus the margin
(Params::defer_margin16, 3 bits per sample) stays under the bound: that estimate is restated here as well (window,
autocorrelation, Levinson-Durbin and encode.rs:3656-3702 through the oracle's stage functions, LpcParams::est8 rounded up as
kernels/lpc.inc rounds it), and the share that defers AND is decided is printed beside the bound's own share.  The exact sizes are the oracle's: each candidate is encoded as a mono frame
at its own width with max_lpc_order 0 (the FIXED size) and 12 (the LPC size wherever LPC is the cheaper one; where it is not,
no bound of the FIXED size can exceed it and the candidate counts as not decided).

    python tools/leaf_bound_tight.py [--frames 64] [--out profiles/leaf_bound_tight.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import _leaf_bound_tight as lbt  # noqa: E402
import _oracle as orc  # noqa: E402
import bench  # noqa: E402

CFG = 3
NAMES = ("left", "right", "mid", "side")


def candidates(frame, bps):
    left, right = frame[:, 0].astype(np.int64), frame[:, 1].astype(np.int64)
    return [(left, bps), (right, bps), ((left + right) >> 1, bps), (left - right, bps + 1)]


def mono_plan(opts, rate, bps, x):
    rc, _, plan = orc.encode_frame(opts, rate, bps, np.asarray(x, dtype=np.int32)[None, :])
    assert rc == 0, rc
    return plan.sub[0]


MARGIN16 = 48          # kDeferMargin16 (csrc/flacenc_gpu.hip)


def estimated_need(opts, x, bps, window):
    """est_bits + margin of kernels/wave_cand_fixed.inc for candidate x: what a bound must reach for the wave to defer"""
    n = len(x)
    w = lbt.wasted_bits(x)
    xs = (np.asarray(x, dtype=np.int64) >> w).astype(np.float64)
    ac = orc.autocorrelate(xs * window, opts.max_lpc_order)
    _, errs = orc.lp_coefficients(ac)
    bits = orc.subframe_bits_by_order(bps - w, orc.lib().orc_lpc_precision(n), n, errs)
    if len(bits) == 0:
        return None
    e = float(bits.min()) * 8.0 / n
    est8 = 255 if e >= 255.0 else int(e) + 1 if e >= 1.0 else 1
    return (est8 * n >> 3) + 17 + w + (MARGIN16 * n >> 4)


def measure(signal, frames):
    cfg = bench.CONFIGS[CFG]
    pcm = bench.make_pcm(1000 + 16 * CFG, bench.DISTINCT, cfg["ch"], cfg["bps"], signal, sections=bench.HI_SECTIONS[CFG])
    pcm = pcm.reshape(-1, bench.BLOCK, cfg["ch"])[:frames]
    with_lpc = bench.orc_options(orc, cfg)   # (context 0 of the bench: seed 1000 + 16 * config)
    fixed_only = with_lpc.copy(max_lpc_order=0)
    window = orc.window(with_lpc.window_kind, with_lpc.window_param, bench.BLOCK)
    rows = []
    for f in range(frames):
        for name, (x, bps) in zip(NAMES, candidates(pcm[f], cfg["bps"])):
            order, present, one = lbt.fixed_bounds(x, bps)
            tight = lbt.fixed_bounds(x, bps, below="kernel")[2]
            need = estimated_need(with_lpc, x, bps, window)
            fx = mono_plan(fixed_only, cfg["rate"], bps, x)
            best = mono_plan(with_lpc, cfg["rate"], bps, x)
            row = dict(frame=f, cand=name, fixed_order=order, present=present, tight=tight, fixed_type=int(fx.type),
                       fixed_bits=int(fx.bits), best_type=int(best.type), best_bits=int(best.bits), lpc_order=int(best.order))
            if fx.type == orc.SUB_FIXED:
                assert fx.order == order, (f, name, fx.order, order)
                assert present <= fx.bits and tight <= fx.bits, row      # both ARE lower bounds
            row["lpc_wins"] = bool(best.type == orc.SUB_LPC)
            row["present_decides"] = bool(row["lpc_wins"] and best.bits < present)
            row["one_decides"] = bool(row["lpc_wins"] and best.bits < one)
            row["tight_decides"] = bool(row["lpc_wins"] and best.bits < tight)
            row["present_defers"] = bool(need is not None and need <= present and row["present_decides"])
            row["tight_defers"] = bool(need is not None and need <= tight and row["tight_decides"])
            rows.append(row)
    n = len(rows)
    fixed = [r for r in rows if r["fixed_type"] == orc.SUB_FIXED]
    won = [r for r in fixed if r["lpc_wins"]]

    def per_sample(v):
        return round(statistics.median(v) / bench.BLOCK, 4) if v else None

    return dict(
        signal=signal, config=CFG, frames=frames, candidates=n,
        lpc_wins_share=round(sum(r["lpc_wins"] for r in rows) / n, 4),
        present_bound_share=round(sum(r["present_decides"] for r in rows) / n, 4),
        one_parameter_bound_share=round(sum(r["one_decides"] for r in rows) / n, 4),
        tight_bound_share=round(sum(r["tight_decides"] for r in rows) / n, 4),
        # ... of those, the candidates the LPC estimate + margin lets defer in the first place (mode 1, the default)
        present_bound_share_by_estimate=round(sum(r["present_defers"] for r in rows) / n, 4),
        tight_bound_share_by_estimate=round(sum(r["tight_defers"] for r in rows) / n, 4),
        share_by_candidate={c: round(sum(r["tight_decides"] for r in rows if r["cand"] == c) / frames, 4) for c in NAMES},
        fixed_orders=sorted({r["fixed_order"] for r in rows}),
        lpc_orders=sorted({r["lpc_order"] for r in won}),
        # medians in bits per sample: what LPC gains over FIXED, and what each bound gives away
        median_fixed_minus_lpc=per_sample([r["fixed_bits"] - r["best_bits"] for r in won]),
        median_slack_present=per_sample([r["fixed_bits"] - r["present"] for r in fixed]),
        median_slack_tight=per_sample([r["fixed_bits"] - r["tight"] for r in fixed]),
        max_slack_tight_bits=max((r["fixed_bits"] - r["tight"] for r in fixed), default=None),
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leaf_bound_tight.json"))
    args = ap.parse_args()
    out = dict(
        what="share of candidates a lower bound of the FIXED size decides for LPC (bound > exact LPC bits), CPU, oracle sizes",
        tool="tools/leaf_bound_tight.py", bound="tests/_leaf_bound_tight.py",
        cpu_shares=[measure(s, args.frames) for s in ("ar2", "hi")])
    for m in out["cpu_shares"]:
        print(json.dumps(m))
    if os.path.exists(args.out):      # keep what other steps have recorded beside the shares
        try:
            old = json.load(open(args.out))
            out = {**old, **out}
        except ValueError:
            pass
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
