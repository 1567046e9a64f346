"""The decision matrix (_decision_matrix.py) against the oracle ALONE: every case must sit on the boundary it declares.
The oracle's FramePlan shows the declared field on each side of a threshold; for ties, the integer restatement below
(the abs-sums over the common tail, Partition::new's estimate, the exact bit count) shows that the tied quantities are
equal, that nothing else is smaller, and which one the oracle took -- and the restatement itself is checked against the
oracle's plan on every case.  No case is skipped or filtered: a case that misses its boundary fails here, so the GPU
test (test_gpu_decisions.py) cannot pass on inputs that miss it."""
import numpy as np
import pytest

import _decision_matrix as dm
import _oracle as orc


# ---------------------------------------------------------------- the restatement (integers only)
fixed_sums, partition_new = dm.fixed_sums, dm.partition_new   # the matrix's searches use the same two


def level_estimates(res, n, order, max_po, rice_max):
    """best_partitions: per partition order the (estimate, [partition]) or None where a partition fails."""
    a = np.concatenate([[0], np.cumsum(np.abs(res))])
    out = []
    for po in range(min((n & -n).bit_length() - 1, max_po) + 1):
        plen = n >> po
        edges = [0] + [plen * (i + 1) - order for i in range(1 << po)]
        parts = [partition_new(int(a[hi] - a[lo]), hi - lo, rice_max) for lo, hi in zip(edges, edges[1:])]
        out.append(None if any(p is None for p in parts) or plen <= order else (sum(p[0] for p in parts), parts))
    return out


def restate(x, bps, max_po):
    """What the reference does with one channel without LPC: a dict of the SubframePlan's fields and of the quantities
    behind them."""
    x = np.asarray(x, dtype=np.int64)
    n = x.size
    if not x.any():
        return dict(type=orc.SUB_CONSTANT, wasted=0, bps=bps, bits=8 + bps)
    wasted = min(int(v & -v).bit_length() - 1 for v in x if v)
    x, eb, rice2 = x >> wasted, bps - wasted, bps > 16
    seqs, sums = fixed_sums(x)
    order = sums.index(min(sums))
    res = seqs[order]
    levels = level_estimates(res, n, order, max_po, 31 if rice2 else 15)
    ests = [None if lv is None else lv[0] for lv in levels]
    out = dict(wasted=wasted, bps=eb, ladder=len(seqs), sums=sums, ests=ests)
    verbatim = dict(out, type=orc.SUB_VERBATIM, bits=8 + wasted + n * eb)
    live = [e for e in ests if e is not None]
    if live:
        po = ests.index(min(live))
        parts = [(k, e) for _, k, e in levels[po][1]]
    elif int(res.min()) < -(1 << 30) or int(res.max()) > (1 << 30) - 1:
        return dict(verbatim, fixed_bits=None)       # the 31-bit fallback cannot hold the residuals: FIXED fails
    else:
        po, parts = 0, [(255, 31)]
    method = int(rice2 and any(15 <= k < 255 for k, _ in parts))
    bits = 8 + wasted + order * eb + 6
    at = 0
    for i, (k, e) in enumerate(parts):
        cnt = (n >> po) - (order if i == 0 else 0)
        r = res[at:at + cnt]
        at += cnt
        bits += 5 if method else 4
        if k < 255:
            u = np.where(r < 0, -2 * r - 1, 2 * r)
            bits += int((u >> k).sum()) + cnt * (1 + k)
        else:
            bits += 5 + e * cnt
    if bits >= n * eb:
        return dict(verbatim, fixed_bits=bits)
    return dict(out, type=orc.SUB_FIXED, order=order, partition_order=po, coding_method=method, bits=bits, fixed_bits=bits,
                rice=[k for k, _ in parts], escape_bits=[e for _, e in parts])


def plan_fields(sp):
    out = dict(type=sp.type, wasted=sp.wasted, bps=sp.bps, bits=sp.bits)
    if sp.type == orc.SUB_FIXED:
        npart = sp.n_partitions
        out.update(order=sp.order, partition_order=sp.partition_order, coding_method=sp.coding_method,
                   rice=list(sp.rice[:npart]), escape_bits=list(sp.escape_bits[:npart]))
    return out


def oracle_mono(x, bps, n, max_po):
    o = orc.options("default", block_size=n, max_partition_order=max_po, max_lpc_order=0, mid_side=0, exhaustive=0)
    rc, data, plan = orc.encode_frame(o, 44100, bps, np.asarray(x, dtype=np.int32).reshape(1, -1))
    assert rc == 0
    return data, plan


def check_mono(case):
    n = case.planar.shape[1]
    _, plan = oracle_mono(case.planar[0], case.bps, n, case.max_po)
    got = plan_fields(plan.sub[0])
    mine = restate(case.planar[0], case.bps, case.max_po)
    for f, v in got.items():          # the restatement is the oracle's, field by field
        assert mine[f] == v, f"{case}: restated {f} {mine[f]} != oracle {v}"
    for f, v in case.expect.items():  # the declared side of the threshold
        if f in ("ladder", "fixed_bits", "sum", "levels_alive", "rice_first"):
            continue
        assert f in got and got[f] == v, f"{case}: oracle {f} {got.get(f)}, declared {v}"
    if "rice_first" in case.expect:   # partition 0 of an order-k predictor: plen - k residuals
        assert got["rice"][0] == case.expect["rice_first"], f"{case}: {got}"
    if "ladder" in case.expect:
        assert mine["ladder"] == case.expect["ladder"], f"{case}: ladder {mine['ladder']}"
        if got["type"] == orc.SUB_FIXED:
            assert got["order"] < mine["ladder"]
    if "fixed_bits" in case.expect:   # bits >= n * bps gives VERBATIM: one below, at, one above
        assert mine["fixed_bits"] == case.expect["fixed_bits"], f"{case}: FIXED bits {mine['fixed_bits']}"
        assert (got["type"] == orc.SUB_VERBATIM) == (mine["fixed_bits"] >= n * mine["bps"]), str(case)
    if "levels_alive" in case.expect:  # every partition order dropped (the fallback, which cannot hold these residuals) or not
        assert any(e is not None for e in mine["ests"]) == case.expect["levels_alive"], f"{case}: {mine['ests']}"
        assert (mine["fixed_bits"] is not None) == case.expect["levels_alive"]
    if "sum" in case.expect:
        assert int(np.abs(case.planar[0].astype(np.int64)).sum()) == case.expect["sum"] and mine["sums"].index(min(mine["sums"])) == 0
    if case.tie:
        vals = mine["sums"] if case.tie["kind"] == "fixed" else mine["ests"]
        tied = [vals[i] for i in case.tie["among"]]
        assert len(set(tied)) == 1 and tied[0] is not None, f"{case}: not a tie: {vals}"
        rest = [v for i, v in enumerate(vals) if i not in case.tie["among"] and v is not None]
        assert all(v > tied[0] for v in rest), f"{case}: the tie is not the minimum: {vals}"
        assert case.tie["taken"] == min(case.tie["among"])
        assert got["order" if case.tie["kind"] == "fixed" else "partition_order"] == case.tie["taken"], f"{case}: {got}"


@pytest.mark.parametrize("n,max_po", dm.MONO_SHAPES)
def test_every_mono_case_sits_on_its_boundary(n, max_po):
    cases = dm.mono_cases(n, max_po)
    assert len(cases) >= 190
    for case in cases:
        check_mono(case)


def test_threshold_neighbours_differ_in_one_sample_by_one():
    """The cases below / at / above a threshold (Case.near) differ by 1 in one sample -- for a predictor of order k, in
    one residual, which is one sample of the k-th difference -- and by one unit of the wasted bits where there are some."""
    seen, groups = 0, {}
    for c in dm.mono_cases(64, 3) + dm.mono_cases(1152, 6) + dm.mono_cases(4096, 6) + dm.big_block_cases():
        if c.near:
            groups.setdefault((c.planar.shape[1], c.family, c.bps, c.max_po, c.near), []).append(c)
        else:
            assert c.family not in ("method", "verbatim") and "wide-k" not in c.name, c
    for key, group in groups.items():
        assert len(group) in (2, 3), key
        order = group[0].expect.get("order", 0)
        for a, b in zip(group, group[1:]):     # in the order they were built: below, at, above
            d = np.abs(np.diff(a.planar[0].astype(np.int64), order) - np.diff(b.planar[0].astype(np.int64), order))
            assert d.sum() == 1 << b.expect.get("wasted", 0) and (d != 0).sum() == 1, (a, b)
            seen += 1
    assert seen > 300


def test_the_matrix_holds_what_it_says():
    assert dm.summary() == dm.COUNTS


def test_big_block_fallback_cases():
    for case in dm.big_block_cases():
        check_mono(case)
        mine = restate(case.planar[0], 16, 6)
        assert mine["ests"] == [None if case.expect["sum"] >= 1 << 30 else 31 * 65535]


# ---------------------------------------------------------------- channel assignments
CODES = (0, 8, 9, 10)   # independent, left/side, side/right, mid/side


def candidates(case):
    left, right = case.planar[0].astype(np.int64), case.planar[1].astype(np.int64)
    return {0: (left, case.bps), 1: (right, case.bps), 8: ((left + right) >> 1, case.bps), 9: (left - right, case.bps + 1)}


def assignment_totals(case, exhaustive, mid_side):
    """The totals the reference compares, in the order it tries the assignments: bits of mono encodes of each candidate
    at its own width (exhaustive), or abs-sums (the fast rule; without mid/side it tries the side pairs first)."""
    n = case.planar.shape[1]
    cand = candidates(case)
    if exhaustive:
        cost = {s: oracle_mono(x, w, n, case.max_po)[1].sub[0].bits for s, (x, w) in cand.items() if mid_side or s != 8}
    else:
        cost = {s: int(np.abs(x).sum()) for s, (x, w) in cand.items()}
    order = [0, 8, 9, 10] if (exhaustive or mid_side) else [8, 9, 0]
    if not mid_side:
        order = [c for c in order if c != 10]
    pair = {0: (0, 1), 8: (0, 9), 9: (9, 1), 10: (8, 9)}
    return [(code, cost[pair[code][0]] + cost[pair[code][1]]) for code in order]


@pytest.mark.parametrize("n,max_po", dm.STEREO_SHAPES)
def test_every_assignment_case(n, max_po):
    for case in dm.stereo_cases(n, max_po):
        for ex in (1, 0):
            for ms in (1, 0):
                o = orc.options("default", block_size=n, max_partition_order=max_po, max_lpc_order=0, mid_side=ms, exhaustive=ex)
                rc, _, plan = orc.encode_frame(o, 44100, case.bps, case.planar)
                assert rc == 0
                totals = assignment_totals(case, ex, ms)
                best = min(t for _, t in totals)
                first = next(code for code, t in totals if t == best)
                where = f"{case} exhaustive {ex} mid_side {ms}: {totals}"
                assert plan.assignment == first, where
                tie = (case.tie or {}).get((ex, ms))
                if tie:
                    tied = [code for code, t in totals if t == best]
                    if tie[0] == "search":
                        assert len(tied) >= 2 and all(plan.sub[c].type != orc.SUB_CONSTANT for c in range(2)), where
                    else:
                        assert tied == tie[0] and first == tie[1], where
                cand = candidates(case)
                for c in range(2):     # each emitted subframe is the mono encode of its candidate
                    x, w = cand[plan.source[c]]
                    assert plan_fields(plan.sub[c]) == plan_fields(oracle_mono(x, w, n, max_po)[1].sub[0]), where
                    want = case.expect.get("wasted_by_source", {}).get(plan.source[c])
                    assert want is None or plan.sub[c].wasted == want, where
        if "wasted_by_source" in case.expect:
            for s, (x, w) in candidates(case).items():
                assert oracle_mono(x, w, n, max_po)[1].sub[0].wasted == case.expect["wasted_by_source"][s], (case, s)


# ---------------------------------------------------------------- the host packer on the oracle's plans
def to_device_plans(oplans, planars, n):
    """The oracle's plans as the C ABI's records, and the residual rows (warm-up + residuals / verbatim samples)."""
    from _compare import expected_row
    from flac_codec_amd._lib import FramePlan, SubframePlan

    nch = planars[0].shape[0]
    plans = (FramePlan * len(oplans))()
    subs = (SubframePlan * (len(oplans) * nch))()
    rows = np.zeros((len(oplans), nch, n), dtype=np.int32)
    for f, (op, planar) in enumerate(zip(oplans, planars)):
        plans[f].assignment, plans[f].channels, plans[f].block_size = op.assignment, nch, n
        body = 0
        for c in range(nch):
            o, s = op.sub[c], subs[f * nch + c]
            for name in ("type", "wasted", "bps", "order", "precision", "shift", "coding_method", "partition_order",
                         "n_partitions", "bits"):
                setattr(s, name, getattr(o, name))
            s.source = op.source[c]
            s.part_len = n >> o.partition_order
            for i in range(o.n_partitions):
                s.rice[i], s.escape_bits[i] = o.rice[i], o.escape_bits[i]
            row = expected_row(s, planar, n)
            rows[f, c, :len(row)] = row
            body += o.bits
        plans[f].body_bits = body
    return plans, subs, rows


@pytest.mark.parametrize("n,max_po", [(64, 3), (4096, 6)])
def test_host_packer_writes_the_oracles_bytes_from_its_plans(n, max_po):
    """flacenc_pack_frames needs no device: the oracle's decisions in, the oracle's bytes out."""
    from flac_codec_amd.gpu import host_pack_frames

    groups = {}
    for case in dm.mono_cases(n, max_po) + dm.stereo_cases(n, max_po):
        groups.setdefault((case.bps, case.planar.shape[0], case.max_po), []).append(case)
    for (bps, nch, po), cases in groups.items():
        o = orc.options("default", block_size=n, max_partition_order=po, max_lpc_order=0, mid_side=1, exhaustive=1)
        enc = [orc.encode_frame(o, 48000, bps, c.planar, frame_number=7 + f) for f, c in enumerate(cases)]
        assert all(rc == 0 for rc, _, _ in enc)
        plans, subs, rows = to_device_plans([p for _, _, p in enc], [c.planar for c in cases], n)
        data, off = host_pack_frames(48000, bps, nch, 7, len(cases), n, plans, subs, rows, threads=2)
        for f, (_, want, _) in enumerate(enc):
            assert data[off[f]:off[f + 1]] == want, f"{cases[f]}: the host packer's frame differs from the oracle's"
