"""tests/_autocorr_edge_matrix.py proven on the CPU, with the oracle and the library's two device-free hooks alone: every
case reaches the kernel it names (flacenc_plan_autocorr_row) by the door it names (flacenc_plan_route_row), skips the
candidates it says it skips, and lands on the edge it aims at; the matrix reaches every instantiation the dispatcher can
launch; and the oracle's autocorrelation is, bit for bit, a plain left fold with one multiply and one add per term."""
import numpy as np
import pytest

import _autocorr_edge_matrix as m
import _oracle as orc

CASES = m.cases()


def frames_to_prove(case):
    """every distinct frame of the case (a batch repeats a period of 16)"""
    fs = list(range(min(case.frames, m.PERIOD)))
    if case.frames - 1 not in fs:
        fs.append(case.frames - 1)
    return fs


def test_every_case_reaches_the_kernel_it_names_by_the_door_it_names():
    for c in CASES:
        assert m.route_of(c) == c.route, c.name
        name, fused, t0, t1 = m.kernel_of(c)
        assert name == c.reach, (c.name, name)
        assert fused == c.fused, (c.name, fused, t0, t1)
        assert (t0, t1) == m.tiles_of(c), c.name
        if c.last != c.block:
            name, fused, _, _ = m.kernel_of(c, last_frame=True)
            assert name == c.reach_last and not fused, (c.name, name)   # a short last frame has its own window: never fused tiles
        else:
            assert c.reach_last is None, c.name
        if c.door == m.RAGGED:
            assert c.lengths and len(c.lengths) == c.frames and max(c.lengths) <= c.block
        assert c.frames <= 17 or c.name.startswith(("groups-stereo-102", "groups-3ch-23")), c.name


def test_every_instantiation_is_reached():
    reached = {c.reach for c in CASES} | {c.reach_last for c in CASES if c.reach_last}
    missing = m.every_instantiation() - reached
    assert not missing, sorted(missing)
    print(f"{len(CASES)} cases reach {len(reached)} instantiations, all {len(m.every_instantiation())} the dispatcher can launch among them")


def test_summary_is_the_table():
    fam, reached = m.summary()
    print(fam)
    assert fam == m.FAMILIES
    assert reached == m.REACHED


def test_shared_construction_and_skipped_candidates():
    """wasted bits on channel 0, both rails for half a frame each and never a whole one, no constant or silent candidate beyond
    the declared count (which is at most 2)"""
    skipped_total = 0
    for c in CASES:
        assert 0 <= c.skipped <= 2
        skipped, rails = 0, set()
        for f in frames_to_prove(c):
            rows = m.frame_of(c, f)
            n = rows.shape[1]
            assert int(np.bitwise_or.reduce(rows[0])) % 4 == 0, (c.name, f)
            hi, lo = (1 << (c.bps - 1)) - 1, -(1 << (c.bps - 1))
            assert rows.min() >= lo and rows.max() <= hi
            last = rows[c.ch - 1]
            top = (hi >> 2) << 2 if c.ch == 1 else hi
            for a, b, sign in m.rail_spans(n, m.slot_of(c, f)):
                if b > a:
                    assert np.all(last[a:b] == (top if sign > 0 else lo)), (c.name, f)
                    assert b - a <= (n + 1) // 2
                    rails.add(sign)
            if n > c.order:
                skipped += sum(x is None for x in m.shifted_windowed(c.ch, c.bps, n, m.slot_of(c, f), c.window))
        assert skipped == c.skipped, (c.name, skipped)
        assert rails == {+1, -1}, c.name
        skipped_total += skipped
    print("candidates the reference does not analyse, over all cases:", skipped_total)


def test_fused_cases_land_on_their_edges():
    seen = set()
    for c in CASES:
        if c.family != "fused":
            continue
        lo, hi = m.flat_run(c.window[0], c.window[1], c.block)
        t0, t1 = m.tiles_of(c)
        maxlag = 16 if c.order <= 16 else 32
        kind = c.aim[0]
        if kind == "lo":
            # (the margin's boundary: flat_lo + maxlag one short of a multiple of 32, on it, one past it)
            assert lo % 32 == c.aim[1] and (lo + maxlag) % 32 in (31, 0, 1), (c.name, lo)
            assert t0 == (lo + maxlag + 31) // 32 and 32 * t0 - (lo + maxlag) == (-(lo + maxlag)) % 32
        elif kind == "hi":
            assert hi % 32 == c.aim[1] and t1 == hi // 32, (c.name, hi)
        elif kind == "none":
            assert hi > lo and t0 >= t1 and hi - lo < 32 + maxlag + 31, (c.name, lo, hi)
        elif kind == "rect":
            assert (lo, hi) == (0, c.block) and (t0, t1) == ((maxlag + 31) // 32, c.block // 32)
        elif kind == "hann":
            assert hi == lo and (t0, t1) == (0, 0)
        else:
            assert (c.bps <= 26) == c.fused and c.ch == 1
        if c.fused:
            assert t0 < t1
            for f in (0, 1):                              # the rails (frame 0: positive, frame 1: negative) sit in fused tiles
                (a, b, _), = m.rail_spans(c.block, m.slot_of(c, f))
                assert max(a, 32 * t0) + 32 <= min(b, 32 * t1), (c.name, a, b, t0, t1)
        else:
            assert t0 >= t1
        seen.add((c.block, c.order > 16) + tuple(c.aim))
    for block in (4096, 1152):
        for r in (15, 16, 17):
            assert (block, False, "lo", r) in seen
        for r in (31, 0, 1):
            assert (block, True, "lo", r) in seen and (block, False, "hi", r) in seen and (block, True, "hi", r) in seen
    assert {(4096, False, "width", b) for b in (25, 26, 27, 32)} <= seen


PATHS = {"order+1": "g", "order+2": "g", "H-1": "g", "H": "g", "TS-1": "g", "TS": "g", "TS+1": "gg", "2TS-1": "gg", "2TS+1": "gfg",
         "31": "g", "33": "g"}


def test_generic_cases_take_both_paths_of_the_tile_loop():
    """a ten-line model of ac_wave's `tbase + TS <= n && t > 0` (generic_tile_paths): every listed length is used for every H,
    as a block or as a short last frame, and takes the tiles its label promises"""
    used = {}
    for c in CASES:
        if c.family != "generic":
            continue
        H = m.h_of(c.order)
        assert c.reach == c.reach_last == f"k_autocorr2<{H}>"
        for n in (c.block, c.last):
            assert n > c.order
            used.setdefault(c.order, {})[n] = m.generic_tile_paths(n, H)
    assert sorted(used) == sorted(m.GENERIC_ORDERS)
    for order, by_len in used.items():
        for n, labels in m.generic_lengths(order).items():
            assert n in by_len, (order, n, labels)
            for label in labels:
                assert by_len[n] == PATHS[label], (order, n, label, by_len[n])
        assert any("f" in p for p in by_len.values()) and any(p.endswith("fg") for p in by_len.values())
    assert set("".join(used[14][1000])) == {"f", "g"} and used[32][4095].count("f") > 100


def test_tiles_cases_cover_the_pipelines_prologue_pairs_and_tail():
    for prod in ("planar-stereo", "planar-indep"):
        for ns in (4, 2):
            for order in (4, 8, 12, 16):
                ntiles = {c.block // 32 for c in CASES if c.family == "tiles" and c.reach == m.ac4(order, ns, prod)}
                assert {1, 2, 3, 4, 5} <= ntiles, (prod, ns, order, ntiles)
        assert {c.block for c in CASES if c.family == "tiles" and c.reach == m.deep(prod)} == {64, 128, 192}
    assert m.case_named("tiles-mono-n65504-2047-tiles").block // 32 == 2047


def test_ragged_batches_mix_their_lengths():
    for c in CASES:
        if c.family != "ragged":
            continue
        TS = m.ts_of(m.h_of(c.order))
        assert {c.order + 1, 31, 32, 33, TS - 1, TS + 1, 4095, 4096} <= set(c.lengths)
        assert any(n <= c.order for n in c.lengths)
        assert list(c.lengths) != sorted(c.lengths) and list(c.lengths) != sorted(c.lengths, reverse=True)
        first_group = c.lengths[: max(64 // m.ncand_of(c), 1)]
        assert len(set(first_group)) > 4                  # mixed lengths inside one workgroup


def test_the_oracles_autocorrelation_is_a_plain_left_fold():
    """every distinct (frame, order, window) of every case: orc.autocorrelate == left fold from -0.0, bit for bit"""
    done = set()
    for c in CASES:
        for f in frames_to_prove(c):
            n, slot = m.length_of(c, f), m.slot_of(c, f)
            key = (c.ch, c.bps, n, slot, c.order, c.window)
            if key in done or n <= c.order:
                continue
            done.add(key)
            rows = m.shifted_windowed(c.ch, c.bps, n, slot, c.window)
            want = m.frame_sums(*key)
            live = [i for i, r in enumerate(rows) if r is not None]
            got = m.left_fold([rows[i] for i in live], c.order)
            for k, i in enumerate(live):
                assert len(want[i]) == min(c.order, n - 1) + 1
                assert np.array_equal(got[k].view(np.int64), want[i].view(np.int64)), (c.name, f, i)
    print(len(done), "distinct frames folded")


def test_left_fold_is_the_scalar_fold():
    """the vectorised fold above against numpy f64 scalars, one lag at a time (so the statement needs no trust in slicing)"""
    xw = m.shifted_windowed(2, 24, 160, 0, (m.TUKEY, 0.5))[3]
    got = m.left_fold([xw], 12)[0]
    for lag in range(13):
        acc = np.float64(-0.0)
        for i in range(len(xw) - lag):
            acc = acc + xw[i] * xw[i + lag]
        assert acc.view(np.int64) == got[lag].view(np.int64)
    assert np.array_equal(got.view(np.int64), orc.autocorrelate(xw, 12).view(np.int64))
