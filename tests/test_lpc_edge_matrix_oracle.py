"""tests/_lpc_edge_matrix.py on the CPU: every case lands in the family it names (oracle alone), and the host
re-decision (lpc_from_autocorr, through its hook flacenc_lpc_host_row) gives the oracle's record on every row.
(The reference's own test_quantization vectors are pinned in test_oracle_kat.py.)  No GPU call."""
import collections

import pytest

import _lpc_edge_matrix as M
from _lpc_edge_matrix import host_record, same_record


def test_every_row_lands_in_its_family():
    rows = M.rows()
    records = [M.prove(c) for c in rows]
    assert {c.L for c in rows} == set(M.ORDERS)
    by_lmax = collections.Counter(M.lmax_of(c.L) for c in rows)
    assert set(by_lmax) == {8, 12, 16, 32}
    assert {r.status for r in records} == {0, 1, 2, 3, 4}
    # every shift 15 .. -16 at every precision 7 .. 13
    reached = {(r.precision, r.true_shift) for r in records if r.status == 0}
    assert reached >= {(p, s) for p in range(7, 14) for s in range(-16, 16)}
    assert {c.n for c in rows if c.family == "precision"} == set(M.PRECISION_N)
    assert sum(M.log2_edge(r.l) for r in records) > 0
    ties = [c for c in rows if c.family == "near_tie"]
    assert {c.L for c in ties} == set(M.ORDERS[1:]) and all(c.want <= 1e-11 for c in ties)
    assert any(c.want > 0 for c in ties) and any(c.want == 0 for c in ties)
    assert any(c.family == "equal_minima" for c in rows)


def test_host_redecision_equals_the_oracle_on_every_row():
    bad = []
    for c in M.rows():
        want = M.oracle_record(c.ac, c.L, c.n, c.bps)
        got = host_record(c.ac, c.L, c.n, c.bps)
        if not same_record(got, want):
            bad.append((c.family, c.L, c.n, c.bps, c.note, int(got["status"]), int(got["order"]), int(got["shift"]),
                        want.status, want.order, want.shift))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("ctx", M.pcm_contexts(), ids=lambda c: c.name)
def test_pcm_reaches_the_branches(ctx):
    records = M.pcm_records(ctx)
    proved = 0
    for f, recs in enumerate(records):
        own = recs[: ctx.channels]
        for ch, rec in enumerate(own):
            if rec is not None:
                proved += M.prove_pcm(ctx, f, ch, rec)
        for rec in recs:
            if rec is None:
                continue
            gap = M.two_best_gap(rec.bits)
            assert gap is None or not (gap < M.MARGIN), (ctx.name, f, gap)
    assert proved > 0
    assert sum(1 for recs in records for r in recs if r is not None and r.status != 0) > 0      # lpc_failed > 0 in every context
