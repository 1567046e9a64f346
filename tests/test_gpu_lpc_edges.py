"""K4 -- Levinson-Durbin, order choice, quantisation (lpc_candidate, csrc/kernels/lpc.inc) -- held to the oracle at its
edges (tests/_lpc_edge_matrix.py; every case proven on the CPU by test_lpc_edge_matrix_oracle.py).

ROWS: f64 autocorrelation rows go through GpuAnalyzer.test_lpc_rows, which launches K4 alone through the product's
launcher (k_lpc_u<8 | 12 | 16 | 32> by the context's max_lpc_order) and returns the raw records, the tie list and the
counters.  PCM: integer frames that reach the failure and clamp branches go through encode_frames (the fused tail of
the in-place autocorrelation kernel, k_lpc_u behind the deep and the generic ones, a ragged batch), and the records
come back through flacgpu_device_buffer 7."""

import numpy as np
import pytest

import _lpc_edge_matrix as M
import _oracle as orc
from _compare import orc_options_for
from _lpc_edge_matrix import host_record, same_record

pytestmark = pytest.mark.gpu

RATE = 48000
_device = {}


def device_rows(L):
    """K4 on every row of the matrix with max_lpc_order L, once: (cases, oracle records, device records, tie rows, counters)."""
    if L not in _device:
        from flac_codec_amd.gpu import GpuAnalyzer

        cases = [c for c in M.rows() if c.L == L]
        ac = np.zeros((len(cases), 36), dtype=np.float64)
        for i, c in enumerate(cases):
            ac[i, : L + 1] = c.ac[: L + 1]
        an = GpuAnalyzer(64, 4, L, False, True, 2, 0.5, 16, 1, max_frames=1)
        try:
            got, ties, counters = an.test_lpc_rows(ac, [c.n for c in cases], [c.bps for c in cases])
        finally:
            an.close()
        want = [M.oracle_record(c.ac, c.L, c.n, c.bps) for c in cases]
        _device[L] = (cases, want, got, ties, counters)
    return _device[L]


@pytest.mark.parametrize("L", M.ORDERS)
def test_rows_equal_the_oracle_and_are_no_ties(L):
    cases, want, got, ties, _ = device_rows(L)
    tie_family = {i for i, c in enumerate(cases) if c.family in M.TIE_FAMILIES}
    bad = [(c.family, c.note, c.n, c.bps, int(g["status"]), int(g["order"]), int(g["shift"]), list(g["qlp"][:4]), w.status, w.order,
            w.shift, w.qlp[:4])
           for i, (c, w, g) in enumerate(zip(cases, want, got)) if i not in tie_family and not same_record(g, w)]
    assert not bad, (len(bad), bad[:6])
    listed = [(cases[i].family, cases[i].note) for i in ties if i not in tie_family]
    assert not listed, listed[:6]


@pytest.mark.parametrize("L", M.ORDERS[1:])
def test_near_ties_are_listed_for_the_host(L):
    cases, want, _, ties, counters = device_rows(L)
    tie_family = [i for i, c in enumerate(cases) if c.family in M.TIE_FAMILIES]
    assert any(cases[i].family == "near_tie" for i in tie_family)
    assert len(ties) == counters[1]
    missing = [(cases[i].family, cases[i].note) for i in tie_family if i not in ties]
    assert not missing, missing
    for i in tie_family:
        c = cases[i]
        assert same_record(host_record(c.ac, c.L, c.n, c.bps), want[i]), (c.family, c.note)


@pytest.mark.parametrize("L", M.ORDERS)
def test_failure_counter(L):
    cases, want, got, _, counters = device_rows(L)
    tie_family = {i for i, c in enumerate(cases) if c.family in M.TIE_FAMILIES}
    assert all(want[i].status == 0 for i in tie_family)       # (either order of a tie quantises: they count nothing)
    expected = sum(1 for w in want if w.status != 0)
    assert expected > 0 and counters[0] == expected, (counters, expected)
    assert sum(1 for g in got if g["status"] != 0) == expected


@pytest.mark.parametrize("L", M.ORDERS)
def test_size_hint(L):
    cases, want, got, _, _ = device_rows(L)
    checked = 0
    for c, w, g in zip(cases, want, got):
        if w.status != 0 or c.family in M.TIE_FAMILIES:
            continue
        v, near = M.est8_rule(w.best_bits, c.n)
        allowed = {v}
        if near:
            e = w.best_bits * 8.0 / c.n
            allowed = {M.est8_rule((e + d) * c.n / 8.0, c.n)[0] for d in (-2e-6, 0.0, 2e-6)}
        print(f"{c.family} {c.note}: est8 {int(g['est8'])}, rule {v}{' (near an integer)' if near else ''}")
        assert int(g["est8"]) in allowed, (c.family, c.note, int(g["est8"]), allowed, w.best_bits)
        checked += 1
    assert checked > 0


def _no_order_on_an_edge(c, w):
    """No order of a tie row has its max |c| in a log2 band (the device may stand on either order before the host re-decides)."""
    coeffs, _ = orc.lp_coefficients(c.ac[: c.L + 1])
    return not any(M.log2_edge(float(np.max(np.abs(coeffs[i])))) for i in range(len(w.bits)))


def test_log2_edge_counter():
    total = expected = 0
    for L in M.ORDERS:
        cases, want, _, _, counters = device_rows(L)
        here = 0
        for c, w in zip(cases, want):
            if c.family in M.TIE_FAMILIES:
                assert _no_order_on_an_edge(c, w), (c.family, c.note)
                continue
            if w.status in (0, 4):
                here += M.log2_edge(w.l)
        print(f"max_lpc_order {L}: log2_edge {counters[2]}, expected {here}")
        assert counters[2] == here, (L, counters, here)
        total += counters[2]
        expected += here
    assert total == expected and total > 0


# ---------------------------------------------------------------------------------------------------------------------
# integer PCM
# ---------------------------------------------------------------------------------------------------------------------
def _encode(an, ctx):
    """(frame bytes per frame, the frames' numbers): whole blocks through encode_frames, the ragged batch from device memory"""
    n = len(ctx.frames)
    if not ctx.ragged:
        planar = np.stack([np.stack([x for _, x in f]) for f in ctx.frames])              # [F][C][block]
        pcm = np.ascontiguousarray(planar.transpose(0, 2, 1)).astype(np.int32).reshape(-1)
        data, off = an.encode_frames(pcm, n, ctx.block, 0, RATE)
        return [data[off[f]:off[f + 1]] for f in range(n)], None
    import torch

    parts, offsets, at = [], [], 0
    for f in ctx.frames:
        inter = np.ascontiguousarray(np.stack([x for _, x in f]).T).astype(np.int32).reshape(-1)
        offsets.append(at)
        parts.append(inter)
        at += (inter.size + 3) & ~3
    host = np.zeros(at + 8, dtype=np.int32)
    for o, p in zip(offsets, parts):
        host[o:o + p.size] = p
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    an.encode_ragged_device([(dev.data_ptr() + 4 * o, len(f[0][1]), k) for k, (o, f) in enumerate(zip(offsets, ctx.frames))], RATE)
    data, off = an.fetch_frames()
    return [data[off[f]:off[f + 1]] for f in range(n)], dev


@pytest.mark.parametrize("ctx", M.pcm_contexts(), ids=lambda c: c.name)
def test_pcm_branches(ctx):
    from flac_codec_amd.gpu import GpuAnalyzer

    n = len(ctx.frames)
    opts = orc_options_for(ctx.block, 6, ctx.L, True, True, ctx.window[0], ctx.window[1])
    want_bytes = []
    for f, frame in enumerate(ctx.frames):
        rc, data, _ = orc.encode_frame(opts, RATE, ctx.bps, np.stack([x for _, x in frame]).astype(np.int32), frame_number=f)
        assert rc == 0
        want_bytes.append(data)
    records = M.pcm_records(ctx)
    an = GpuAnalyzer(ctx.block, 6, ctx.L, True, True, ctx.window[0], ctx.window[1], ctx.bps, ctx.channels, max_frames=n)
    try:
        got_bytes, keep = _encode(an, ctx)
        for f in range(n):
            assert got_bytes[f] == want_bytes[f], f"{ctx.name}: frame {f} ({[t for t, _ in ctx.frames[f]]}) differs from the oracle's"
        res, _ = an.verify_device(RATE, 0)
        assert (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs, res.samples_differ) == (n, 0, 0, 0, 0)
        ncand = an.candidates_per_frame()
        got = an.lpc_params().reshape(n, ncand)
        stats = an.stats()
        del keep
    finally:
        an.close()
    failed = 0
    for f, recs in enumerate(records):
        assert len(recs) == ncand
        for c, want in enumerate(recs):
            if want is None:
                continue                                   # an all-zero candidate gets no LPC analysis
            failed += want.status != 0
            assert same_record(got[f, c], want), (ctx.name, f, c, int(got[f, c]["status"]), int(got[f, c]["order"]),
                                                  int(got[f, c]["shift"]), list(got[f, c]["qlp"][:4]), want.status, want.order, want.shift,
                                                  want.qlp[:4])
    print(f"{ctx.name}: lpc_failed {stats.lpc_failed}, expected {failed}; order_ties {stats.order_ties}")
    assert failed > 0 and stats.lpc_failed == failed
    assert stats.order_ties == 0
