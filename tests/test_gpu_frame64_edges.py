"""k_frame64 / wave_subframe (csrc/kernels/pack.inc) held to hand-built plans at their Rice, escape, word and CRC edges
(tests/_frame64_edge_matrix.py; every case proven on the CPU by test_frame64_edge_matrix_host.py).

The cases of one shape are the frames of one context and one flacgpu_pack_plans call.  Offsets and bytes must equal the
Python writer's frame by frame, twice on the same context; once per block length, channel count and instantiation the
same plans go through the generic packer (FLACGPU_NO_FRAME64), so that a failure points at the right kernel.  A failure
prints the geometry's description of the first differing byte.  The last test counts the compared cases against the
matrix: run the module whole."""
import pytest

import _frame64_edge_matrix as M

pytestmark = pytest.mark.gpu

SHAPES = M.shapes()
COMPARED = {}                                  # case name -> frames compared on k_frame64


def analyzer(sh, n_frames):
    from flac_codec_amd.gpu import GpuAnalyzer

    return GpuAnalyzer(sh.block, 6, sh.max_lpc, bool(sh.mid_side), bool(sh.exhaustive), 2, 0.5, sh.bps, sh.C, max_frames=n_frames)


def same(b, got, where, count=None):
    """Every frame's offsets and bytes against the expected ones; the model's description of the first differing byte."""
    data, off = got
    want, want_off = M.batch_bytes(b)
    fl = M.batch_frames(b)
    assert len(off) == len(want_off), (where, len(off), len(want_off))
    for f, (bt, i) in enumerate(fl):
        a, w = bytes(data[off[f]:off[f + 1]]), want[want_off[f]:want_off[f + 1]]
        if (off[f], off[f + 1]) != (want_off[f], want_off[f + 1]) or a != w:
            at = next((j for j in range(min(len(a), len(w))) if a[j] != w[j]), -1)
            raise AssertionError("%s: offsets %s, expected %s; %s" % (where, list(off[f:f + 2]), want_off[f:f + 2], M.describe(b, f, at)))
        if count is not None:
            count[bt.case.name] = count.get(bt.case.name, 0) + 1
    assert len(data) == want_off[-1], (where, "bytes behind the last frame")


def packed(an, b, plans, subs):
    sh = b.shape
    return an.pack_plans(M.interleaved(b), len(M.batch_frames(b)), sh.block, plans, subs, sh.first, sh.rate)


@pytest.mark.parametrize("sh", SHAPES, ids=M.shape_id)
def test_every_frame_byte_for_byte(sh):
    from test_route_table import route

    b = M.batch_of(sh)
    n = len(M.batch_frames(b))
    assert route(M.route_inputs(sh, n))[3] == n
    plans, subs, _ = M.plan_arrays(b)
    an = analyzer(sh, n)
    try:
        count = {}
        same(b, packed(an, b, plans, subs), "k_frame64<%d,%d,%d>, call 0" % M.launcher(sh), count)
        same(b, packed(an, b, plans, subs), "k_frame64<%d,%d,%d>, call 1" % M.launcher(sh))      # the same context, the same bytes
        COMPARED.update(count)
    finally:
        an.close()


@pytest.mark.parametrize("sh", M.parity_shapes(), ids=M.shape_id)
def test_the_generic_packer_gives_the_same_bytes(monkeypatch, sh):
    """FLACGPU_NO_FRAME64: k_emit + k_pack + k_crc on the same plans, once per block length, channel count and depth."""
    monkeypatch.setenv("FLACGPU_NO_FRAME64", "1")
    b = M.batch_of(sh)
    plans, subs, _ = M.plan_arrays(b)
    an = analyzer(sh, len(M.batch_frames(b)))
    try:
        same(b, packed(an, b, plans, subs), "the generic packer")
    finally:
        an.close()


def test_a_plan_the_image_cannot_hold_is_refused_and_the_context_goes_on():
    """One bit more than the launch's image holds: flacgpu_pack_plans returns the error before anything is copied or
    launched (host/plan_check.cpp; its refusals are proven on the CPU by test_plan_check_host.py), and the same context
    packs a good batch afterwards."""
    from flac_codec_amd.gpu import GpuError

    sh = next(s for s in SHAPES if s.block == 1024 and s.C == 2)
    b = M.batch_of(sh)
    n = len(M.batch_frames(b))
    plans, subs, _ = M.plan_arrays(b)
    an = analyzer(sh, n)
    try:
        keep = plans[1].body_bits, subs[2].bits
        over = M.max_body_bits(sh) + 1 - plans[1].body_bits
        plans[1].body_bits += over
        subs[2].bits += over
        with pytest.raises(GpuError) as e:
            packed(an, b, plans, subs)
        assert e.value.code == -1 and "frame 1" in str(e.value) and "body_bits over the image" in str(e.value), str(e.value)
        plans[1].body_bits, subs[2].bits = keep
        same(b, packed(an, b, plans, subs), "after the refusal")
    finally:
        an.close()


def test_every_case_of_the_matrix_was_compared():
    want = {bt.case.name: len(bt.recs) for b in M.batches() for bt in b.built}
    assert len(want) == len(M.case_list())
    assert COMPARED == want, sorted(set(want) - set(COMPARED))
