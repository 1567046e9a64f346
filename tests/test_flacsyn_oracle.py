"""The hand-built streams of _foreign_matrix.py on the CPU: the writer (_flacsyn.py) against the oracle's decoder and
against the oracle's encoder, so that a failure of test_gpu_decode_foreign.py is the kernel's fault, not the writer's."""
import numpy as np
import pytest

import _flacsyn as fs
import _foreign_matrix as fm
import _oracle as orc
from _pcm import synth_fast

# Every syntax feature the matrix has to reach.  The union of what the writer recorded must be exactly this, so that a
# dropped case fails here.  (Built from _flacsyn streams alone: this project's encoder covers none of it.)
REQUIRED = set(
    [("kind", "constant"), ("kind", "verbatim")]
    + [("fixed_order", o) for o in (0, 1, 2, 3, 4)]
    + [("lpc_order", o) for o in range(1, 33)]
    + [("residuals", kind, left) for kind in ("fixed", "lpc") for left in (0, 1)]   # n == order, n == order + 1
    + [("lpc_precision", p) for p in range(1, 16)]
    + [("lpc_shift", s) for s in range(0, 16)]
    + [("lpc_coef", "lowest"), ("lpc_coef", "highest"), ("lpc_sum_bits", "49+")]
    + [("rice_k", k) for k in range(0, 15)]
    + [("rice2_k", k) for k in range(0, 31)]
    + [("escape_bits", b) for b in (0, 1, 2, 17, 31)]
    + [("porder", 0)]
    + [("porder", 16, po) for po in (1, 2, 3, 4)]
    + [("porder", 4096, po) for po in range(1, 13)]
    + [("porder", 32768, 15), ("porder", 32, 3), ("porder", 64, 2), ("porder", 64, 3)]
    + [("empty_partition0", "rice"), ("empty_partition0", "escape")]
    + [("alternating_partitions", 0), ("alternating_partitions", 1)]
    + [("rice_code_bits", b) for b in (31, 32, 33, 64, 65)]
    + [("rice_quotient", "hundreds"), ("rice_quotient", "thousands")]
    + [("rice33_every_phase", k) for k in (2, 14, 28, 30)]
    + [("wasted", kind, w) for kind in ("constant", "verbatim", "fixed") for w in (1, 2, 8, "bps-1")]
    + [("wasted", "lpc", w) for w in (1, 2, "bps-1")]
    + [("wasted", "fixed", 3), ("wasted_at_32",)]
    + [("wasted_on_side", b) for b in (9, 13, 17, 21, 25, 33)]
    + [("channels", c) for c in range(1, 9)]
    + [("assignment", a) for a in range(0, 11)]
    + [("side_bps", side, b) for side in ("left", "right", "mid") for b in (9, 13, 17, 21, 25, 33)]
    + [("side_bps", "mid", b) for b in (5, 11, 18, 32)]
    + [("side_full_width", side, b) for side in ("left", "right", "mid") for b in (9, 13, 17, 21, 25, 33)]
    + [("side_full_width", "mid", 5)]
    + [("side33", side) for side in ("left", "right", "mid")]
    + [("side33_kind", kind) for kind in ("constant", "verbatim", "fixed", "lpc")]
    + [("mid_side", "odd_sum"), ("mid_side", "even_sum"), ("mid_side", "negative_side")]
    + [("stream_bps", b) for b in (4, 8, 10, 12, 16, 17, 20, 24, 31, 32)]
    + [("bps_code", c) for c in (0, 1, 2, 4, 5, 6, 7)]
    + [("bcode", c) for c in range(1, 16)]
    + [("bcode_n", 6, 1), ("bcode_n", 6, 256), ("bcode_n", 7, 257), ("bcode_n", 7, 65535), ("bcode_n", 6, 16),
       ("bcode_n", 6, 192), ("bcode_n", 7, 256), ("bcode_n", 7, 4096)]
    + [("rcode", c) for c in range(0, 15)]
    + [("number_bytes", b) for b in range(1, 8)]
    + [("blocking", 0), ("blocking", 1)]
    + [("metadata", t) for t in (1, 2, 3, 4)]
    + [("min_frame", "exact"), ("min_frame", 0), ("total_samples", "exact"), ("total_samples", 0)]
    + [("md5", "right"), ("md5", "zero"), ("md5", "wrong")])


def test_every_valid_case_decodes_on_the_oracle():
    cases = fm.valid_cases()
    assert 100 <= len(cases) <= 400 and sum(s.coded_samples for s in cases) <= 500_000
    for s in cases:
        rc, pcm, info = orc.decode_stream(s.blob)
        assert rc == 0, s.name
        assert np.array_equal(pcm, s.pcm), s.name
        assert info.frames == s.n_frames, s.name
        assert info.md5_ok == {1: 1, 2: -1, 0: 0}[s.md5_status], s.name
        assert (info.channels, info.bps, info.sample_rate) == (s.channels, s.bps, s.rate), s.name


def test_feature_coverage_is_complete():
    got = set().union(*[s.features for s in fm.valid_cases()])
    assert got - REQUIRED == set(), "recorded but not listed"
    assert REQUIRED - got == set(), "listed but no case has it"


def test_variable_block_size_stream_shape():
    st = [s for s in fm.valid_cases() if s.name == "variable-block-size"][0]
    assert st.n_frames == 5 and st.pcm.size == 16 + 4096 + 1 + 577 + 192
    st = [s for s in fm.valid_cases() if s.name == "fixed-block-last-1"][0]
    assert st.n_frames == 3 and st.pcm.size == 192 + 192 + 1


@pytest.mark.parametrize("reason", [r for r, _, _ in fm.INVALID])
def test_invalid_case_is_refused_by_the_oracle(reason):
    st = dict(fm.invalid_cases())[reason]
    rc, _, _ = orc.decode_stream(st.blob)
    assert rc != 0


def _sub_from_plan(sp, n):
    """The oracle encoder's decisions for one subframe as a _flacsyn subframe."""
    kw = dict(wasted=sp.wasted)
    if sp.type == orc.SUB_CONSTANT:
        return fs.constant(**kw)
    if sp.type == orc.SUB_VERBATIM:
        return fs.verbatim(**kw)
    parts = 1 << sp.partition_order
    assert sp.n_partitions == parts
    params = tuple(("escape", sp.escape_bits[p]) if sp.rice[p] == 0xFF else sp.rice[p] for p in range(parts))
    kw.update(method=sp.coding_method, porder=sp.partition_order, params=params)
    if sp.type == orc.SUB_FIXED:
        return fs.fixed(sp.order, **kw)
    return fs.lpc(sp.order, sp.precision, sp.shift, list(sp.coeffs[:sp.order]), **kw)


@pytest.mark.parametrize("ch,bps,preset", [(1, 16, "fast"), (2, 16, "best"), (2, 24, "fast"), (1, 24, "best"),
                                           (2, 16, "default")])
def test_writer_reemits_the_encoders_frames_byte_for_byte(ch, bps, preset):
    """Pins the bit layout, both CRCs and the zigzag mapping: the oracle encoder's frame, written again from its own
    plan, is the same bytes."""
    n = 1152
    opts = orc.options(preset, block_size=n)
    pcm = synth_fast(300 + ch + bps, ch, bps, n * 3)
    planar = pcm.reshape(-1, ch).T
    kinds = set()
    for f in range(3):
        block = np.ascontiguousarray(planar[:, f * n:(f + 1) * n])
        rc, data, plan = orc.encode_frame(opts, 44100, bps, block, frame_number=f)
        assert rc == 0
        subs = [_sub_from_plan(plan.sub[c], n) for c in range(ch)]
        kinds.update(s["kind"] for s in subs)
        fr = fs.Frame(block.tolist(), subs, assignment=plan.assignment, number=f,
                      rcode=fs.RATE_CODES[44100])
        again = fs.write_frame(44100, bps, fr, set())
        assert again == data, f"frame {f}"
        assert fs.crc16(data[:-2]) == int.from_bytes(data[-2:], "big") == orc.crc16(data[:-2])
    assert kinds & {"fixed", "lpc"}
