"""flacgpu_pack_plans refuses plans the kernels cannot hold (csrc/host/plan_check.cpp check_plans, through the
flacenc_check_plans_row hook): one case per refused field, and the image bound of both stereo images one bit under and one
bit over.  CPU-only: nothing here is ever sent to a device."""
import pytest

import _frame64_edge_matrix as M
from test_frame64_edge_matrix_host import check_plans

STEREO = M.shape(4096, 2, 16)
MONO_SHORT = M.shape(1152, 1, 16)
EIGHT = M.shape(4096, 8, 16, max_lpc=12)


def good(sh, n_frames=2, last_len=None):
    """Two frames the check takes: subframe 0 LPC of order 2 with four Rice partitions, the others CONSTANT (stereo: the
    second the side channel of assignment 8)."""
    from flac_codec_amd._lib import FramePlan, SubframePlan

    plans, subs = (FramePlan * n_frames)(), (SubframePlan * (n_frames * sh.C))()
    for f in range(n_frames):
        n = last_len if last_len and f + 1 == n_frames else sh.block
        plans[f].assignment, plans[f].channels, plans[f].block_size = (8 if sh.C == 2 else 0), sh.C, n
        for c in range(sh.C):
            sp = subs[f * sh.C + c]
            side = sh.C == 2 and c == 1
            sp.source = 9 if side else c
            sp.bps = sh.bps + (1 if side else 0)
            sp.bits = 8 + sp.bps
            if c == 0:
                sp.type, sp.order, sp.precision, sp.shift, sp.coding_method, sp.partition_order = 3, 2, 12, 10, 0, 2
                sp.n_partitions, sp.part_len = 4, n // 4
                sp.coeffs[0], sp.coeffs[1] = 2047, -2048
                for i in range(4):
                    sp.rice[i] = 3
                sp.bits = 8 + 2 * sp.bps + 9 + 24 + 6 + 4 * 4 + 5 * (n - 2)
        plans[f].body_bits = sum(subs[f * sh.C + c].bits for c in range(sh.C))
    return plans, subs


def test_a_good_plan_is_taken():
    for sh in (STEREO, MONO_SHORT, EIGHT):
        plans, subs = good(sh)
        assert check_plans(sh, 2, plans, subs) is None


def frame_field(name, value):
    return lambda plans, subs, sh: setattr(plans[1], name, value)


def sub_field(name, value, c=0):
    return lambda plans, subs, sh: setattr(subs[sh.C + c], name, value)


def rice_at(i, k, eb=None):
    def f(plans, subs, sh):
        subs[sh.C].rice[i] = k
        if eb is not None:
            subs[sh.C].escape_bits[i] = eb
    return f


def coef_at(j, v):
    return lambda plans, subs, sh: subs[sh.C].coeffs.__setitem__(j, v)


def both(*fs_):
    return lambda plans, subs, sh: [f(plans, subs, sh) for f in fs_]


# (shape, what is changed in frame 1, the subframe named -- channels: the frame's own record --, the field named)
REFUSALS = [
    ("channels", STEREO, frame_field("channels", 1), 2, "channels"),
    ("block_size", STEREO, frame_field("block_size", 4095), 2, "block_size"),
    ("assignment_unknown", STEREO, frame_field("assignment", 7), 2, "assignment"),
    ("assignment_on_independent_channels", MONO_SHORT, frame_field("assignment", 8), 1, "assignment"),
    ("type", STEREO, sub_field("type", 4), 0, "type"),
    ("source_stereo", STEREO, sub_field("source", 2), 0, "source"),
    ("source_independent", MONO_SHORT, sub_field("source", 1), 0, "source"),
    ("bps", STEREO, sub_field("bps", 17), 0, "bps"),
    ("bps_of_the_side", STEREO, both(sub_field("bps", 16, 1), sub_field("bits", 24, 1)), 1, "bps"),
    ("wasted", STEREO, sub_field("wasted", 16), 0, "wasted"),
    ("wasted_without_bps", STEREO, sub_field("wasted", 3), 0, "bps"),
    ("order_lpc_over_the_context", STEREO, sub_field("order", 17), 0, "order"),
    ("order_lpc_zero", STEREO, sub_field("order", 0), 0, "order"),
    ("order_fixed", STEREO, both(sub_field("type", 2), sub_field("order", 5)), 0, "order"),
    ("order_over_the_partition", M.shape(256, 1, 16), both(sub_field("partition_order", 6), sub_field("n_partitions", 64),
                                                            sub_field("part_len", 4), sub_field("order", 8)), 0, "order"),
    ("precision_zero", STEREO, sub_field("precision", 0), 0, "precision"),
    ("precision", STEREO, sub_field("precision", 16), 0, "precision"),
    ("shift", STEREO, sub_field("shift", 16), 0, "shift"),
    ("coefficient", STEREO, coef_at(1, 2048), 0, "coeffs"),
    ("coding_method", STEREO, sub_field("coding_method", 2), 0, "coding_method"),
    ("rice_method_0", STEREO, rice_at(2, 15), 0, "rice"),
    ("rice_method_1", STEREO, both(sub_field("coding_method", 1), rice_at(3, 31)), 0, "rice"),
    ("escape_bits", STEREO, rice_at(1, 0xFF, 32), 0, "escape_bits"),
    ("partition_order", STEREO, both(sub_field("partition_order", 7), sub_field("n_partitions", 128), sub_field("part_len", 32)), 0,
     "partition_order"),
    ("n_partitions", STEREO, sub_field("n_partitions", 8), 0, "n_partitions"),
    ("part_len", STEREO, sub_field("part_len", 1023), 0, "part_len"),
    ("body_bits", STEREO, frame_field("body_bits", 1), 2, "body_bits"),
]


@pytest.mark.parametrize("name,sh,change,subframe,field", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_one_field_out_of_range_is_named(name, sh, change, subframe, field):
    plans, subs = good(sh)
    change(plans, subs, sh)
    assert check_plans(sh, 2, plans, subs) == (1, subframe, field)


def test_the_contexts_max_partition_order():
    """partition order 2 on a context created with max_partition_order 2, 1 and 8 (the effective order is capped at 6)"""
    plans, subs = good(STEREO)
    assert check_plans(STEREO, 2, plans, subs, po=2) is None
    assert check_plans(STEREO, 2, plans, subs, po=1) == (0, 0, "partition_order")
    assert check_plans(STEREO, 2, plans, subs, po=8) is None
    for f in (0, 1):
        subs[2 * f].partition_order, subs[2 * f].n_partitions, subs[2 * f].part_len = 7, 128, 32
    assert check_plans(STEREO, 2, plans, subs, po=8) == (0, 0, "partition_order")


def test_the_largest_rice2_parameter_and_escape_width():
    plans, subs = good(STEREO)
    subs[2].coding_method = 1
    subs[2].rice[0] = 30
    subs[2].rice[1], subs[2].escape_bits[1] = 0xFF, 31
    assert check_plans(STEREO, 2, plans, subs) is None


def test_the_last_frame_has_the_batchs_last_length():
    from test_route_table import hook_input

    sh = MONO_SHORT
    plans, subs = good(sh, 2, last_len=1000)
    row = dict(M.route_inputs(sh, 2), short_last=152)
    assert hook_input(row)[8] == 1000
    # (through the hook's own row: the last frame is 1000 samples long, and goes to the generic packer)
    import ctypes as C

    from flac_codec_amd import _lib

    L = _lib.lib()
    out, field = (C.c_uint32 * 3)(), C.create_string_buffer(64)
    vin = (C.c_int32 * 18)(*hook_input(row))
    assert L.flacenc_check_plans_row(vin, 1 << 40, plans, subs, out, field, 64) == 0
    plans[1].block_size = 1152
    assert L.flacenc_check_plans_row(vin, 1 << 40, plans, subs, out, field, 64) == 1 and (out[0], field.value) == (1, b"block_size")


@pytest.mark.parametrize("sh", [M.shape(4096, 2, 24), M.shape(4096, 2, 24, exhaustive=0), M.shape(1024, 2, 16), M.shape(1024, 2, 16, exhaustive=0)],
                         ids=M.shape_id)
def test_the_image_bound_of_both_stereo_images(sh):
    """A frame may declare the body its launch's image holds under the longest header, and not one bit more.  The image of
    the exhaustive channel choice is the smaller one (two VERBATIM subframes of the stream's width)."""
    words = M.fb_words_exhaustive_stereo(sh.bps, sh.block) if sh.exhaustive else M.fb_words(2, sh.bps, sh.block)
    top = (words - 2) * 32 - 18 * 8
    assert top == M.max_body_bits(sh) and top >= 2 * (8 + sh.block * sh.bps)          # ... which holds whatever the encoder decides
    assert M.fb_words_exhaustive_stereo(sh.bps, sh.block) < M.fb_words(2, sh.bps, sh.block)
    for over in (0, 1):
        plans, subs = good(sh)
        subs[2].bits += top + over - plans[1].body_bits
        plans[1].body_bits = top + over
        assert check_plans(sh, 2, plans, subs) == ((1, 2, "body_bits over the image") if over else None)


def test_the_crc_rows_bound_where_it_is_the_smaller():
    sh = M.shape(4096, 1, 25)                                       # one wave: 3 * 17 * 64 words, less than the image
    top = 8 * (4 * 3 * 17 * 64 + 3 - 16)
    assert top == M.max_body_bits(sh) < (M.image_words(sh) - 2) * 32 - 18 * 8
    for over in (0, 1):
        plans, subs = good(sh)
        subs[1].bits += top + over - plans[1].body_bits
        plans[1].body_bits = top + over
        assert check_plans(sh, 2, plans, subs) == ((1, 1, "body_bits over the CRC rows") if over else None)


def test_a_subframe_of_the_subframe_kernel_and_of_the_generic_packer():
    plans, subs = good(EIGHT)                                        # k_sub64: a subframe's image holds its VERBATIM form
    for over in (0, 1):
        subs[8].bits = 8 + 4096 * 16 + over
        plans[1].body_bits = sum(subs[8 + c].bits for c in range(8))
        assert check_plans(EIGHT, 2, plans, subs) == ((1, 0, "bits") if over else None)
    sh = M.shape(4608, 1, 16)                                        # no wave block length: k_pack's bit string
    plans, subs = good(sh)
    for over in (0, 1):
        subs[1].bits = 40 + 33 * 4608 + over
        plans[1].body_bits = subs[1].bits
        assert check_plans(sh, 2, plans, subs) == ((1, 0, "bits") if over else None)


def test_the_output_buffer():
    plans, subs = good(STEREO)
    total = sum(16 + (plans[f].body_bits + 7) // 8 + 2 for f in range(2))
    assert check_plans(STEREO, 2, plans, subs, out_cap=total) is None
    assert check_plans(STEREO, 2, plans, subs, out_cap=total - 1) == (1, 2, "total bytes")
