"""tests/_frame64_edge_matrix.py proven without a device: the two references agree on every frame, every case is FLAC the
oracle decodes back to its PCM, the geometry record reproduces every frame, the matrix reaches every class it names,
every case is a plan flacgpu_pack_plans takes (host/plan_check.cpp), and every shape's batch goes to the k_frame64
instantiation it declares."""
import ctypes as C

import numpy as np
import pytest

import _flacsyn as fs
import _frame64_edge_matrix as M
import _oracle as orc
from test_route_table import hook_input, route

SHAPES = M.shapes()


def check_plans(sh, n_frames, plans, subs, out_cap=1 << 40, knobs=1, po=6):
    """flacenc_check_plans_row: None, or (frame, subframe, field)"""
    from flac_codec_amd import _lib
    from flac_codec_amd._lib import FramePlan, SubframePlan

    L = _lib.lib()
    L.flacenc_check_plans_row.restype = C.c_int
    L.flacenc_check_plans_row.argtypes = [C.POINTER(C.c_int32), C.c_uint64, C.POINTER(FramePlan), C.POINTER(SubframePlan),
                                          C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    vin = (C.c_int32 * 18)(*hook_input(M.route_inputs(sh, n_frames, knobs, po)))
    out = (C.c_uint32 * 3)()
    field = C.create_string_buffer(64)
    if not L.flacenc_check_plans_row(vin, out_cap, plans, subs, out, field, 64):
        return None
    assert out[2] == M.image_words(sh), "the model's image is not the library's"
    return out[0], out[1], field.value.decode()


@pytest.mark.parametrize("sh", SHAPES, ids=M.shape_id)
def test_both_references_agree_and_the_model_holds(sh):
    from flac_codec_amd.gpu import host_pack_frames

    b = M.batch_of(sh)
    want, want_off = M.batch_bytes(b)
    plans, subs, rows = M.plan_arrays(b)
    n = len(want_off) - 1
    data, off = host_pack_frames(sh.rate, sh.bps, sh.C, sh.first, n, sh.block, plans, subs, rows)
    assert list(off) == want_off, "the host packer's offsets are not the Python writer's"
    for f, (bt, i) in enumerate(M.batch_frames(b)):
        assert bytes(data[off[f]:off[f + 1]]) == bt.recs[i].data, (bt.case.name, i, "the two references differ")
        M.self_check(bt.recs[i])
    # a plan flacgpu_pack_plans takes, on the kernel the shape declares
    assert check_plans(sh, n, plans, subs) is None
    r = route(M.route_inputs(sh, n))
    assert r[3] == n, (sh, r, "not every frame goes to the wave assembly kernel")
    assert route(M.route_inputs(sh, n, knobs=1 | 8))[3] == 0         # ... and FLACGPU_NO_FRAME64 sends every one to the generic packer
    if sh in M.parity_shapes():                                      # ... whose LDS bit string holds every subframe of the parity run
        assert check_plans(sh, n, plans, subs, knobs=1 | 8) is None


@pytest.mark.parametrize("sh", SHAPES, ids=M.shape_id)
def test_every_case_is_flac(sh):
    for bt in M.batch_of(sh).built:
        st = fs.write_stream(sh.rate, sh.bps, bt.frames)
        assert st.frame_bytes == [r.data for r in bt.recs]
        rc, pcm, info = orc.decode_stream(st.blob)
        assert rc == 0 and info.md5_ok == 1 and np.array_equal(pcm, st.pcm), (bt.case.name, rc)


def test_every_required_class_is_reached():
    n = M.reached(M.batches())
    missing = [c for c in M.REQUIRED if not n[c]]
    assert not missing, missing
    assert len(set(M.REQUIRED)) == len(M.REQUIRED)
    # classes that cannot exist
    # S == 0: the whole words in front of the CRC-16 are never none -- the shortest frame (one CONSTANT channel of at most 8 bits) is
    # 6 header bytes + 2 + 2, so nw4 >= 2
    assert min(bt.recs[i].geo.flen for b in M.batches() for bt, i in M.batch_frames(b)) == 10 == 6 + (8 + 8 + 7) // 8 + 2
    assert not any(k.startswith("d_") and "_S0_" in k for k in n)
    # a one-bit field (k = 0) has no bit to leave in the word before: it never straddles
    assert n["a_w1_straddle"] == 0 and "a_w1_straddle" not in M.REQUIRED
    # all 24 instantiations launch_frame64 reaches without Params::inter, every one declared by a case
    inst = {k for k in n if k.startswith("i_")}
    assert inst == {"i_%d_%d_%d" % (64 * c, spl, maxo) for c in (1, 2, 3, 4) for spl, maxo in ((16, 16), (18, 16), (32, 16), (36, 16), (64, 16), (64, 32))}
    assert len(inst) == 24


@pytest.mark.parametrize("sh", [s for s in SHAPES if s.rate == 44100 and s.block in (4096, 1152)], ids=M.shape_id)
def test_the_model_states_the_librarys_bound(sh):
    """max_body_bits() is kernels/shape.h frame_fb_max_body_bits and the three CRC rows: one bit more is refused."""
    from flac_codec_amd._lib import FramePlan, SubframePlan

    plans, subs = (FramePlan * 1)(), (SubframePlan * sh.C)()
    plans[0].channels, plans[0].block_size = sh.C, sh.block
    for over in (0, 1):
        body = M.max_body_bits(sh) + over
        plans[0].body_bits = body
        for c in range(sh.C):
            subs[c].type, subs[c].bps, subs[c].source = 1, sh.bps, c
            subs[c].bits = body - (sh.C - 1) * (8 + sh.bps) if c == 0 else 8 + sh.bps
        got = check_plans(sh, 1, plans, subs)
        assert (got is None) == (over == 0), (sh, body, got)
        if over:
            assert got[:2] == (0, sh.C) and got[2].startswith("body_bits over"), got
