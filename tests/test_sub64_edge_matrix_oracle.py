"""tests/_sub64_edge_matrix.py on the CPU: the model of k_sub64's bit geometry reproduces the CRC-16 and the edge words of
every frame of the matrix (the oracle's frames; the host packer's for hand-built plans), every class the matrix names is
reached, and the hand-built frames decode back to their PCM with the oracle's decoder.  No GPU call."""
import numpy as np
import pytest

import _oracle as orc
import _sub64_edge_matrix as M


@pytest.mark.parametrize("cls", "abcdefgh")
def test_model_reproduces_crc_and_edge_words(cls):
    checked = 0
    for case in M.cases():
        if case.cls != cls:
            continue
        for f, ((data, _, _), geo) in enumerate(zip(M.encoded(case), M.geometries(case))):
            try:
                M.self_check(data, geo)
            except AssertionError:
                print(M.describe(case, f))
                raise
            checked += 1
    assert checked > 0


def test_every_class_is_reached():
    n = M.reached(M.cases())
    for name in M.REQUIRED:
        print("%-44s %d" % (name, n[name]))
    missing = [name for name in M.REQUIRED if n[name] == 0]
    assert not missing, missing


def test_the_issue_table_holds():
    """The four rows the work was planned from, read off the model."""
    by = {c.name: c for c in M.cases()}
    g = M.geometries(by["one_loud_seven_silent_b4@0"])[1]
    assert g.hbytes == 6 and g.begin & 3 == 0
    s2, s3, s4 = g.subs[2:5]
    assert (s2.nw, s3.nw, s4.nw) == (1, 1, 2) and (s2.lead, s3.lead, s4.lead) == (4, 16, 28) and s2.w0 == s3.w0 == s4.w0
    assert g.words[s2.w0] == ["tail1", "head2", "head3", "head4"]
    g = M.geometries(by["one_loud_seven_silent_b4@1"])[1]
    assert g.subs[6].img_end > g.crc_at and (g.subs[7].nw4, g.subs[7].S) == (0, 0)
    for C_ in (5, 8):
        got = {}
        for k in range(4):
            g = M.geometries(by["noise17_c%d@%d" % (C_, k)])[1]
            assert g.begin & 3 == k
            got[k] = (g.subs[-1].nw4, g.subs[-1].S, g.subs[-1].padw)
        assert sorted(got.values()) == [(2176, 2, 0)] * 3 + [(2177, 3, 1087)], got     # (which alignment: 2 at 8 channels, 1 at 5)
    lens, nws = set(), set()
    for k in range(4):
        g = M.geometries(by["five_silent_of_seven_b16@%d" % k])[1]
        nws.add(g.subs[-1].nw)
        lens.add(g.subs[-1].len3)
    assert lens == {0, 1, 2, 3} and 1 in nws


def test_four_bit_cases_take_the_rows_route():
    """4-bit samples are below the transposing loads' width: k_sub64<64,16> on planar rows, every frame on the wave kernels"""
    from test_route_table import SPLIT, SPLIT_XPOSE, route

    seen = 0
    for case in M.cases():
        if case.plans is not None:
            continue
        r = route(M.route_inputs(case))
        assert r[3] == len(case.frames), case.name                     # every frame assembled by k_sub64
        if case.bps == 4 or case.C in (5, 7):
            assert r[0] == SPLIT, (case.name, r)
            seen += case.bps == 4
        else:
            assert r[0] == SPLIT_XPOSE, (case.name, r)
            assert route(M.route_inputs(case, knobs=32))[0] == SPLIT, case.name
    assert seen > 0


def streaminfo(case, total_samples):
    packed = (case.rate << 44) | ((case.C - 1) << 41) | ((case.bps - 1) << 36) | total_samples
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + (M.B).to_bytes(2, "big") * 2 + bytes(6) + packed.to_bytes(8, "big") + bytes(16)


def test_hand_built_frames_decode_to_their_pcm():
    seen = 0
    for case in M.cases():
        if case.plans is None:
            continue
        data, _ = M.batch_bytes(case)
        rc, out, info = orc.decode_stream(streaminfo(case, M.B * len(case.frames)) + data)
        assert rc == 0 and info.frames == len(case.frames), case.name
        assert np.array_equal(out, M.interleaved(case)), case.name
        seen += 1
    assert seen > 0
