"""The encoder's route decision (csrc/host/batch_route.cpp plan_route, through the flacenc_plan_route_row hook): which input path,
which frames on the wave kernels, K4 fused or not, range cutting, two ranges, host output.  CPU-only.

tests/golden/route_table.txt was written (python tests/test_route_table.py --write) when plan_route still held the dispatcher's
former inline expressions moved over verbatim; every later form of the function must reproduce it exactly.

THE SAMPLING RULE.  The axes' cross product has 10^9 rows; the table holds
  * SWEEPS: from each base row of BASES, every axis in turn run through all of its values, the others held; and
  * 700 SEEDED rows: a 64-bit LCG (seed 0x5EED) draws every axis, in AXES' order -- one draw decides whether the axis keeps the
    value of the base row (BASES[row number % len(BASES)]; two draws in three) or takes the value a second draw picks.
Both are functions of this file alone.  The properties below are what used to be the dispatcher's "internal:" run-time errors."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flac-codec_amd", "csrc", "host")
TABLE = os.path.join(ROOT, "tests", "golden", "route_table.txt")

K0_COPY, K0_PACKED, PLANAR_IN_PLACE, DIRECT_STEREO, SPLIT, SPLIT_XPOSE = range(6)
IN_PLACE = (DIRECT_STEREO, SPLIT, SPLIT_XPOSE)
KNOBS = {"default": 0, "no_direct": 1, "no_w64": 2, "no_fused_pack": 4, "no_frame64": 8, "no_direct_short": 16, "no_xpose": 32,
         "no_hand": 64, "experiment_mfma_ac": 128}

# (name, values); last_len is 0 for "the block size" and 1 for "one sample short"; chunk is FLACGPU_TUNE_CHUNK_MSAMPLES, -1: unset
AXES = [
    ("channels", [1, 2, 3, 4, 5, 6, 7, 8]),
    ("bps", [8, 16, 20, 24, 25, 26, 32]),
    ("block", [4096, 2304, 2048, 1152, 1024, 4608, 576, 16384]),
    ("order", [0, 8, 16, 17, 32]),
    ("po", [0, 6, 8]),
    ("exhaustive", [1, 0]),
    ("layout", [0, 1]),
    ("aligned", [1, 0]),
    ("short_last", [0, 1]),
    ("n_frames", [1, 2, 300, 1500]),
    ("packed", [0, 2, 3]),
    ("lag_split", [4, 2]),
    ("timing", [0, 1]),
    ("segments", [0, 1]),
    ("knobs", list(KNOBS.values())),
    ("chunk", [-1, 0, 4]),
    ("two_ranges", [0, 1]),
    ("whole_call", [0, 1]),
]
NAMES = [a for a, _ in AXES]


def base(**kw):
    row = dict(channels=2, bps=24, block=4096, order=8, po=6, exhaustive=1, layout=0, aligned=1, short_last=0, n_frames=1500,
               packed=0, lag_split=4, timing=0, segments=0, knobs=0, chunk=4, two_ranges=0, whole_call=1)
    row.update(kw)
    return row


BASES = [
    base(),                                          # stereo read in place, cut into ranges
    base(channels=4),                                # independent channels read in place by every stage
    base(channels=8, bps=16),                        # ... assembled by the subframe kernel
    base(channels=5, chunk=-1),                      # ... with the planar rows kept
    base(channels=1, whole_call=0),                  # one channel: its own planar row
    base(two_ranges=1, chunk=-1),                    # the two-stream branch
    base(whole_call=0, segments=1, n_frames=300),    # device segments that want to stay where they are
    base(whole_call=0, block=1152, n_frames=2),      # a short wave block length
    base(whole_call=0, packed=3, n_frames=300),      # stream-width upload
]


def rows():
    out = []
    for b in BASES:
        out.append(dict(b))
        for name, values in AXES:
            for v in values:
                if v != b[name]:
                    out.append(dict(b, **{name: v}))
    state = 0x5EED

    def draw(n):
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (state >> 33) % n

    for i in range(700):
        b = BASES[i % len(BASES)]
        row = {}
        for name, values in AXES:
            keep = draw(3) != 0
            pick = values[draw(len(values))]
            row[name] = b[name] if keep else pick
        out.append(row)
    return out


def hook_input(row):
    last = row["block"] - row["short_last"]
    return [row["channels"], row["bps"], row["block"], row["order"], row["po"], row["exhaustive"], row["layout"], row["aligned"],
            last, row["n_frames"], row["packed"], row["lag_split"], row["timing"], row["segments"], row["knobs"], row["chunk"],
            row["two_ranges"], row["whole_call"]]


def route(row):
    from flac_codec_amd import _lib

    L = _lib.lib()
    L.flacenc_plan_route_row.restype = None
    L.flacenc_plan_route_row.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    vin = (C.c_int32 * 18)(*hook_input(row))
    vout = (C.c_uint32 * 9)()
    L.flacenc_plan_route_row(vin, vout)
    return list(vout)


def line(row, out):
    return ",".join(str(v) for v in hook_input(row)) + " " + ",".join(str(v) for v in out)


@pytest.fixture(scope="module")
def table():
    rs = rows()
    return rs, [route(r) for r in rs]


def test_every_axis_value_is_sampled():
    rs = rows()
    for name, values in AXES:
        assert {r[name] for r in rs} == set(values), name
    assert len({tuple(hook_input(r)) for r in rs}) > 1000


def test_table_is_reproduced_exactly(table):
    rs, outs = table
    with open(TABLE) as f:
        want = f.read().splitlines()
    got = [line(r, o) for r, o in zip(rs, outs)]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "row %d" % i
    assert os.path.getsize(TABLE) < 100 * 1024


def test_every_kind_of_route_is_reached(table):
    _, outs = table
    assert {o[0] for o in outs} == set(range(6))
    assert any(o[5] for o in outs) and any(o[6] for o in outs) and any(o[1] for o in outs) and any(o[8] for o in outs)
    assert any(o[4] for o in outs) and any(not o[4] for o in outs) and any(o[7] for o in outs)
    assert any(0 < o[2] < r["n_frames"] for r, o in zip(*table[:2])) and any(o[2] == 0 for o in outs)


def test_former_internal_errors_hold_as_properties(table):
    for r, o in zip(*table):
        inp, hand, fast_a, fast_p, k4, rng, two, host_out, seg_in_place = o
        n = r["n_frames"]
        if rng:      # a ranged batch: every frame on the in-place wave kernels, K4 inside the autocorrelation kernel
            assert inp in IN_PLACE and fast_a == n and fast_p == n and k4, r
            assert not two and r["whole_call"]
        if inp == SPLIT_XPOSE:   # nobody writes the planar rows: no frame may go to the generic packer, which reads them
            assert fast_p == n, r
        if seg_in_place:         # an in-place announcement never comes with a copying route
            assert r["segments"] and inp in IN_PLACE and r["channels"] >= 2, r
        if r["segments"] and inp in IN_PLACE and r["channels"] >= 2:
            assert seg_in_place, r    # ... and whatever can stay in place is granted; anything else is "gather"
        if two:
            assert fast_a == n and fast_p == n and r["whole_call"] and r["two_ranges"], r
            assert inp in (K0_COPY, PLANAR_IN_PLACE) and not hand and not k4
        if hand:
            assert inp == DIRECT_STEREO and r["block"] == 4096 and r["order"] > 0, r
        if host_out:
            assert fast_p == n
        assert fast_a in (0, n - 1, n) and fast_p in (0, n - 1, n)


def test_under_address_sanitizer(tmp_path, table):
    """tools/route_table_check.cpp + batch_route.cpp, a stand-alone program built with ASan and UBSan, walks the same rows."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + san + [str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")], capture_output=True,
                           text=True)
    if probe.returncode:
        pytest.skip("the sanitizer runtime cannot be linked here: " + (probe.stderr.strip().splitlines() or ["?"])[-1])
    exe = tmp_path / "route_table_check"
    made = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + san + [
        "-I" + HOST, os.path.join(ROOT, "tools", "route_table_check.cpp"), os.path.join(HOST, "batch_route.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    rs, outs = table
    (tmp_path / "rows.txt").write_text("".join(" ".join(str(v) for v in hook_input(r)) + "\n" for r in rs))
    run = subprocess.run([str(exe), str(tmp_path / "rows.txt")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines() == [" ".join(str(v) for v in o) for o in outs]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_route_table.py --write   (only when the table's ROWS change, never its routes)")
    sys.path.insert(0, ROOT)
    with open(TABLE, "w") as f:
        for r in rows():
            f.write(line(r, route(r)) + "\n")
