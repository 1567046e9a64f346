"""The input schedule of k_autocorr4 (kernels/shape.h: ac4_fetch_slot, ac4_fetch_next), compiled into a host program
(tools/ac4_fetch_rule_check.cpp) and walked for every tile: each tile is converted exactly once, out of the staging set its
own loads went to, nothing is requested over a set that still holds an unconverted tile, and no request leaves the frame."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ac4_fetch_rule_check.cpp")
INC = os.path.join(ROOT, "flac-codec_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ac4rule") / "ac4_fetch_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", INC, "-o", exe, SRC])
    return exe


def trace(program, ntiles, depth=None):
    args = [program, str(ntiles)] + ([str(depth)] if depth else [])
    lines = subprocess.check_output(args, text=True).split("\n")
    ev = [tuple([l.split()[0]] + [int(x) for x in l.split()[1:]]) for l in lines if l]
    assert ev[0][0] == "D"
    return ev[0][1], ev[1:]


def check(ev, ntiles, depth):
    held = {}           # set -> (index, tile, converted)
    converted = {}      # tile index -> times
    for e in ev:
        if e[0] == "R":
            _, idx, tile, s = e
            assert tile <= ntiles - 1, f"request {idx} reads tile {tile} past the frame's {ntiles} tiles"
            assert tile == min(idx, ntiles - 1)
            assert s < depth
            if s in held:
                h_idx, _, done = held[s]
                # a set is refilled only behind the conversion of what it held (a clamped repeat may be dropped)
                assert done or h_idx >= ntiles, f"request {idx} overwrites set {s} with tile {h_idx} unconverted"
            held[s] = (idx, tile, False)
        else:
            _, idx, s = e
            assert s in held, f"conversion of tile {idx} reads set {s}, which nothing was requested into"
            h_idx, h_tile, done = held[s]
            assert not done, f"tile {idx}: set {s} was converted already"
            assert h_idx == idx, f"tile {idx} converted from set {s}, which holds the loads of tile {h_idx}"
            if idx < ntiles:
                assert h_tile == idx
            else:
                assert h_tile == ntiles - 1     # the repeat behind the frame's end: the last tile again, read by nobody
            held[s] = (h_idx, h_tile, True)
            converted[idx] = converted.get(idx, 0) + 1
    for t in range(ntiles):
        assert converted.get(t, 0) == 1, f"tile {t} converted {converted.get(t, 0)} times"
    assert all(t <= ntiles for t in converted), "only ONE repeat behind the last tile (it fills the idle buffer)"


@pytest.mark.parametrize("ntiles", [1, 2, 3, 4, 128])
def test_the_librarys_depth(program, ntiles):
    depth, ev = trace(program, ntiles)
    assert depth in (1, 2)
    check(ev, ntiles, depth)


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("ntiles", [1, 2, 3, 4, 128])
def test_both_depths(program, ntiles, depth):
    d, ev = trace(program, ntiles, depth)
    assert d == depth
    check(ev, ntiles, depth)
    # tile t + 1 is requested `depth` tiles before the tile that converts it
    req_at = {}
    step = 0
    for e in ev:
        if e[0] == "C":
            step += 1          # conversions number the steps: C 0 before the loop, C t + 1 inside tile t
            if e[1] >= depth + 1:
                assert step - req_at[e[1]] == depth
        else:
            req_at.setdefault(e[1], step)


def test_the_check_sees_a_wrong_set(program):
    _, ev = trace(program, 4, 2)
    bad = [(("C", e[1], 1 - e[2]) if e[0] == "C" and e[1] == 2 else e) for e in ev]
    with pytest.raises(AssertionError):
        check(bad, 4, 2)
