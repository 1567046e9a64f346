#!/usr/bin/env python3
"""Writes the INPUTS file of tools/session_check.cpp: raw frame streams back to back, each a 32-bit little-endian length
and that many bytes.  The streams are the tests' own (tests/_raw_frames.py, tests/_session_model.py), fixed by their
seeds: every 97th input of the raw scan's tests (head cuts, tail cuts, single-byte flips, look-alike regions), the mixed
and the uniform stream, the look-alike stream of the session tests and three of the uniform set -- 30 streams.

    python tools/session_check_inputs.py INPUTS
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def streams():
    import _raw_frames as rf
    import _session_model as sm

    out = [blob for _, blob in rf.all_cases()[::97]]
    out += [rf.mixed().blob, rf.uniform().blob, sm.lookalike_stream()[0]]
    out += [raw.blob for raw, _ in rf.uniform_set()[:3]]
    return out


def main(argv):
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    blobs = streams()
    with open(argv[1], "wb") as f:
        for b in blobs:
            f.write(struct.pack("<I", len(b)) + b)
    print(f"{len(blobs)} streams, {sum(len(b) for b in blobs)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
