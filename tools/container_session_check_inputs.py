#!/usr/bin/env python3
"""Writes the INPUTS file of tools/container_session_check.cpp: .flac streams back to back, each a 32-bit little-endian
length and that many bytes.  The streams are the tests' own, fixed by their seeds: the metadata walk's edge cases and
every 5th truncation (tests/_meta_cases.py), every 9th damaged stream of the scan's tests (tests/_scan_model.py) and every
8th valid stream of the foreign matrix (tests/_foreign_matrix.py).

    python tools/container_session_check_inputs.py INPUTS
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def streams():
    import _meta_cases as mc
    import _scan_model as scm

    out = [blob for _, blob in mc.edges() + mc.truncations()[::5]]
    out += [blob for _, blob in scm.damaged_cases()[::9]]
    out += [blob for _, blob in mc.foreign()[::8]]
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
