#!/usr/bin/env python3
"""Verify FLAC files on the GPU, like `flac -t file1.flac file2.flac ...`: every file in one batch (frames found,
decoded, CRC-16 and MD5 checked on the device), one line per file.

    python examples/flacverify.py a.flac b.flac ...
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flac_codec_amd.decode import Verified, verify_many  # noqa: E402


def line(path, result):
    if result is Verified.MD5_MATCH:
        return f"{path}: ok"
    if result is Verified.MD5_MISMATCH:
        return f"{path}: bad - MD5 mismatch"
    if result is Verified.NO_MD5:
        return f"{path}: ok - no MD5"
    return f"{path}: error - {result}"


def main(argv):
    paths = argv[1:]
    for p, r in zip(paths, verify_many(paths)):
        print(line(p, r))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
