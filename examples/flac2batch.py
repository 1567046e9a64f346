#!/usr/bin/env python3
"""FLAC files to one padded float32 batch on the GPU: every file decoded in one call straight into a
[files, channels, samples] tensor of samples in [-1, 1), zero-padded to the longest file, saved as .npy.

    python examples/flac2batch.py out.npy a.flac b.flac ...

Prints one line per file: its length in samples (the batch's lengths vector) and the MD5 verdict.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flac_codec_amd.gpu import decode_many  # noqa: E402


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    out, paths = argv[1], argv[2:]
    blobs = []
    for p in paths:
        with open(p, "rb") as f:
            blobs.append(f.read())
    batch, streams = decode_many(blobs, out="host", dtype="float32", layout="padded")
    np.save(out, batch)
    verdict = {0: "MD5 mismatch", 1: "ok", 2: "ok - no MD5"}
    bad = 0
    for p, s in zip(paths, streams):
        clean = s.rc == 0 and not s.info.bad_frames and not s.info.bad_crc16 and s.info.md5_status != 0
        bad += not clean
        what = verdict[s.info.md5_status] if clean or s.rc == 0 and s.info.md5_status == 0 else "error"
        print(f"{p}: {s.info.decoded_samples} samples x {s.info.channels} channels, {what}")
    print(f"{out}: {batch.shape} float32")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
