#!/usr/bin/env python3
"""Random fixed-length crops of FLAC files on the GPU: the files are scanned once and stay compressed in device
memory; every round draws one crop per file at a random position and decodes only the frames it touches, straight into
a [files, channels, samples] float32 tensor of samples in [-1, 1).

    python examples/flac_crops.py [--seconds 5] [--rounds 20] [--seed 0] a.flac b.flac ...

Prints the time of the scan and of the rounds.  A file shorter than the crop gives a zero-padded row (the valid length
is in the round's results).
"""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    import torch

    torch.cuda.init()   # torch's HIP runtime first
    from flac_codec_amd.gpu import Decoder, decode_windows

    blobs = []
    for p in args.files:
        with open(p, "rb") as f:
            blobs.append(f.read())
    dec = Decoder()
    t0 = time.perf_counter()
    recs, _ = dec.scan(blobs)
    print(f"scan: {len(blobs)} files, {sum(len(b) for b in blobs)} bytes, {time.perf_counter() - t0:.3f} s")
    good = [i for i in range(len(blobs)) if recs[i].rc == 0]
    for i in set(range(len(blobs))) - set(good):
        print(f"{args.files[i]}: not a FLAC stream, skipped")
    if not good:
        return 1
    length = {i: int(args.seconds * recs[i].info.sample_rate) for i in good}
    pad_to = max(length.values())
    rng = random.Random(args.seed)
    times, bad = [], 0
    for _ in range(args.rounds):
        windows = [(i, rng.randint(0, max(recs[i].info.decoded_samples - length[i], 0)), length[i]) for i in good]
        t0 = time.perf_counter()
        batch, results = decode_windows(dec, recs, windows, dtype="float32", out="device", pad_to=pad_to)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        bad += sum(r.bad_frames + r.bad_crc16 for r in results)
    dec.close()
    times.sort()
    print(f"{args.rounds} rounds of {tuple(batch.shape)} float32 crops: median {times[len(times) // 2] * 1e3:.2f} ms, "
          f"min {times[0] * 1e3:.2f} ms, max {times[-1] * 1e3:.2f} ms; {bad} bad frames")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
