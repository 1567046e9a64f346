#!/usr/bin/env python3
"""Decode the whole frames inside a byte range of a FLAC file on the GPU, without the file's head: the range may start
and end in the middle of a frame, as one fetched from a large file by an index of the caller's own does.

    python examples/flac_byte_range.py --offset 1000000 --length 65536 a.flac

Only the range is read from the file.  Prints every whole frame found in it -- where it starts in the file, the number
its header carries (a frame number, or a sample number for a variable-block-size stream) and the shape of its samples --
and how many bytes of the range belong to no whole frame.  The frames must carry their own sample rate and sample size
("subset" headers), as nearly every encoder writes them.  A frame is recognised by the header behind it, so the last whole
frame of the range is lost when less than a header of the next one follows; --speculative ends such a frame by its own
bits and keeps it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--offset", type=int, required=True, help="first byte of the range in the file")
    ap.add_argument("--length", type=int, required=True, help="bytes in the range")
    ap.add_argument("--speculative", action="store_true",
                    help="end a frame that no header ends by its own bits (keeps the range's last whole frame)")
    ap.add_argument("file")
    args = ap.parse_args()
    from flac_codec_amd.gpu import decode_frames

    with open(args.file, "rb") as f:
        f.seek(args.offset)
        data = f.read(args.length)
    samples, frames, raw = decode_frames([data], out="host", speculative=args.speculative)
    bad = 0
    for fr in frames:
        n, ch = int(fr["block_size"]), int(fr["channels"])
        pcm = samples[int(fr["out_offset"]):int(fr["out_offset"]) + n * ch].reshape(n, ch)
        what = "sample" if fr["blocking"] else "frame"
        state = "" if not fr["status"] else "  DOES NOT DECODE"
        if fr["reserved"] & 1:
            state += "  (ended by its own bits)"
        bad += bool(fr["status"])
        print(f"byte {args.offset + int(fr['byte_offset'])}: {what} number {int(fr['number'])}, {tuple(pcm.shape)} samples, "
              f"{int(fr['sample_rate'])} Hz, {int(fr['bits_per_sample'])} bits{state}")
    print(f"{raw[0].frames} whole frames in {len(data)} bytes; {raw[0].skipped_bytes} bytes in {raw[0].gaps} run(s) "
          f"belong to none")
    return 1 if bad or not raw[0].frames else 0


if __name__ == "__main__":
    sys.exit(main())
