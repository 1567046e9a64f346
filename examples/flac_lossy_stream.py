#!/usr/bin/env python3
"""Decode what is left of a FLAC file onto its timeline on the GPU: frames lost on the way, or only a byte range of the
file at hand, and the samples still stand at their right times, with zeros where nothing arrived.

    python examples/flac_lossy_stream.py --drop 7 a.flac                      every 7th frame removed
    python examples/flac_lossy_stream.py --offset 30000 --length 50000 a.flac   a byte range, cut anywhere

The frames are placed by the frame or sample numbers their headers carry, so the file's head is not needed.  Prints
where the decoded stretch sits in the file (in samples and seconds from the file's first sample), every gap in seconds,
and how much of the stretch holds decoded samples; --wav writes the stretch, zeros included, as a WAV file.  The frames
must carry their own sample rate and sample size ("subset" headers), as nearly every encoder writes them, and a stream of
fixed block size must keep that size up to its last frame.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--drop", type=int, default=0, help="remove every Nth frame of the file (N >= 2)")
    ap.add_argument("--offset", type=int, help="first byte of a range of the file")
    ap.add_argument("--length", type=int, help="bytes in the range")
    ap.add_argument("--speculative", action="store_true",
                    help="end a frame that no header ends by its own bits (a lost frame then costs that frame alone)")
    ap.add_argument("--wav", help="write the decoded stretch as a 16-bit WAV file")
    ap.add_argument("file")
    args = ap.parse_args()
    if (args.offset is None) != (args.length is None) or (args.drop and args.offset is not None) or args.drop == 1:
        ap.error("give --drop N (N >= 2), or --offset and --length, or neither")
    import numpy as np

    from flac_codec_amd.gpu import decode_timeline, scan_frames_host, scan_stream_host

    with open(args.file, "rb") as f:
        if args.offset is not None:
            f.seek(args.offset)
            data = f.read(args.length)
        else:
            whole = f.read()
            data = whole[int(scan_stream_host(whole)[1][0]):]   # the frames alone: a transport carries no file head
    if args.drop:
        frames = scan_frames_host(data)[0]
        data = b"".join(data[int(r["byte_offset"]):int(r["byte_offset"]) + int(r["bytes"])]
                        for k, r in enumerate(frames) if (k + 1) % args.drop)
        print(f"{len(frames) // args.drop} of {len(frames)} frames removed")
    batch, mask, results, _ = decode_timeline([data], dtype="float32", out="host", speculative=args.speculative)
    r = results[0]
    if r.rc:
        print("no timeline: no whole frame, frames of different formats, or frame numbers that do not count time")
        return 1
    rate = int(scan_frames_host(data, args.speculative)[0][0]["sample_rate"])
    first, n = r.first_sample, r.timeline_samples
    print(f"samples {first} .. {first + n} of the file ({first / rate:.3f} s .. {(first + n) / rate:.3f} s): "
          f"{r.placed} frames placed, {r.dropped} dropped, {r.concealed} did not decode")
    valid = mask[0, :n].astype(bool)
    edges = np.flatnonzero(np.diff(np.concatenate(([1], valid.astype(np.int8), [1]))))
    for a, b in zip(edges[::2], edges[1::2]):
        print(f"  nothing for {(b - a) / rate:.3f} s at {(first + a) / rate:.3f} s")
    print(f"{int(valid.sum())} of {n} samples decoded ({r.gaps} gaps of {r.gap_samples} samples in all)")
    if args.wav:
        import wave

        pcm = np.clip(np.rint(batch[0, :, :n].T * 32768.0), -32768, 32767).astype("<i2")
        with wave.open(args.wav, "wb") as w:
            w.setnchannels(pcm.shape[1])
            w.setsampwidth(2)
            w.setframerate(rate)
            w.writeframes(pcm.tobytes())
    return 0


if __name__ == "__main__":
    sys.exit(main())
