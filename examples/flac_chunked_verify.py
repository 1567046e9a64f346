#!/usr/bin/env python3
"""`flac -t` for files read in pieces: every file is read --chunk bytes at a time, the pieces of all files go through ONE
container session together (gpu.DecoderSession(container=True): the metadata walked across feeds, frames decided as the
bytes arrive, every feed's samples decoded and hashed on the GPU), and the verdict is what the one-shot decode of the
whole file gives -- without any file ever being held whole.

    python examples/flac_chunked_verify.py [--chunk 65536] [--max-frame-bytes 1048576] FILE.flac [FILE.flac ...]

Prints one line per file, as `flac -t` does: "FILE: ok" (the decoded PCM has STREAMINFO's MD5), "ok, no MD5 in
STREAMINFO", or what is wrong.  Exit status 1 when a file is not ok.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def verdict_line(v, skipped):
    info = v.info
    if v.rc:
        return False, "ERROR, not a FLAC stream or no usable STREAMINFO"
    problems = []
    if info.bad_frames:
        problems.append(f"lost synchronisation or a frame that does not parse behind frame {info.frames - 1} "
                        f"({skipped} bytes not decoded)" if skipped else f"{info.bad_frames} frames that do not parse")
    if info.bad_crc16:
        problems.append(f"{info.bad_crc16} frames with a wrong CRC-16")
    if info.total_samples and info.total_samples != info.decoded_samples:
        problems.append(f"{info.decoded_samples} samples decoded, STREAMINFO says {info.total_samples}")
    if info.md5_status == 0:
        problems.append("MD5 mismatch")
    if problems:
        return False, "ERROR, " + "; ".join(problems)
    what = {1: "ok", 2: "ok, no MD5 in STREAMINFO", 3: "decoded, MD5 not taken"}[info.md5_status]
    return True, f"{what} ({info.frames} frames, {info.decoded_samples} samples, {info.channels} ch, {info.bits_per_sample} bit)"


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="+")
    ap.add_argument("--chunk", type=int, default=65536, help="bytes read from every file per feed")
    ap.add_argument("--max-frame-bytes", type=int, default=1 << 20, help="no frame is longer (16 .. 2^22)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv[1:])
    if args.chunk < 1:
        ap.error("--chunk must be at least 1")

    import torch

    torch.cuda.init()   # torch's HIP runtime first, as in decode_many
    from flac_codec_amd import gpu

    handles = [open(name, "rb") for name in args.files]
    session = gpu.DecoderSession(len(handles), args.max_frame_bytes, device=args.device, container=True)
    try:
        open_files = len(handles)
        while open_files:
            chunks = [f.read(args.chunk) if f else b"" for f in handles]
            for k, c in enumerate(chunks):
                if handles[k] and not c:   # end of file
                    handles[k].close()
                    handles[k] = None
                    open_files -= 1
            session.feed(chunks)
            session.decode(out="device")   # decodes this feed's frames and hashes them into the files' MD5 chains
        _, raw = session.finish()
        session.decode(out="device")
        verdicts = session.verdict()
    finally:
        session.close()
        for f in handles:
            if f:
                f.close()
    ok = True
    for name, v, r in zip(args.files, verdicts, raw):
        good, line = verdict_line(v, int(r.skipped_bytes))
        ok &= good
        print(f"{name}: {line}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
