#!/usr/bin/env python3
"""A batch of audio in device memory -> a shard of .flac files in device memory -> the batch again, with no host copy
in either direction: BatchEncoder.encode_device(out="device") leaves every finished file in a slot of one uint8 tensor
on the GPU and returns views of them, and decode_many takes those views where they lie.  Only frame sizes, digests and
the streams' headers cross the link on the way in, and the scan's records on the way out.

    python examples/batch2shard.py [--streams 8] [--seconds 2.0] [--rate 44100]

The views are what a caller keeps as a compressed shard in HBM, gathers over RCCL, or hands to Decoder.scan and
decode_windows for random crops (examples/flac_device_shard.py).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rate", type=int, default=44100)
    args = ap.parse_args()
    import torch

    torch.cuda.init()   # torch's HIP runtime first
    from flac_codec_amd.encode import BatchEncoder, Options
    from flac_codec_amd.gpu import decode_many

    # ---- the batch: float32 [B, C, T] on the GPU, every stream of its own length
    T = int(args.seconds * args.rate)
    t = torch.arange(T, device="cuda", dtype=torch.float32)
    k = torch.arange(1, args.streams + 1, device="cuda", dtype=torch.float32)[:, None]
    left = 0.4 * torch.sin(t[None, :] * 0.01 * k) + 0.05 * torch.sin(t[None, :] * 0.37)
    batch = torch.stack([left, 0.7 * left + 0.02 * torch.cos(t[None, :] * 0.11 * k)], 1).contiguous()
    lengths = [T - 97 * i for i in range(args.streams)]

    # ---- encode: the files stay on the GPU
    enc = BatchEncoder(Options.default())
    views = enc.encode_device(batch, lengths, sample_rate=args.rate, bits_per_sample=16, out="device")
    assert all(v.is_cuda for v in views) and enc.last_status == [0] * args.streams
    coded = sum(v.numel() for v in views)
    print(f"{args.streams} streams, {sum(lengths) * 2} samples -> {coded} bytes of .flac in device memory "
          f"({coded / (sum(lengths) * 4):.2f} of 16-bit PCM)")
    shard = torch.cat(views)   # a tight shard and its index, if the slots' gaps are unwanted
    index, at = [], 0
    for v in views:
        index.append((at, v.numel()))
        at += v.numel()

    # ---- decode them where they lie, MD5 checked on the device
    back, streams = decode_many([shard[o:o + n] for o, n in index], out="device", dtype="float32", layout="padded", pad_to=T)
    ok = True
    for i, (s, n) in enumerate(zip(streams, lengths)):
        want = torch.clamp(torch.round(batch[i, :, :n] * 32768.0), -32768, 32767) / 32768.0   # the encoder's quantisation
        ok &= s.rc == 0 and s.info.md5_status == 1 and bool(torch.equal(back[i, :, :n], want))
    print("decoded on the device:", "the quantised batch, every MD5 good" if ok else "DIFFERENT samples")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
