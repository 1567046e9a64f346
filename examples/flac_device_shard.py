#!/usr/bin/env python3
"""A dataset shard that lives in device memory: FLAC files packed into ONE uint8 tensor on the GPU plus an index --
what a rank receives over RCCL, or a shard file loaded straight onto the device -- scanned where it lies and cropped
from there.  The compressed bytes never travel back to the host: the scan gathers them on the device
(flacgpu_decoder_scan_device), and every step decodes only the frames its random crops touch.

    python examples/flac_device_shard.py [--seconds 1] [--steps 20] [--seed 0] a.flac b.flac ...

Then the round trip without a host copy: a few blocks of PCM in device memory are encoded (flacgpu_encode_device
leaves the frames in device memory), those frames are scanned as a raw frame stream where they lie, and decoded back
into device memory.
"""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class DeviceBytes:
    """`nbytes` of device memory at `ptr`, for torch.as_tensor: a view, no copy."""

    def __init__(self, ptr, nbytes, typestr="|u1", itemsize=1):
        self.__cuda_array_interface__ = {"shape": (nbytes // itemsize,), "typestr": typestr, "data": (ptr, False),
                                         "version": 2}


def round_trip(torch):
    import numpy as np

    from flac_codec_amd.gpu import Decoder, GpuAnalyzer, decode_frames

    block, frames, last, rate = 4096, 6, 1000, 44100
    samples = block * (frames - 1) + last
    t = torch.arange(samples, device="cuda", dtype=torch.float32)
    left = (8000 * torch.sin(t * 0.031)).to(torch.int32)
    pcm = torch.stack([left, left // 2 + (t % 7).to(torch.int32)], 1).contiguous()   # [samples, 2] interleaved
    stream = torch.cuda.Stream()   # one stream orders it all: the encoder, the read of the length, the scan
    stream.wait_stream(torch.cuda.current_stream())
    an = GpuAnalyzer(block, 6, 12, True, True, 2, 0.5, 16, 2, max_frames=frames)
    dec = Decoder()
    try:
        with torch.cuda.stream(stream):
            an.encode_device(pcm.data_ptr(), frames, last, 0, rate, stream=stream.cuda_stream)
            offsets = torch.as_tensor(DeviceBytes(an.device_buffer(5), 8 * (frames + 1), "<i8", 8), device="cuda")
            total = int(offsets[frames])   # eight bytes come down: how long the frames are, not the frames
            coded = torch.as_tensor(DeviceBytes(an.device_buffer(4), total), device="cuda")
            out, records, raw = decode_frames([coded], out="device", decoder=dec)   # scanned behind `stream`
            ok = bool((records["status"] == 0).all()) and torch.equal(out, pcm.reshape(-1))
        print(f"round trip on the device: {samples} stereo samples -> {total} bytes in {len(records)} frames -> "
              f"{'the same samples' if ok else 'DIFFERENT samples'}")
        assert np.array_equal(records["block_size"], [block] * (frames - 1) + [last])
        return ok
    finally:
        dec.close()
        an.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    import numpy as np
    import torch

    torch.cuda.init()   # torch's HIP runtime first
    from flac_codec_amd.gpu import Decoder, decode_many, decode_windows

    bad = 0
    if args.files:
        # ---- the shard: one tensor, one index.  (Here it is read from files; from now on it is device memory only.)
        index, parts, at = [], [], 0
        for p in args.files:
            data = np.fromfile(p, dtype=np.uint8)
            index.append((at, data.size))
            parts.append(data)
            at += data.size
        shard = torch.from_numpy(np.concatenate(parts)).to("cuda")
        del parts
        views = [shard[o:o + n] for o, n in index]
        dec = Decoder()
        t0 = time.perf_counter()
        _, streams = decode_many(views, out="device", decoder=dec)   # scan + one full decode with the MD5: the shard is sound
        recs, _ = dec.scan(views)   # the scan the crops are taken from; `shard` itself could be freed now
        print(f"scan + verify: {len(views)} streams, {shard.numel()} bytes in device memory, {time.perf_counter() - t0:.3f} s")
        good = [i for i, s in enumerate(streams) if s.rc == 0 and not s.info.bad_frames and not s.info.bad_crc16]
        for i in set(range(len(views))) - set(good):
            print(f"{args.files[i]}: not a sound FLAC stream, skipped")
        if not good:
            return 1
        length = {i: int(args.seconds * recs[i].info.sample_rate) for i in good}
        rng = random.Random(args.seed)
        times = []
        for _ in range(args.steps):
            windows = [(i, rng.randint(0, max(recs[i].info.decoded_samples - length[i], 0)), length[i]) for i in good]
            t0 = time.perf_counter()
            batch, results = decode_windows(dec, recs, windows, dtype="float32", out="device", pad_to=max(length.values()))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            bad += sum(r.bad_frames + r.bad_crc16 for r in results)
        dec.close()
        times.sort()
        print(f"{args.steps} steps of {tuple(batch.shape)} float32 crops: median {times[len(times) // 2] * 1e3:.2f} ms; "
              f"{bad} bad frames")
    ok = round_trip(torch)
    return 0 if ok and not bad else 1


if __name__ == "__main__":
    sys.exit(main())
