#!/usr/bin/env python3
"""FLAC files -> one padded float32 batch on the GPU -> FLAC files again, the samples never leaving the GPU in between:
decode_many(float32, padded) gives a [files, channels, samples] tensor, BatchEncoder.encode_device turns such a tensor
(here the decoded one; in practice a model's or an augmentation pipeline's output) into .flac bytes.

    python examples/batch2flac.py [--dtype float32|int24] out_dir a.flac b.flac ...

The files of one call must share sample rate, bit depth (at most 25 bits: float32 holds them exactly) and channel count.
--dtype int24 keeps the batch as packed 24-bit samples instead ([files, channels, samples, 3] uint8, 3 bytes a sample
where float32 and int32 take 4; at most 24 bits).  Asserts that decoding the new files gives the same tensor.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flac_codec_amd.encode import BatchEncoder, Options  # noqa: E402
from flac_codec_amd.gpu import decode_many  # noqa: E402


def main(argv):
    dtype = "float32"
    if len(argv) > 2 and argv[1] == "--dtype":
        dtype, argv = argv[2], argv[:1] + argv[3:]
    if len(argv) < 3 or dtype not in ("float32", "int24"):
        print(__doc__)
        return 2
    import torch

    out_dir, paths = argv[1], argv[2:]
    blobs = []
    for p in paths:
        with open(p, "rb") as f:
            blobs.append(f.read())
    batch, streams = decode_many(blobs, dtype=dtype, layout="padded")
    shapes = {(s.rc, s.info.sample_rate, s.info.bits_per_sample, s.info.channels) for s in streams}
    if len(shapes) != 1 or next(iter(shapes))[0] != 0:
        print("the files must all decode and share sample rate, bit depth and channel count")
        return 1
    _, rate, bps, _ = next(iter(shapes))
    lengths = [s.info.decoded_samples for s in streams]
    enc = BatchEncoder(Options.default())
    files = enc.encode_device(batch, lengths, sample_rate=rate, bits_per_sample=bps,
                              dtype="int24" if dtype == "int24" else None)
    os.makedirs(out_dir, exist_ok=True)
    for p, data, altered in zip(paths, files, enc.last_altered):
        with open(os.path.join(out_dir, os.path.basename(p)), "wb") as f:
            f.write(data)
        print(f"{p}: {len(data)} bytes, {altered} samples altered")
    again, checked = decode_many(files, dtype=dtype, layout="padded", pad_to=batch.shape[2])
    assert all(s.rc == 0 and s.info.md5_status == 1 for s in checked)
    assert torch.equal(again, batch), "the second decode differs"
    print(f"{len(files)} files, {tuple(batch.shape)} {dtype}: the second decode gives the same tensor")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
