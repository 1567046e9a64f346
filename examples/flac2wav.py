#!/usr/bin/env python3
"""FLAC files to WAV files, every file decoded in one GPU call straight into its WAV data chunk: decode_many(out="host")
with dtype "int16" for streams of 9-16 bits and "int24" for 17-24 bits writes the samples left-justified in WAV's own
container (2 or 3 little-endian bytes per sample), so the buffer that comes back is written out as it stands.

    python examples/flac2wav.py out_dir a.flac b.flac ...

Files of both groups may be mixed: each group is one call.  Other bit depths (8 and fewer: WAV stores them unsigned;
more than 24) are refused with a message.
"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flac_codec_amd.gpu import Decoder, decode_many, scan_stream_host  # noqa: E402


def wav_header(rate, channels, container_bits, data_bytes):
    """The 44 bytes in front of the samples; a data chunk of odd length is followed by one pad byte, which the RIFF
    size counts and the chunk's own size does not."""
    block = channels * container_bits // 8
    return (b"RIFF" + struct.pack("<I", 36 + data_bytes + data_bytes % 2) + b"WAVEfmt " +
            struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * block, block, container_bits) +
            b"data" + struct.pack("<I", data_bytes))


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    out_dir, paths = argv[1], argv[2:]
    groups = {"int16": [], "int24": []}
    for p in paths:
        with open(p, "rb") as f:
            blob = f.read()
        bps = scan_stream_host(blob)[0].bits_per_sample
        if not 9 <= bps <= 24:
            print(f"{p}: {bps} bits per sample; this example writes 9-24 bits")
            return 1
        groups["int16" if bps <= 16 else "int24"].append((p, blob))
    os.makedirs(out_dir, exist_ok=True)
    dec = Decoder()
    bad = 0
    for dtype, files in groups.items():
        if not files:
            continue
        _, streams = decode_many([b for _, b in files], out="host", dtype=dtype, decoder=dec)
        for (p, _), s in zip(files, streams):
            if s.rc != 0 or s.info.bad_frames or s.info.bad_crc16 or s.info.md5_status == 0:
                print(f"{p}: error")
                bad += 1
                continue
            data = np.ascontiguousarray(s.pcm).view(np.uint8).reshape(-1)   # [samples, channels(, 3)]: the data chunk
            if data.size + 37 > 0xFFFFFFFF:
                print(f"{p}: {data.size} bytes of samples do not fit a plain WAV file")
                bad += 1
                continue
            name = os.path.splitext(os.path.basename(p))[0] + ".wav"
            with open(os.path.join(out_dir, name), "wb") as f:
                f.write(wav_header(s.info.sample_rate, s.info.channels, 16 if dtype == "int16" else 24, data.size))
                f.write(data)
                if data.size % 2:   # mono 24-bit with an odd number of samples
                    f.write(b"\0")
            print(f"{p}: {s.info.decoded_samples} samples x {s.info.channels} channels, {s.info.bits_per_sample} bits "
                  f"-> {name} ({dtype})")
    dec.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
