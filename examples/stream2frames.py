#!/usr/bin/env python3
"""A batch of streams that comes into being on the GPU a packet at a time -> raw FLAC frames, through a device stream
writer: every packet of every stream becomes ONE header-less subset frame, numbered with its stream's own count, as soon
as it exists -- what a network sender or a ring buffer wants, and what FlacStreamWriter does for one stream on the host.
The samples never visit the host, and all the streams' frames of one step are one GPU batch, whatever their lengths.

    python examples/stream2frames.py [streams] [packets]

The "generator" is stream2flac.py's bank of detuned sines, cut into packets of 20 ms, the last packet of a stream a
little shorter.  The frames go back through the batch decoder's raw frame path (gpu.decode_frames) and are compared with
what was generated.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # (stream2flac.py, also when this file is loaded by path)

from flac_codec_amd.encode import BatchEncoder, Options  # noqa: E402
from stream2flac import one_second  # noqa: E402


def options():
    return Options.default()


def stream_frames(n_streams=8, packets=10, sample_rate=48000, channels=1, device="cuda"):
    """-> (every stream's frames, one bytes object per packet; the packets [streams, channels, n] for comparison)"""
    import torch

    packet = sample_rate // 50
    enc = BatchEncoder(options())
    frames, kept = [[] for _ in range(n_streams)], []
    with enc.open_device_stream_writer(n_streams, sample_rate, 16, channels, max_block=packet) as writer:
        for step in range(packets):
            n = packet if step + 1 < packets else packet - 7
            chunk = one_second(torch, step, n_streams, channels, n, sample_rate, device)
            for k, frame in enumerate(writer.write(chunk, [n] * n_streams)):   # one frame per stream, ready to send
                frames[k].append(frame)
            kept.append(chunk)             # (only for the comparison below: a real loop drops the chunk here)
        assert writer.frame_numbers == [packets] * n_streams
    return frames, kept


def decode_back(frames, device=-1):
    """every stream's concatenated frames through the raw frame decoder -> [(samples [n, channels] int32, frame numbers)]"""
    from flac_codec_amd import gpu

    flat, records, raw = gpu.decode_frames([b"".join(f) for f in frames], device=device, out="host")
    out = []
    for k in range(len(frames)):
        mine = records[records["stream"] == k]
        assert raw[k].frames == len(frames[k]) == len(mine) and raw[k].skipped_bytes == 0 and not mine["status"].any()
        parts = [flat[int(r["out_offset"]):int(r["out_offset"]) + int(r["block_size"]) * int(r["channels"])]
                 .reshape(int(r["block_size"]), int(r["channels"])) for r in mine]
        out.append((parts, [int(r["number"]) for r in mine]))
    return out


def main(argv):
    import torch

    n_streams = int(argv[1]) if len(argv) > 1 else 8
    packets = int(argv[2]) if len(argv) > 2 else 10
    frames, kept = stream_frames(n_streams, packets)
    for k, (parts, numbers) in enumerate(decode_back(frames)):
        assert numbers == list(range(packets))
        for step, part in enumerate(parts):
            want = torch.clamp(torch.round(kept[step][k].double() * 32768.0), -32768, 32767).to(torch.int32).T.cpu().numpy()
            assert (part == want).all(), f"stream {k}, packet {step}: the decoded samples differ"
    sizes = [len(f) for per in frames for f in per]
    print(f"{n_streams} streams x {packets} packets: {len(sizes)} frames, {sum(sizes)} bytes, decoded back identical")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
