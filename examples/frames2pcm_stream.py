#!/usr/bin/env python3
"""The receiving end of stream2frames.py: raw FLAC frames of a batch of streams -> PCM, as the bytes arrive, through a
decoder session (gpu.DecoderSession).  Two receivers see the same bytes:

  1. write by write, as the device stream writer emits them: one whole frame per stream per feed, so every feed says
     flush=True ("what I have fed ends on a frame boundary") and each frame's samples are out in the same step;
  2. re-cut at arbitrary sizes, as a socket delivers them: no flush until the end, a frame comes out once the header
     behind it has arrived, and the bytes that cannot be judged yet wait in device memory.

Both must give the PCM that was generated.

    python examples/frames2pcm_stream.py [streams] [packets]
"""
import hashlib
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from stream2frames import stream_frames  # noqa: E402


def receive(session, feeds, n_streams):
    """feeds: [(one chunk per stream, flush)] -> per stream the decoded frames [n, channels] in order, and for every
    feed how many frames it gave."""
    pcm, counts = [[] for _ in range(n_streams)], []
    for chunks, flush in feeds + [(None, True)]:
        frames, _ = session.finish() if chunks is None else session.feed(chunks, flush)
        flat, decoded = session.decode_frames(out="host")
        assert not decoded["status"].any()
        for r in decoded:
            at, n, c = int(r["out_offset"]), int(r["block_size"]), int(r["channels"])
            pcm[int(r["stream"])].append(flat[at:at + n * c].reshape(n, c))
        counts.append(len(frames))
    return pcm, counts


def digest(pcm):
    h = hashlib.sha256()
    for stream in pcm:
        for part in stream:
            h.update(part.tobytes())
    return h.hexdigest()


def main(argv):
    import numpy as np
    import torch

    from flac_codec_amd import gpu

    n_streams = int(argv[1]) if len(argv) > 1 else 8
    packets = int(argv[2]) if len(argv) > 2 else 10
    frames, kept = stream_frames(n_streams, packets)
    bound = max(len(f) for per in frames for f in per)   # no frame of these streams is longer

    # 1. the writer's writes, one frame per stream per feed
    session = gpu.DecoderSession(n_streams, bound)
    as_written, counts = receive(session, [([per[step] for per in frames], True) for step in range(packets)], n_streams)
    session.close()
    assert counts == [n_streams] * packets + [0], counts   # every frame in the step it was fed in

    # 2. the same bytes, cut where a socket would cut them
    rng = random.Random(1)
    blobs, at, feeds = [b"".join(per) for per in frames], [0] * n_streams, []
    while any(a < len(b) for a, b in zip(at, blobs)):
        chunks = []
        for k in range(n_streams):
            n = rng.choice((0, 1, 97, 512, 1460))
            chunks.append(blobs[k][at[k]:at[k] + n])
            at[k] += len(chunks[-1])
        feeds.append((chunks, False))
    session = gpu.DecoderSession(n_streams, bound)
    as_delivered, counts = receive(session, feeds, n_streams)
    held, fed = session.pending()
    session.close()
    assert held == [0] * n_streams and fed == sum(len(b) for b in blobs)

    for k in range(n_streams):
        for step in range(packets):
            want = torch.clamp(torch.round(kept[step][k].double() * 32768.0), -32768, 32767).to(torch.int32).T.cpu().numpy()
            assert np.array_equal(as_written[k][step], want), f"stream {k}, packet {step}: the decoded samples differ"
    a, b = digest(as_written), digest(as_delivered)
    assert a == b
    print(f"{n_streams} streams x {packets} packets, {sum(len(b) for b in blobs)} bytes: fed write by write "
          f"({packets} feeds) and re-cut into {len(feeds)} feeds of arbitrary sizes: identical PCM (sha256 {a[:16]})")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
