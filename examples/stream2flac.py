#!/usr/bin/env python3
"""A batch of clips that comes into being on the GPU a second at a time -> FLAC files, through a device session: every
second is handed to DeviceSession.write as soon as it exists, so the whole batch never has to sit in device memory as
float32, and the samples never visit the host.

    python examples/stream2flac.py [--unknown-total] out_dir [clips] [seconds]

The "generator" here is a bank of detuned sines with a little noise; in practice it is a model's step, a capture loop or
an augmentation pipeline that walks a long recording window by window.  The files are byte for byte what
BatchEncoder.encode_device writes for the finished clips.

--unknown-total: the session is opened without the clips' lengths, as a generator that does not know when it will stop
must open it.  The files are then FlacSampleWriter's with total_samples=None: no placeholder SEEKTABLE in front of the
frames, the seek table inside the PADDING block, the sample count filled in at finalize -- the same frames, another header.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flac_codec_amd.encode import BatchEncoder, Options  # noqa: E402


def options():
    return Options.default()


def one_second(torch, step, n_clips, channels, samples, sample_rate, device):
    """[clips, channels, samples] float32 in [-1, 1): second `step` of every clip"""
    g = torch.Generator(device=device).manual_seed(1000 + step)
    t = (torch.arange(samples, device=device) + step * sample_rate) / sample_rate
    f = 110.0 * (1 + torch.arange(n_clips, device=device))[:, None, None] * (1 + 0.01 * torch.arange(channels, device=device))[None, :, None]
    x = 0.5 * torch.sin(2 * torch.pi * f * t[None, None, :])
    return (x + 0.01 * torch.randn(x.shape, generator=g, device=device)).float().contiguous()


def stream_clips(n_clips=4, seconds=5.0, sample_rate=44100, channels=2, device="cuda", unknown_total=False):
    """-> (the .flac bytes of every clip, the finished clips [clips, channels, total] for comparison)"""
    import torch

    total = int(seconds * sample_rate)
    enc = BatchEncoder(options())
    kept = []
    totals = [None if unknown_total else total] * n_clips   # (None: the loop below could stop whenever it likes)
    with enc.open_device_session(totals, sample_rate, 16, channels, max_chunk=sample_rate) as session:
        for step, at in enumerate(range(0, total, sample_rate)):
            n = min(sample_rate, total - at)
            chunk = one_second(torch, step, n_clips, channels, n, sample_rate, device)
            session.write(chunk)          # the frames this second completes are kept by the session
            kept.append(chunk)            # (only for the comparison below: a real loop drops the chunk here)
        files = session.finalize()
    return files, torch.cat(kept, dim=2).contiguous()


def main(argv):
    unknown_total = "--unknown-total" in argv
    argv = [a for a in argv if a != "--unknown-total"]
    if len(argv) < 2:
        print(__doc__)
        return 2
    out_dir = argv[1]
    n_clips = int(argv[2]) if len(argv) > 2 else 4
    seconds = float(argv[3]) if len(argv) > 3 else 5.0
    files, clips = stream_clips(n_clips, seconds, unknown_total=unknown_total)
    os.makedirs(out_dir, exist_ok=True)
    for i, data in enumerate(files):
        with open(os.path.join(out_dir, f"clip{i:03d}.flac"), "wb") as f:
            f.write(data)
    whole = BatchEncoder(options()).encode_device(clips, None, sample_rate=44100, bits_per_sample=16)
    if unknown_total:   # the same frames behind another header: compare from the first frame on
        from flac_codec_amd.gpu import scan_stream_host

        first = [[int(scan_stream_host(f)[1][0]) for f in both] for both in zip(files, whole)]
        assert all(f[a:] == w[b:] for f, w, (a, b) in zip(files, whole, first)), "the session's frames differ from the one-shot call's"
        print(f"{len(files)} clips of {clips.shape[2]} samples, {sum(map(len, files))} bytes: the frames of encode_device's files")
        return 0
    assert whole == files, "the session's files differ from the one-shot call's"
    print(f"{len(files)} clips of {clips.shape[2]} samples, {sum(map(len, files))} bytes: identical to encode_device's")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
