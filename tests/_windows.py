"""Sample windows for the flacgpu_decoder_decode_windows tests (test_decode_windows_abi.py on the CPU,
test_gpu_decode_windows.py on the GPU): a model of the frame selection that shares nothing with the library's (a running
sum of the block sizes and a linear search, where the library searches by halving), and the window shapes both tests
use, each chosen for an edge of the selection or of the clipped store."""
import random


def model_frames(sizes, start, length):
    """(first, count, skip) of the frames that samples [start, start + length) touch; (0, 0, 0) for none."""
    end = min(start + length, sum(sizes))
    first, count, skip, at = 0, 0, 0, 0
    if start >= end:   # empty, or past the end
        return first, count, skip
    for k, n in enumerate(sizes):
        if at < end and at + n > start:
            if not count:
                first, skip = k, start - at
            count += 1
        at += n
    return first, count, skip


def fixed_windows(sizes):
    """[(start, length)] for a stream of these block sizes, without repeats, in a fixed order."""
    sizes = [int(n) for n in sizes]
    T, F = sum(sizes), len(sizes)
    starts = [sum(sizes[:k]) for k in range(F)]
    out = [(0, T), (0, 1), (max(T - 1, 0), 1)]              # the whole stream, the first sample, the last alone
    out += [(b - 1, 2) for b in starts[1:]]                # two samples across every frame boundary
    if F:
        k = F // 2
        mid = starts[k] + sizes[k] // 2                    # inside frame k (its first sample when it has but one)
        out += [(starts[k], sizes[k]),                     # exactly one frame
                (starts[k] + 1, max(sizes[k] - 2, 0)),     # ... without its first and last sample
                (mid, T - mid + 5),                        # from mid-frame to five past the end
                (mid, 0), (starts[k], 0)]                  # empty: mid-frame, on a boundary
    out += [(T, 4), (T + 100, 3), (0, 0)]                  # at the end, past it, empty at 0
    seen, uniq = set(), []
    for w in out:
        if w not in seen:
            seen.add(w)
            uniq.append(w)
    return uniq


def random_windows(rng, sizes, count):
    """`count` windows of a seeded random.Random: starts up to a little past the end, short and long lengths."""
    T = sum(int(n) for n in sizes)
    out = []
    for _ in range(count):
        start = rng.randint(0, T + 3)
        out.append((start, rng.randint(0, max(T - start, 0) + 3) if rng.random() < 0.5 else rng.randint(0, 40)))
    return out


def rng_of(seed):
    return random.Random(seed)
