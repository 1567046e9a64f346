"""The device front ends' short last blocks as ONE ragged batch (csrc/host/device_blocks.h encode_tail_blocks):
BatchEncoder.encode_device and encode_device(out="device"); and a session fed in three uneven writes, whose finalize goes
through the same function but keeps one one-frame call per tail (DESIGN.md 4c "Short last blocks as one batch").

Every front end must produce, stream by stream, the bytes of the same call with FLACGPU_NO_RAGGED=1 -- the loop of one-frame
calls this replaced, run in a fresh child process because knobs are read once -- and of flacenc_encode_many on the
converted samples.  flacenc_device_tail_stats shows which path ran.

Input A: 70 streams of 16-bit mono in a float32 padded tensor, lengths k * 4096 + t with k in 0..2 and t over the lengths of
tests/test_gpu_ragged.py -- some streams have no whole block at all, some (t = 4096) no tail.  Input B: 12 streams of 24-bit
stereo (int32)."""
import ctypes as C
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 1152, 4032, 4095, 4096]
B = 4096
OK, IO = 0, -130
GUARD = 48
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def inputs():
    """(computed once, never modified) name -> (host array [n, channels, T] (float32 / int32), lengths, sample rate, bits, channels); a function of this file alone"""
    rng = np.random.default_rng(2020)
    la = [((i // len(LENGTHS) + i) % 3) * B + LENGTHS[i % len(LENGTHS)] for i in range(70)]
    a = np.zeros((70, 1, max(la)), dtype=np.float32)
    for i, n in enumerate(la):
        t = np.arange(n)
        a[i, 0, :n] = (0.6 * np.sin(2 * np.pi * t * (0.003 + 0.0007 * i)) + rng.uniform(-0.3, 0.3, n)).astype(np.float32)
    lb = [(i % 3) * B + LENGTHS[(5 * i + 2) % len(LENGTHS)] for i in range(12)]   # (i = 4: 4096, no tail)
    b = np.zeros((12, 2, max(lb)), dtype=np.int32)
    for i, n in enumerate(lb):
        left = rng.integers(-(1 << 23), 1 << 23, n)
        b[i, 0, :n] = left
        b[i, 1, :n] = np.clip(left // 2 + rng.integers(-5000, 5000, n), -(1 << 23), (1 << 23) - 1)
    return {"mono16_f32": (a, la, 16000, 16, 1), "stereo24_i32": (b, lb, 48000, 24, 2)}


def converted(x, lengths, bits):
    """the interleaved int32 streams the ingest makes of the tensor (float32: x * 2^(bits - 1), nearest even, clamped)"""
    out = []
    for i, n in enumerate(lengths):
        v = x[i, :, :n]
        if x.dtype == np.float32:
            v = np.clip(np.rint(v.astype(np.float64) * (1 << (bits - 1))), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        out.append(np.ascontiguousarray(v.astype(np.int32).T).reshape(-1))
    return out


def tail_stats():
    from flac_codec_amd.encode import _stream_lib

    f, b = C.c_uint64(0), C.c_uint64(0)
    _stream_lib().flacenc_device_tail_stats(C.byref(f), C.byref(b))
    return int(f.value), int(b.value)


def cuts(n):
    """three uneven writes of a stream of n samples"""
    a = (3 * n) // 10
    b = a + (45 * n) // 100
    return [(0, a), (a, b), (b, n)]


def front_ends():
    """{(input, front end): (files, (tail_frames, tail_batches))} of this process"""
    import torch

    from flac_codec_amd.encode import BatchEncoder, Options

    out = {}
    for name, (x, lengths, rate, bits, channels) in inputs().items():
        t = torch.from_numpy(x).cuda()
        enc = BatchEncoder(Options.default())
        files = enc.encode_device(t, lengths, sample_rate=rate, bits_per_sample=bits)
        out[name, "host"] = (files, tail_stats())
        views = enc.encode_device(t, lengths, sample_rate=rate, bits_per_sample=bits, out="device")
        stats = tail_stats()
        out[name, "device"] = ([v.cpu().numpy().tobytes() for v in views], stats)
        pieces = [cuts(n) for n in lengths]
        most = max(e - s for p in pieces for s, e in p)
        with enc.open_device_session(lengths, rate, bits, channels, max_chunk=most) as ses:
            for w in range(3):
                chunk = np.zeros((len(lengths), channels, most), dtype=x.dtype)
                for i, p in enumerate(pieces):
                    s, e = p[w]
                    chunk[i, :, :e - s] = x[i, :, s:e]
                ses.write(torch.from_numpy(chunk).cuda(), [p[w][1] - p[w][0] for p in pieces])
            files = ses.finalize()
            out[name, "session"] = (files, tail_stats())
    return out


@pytest.fixture(scope="module")
def ragged():
    return front_ends()


@pytest.fixture(scope="module")
def one_by_one(tmp_path_factory):
    """the same calls in a fresh child process under FLACGPU_NO_RAGGED=1 (knobs are read once per process)"""
    path = tmp_path_factory.mktemp("no_ragged") / "out.pickle"
    env = dict(os.environ, FLACGPU_NO_RAGGED="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with open(path, "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def host_reference():
    from flac_codec_amd.encode import BatchEncoder, Options

    ref = {}
    for name, (x, lengths, rate, bits, channels) in inputs().items():
        ref[name] = [bytes(v) for v in BatchEncoder(Options.default()).encode(converted(x, lengths, bits), rate, bits, channels)]
    return ref


@pytest.mark.parametrize("front_end", ["host", "device", "session"])
@pytest.mark.parametrize("name", ["mono16_f32", "stereo24_i32"])
def test_bytes_are_those_of_the_one_frame_loop_and_of_the_host_encoder(ragged, one_by_one, host_reference, name, front_end):
    files, _ = ragged[name, front_end]
    old, _ = one_by_one[name, front_end]
    lengths = inputs()[name][1]
    assert len(files) == len(old) == len(lengths)
    for i, n in enumerate(lengths):
        assert bytes(files[i]) == bytes(old[i]), f"stream {i} ({n} samples): differs from the FLACGPU_NO_RAGGED=1 run"
        assert bytes(files[i]) == host_reference[name][i], f"stream {i} ({n} samples): differs from flacenc_encode_many"


@pytest.mark.parametrize("front_end", ["host", "device", "session"])
@pytest.mark.parametrize("name", ["mono16_f32", "stereo24_i32"])
def test_tail_stats_show_which_path_ran(ragged, one_by_one, name, front_end):
    with_tail = sum(1 for n in inputs()[name][1] if n % B)
    assert 0 < with_tail < len(inputs()[name][1])
    if front_end == "session":   # finalize keeps the one-frame loop (its leg failed the regression condition)
        assert ragged[name, front_end][1] == (with_tail, with_tail)
    else:
        assert ragged[name, front_end][1] == (with_tail, 1)        # every tail, ONE batch
    assert one_by_one[name, front_end][1] == (with_tail, with_tail)   # the knob: one call per tail


def test_a_slot_one_byte_too_small_fails_that_stream_alone(ragged):
    import torch

    from flac_codec_amd.encode import BatchEncoder, Options

    name = "mono16_f32"
    x, lengths, rate, bits, channels = inputs()[name]
    files = ragged[name, "device"][0]
    # victims: a stream that is nothing but a tail, and one with whole blocks in front of its tail
    victims = [next(i for i, n in enumerate(lengths) if n < B), next(i for i, n in enumerate(lengths) if n > B and n % B)]
    slots, at = [], GUARD + 5
    for i, f in enumerate(files):
        cap = len(f) - 1 if i in victims else len(f)
        slots.append((at, cap))
        at += cap + GUARD + (i % 7)
    shard = torch.full((at + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    enc = BatchEncoder(Options.default())
    with pytest.raises(Exception):
        enc.encode_device(torch.from_numpy(x).cuda(), lengths, sample_rate=rate, bits_per_sample=bits, out="device", shard=shard,
                          slots=slots)
    assert [s for s in enc.last_status] == [IO if i in victims else OK for i in range(len(files))]
    got = shard.cpu().numpy()
    inside = np.zeros(got.size, dtype=bool)
    for i, (o, cap) in enumerate(slots):
        inside[o:o + cap] = True
        if i not in victims:
            assert got[o:o + cap].tobytes() == files[i], f"stream {i}"
    assert np.all(got[~inside] == CANARY), "a byte outside the slots was written"


def test_a_tail_cap_one_byte_too_small_fails_that_stream_alone(ragged):
    import torch

    from flac_codec_amd import _lib
    from flac_codec_amd.encode import BatchEncoder, Options, _stream_lib

    name = "stereo24_i32"
    x, lengths, rate, bits, channels = inputs()[name]
    files = ragged[name, "session"][0]
    L = _stream_lib()
    enc = BatchEncoder(Options.default())
    n = len(lengths)
    victim = next(i for i, m in enumerate(lengths) if m > B and m % B)
    with enc.open_device_session(lengths, rate, bits, channels, max_chunk=max(lengths), keep=False) as ses:
        frames = ses.write(torch.from_numpy(x).cuda(), lengths)
        finals = (_lib.SessionFinal * n)()
        bufs = []
        for i in range(n):
            hlen = ses.header_len(i)
            tail_len = len(files[i]) - hlen - len(frames[i])
            assert (tail_len > 0) == (lengths[i] % B != 0)
            cap = tail_len - 1 if i == victim else tail_len
            hb = np.full(hlen + 2 * GUARD, CANARY, dtype=np.uint8)
            tb = np.full(cap + 2 * GUARD, CANARY, dtype=np.uint8)
            bufs.append((hb, tb, hlen, cap))
            finals[i].header, finals[i].header_cap = hb.ctypes.data + GUARD, hlen
            finals[i].tail, finals[i].tail_cap = tb.ctypes.data + GUARD, cap
        rc = L.flacenc_device_session_finalize(ses._h, finals)
        assert rc == IO
        for i, (hb, tb, hlen, cap) in enumerate(bufs):
            assert np.all(hb[:GUARD] == CANARY) and np.all(hb[GUARD + hlen:] == CANARY)
            assert np.all(tb[:GUARD] == CANARY) and np.all(tb[GUARD + cap:] == CANARY)
            if i == victim:
                assert finals[i].status == IO and finals[i].tail_len == 0
                assert np.all(tb == CANARY)
                continue
            assert finals[i].status == OK and finals[i].tail_len == cap and finals[i].header_len == hlen
            whole = hb[GUARD:GUARD + hlen].tobytes() + frames[i] + tb[GUARD:GUARD + cap].tobytes()
            assert whole == files[i], f"stream {i}"


if __name__ == "__main__":   # the child of the `one_by_one` fixture
    sys.path.insert(0, ROOT)
    import torch

    torch.cuda.init()        # torch's HIP runtime first, as tests/conftest.py does
    result = {k: ([bytes(f) for f in files], stats) for k, (files, stats) in front_ends().items()}
    with open(sys.argv[1], "wb") as f:
        pickle.dump(result, f)
