"""flacenc_device_stream_writer_* / BatchEncoder.open_device_stream_writer on the GPU: n streams in device memory, ONE raw
subset frame per stream and write.

The expected bytes are the oracle's encode_frame(.., frame_number=k, subset=True) -- FlacStreamWriter::write,
encode.rs:1094-1274 -- for the samples of every chunk with the number the stream has reached; nothing expected comes from
the writer.  The same scenarios run once more in a child process under FLACGPU_NO_RAGGED=1 (the one-frame loop; knobs are
read once per process) and must give the same bytes.  Padding and gaps of every chunk tensor hold filler, every out buffer
has guard bytes round it (the helpers of tests/test_gpu_device_session.py)."""
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
I32, I16, F32, S24 = 0, 1, 2, 24
FLAT, PADDED = 0, 1
OK, IO, INVALID_ARG, UNSUPPORTED, EXCESSIVE_FRAME_NUMBER = 0, -130, -140, -151, -119
GUARD = 64
MAX_NUMBER = (1 << 36) - 1

# name -> (options, rate, bps, channels, max_block, first numbers, [(lengths, dtype, layout)], the same samples in every write)
SCENARIOS = {
    # three distinct lengths in one call; a stream that is skipped; type and layout change from write to write
    "stereo16": ("default", 44100, 16, 2, 4096, None,
                 [([1, 16, 4096], I16, PADDED), ([0, 4095, 17], F32, FLAT), ([192, 192, 192], I32, PADDED)], False),
    "mono24_s24": ("default", 48000, 24, 1, 1000, None, [([191, 192, 1000], S24, PADDED), ([1000, 0, 5], S24, FLAT)], False),
    "eight_channels_8_bit": ("default", 32000, 8, 8, 100, None, [([33, 64, 100], I16, PADDED), ([100, 1, 0], I32, FLAT)], False),
    # sample rates the frame header codes behind itself: in Hz (16 bits), in tens of Hz
    "rate_in_hz": ("default", 22051, 16, 1, 64, None, [([64, 17], I16, PADDED)], False),
    "rate_in_tens_of_hz": ("default", 12340, 16, 1, 64, None, [([64, 17], I16, PADDED)], False),
    # the coded frame number grows by a byte between the two writes: 127 -> 128, 2047 -> 2048, 65535 -> 65536
    "first_numbers": ("default", 44100, 16, 1, 64, [127, 2047, 65535], [([40, 40, 40], I16, PADDED)] * 2, True),
    "best": ("best", 44100, 16, 2, 4096, None, [([4096, 4096, 100], I16, PADDED)], False),              # max partition order 6
    "partition_order_7_at_4095": ("mpo7", 44100, 16, 2, 4096, None, [([4095, 17, 4095], I16, PADDED)], False),
    # max_block below 16, the smallest block size an analysis context has: the contexts are of 16
    "max_block_8": ("default", 44100, 16, 1, 8, None, [([1, 8, 5], I16, PADDED), ([8, 0, 3], I32, FLAT)], False),
    "max_block_15_stereo_24_bit": ("default", 48000, 24, 2, 15, None, [([15, 2, 7], S24, PADDED)], False),
    "max_block_1": ("default", 8000, 8, 3, 1, None, [([1, 0, 1], I16, FLAT), ([1, 1, 1], I32, PADDED)], False),
}


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible to torch")
    return torch


def _L():
    from flac_codec_amd.encode import _stream_lib

    return _stream_lib()


def options_of(kind):
    from flac_codec_amd.encode import Options

    if kind == "best":
        return Options.best()
    if kind == "mpo7":
        return Options.default().max_partition_order(7)
    return Options.default()


@functools.lru_cache(maxsize=None)
def chunk_samples(name, w, k):
    """[n, channels] int32: what stream k brings in write w of a scenario; computed once, never modified"""
    from test_gpu_encode_device import signal

    _, _, bps, channels, _, _, writes, same = SCENARIOS[name]
    seed = 7000 + 97 * sorted(SCENARIOS).index(name) + (0 if same else 10 * w) + k
    return signal(seed, writes[w][0][k], channels, bps)


@functools.lru_cache(maxsize=None)
def oracle_frame(kind, rate, bps, number, name, w, k):
    import _oracle as orc
    from test_stream_header_unknown_total import orc_opts_from

    rc, data, _ = orc.encode_frame(orc_opts_from(options_of(kind)), rate, bps, chunk_samples(name, w, k).T, frame_number=number,
                                   subset=True)
    assert rc == 0 and data
    return data


def expected(name):
    """[write][stream] -> the oracle's frame (b"" for a stream without samples), and the numbers reached"""
    kind, rate, bps, _, _, first, writes, _ = SCENARIOS[name]
    numbers = list(first) if first else [0] * len(writes[0][0])
    out = []
    for w, (lengths, _, _) in enumerate(writes):
        row = []
        for k, n in enumerate(lengths):
            row.append(oracle_frame(kind, rate, bps, numbers[k], name, w, k) if n else b"")
            numbers[k] += 1 if n else 0
        out.append(row)
    return out, numbers


class Writer:
    """the C ABI, with guard bytes round every out buffer"""

    def __init__(self, o, n, rate, bps, channels, max_block, first=None):
        self.co = o._c_options()
        self.n, self.bps, self.channels = n, bps, channels
        self.h = C.c_void_p()
        arr = (C.c_uint64 * max(n, 1))(*first) if first else None
        self.open_rc = _L().flacenc_device_stream_writer_open(C.byref(self.co), rate, bps, channels, n, max_block, arr, C.byref(self.h))

    def numbers(self):
        return [int(_L().flacenc_device_stream_writer_frame_number(self.h, i)) for i in range(self.n)]

    def write(self, host, fmt_args, offs, lengths, caps=None):
        """-> (rc, [status], [altered], [bytes]); asserts the guards; a call refused as a whole: (rc, None, None, None)"""
        from flac_codec_amd import _lib

        t = _torch().from_numpy(host).cuda()
        fmt = _lib.OutFormat(*fmt_args)
        chunks = (_lib.SessionChunk * max(self.n, 1))()
        bufs = []
        for i in range(self.n):
            cap = 18 + 2 * self.channels + (lengths[i] * self.channels * (self.bps + 1) + 7) // 8 if lengths[i] else 0
            if caps is not None and caps[i] is not None:
                cap = caps[i]
            bufs.append(np.full(cap + 2 * GUARD, 0xA5, dtype=np.uint8))
            chunks[i].in_offset, chunks[i].samples = offs[i], lengths[i]
            chunks[i].out, chunks[i].out_cap = bufs[i].ctypes.data + GUARD, cap
            chunks[i].out_len, chunks[i].status, chunks[i].altered = 777, 55, 99   # a refused call writes no field
        rc = _L().flacenc_device_stream_writer_write(self.h, t.data_ptr() if t.numel() else None, C.byref(fmt), chunks, None)
        status = [int(chunks[i].status) for i in range(self.n)]
        if rc != 0:
            assert all(s == 55 for s in status)
            assert all((int(chunks[i].out_len), int(chunks[i].altered)) == (777, 99) for i in range(self.n))
            assert all((b == 0xA5).all() for b in bufs)
            return rc, None, None, None
        out = []
        for i in range(self.n):
            used = int(chunks[i].out_len)
            assert (bufs[i][:GUARD] == 0xA5).all() and (bufs[i][GUARD + used:] == 0xA5).all(), f"guard bytes of stream {i}'s out"
            out.append(bufs[i][GUARD:GUARD + used].tobytes())
        return rc, status, [int(chunks[i].altered) for i in range(self.n)], out

    def close(self):
        _L().flacenc_device_stream_writer_close(self.h)
        self.h = C.c_void_p()


def feed(w, name, write, caps=None):
    from test_gpu_device_session import chunk_tensor

    _, _, bps, channels, _, _, writes, _ = SCENARIOS[name]
    lengths, dtype, layout = writes[write]
    pieces = [chunk_samples(name, write, k) for k in range(len(lengths))]
    host, fmt, offs = chunk_tensor(pieces, dtype, layout, bps, channels)
    return w.write(host, fmt, offs, lengths, caps=caps)


def run_scenario(name):
    """-> ([write][stream] frames, the numbers after the last write)"""
    kind, rate, bps, channels, max_block, first, writes, _ = SCENARIOS[name]
    w = Writer(options_of(kind), len(writes[0][0]), rate, bps, channels, max_block, first)
    assert w.open_rc == 0
    assert w.numbers() == (list(first) if first else [0] * w.n)
    frames = []
    for k in range(len(writes)):
        rc, status, altered, out = feed(w, name, k)
        assert rc == 0 and status == [0] * w.n and altered == [0] * w.n, (name, k, rc, status)
        frames.append(out)
    numbers = w.numbers()
    w.close()
    return frames, numbers


def all_scenarios():
    return {name: run_scenario(name) for name in SCENARIOS}


@pytest.fixture(scope="module")
def ragged():
    return all_scenarios()


@pytest.fixture(scope="module")
def one_by_one(tmp_path_factory):
    """the same writes in a fresh child process under FLACGPU_NO_RAGGED=1"""
    path = tmp_path_factory.mktemp("writer_no_ragged") / "out.pickle"
    env = dict(os.environ, FLACGPU_NO_RAGGED="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with open(path, "rb") as f:
        return pickle.load(f)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_frames_are_the_oracles(ragged, name):
    frames, numbers = ragged[name]
    want, want_numbers = expected(name)
    lengths = [w[0] for w in SCENARIOS[name][6]]
    for w, row in enumerate(frames):
        for k, got in enumerate(row):
            assert (len(got) > 0) == (lengths[w][k] > 0)
            assert got == want[w][k], f"{name}: write {w}, stream {k} ({lengths[w][k]} samples): differs from the oracle's frame"
    assert numbers == want_numbers   # a stream that brought nothing keeps its number


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_the_one_frame_loop_gives_the_same_bytes(ragged, one_by_one, name):
    assert one_by_one[name] == ragged[name]


def test_the_coded_number_grows_by_a_byte(ragged):
    (first, second), numbers = ragged["first_numbers"]
    assert numbers == [129, 2049, 65537]
    assert [len(b) - len(a) for a, b in zip(first, second)] == [1, 1, 1]   # the same samples, a longer number


def test_round_trip_through_the_raw_frame_decoder(ragged):
    from flac_codec_amd import gpu

    for name in SCENARIOS:
        frames, _ = ragged[name]
        first = SCENARIOS[name][5] or [0] * len(frames[0])
        blobs = [b"".join(row[k] for row in frames) for k in range(len(frames[0]))]
        flat, records, raw = gpu.decode_frames(blobs, out="host")
        for k in range(len(blobs)):
            mine = records[records["stream"] == k]
            brought = [w for w in range(len(frames)) if frames[w][k]]
            assert raw[k].frames == len(mine) == len(brought) and raw[k].skipped_bytes == 0 and not mine["status"].any()
            assert [int(r["number"]) for r in mine] == list(range(first[k], first[k] + len(brought)))
            for r, w in zip(mine, brought):
                want = chunk_samples(name, w, k)
                got = flat[int(r["out_offset"]):int(r["out_offset"]) + want.size].reshape(want.shape)
                assert int(r["block_size"]) == len(want) and np.array_equal(got, want), (name, k, w)


def test_refused_writes_change_nothing():
    from test_gpu_device_session import chunk_tensor
    from test_gpu_encode_device import signal

    w = Writer(options_of("mpo7"), 3, 44100, 16, 2, 4096)
    assert w.open_rc == 0
    name = "partition_order_7_at_4095"
    # a 4096-sample frame under max partition order 7: effective order 7 > 6, the whole write is refused
    pieces = [signal(1, 17, 2, 16), signal(2, 4096, 2, 16), signal(3, 5, 2, 16)]
    host, fmt, offs = chunk_tensor(pieces, I16, PADDED, 16, 2)
    rc, status, _, _ = w.write(host, fmt, offs, [17, 4096, 5])
    assert rc == UNSUPPORTED and status is None and w.numbers() == [0, 0, 0]
    assert b"stream 1" in _L().flacenc_last_error() and b"partition order" in _L().flacenc_last_error()
    # a chunk of max_block + 1
    pieces = [signal(1, 4097, 2, 16), signal(2, 1, 2, 16), signal(3, 1, 2, 16)]
    host, fmt, offs = chunk_tensor(pieces, I16, PADDED, 16, 2)
    rc, status, _, _ = w.write(host, fmt, offs, [4097, 1, 1])
    assert rc == INVALID_ARG and status is None and b"max_block" in _L().flacenc_last_error() and w.numbers() == [0, 0, 0]
    # what the batch plan refuses for the tensor: an unknown layout; a chunk longer than samples_padded; float32 is fine at
    # 16 bits, packed 24-bit input at ... 16 bits too, int16 at 24 bits would not be -- but that is another writer's shape
    pieces = [signal(1, 10, 2, 16)] * 3
    host, fmt, offs = chunk_tensor(pieces, I16, PADDED, 16, 2)
    assert w.write(host, (I16, 7, fmt[2], 0, fmt[4]), offs, [10, 10, 10])[0] == INVALID_ARG
    assert w.write(host, (I16, PADDED, fmt[2], 0, 9), offs, [10, 10, 10])[0] == INVALID_ARG
    assert w.write(host, (I16, PADDED, 1, 0, fmt[4]), offs, [10, 10, 10])[0] == INVALID_ARG   # channels_padded < channels
    assert w.numbers() == [0, 0, 0]
    # the next correct write gives the frames numbered 0
    rc, status, altered, out = feed(w, name, 0)
    assert rc == 0 and status == [0, 0, 0] and out == expected(name)[0][0] and w.numbers() == [1, 1, 1]
    # a write without any samples runs and changes nothing
    host, fmt, offs = chunk_tensor([signal(1, 0, 2, 16)] * 3, I16, FLAT, 16, 2)
    rc, status, altered, out = w.write(host, fmt, offs, [0, 0, 0])
    assert rc == 0 and status == [0, 0, 0] and out == [b"", b"", b""] and w.numbers() == [1, 1, 1]
    w.close()
    # a writer for 24 bits refuses int16 input
    w = Writer(options_of("default"), 1, 48000, 24, 1, 64)
    host, fmt, offs = chunk_tensor([signal(1, 10, 1, 16)], I16, PADDED, 16, 1)
    assert w.write(host, fmt, offs, [10])[0] == UNSUPPORTED and w.numbers() == [0]
    w.close()


def test_an_out_one_byte_short_keeps_the_number_and_the_stream(ragged):
    name = "stereo16"
    want, _ = expected(name)
    kind, rate, bps, channels, max_block, _, _, _ = SCENARIOS[name]
    w = Writer(options_of(kind), 3, rate, bps, channels, max_block)
    rc, status, _, out = feed(w, name, 0, caps=[None, len(want[0][1]) - 1, None])
    assert rc == 0 and status == [0, IO, 0] and out == [want[0][0], b"", want[0][2]]
    assert w.numbers() == [1, 0, 1]
    # the same chunks once more, with room: stream 1's frame has the number it would have had; the others have moved on
    rc, status, _, out = feed(w, name, 0, caps=[None, len(want[0][1]), None])
    assert rc == 0 and status == [0, 0, 0] and out[1] == want[0][1] and w.numbers() == [2, 1, 2]
    assert out[0] == oracle_frame(kind, rate, bps, 1, name, 0, 0) and out[2] == oracle_frame(kind, rate, bps, 1, name, 0, 2)
    # no buffer at all is too small as well
    rc, status, _, out = feed(w, name, 0, caps=[0, None, None])
    assert rc == 0 and status == [IO, 0, 0] and w.numbers() == [2, 2, 3]
    w.close()


def test_the_frame_number_limit():
    """flacenc_stream_writer_write at FrameNumber::MAX_FRAME_NUMBER: the frame is written, the count cannot go on"""
    name = "rate_in_hz"
    kind, rate, bps, channels, max_block, _, _, _ = SCENARIOS[name]
    w = Writer(options_of(kind), 2, rate, bps, channels, max_block, [MAX_NUMBER, MAX_NUMBER - 1])
    assert w.open_rc == 0
    # stream 0 stands at the limit: its frame is written, its status says that the count cannot go on; stream 1 reaches it
    rc, status, _, out = feed(w, name, 0)
    assert rc == 0 and status == [EXCESSIVE_FRAME_NUMBER, 0]
    assert out == [oracle_frame(kind, rate, bps, MAX_NUMBER, name, 0, 0), oracle_frame(kind, rate, bps, MAX_NUMBER - 1, name, 0, 1)]
    assert w.numbers() == [MAX_NUMBER, MAX_NUMBER]
    # once more: now both stand at the limit, and both keep writing frames with that number
    rc, status, _, out = feed(w, name, 0)
    assert rc == 0 and status == [EXCESSIVE_FRAME_NUMBER, EXCESSIVE_FRAME_NUMBER]
    assert out == [oracle_frame(kind, rate, bps, MAX_NUMBER, name, 0, k) for k in range(2)]
    assert w.numbers() == [MAX_NUMBER, MAX_NUMBER]
    w.close()


def test_tail_stats_keep_the_preceding_one_shot_calls_figures():
    torch = _torch()
    from flac_codec_amd.encode import BatchEncoder, Options

    def tail_stats():
        a, b = C.c_uint64(123), C.c_uint64(456)
        _L().flacenc_device_tail_stats(C.byref(a), C.byref(b))
        return a.value, b.value

    x = torch.zeros((3, 1, 4096 + 5), dtype=torch.int16, device="cuda")
    BatchEncoder(Options.default()).encode_device(x, [100, 4096 + 5, 4096], sample_rate=44100, bits_per_sample=16)
    before = tail_stats()
    assert before[0] == 2 and before[1] >= 1   # two short last blocks
    w = Writer(options_of("default"), 3, 44100, 16, 2, 4096)
    rc, status, _, out = feed(w, "stereo16", 0)
    assert rc == 0 and all(out)
    assert tail_stats() == before
    w.close()


def test_python_writer_and_the_examples_loop(ragged):
    torch = _torch()
    from flac_codec_amd.encode import BatchEncoder, Unsupported
    from test_gpu_device_session import chunk_tensor

    name = "stereo16"
    kind, rate, bps, channels, max_block, _, writes, _ = SCENARIOS[name]
    enc = BatchEncoder(options_of(kind))
    with enc.open_device_stream_writer(3, rate, bps, channels, max_block) as writer:
        for w, (lengths, dtype, layout) in enumerate(writes):   # every write in its scenario's own type and layout
            host, fmt, offs = chunk_tensor([chunk_samples(name, w, k) for k in range(3)], dtype, layout, bps, channels)
            if layout == PADDED:   # (the Python form takes a padded tensor's channel count from its shape)
                got = writer.write(torch.from_numpy(np.ascontiguousarray(host[:, :channels])).cuda(), lengths)
            else:
                got = writer.write(torch.from_numpy(host).cuda(), lengths, offsets=offs)
            assert got == ragged[name][0][w]
            assert writer.last_status == [0, 0, 0] and writer.last_altered == [0, 0, 0]
        assert writer.frame_numbers == ragged[name][1]
    with BatchEncoder(options_of("mpo7")).open_device_stream_writer(1, rate, bps, channels, max_block, first_numbers=[9]) as writer:
        with pytest.raises(Unsupported):
            writer.write(torch.zeros((1, 2, 4096), dtype=torch.int16, device="cuda"), [4096])
        assert writer.frame_numbers == [9]
    # the example's loop at a small size
    import importlib.util

    spec = importlib.util.spec_from_file_location("stream2frames", os.path.join(ROOT, "examples", "stream2frames.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    frames, kept = mod.stream_frames(n_streams=3, packets=3, sample_rate=8000, channels=2, device="cuda")
    for k, (parts, numbers) in enumerate(mod.decode_back(frames)):
        assert numbers == [0, 1, 2]
        for step, part in enumerate(parts):
            want = torch.clamp(torch.round(kept[step][k].double() * 32768.0), -32768, 32767).to(torch.int32).T.cpu().numpy()
            assert np.array_equal(part, want)


if __name__ == "__main__":   # the child of the `one_by_one` fixture
    sys.path.insert(0, ROOT)
    import torch

    torch.cuda.init()        # torch's HIP runtime first, as tests/conftest.py does
    with open(sys.argv[1], "wb") as f:
        pickle.dump(all_scenarios(), f)
