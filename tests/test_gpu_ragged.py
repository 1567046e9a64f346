"""A RAGGED batch (flacgpu_encode_ragged_device): frames of any length 1 .. block_size, of any streams, as ONE batch on the
generic kernels, each with its frame's own length and window (k_autocorr_ragged, Params::frame_n).

The contract: frame f's bytes are exactly what a one-frame flacgpu_encode_device call gives for the same samples, length
and frame number, whatever else is in the batch.  Every test builds one batch, takes that call on a one-frame context for
each frame as the reference, and then has the whole batch decoded back and compared on the device (samples_differ == 0).

Lengths lie on both sides of the FIXED order (4), the LPC order (12 / 32), the autocorrelation's history and tile (16, 32,
64) and the partition tree (2^k); 256 is the tail of a 10 s clip at 16 kHz; 4096 is a whole block out of the generic chain,
whose reference comes from the wave kernels.  Contents cycle through noise at full scale, a sine, silence (CONSTANT), a
constant, two wasted bits and, for stereo, anti-phase full scale.  Every frame's samples start at an odd element offset of
one device buffer: none is 16-byte aligned by accident."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 1152, 4032, 4095, 4096]
RATE = 16000


def lengths_for(block_size, n_frames=None, seed=5):
    """The list cut at block_size (+ block_size - 1), then ten of them again (more for n_frames), shuffled with a fixed seed."""
    base = [n for n in LENGTHS if n <= block_size]
    if block_size - 1 not in base:
        base.append(block_size - 1)
    rng = np.random.default_rng(seed)
    extra = 10 if n_frames is None else n_frames - len(base)
    out = base + [base[int(i)] for i in rng.integers(0, len(base), extra)]
    return [out[int(i)] for i in rng.permutation(len(out))]


def content(kind, n, channels, bps, rng):
    """[n, channels] int64 samples of `bps` bits"""
    full = 1 << (bps - 1)
    noise = rng.integers(-full, full, (n, channels), dtype=np.int64)
    kind %= 6 if channels == 2 else 5
    if kind == 0:
        return noise
    if kind == 1:
        t = np.arange(n, dtype=np.float64)[:, None]
        return np.rint(0.7 * (full - 1) * np.sin(2 * np.pi * t * (0.01 + 0.003 * np.arange(channels)[None, :]))).astype(np.int64)
    if kind == 2:
        return np.zeros((n, channels), dtype=np.int64)
    if kind == 3:
        return np.tile((np.arange(channels, dtype=np.int64) * 37 + 1234) % (full - 1) * (1 - 2 * (np.arange(channels) % 2)), (n, 1))
    if kind == 4:
        return (noise >> 2) << 2
    left = np.clip(noise[:, 0], -(full - 1), full - 1)
    return np.stack([left, -left], axis=1)


class Batch:
    """One ragged batch in device memory, its frames' one-frame references, and what to ask the encoder for."""

    def __init__(self, channels, bps, block_size, order, exhaustive, lengths, seed, make=content):
        import torch

        self.channels, self.bps, self.block_size, self.order, self.exhaustive = channels, bps, block_size, order, exhaustive
        self.lengths = list(lengths)
        rng = np.random.default_rng(seed)
        self.samples, at, offsets = [], 1, []
        for k, n in enumerate(self.lengths):
            self.samples.append(np.ascontiguousarray(make(k, n, channels, bps, rng).astype(np.int64).astype(np.int32)))
            at |= 1                                   # an odd element offset
            offsets.append(at)
            at += n * channels
        host = np.zeros(at + 8, dtype=np.int32)
        for s, o in zip(self.samples, offsets):
            host[o:o + s.size] = s.reshape(-1)
        self.device = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        base = self.device.data_ptr()
        self.numbers = [(1000 + 37 * k) if k % 7 else 0x7FFFFFF0 + k for k in range(len(self.lengths))]
        self.frames = [(base + 4 * o, n, num) for o, n, num in zip(offsets, self.lengths, self.numbers)]
        assert all((p % 16) != 0 for p, _, _ in self.frames)
        self._reference = None

    def analyzer(self, max_frames):
        from flac_codec_amd.gpu import GpuAnalyzer

        return GpuAnalyzer(self.block_size, 6, self.order, True, self.exhaustive, 2, 0.5, self.bps, self.channels,
                           max_frames=max_frames)

    def reference(self):
        """every frame through a one-frame flacgpu_encode_device call on a one-frame context (computed once)"""
        if self._reference is None:
            an = self.analyzer(1)
            out = []
            for ptr, n, num in self.frames:
                an.encode_device(ptr, 1, n, num, RATE)
                data, off = an.fetch_frames()
                assert off[0] == 0 and off[1] == len(data)
                out.append(data)
            an.close()
            self._reference = out
        return self._reference

    def check(self, an, frames=None, reference=None):
        """encode the batch on `an`, compare every frame with its reference, verify the batch on the device"""
        frames = self.frames if frames is None else frames
        reference = self.reference() if reference is None else reference
        an.encode_ragged_device(frames, RATE)
        data, off = an.fetch_frames()
        assert len(off) == len(frames) + 1 and off[-1] == len(data)
        for f, want in enumerate(reference):
            got = data[off[f]:off[f + 1]]
            assert got == want, (f"frame {f} ({frames[f][1]} samples, number {frames[f][2]}): {len(got)} bytes differ from the "
                                 f"one-frame call's {len(want)}")
        res, _ = an.verify_device(RATE, 0)
        assert (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs, res.samples_differ) == (len(frames), 0, 0, 0, 0)
        return data, off

    def check_decodes(self, data, off):
        """every frame as a raw frame stream of its own through gpu.decode_frames: the input samples"""
        from flac_codec_amd import gpu

        blobs = [data[off[f]:off[f + 1]] for f in range(len(self.lengths))]
        flat, frames, _ = gpu.decode_frames(blobs, out="host")
        assert len(frames) == len(blobs)
        for f, rec in enumerate(frames):
            n = self.lengths[f]
            assert int(rec["stream"]) == f and int(rec["status"]) == 0 and int(rec["block_size"]) == n
            assert int(rec["number"]) == self.numbers[f]
            at = int(rec["out_offset"])
            assert np.array_equal(flat[at:at + n * self.channels].reshape(n, self.channels), self.samples[f]), f"frame {f}"


# (channels, bps, block_size, LPC order, exhaustive channel choice, frames -- None: the list + ten duplicates, decode back too)
SHAPES = {
    "mono16": (1, 16, 4096, 12, True, None, True),
    "mono16_70_frames": (1, 16, 4096, 12, True, 70, False),      # more than 64 candidates: a second workgroup
    "stereo16_exhaustive_lpc32": (2, 16, 4096, 32, True, None, True),
    "stereo24_fast_choice": (2, 24, 4096, 12, False, None, False),   # k_stereo_stats / K0's sums with per-frame lengths
    "stereo32": (2, 32, 4096, 12, True, None, False),             # independent channels, wide samples
    "three_channels_1152": (3, 16, 1152, 12, True, None, False),
    "eight_channels24": (8, 24, 4096, 12, True, None, False),
    "mono16_block16": (1, 16, 16, 12, True, None, False),
    "stereo16_no_lpc": (2, 16, 4096, 0, True, None, False),       # no autocorrelation at all
}
_batches = {}


def batch_of(name):
    if name not in _batches:
        channels, bps, block, order, exhaustive, n_frames, _ = SHAPES[name]
        _batches[name] = Batch(channels, bps, block, order, exhaustive, lengths_for(block, n_frames), 2000 + list(SHAPES).index(name))
    return _batches[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_frame_is_its_one_frame_call(name):
    b = batch_of(name)
    an = b.analyzer(len(b.lengths))
    data, off = b.check(an)
    if SHAPES[name][6]:
        b.check_decodes(data, off)
    an.close()


@pytest.mark.parametrize("name", ["mono16_70_frames", "stereo16_exhaustive_lpc32", "three_channels_1152"])
def test_autocorrelation_rows_are_the_references_bit_for_bit(name):
    """k_autocorr_ragged's sums themselves, not the frames they lead to: every candidate's row of a mixed-length batch (two
    workgroups for the 70 mono frames; lengths on both sides of the tile, the history and the order) against the oracle's
    left fold over that frame's own window, as tests/test_gpu_autocorr_bits.py pins the rest of the kernel family."""
    import _oracle as orc
    from test_gpu_autocorr_bits import candidates_of, device_ac

    b = batch_of(name)
    stereo = b.channels == 2
    ncand = 4 if stereo else b.channels
    an = b.analyzer(len(b.lengths))
    an.encode_ragged_device(b.frames, RATE)
    an.stats()     # (synchronises)
    got = device_ac(an, len(b.lengths) * ncand)
    an.close()
    checked = 0
    for f, n in enumerate(b.lengths):
        w = orc.window(2, 0.5, n)
        for c, row in enumerate(candidates_of(b.samples[f].astype(np.int64).T, stereo)):
            row = np.asarray(row, dtype=np.int64)
            orv = int(np.bitwise_or.reduce(row))
            if orv == 0:
                continue                               # an all-zero candidate gets no LPC analysis
            wasted = (orv & -orv).bit_length() - 1
            want = orc.autocorrelate((row >> wasted).astype(np.float64) * w, b.order)
            lags = min(len(want), n)                   # (lag k of an n-sample frame has terms only for k < n)
            have = got[f * ncand + c][:lags]
            assert np.array_equal(have.view(np.int64), want[:lags].view(np.int64)), (f, n, c, have, want[:lags])
            checked += 1
    assert checked >= len(b.lengths) * ncand // 2      # (the silent frames, and the mid of the anti-phase ones, are skipped)


def test_order_of_the_batch_does_not_matter():
    b = batch_of("mono16")
    an = b.analyzer(len(b.lengths) + 3)           # (a context with room to spare)
    order = list(np.random.default_rng(77).permutation(len(b.lengths)))
    ref = b.reference()
    b.check(an, [b.frames[i] for i in order], [ref[i] for i in order])
    half = order[: len(order) // 2]               # ... nor do the other frames
    b.check(an, [b.frames[i] for i in half], [ref[i] for i in half])
    an.close()


def test_one_workgroup_holds_lengths_1_and_4096_side_by_side():
    b = Batch(1, 16, 4096, 12, True, [1, 4096] * 32, 31)
    an = b.analyzer(64)
    b.check(an)
    an.close()


def test_host_redecision_takes_each_frames_own_length(monkeypatch):
    """resolve_order_ties with the tie knobs of tests/test_gpu_analysis.py: the device's order estimates are skewed inside a
    wide band, so many candidates are re-decided on the host -- from each frame's OWN length.  The bytes must be those of
    the undisturbed run (band 1e-30, no skew).  First-order autoregressive frames, whose orders nearly tie."""
    from scipy.signal import lfilter

    def ar1(k, n, channels, bps, rng):
        return np.stack([np.clip(np.rint(lfilter([1.0], [1.0, -0.9], rng.uniform(-1500, 1500, size=n))), -32768, 32767)
                         for _ in range(channels)], axis=1)

    channels, bps, block, order, exhaustive, _, _ = SHAPES["stereo16_exhaustive_lpc32"]
    b = Batch(channels, bps, block, order, exhaustive, lengths_for(block), 41, make=ar1)

    def run(env):
        for k in ("FLACGPU_TIE_BAND", "FLACGPU_TIE_PERTURB"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("FLACGPU_TEST_KNOBS", "1")   # the tie knobs are test-only: ignored without this
        an = b.analyzer(len(b.lengths))
        an.encode_ragged_device(b.frames, RATE)
        data, off = an.fetch_frames()
        st = an.stats()
        res, _ = an.verify_device(RATE, 0)
        assert (res.bad_structure, res.bad_crc16, res.samples_differ) == (0, 0, 0)
        an.close()
        return data, list(off), st

    plain, off_p, st_p = run({"FLACGPU_TIE_BAND": "1e-30"})
    skew, off_s, _ = run({"FLACGPU_TIE_BAND": "1e-30", "FLACGPU_TIE_PERTURB": "-1e-3"})
    data, off, st = run({"FLACGPU_TIE_BAND": "1e-2", "FLACGPU_TIE_PERTURB": "-1e-3"})
    assert st.order_ties > 0 and st.order_ties_resolved == st.order_ties
    assert (data, off) == (plain, off_p), "the host's re-decision did not restore the undisturbed bytes"
    assert skew != plain, "the skew changed nothing: the test does not exercise the re-decision"
    for k in ("FLACGPU_TIE_BAND", "FLACGPU_TIE_PERTURB", "FLACGPU_TEST_KNOBS"):
        monkeypatch.delenv(k, raising=False)
    ref = b.reference()                                   # (one-frame calls, production settings)
    assert [plain[off_p[f]:off_p[f + 1]] for f in range(len(ref))] == ref


def test_window_pool_is_kept_between_batches():
    b = batch_of("mono16")
    an = b.analyzer(len(b.lengths))
    assert an.ragged_pool_uploads() == 0
    b.check(an)
    assert an.ragged_pool_uploads() == 1
    b.check(an)                                    # the same batch again: nothing uploaded
    assert an.ragged_pool_uploads() == 1
    ref = b.reference()
    some = [f for f in range(len(b.lengths)) if b.lengths[f] in (256, 17, 4095)]
    b.check(an, [b.frames[f] for f in reversed(some)], [ref[f] for f in reversed(some)])   # lengths the pool holds, another order
    assert an.ragged_pool_uploads() == 1
    other = Batch(1, 16, 4096, 12, True, [7, 100, 7, 2048, 4096, 999], 53)   # another set of lengths: a new pool
    other.check(an)
    assert an.ragged_pool_uploads() == 2
    b.check(an)                                    # ... and back
    assert an.ragged_pool_uploads() == 3
    an.close()


def test_refused_batches_launch_nothing_and_keep_the_batch_in_hand():
    from flac_codec_amd.gpu import GpuError

    b = batch_of("mono16")
    an = b.analyzer(len(b.lengths))
    data, off = b.check(an)
    ptr = b.frames[0][0]
    for frames, code, text in (([b.frames[0], (ptr, 0, 5)], -1, "frame 1 has no samples"),
                               ([(ptr, 4097, 5)], -1, "frame 0 has 4097 samples"),
                               (b.frames + [b.frames[0]], -1, "more than the context"),
                               ([], -1, "no frames"),
                               ([(0, 5, 5)], -1, "no PCM")):
        with pytest.raises(GpuError) as e:
            an.encode_ragged_device(frames, RATE)
        assert e.value.code == code and text in str(e.value), str(e.value)
        again, off_again = an.fetch_frames()
        assert again == data and list(off_again) == list(off)
    an.close()
    # the partition order rule of a short last frame: 128 samples under max_partition_order 8
    from flac_codec_amd.gpu import GpuAnalyzer

    an8 = GpuAnalyzer(4000, 8, 12, True, True, 2, 0.5, 16, 1, max_frames=4)
    with pytest.raises(GpuError) as e:
        an8.encode_ragged_device([(ptr, 100, 0), (ptr, 128, 1)], RATE)
    assert e.value.code == -2 and "frame 1 (128 samples)" in str(e.value)
    an8.encode_ragged_device([(ptr, 100, 0), (ptr, 192, 1)], RATE)
    _, off8 = an8.fetch_frames()
    assert len(off8) == 3
    an8.close()
