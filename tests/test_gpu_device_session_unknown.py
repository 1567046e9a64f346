"""flacenc_device_session_open_ex on the GPU: streams whose length is not known when they start (total_known[i] == 0).

The contract: header || frames of every write || tail is byte for byte the file of FlacSampleWriter::new(.., None) fed the
same samples -- the oracle's encode_stream(total_known=False), also compared with flacenc_sample_writer_new(has_total=0).
Nothing expected comes from the sessions.  Padding and gaps of every chunk tensor hold filler, every out / header / tail
buffer has guard bytes round it (the helpers of tests/test_gpu_device_session.py)."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import _oracle as orc
from test_gpu_device_session import (F32, FLAT, I16, I32, NO_MD5, PADDED, S24, Session, _L, _le, as_elements, chunk_tensor,
                                     one_shot, opts, schedule, whole_streams)
from test_stream_header_unknown_total import OPTION_SETS, orc_opts_from

pytestmark = pytest.mark.gpu

NO_SAMPLES, MISMATCH, INVALID_ARG = -118, -117, -140


class SessionEx(Session):
    """Session through flacenc_device_session_open_ex; totals[i] is None: stream i's total is unknown"""

    def __init__(self, o, totals, rate, bps, channels, max_chunk, flags=0, null_known=False, junk=0):
        self.co = o._c_options()
        self.n, self.bps, self.channels, self.block = len(totals), bps, channels, int(self.co.block_size)
        self.h = C.c_void_p()
        arr = (C.c_uint64 * max(self.n, 1))(*[junk if t is None else t for t in totals])   # an unknown stream's entry is ignored
        known = None if null_known else (C.c_uint8 * max(self.n, 1))(*[int(t is not None) for t in totals])
        self.open_rc = _L().flacenc_device_session_open_ex(C.byref(self.co), rate, bps, channels, arr, known, self.n, max_chunk,
                                                           flags, C.byref(self.h))
        self.frames = [b""] * self.n
        self.pending = [0] * self.n


def options_of(block, name="default"):
    return OPTION_SETS[name][0](opts(block))


@functools.lru_cache(maxsize=None)
def unknown_total_files(block, seed, totals, channels, bps, rate, name="default"):
    """the files of FlacSampleWriter::new(.., None): the oracle's, and equal to them the host writer's; once per shape"""
    from flac_codec_amd.encode import FlacSampleWriter

    files = []
    for s in whole_streams(seed, totals, channels, bps):
        if not len(s):   # (no file: FlacSampleWriter's finalize gives NoSamples)
            files.append(None)
            continue
        o = options_of(block, name)
        rc, ref, _ = orc.encode_stream(orc_opts_from(o), rate, bps, channels, s.reshape(-1), total_known=False,
                                       tags=OPTION_SETS[name][1])
        assert rc == 0
        w = FlacSampleWriter(None, o, rate, bps, channels, None)
        w.write(s.reshape(-1))
        w.finalize()
        assert w.getvalue() == ref, "flacenc_sample_writer_new(has_total=0) differs from the oracle"
        w.close()
        files.append(ref)
    return tuple(files)


def feed(s, streams, writes, formats, bps, channels):
    at = [0] * len(streams)
    for w, take in enumerate(writes):
        dtype, layout = formats[w % len(formats)]
        pieces = [streams[k][at[k]:at[k] + take[k]] for k in range(len(streams))]
        host, fmt, offs = chunk_tensor(pieces, dtype, layout, bps, channels)
        rc, status, altered, out = s.write(host, fmt, offs, take)
        assert rc == 0 and status == [0] * len(streams) and altered == [0] * len(streams), (w, rc, status)
        for k in range(len(streams)):   # exactly the blocks that this write completes
            assert (len(out[k]) > 0) == ((at[k] + take[k]) // s.block > at[k] // s.block), (w, k)
        at = [a + b for a, b in zip(at, take)]
    return at


def run_unknown(block, seed, totals, channels, bps, writes, formats, rate=44100, flags=0, name="default"):
    streams = whole_streams(seed, tuple(totals), channels, bps)
    want = unknown_total_files(block, seed, tuple(totals), channels, bps, rate, name)
    s = SessionEx(options_of(block, name), [None] * len(totals), rate, bps, channels, max(max(w) for w in writes), flags,
                  junk=5)   # (a junk total below every stream's length: it must be ignored)
    assert s.open_rc == 0
    hlens = [int(_L().flacenc_device_session_header_len(s.h, k)) for k in range(len(totals))]
    assert feed(s, streams, writes, formats, bps, channels) == list(totals)
    rc, fin = s.finalize()
    assert rc == 0
    for k, (st, header, tail, altered, md5) in enumerate(fin):
        assert st == 0 and altered == 0
        assert len(header) == hlens[k] == int(_L().flacenc_device_session_header_len(s.h, k))   # fixed at open
        assert (len(tail) > 0) == (totals[k] % block != 0)
        digest = hashlib.md5(_le(streams[k], bps)).digest()
        expect = want[k]
        assert expect[26:42] == digest
        if flags & NO_MD5:
            digest = bytes(16)
            expect = expect[:26] + digest + expect[42:]
        assert md5 == digest
        assert header + s.frames[k] + tail == expect, f"stream {k} of {totals}: bytes differ"
    s.close()


def test_stereo_16_bit_block_4096_int16_padded():
    """carries of 1 and 4095 samples (x 2 channels: no multiple of 4 elements, the gather route) and of 0 (in place);
    chunks of 0, 1, 4095, 4096 and 4097 samples"""
    totals = (1, 4096, 2 * 4096 + 5)
    writes = schedule(totals, [1, 4095, 4097, 0, 4096])
    assert {v for w in writes for v in w} >= {0, 1, 4095, 4096, 4097}
    run_unknown(4096, 21, totals, 2, 16, writes, [(I16, PADDED)])


def test_mono_24_bit_block_192_s24_padded():
    totals = (191, 192, 385)
    run_unknown(192, 22, totals, 1, 24, schedule(totals, [100, 0, 191, 1, 193]), [(S24, PADDED)], rate=48000)


def test_stereo_32_bit_block_256_int32_flat():
    totals = (255, 256, 3 * 256 + 7)
    run_unknown(256, 23, totals, 2, 32, schedule(totals, [300, 7, 0, 256]), [(I32, FLAT)], rate=96000)


@pytest.mark.parametrize("name", [n for n in OPTION_SETS if n != "default"])
def test_header_options(name):
    """a PADDING block too small for the seek table, none, no seek table, one point per frame, a tag"""
    totals = (1, 4096, 2 * 4096 + 5)
    run_unknown(4096, 21, totals, 2, 16, schedule(totals, [4097, 1, 4096]), [(I16, PADDED)], name=name)


def test_no_md5():
    totals = (1, 4096, 2 * 4096 + 5)
    run_unknown(4096, 21, totals, 2, 16, schedule(totals, [4096, 4097]), [(I16, PADDED)], flags=NO_MD5)


def test_known_and_unknown_streams_in_one_session():
    block, totals, rate = 256, (2 * 256 + 9, 3 * 256, 77), 44100
    streams = whole_streams(24, totals, 2, 16)
    writes = schedule(totals, [130, 0, 300, 41])
    formats = [(F32, PADDED), (I16, FLAT)]
    # today's open, every total declared
    known = Session(opts(block), totals, rate, 16, 2, 300)
    feed(known, streams, writes, formats, 16, 2)
    rc, kfin = known.finalize()
    assert rc == 0
    for k, w in enumerate(one_shot(block, 24, totals, 2, 16, rate)):
        assert kfin[k][1] + known.frames[k] + kfin[k][2] == w[1]
    # stream 0 known, streams 1 and 2 not
    mixed = SessionEx(opts(block), [totals[0], None, None], rate, 16, 2, 300)
    assert mixed.open_rc == 0
    feed(mixed, streams, writes, formats, 16, 2)
    rc, mfin = mixed.finalize()
    assert rc == 0
    assert mfin[0] == kfin[0] and mixed.frames[0] == known.frames[0]
    want = unknown_total_files(block, 24, totals, 2, 16, rate)
    for k in (1, 2):
        assert mixed.frames[k] == known.frames[k] and mfin[k][2] == kfin[k][2]      # frames and tail do not depend on the total
        assert mfin[k][3:] == kfin[k][3:]                                            # nor do altered and md5
        assert mfin[k][1] != kfin[k][1]                                              # the header does
        assert mfin[k][1] + mixed.frames[k] + mfin[k][2] == want[k]
    known.close()
    mixed.close()


def test_a_stream_that_receives_nothing():
    block, totals, rate = 256, (300, 0, 256), 44100
    streams = whole_streams(25, totals, 1, 16)
    want = unknown_total_files(block, 25, totals, 1, 16, rate)
    s = SessionEx(opts(block), [None] * 3, rate, 16, 1, 200)
    assert s.open_rc == 0 and _L().flacenc_device_session_header_len(s.h, 1) == _L().flacenc_device_session_header_len(s.h, 0) > 0
    feed(s, streams, schedule(totals, [200, 100]), [(I16, PADDED)], 16, 1)
    rc, fin = s.finalize()   # (Session.finalize asserts that nothing but header_len / tail_len bytes was written)
    assert rc == NO_SAMPLES and [f[0] for f in fin] == [0, NO_SAMPLES, 0]
    assert fin[1][1:3] == (b"", b"") and fin[1][4] == bytes(16)
    assert fin[0][1] + s.frames[0] + fin[0][2] == want[0] and fin[2][1] + s.frames[2] + fin[2][2] == want[2]
    s.close()


def test_a_known_stream_keeps_its_checks_beside_an_unknown_one():
    block, rate = 64, 44100
    streams = whole_streams(26, (200, 200), 1, 16)
    s = SessionEx(opts(block), [150, None], rate, 16, 1, 200)
    host, fmt, offs = chunk_tensor([streams[0][:151], streams[1][:151]], I16, PADDED, 16, 1)
    rc, status, _, _ = s.write(host, fmt, offs, [151, 151])               # past stream 0's declared total: refused as a whole
    assert rc == INVALID_ARG and b"total" in _L().flacenc_last_error()
    host, fmt, offs = chunk_tensor([streams[0][:100], streams[1]], I16, PADDED, 16, 1)
    rc, status, _, _ = s.write(host, fmt, offs, [100, 200])               # the unknown stream may take any amount
    assert rc == 0 and status == [0, 0]
    rc, fin = s.finalize()
    assert rc == MISMATCH and [f[0] for f in fin] == [MISMATCH, 0]        # SampleCountMismatch is a known total's error
    want = unknown_total_files(block, 26, (200, 200), 1, 16, rate)
    assert fin[1][1] + s.frames[1] + fin[1][2] == want[1]
    s.close()
    # a declared total of 0 is still dead at open; an unknown one beside it is not
    s = SessionEx(opts(block), [0, None], rate, 16, 1, 200)
    assert s.open_rc == 0 and _L().flacenc_device_session_header_len(s.h, 0) == 0 < _L().flacenc_device_session_header_len(s.h, 1)
    s.close()
    # totals may be NULL when no stream declares one, and only then
    h = C.c_void_p()
    co = opts(block)._c_options()
    none, one = (C.c_uint8 * 2)(0, 0), (C.c_uint8 * 2)(0, 1)
    assert _L().flacenc_device_session_open_ex(C.byref(co), rate, 16, 1, None, one, 2, 100, 0, C.byref(h)) == INVALID_ARG
    assert _L().flacenc_device_session_open_ex(C.byref(co), rate, 16, 1, None, none, 2, 100, 0, C.byref(h)) == 0
    _L().flacenc_device_session_close(h)


def test_total_known_null_is_open():
    block, totals, rate = 256, (700, 256, 5), 22050
    streams = whole_streams(27, totals, 2, 16)
    writes = schedule(totals, [256, 33, 300])
    got = []
    for ex in (False, True):
        s = SessionEx(opts(block), list(totals), rate, 16, 2, 300, null_known=True) if ex else Session(opts(block), totals, rate, 16, 2, 300)
        assert s.open_rc == 0
        feed(s, streams, writes, [(I16, FLAT)], 16, 2)
        rc, fin = s.finalize()
        assert rc == 0
        got.append([(f, s.frames[k]) for k, f in enumerate(fin)])
        s.close()
    assert got[0] == got[1]
    for k, w in enumerate(one_shot(block, 27, totals, 2, 16, rate)):
        assert got[1][k][0][1] + got[1][k][1] + got[1][k][0][2] == w[1]
    # ... and its dead-at-open rule
    s = SessionEx(opts(block), [0, 10], rate, 16, 2, 300, null_known=True)
    assert s.open_rc == 0 and _L().flacenc_device_session_header_len(s.h, 0) == 0
    s.close()


def test_python_sessions_with_none_totals_and_the_examples_loop():
    import torch

    from flac_codec_amd.encode import BatchEncoder

    block, totals, rate = 256, (1000, 777, 256), 22050
    streams = whole_streams(28, totals, 2, 16)
    want = unknown_total_files(block, 28, totals, 2, 16, rate)
    known = one_shot(block, 28, totals, 2, 16, rate)
    full = np.zeros((3, 2, 1000), dtype=np.float32)
    for k, s in enumerate(streams):
        full[k, :, :len(s)] = as_elements(s, F32, 16).T
    dev = torch.from_numpy(full).cuda()
    enc = BatchEncoder(opts(block))
    for declared, expect in (((None, 777, None), (want[0], known[1][1], want[2])), (None, want)):
        with enc.open_device_session(declared, rate, 16, 2, max_chunk=300, n_streams=3) as ses:
            for a in range(0, 1000, 300):
                ses.write(dev[:, :, a:a + 300].contiguous(), [max(0, min(t, a + 300) - a) for t in totals])
            files = ses.finalize()
        assert files == list(expect)
    with pytest.raises(ValueError):
        enc.open_device_session(None, rate, 16, 2, max_chunk=300)
    # the example's loop with --unknown-total, at a small size
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "stream2flac.py")
    spec = importlib.util.spec_from_file_location("stream2flac", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    files, clips = mod.stream_clips(n_clips=3, seconds=2.5, sample_rate=8000, channels=1, device=dev.device, unknown_total=True)
    q = torch.clamp(torch.round(clips.double() * 32768.0), -32768, 32767).to(torch.int32).cpu().numpy()
    for k in range(3):
        rc, ref, _ = orc.encode_stream(orc_opts_from(mod.options()), 8000, 16, 1, q[k].T.reshape(-1), total_known=False)
        assert rc == 0 and files[k] == ref
