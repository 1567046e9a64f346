"""The asynchronous host path (flacgpu_encode_packed_async / frames_ready / fetch_frames_async /
wait): PCM uploaded at its stream width -- the little-endian bytes FlacByteWriter::write receives
and update_md5 hashes (/root/reference/src/encode.rs:359, 1292-1318) -- and widened by K0 on the
device must give exactly the oracle's frame bytes; and the pipelined writers built on it (several
batches in flight, MD5 on its own thread) exactly the oracle's .flac."""
import numpy as np
import pytest

import _oracle as orc
from _compare import orc_options_for, planar_frames
from _pcm import synth_fast

pytestmark = pytest.mark.gpu


def le_bytes(pcm, width):
    a = np.asarray(pcm, dtype="<i4").view(np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(a[:, :width]).reshape(-1)


def run_packed(pcm, channels, bps, block_size=4096, max_po=6, max_lpc=12, rate=48000, first_frame=7,
               pinned=True):
    from flac_codec_amd.gpu import GpuAnalyzer

    frames = planar_frames(pcm, channels, block_size)
    n_frames, last = len(frames), frames[-1].shape[1]
    width = (bps + 7) // 8
    an = GpuAnalyzer(block_size, max_po, max_lpc, True, True, 2, 0.5, bps, channels, max_frames=n_frames)
    used = pcm[: ((n_frames - 1) * block_size + last) * channels]
    supported = an.packed_input_supported(width)
    data, off = an.encode_packed(le_bytes(used, width if supported else 4), width if supported else 4,
                                 n_frames, last, first_frame, rate, pinned=pinned)
    oopts = orc_options_for(block_size, max_po, max_lpc, True, True)
    for f, planar in enumerate(frames):
        rc, fb, _ = orc.encode_frame(oopts, rate, bps, planar, frame_number=first_frame + f)
        assert rc == 0
        assert data[off[f]:off[f + 1]] == fb, f"frame {f} differs from the oracle (width {width}, supported {supported})"
    an.close()
    return supported


@pytest.mark.parametrize("channels,bps", [(2, 24), (2, 16), (1, 8), (2, 20), (3, 24), (8, 24), (1, 16),
                                          (5, 16), (6, 12), (2, 32)])
def test_packed_upload_matches_oracle(channels, bps):
    pcm = synth_fast(900 + channels * 40 + bps, channels, bps, 4096 * 5 + 777)
    supported = run_packed(pcm, channels, bps, max_lpc=12 if bps <= 24 else 8)
    assert supported == (bps <= 24)


def test_packed_other_block_sizes_and_pageable_memory():
    # 1152: a whole number of 16-byte groups for stereo 16-bit; 4608 with 3 channels x 3 bytes too
    assert run_packed(synth_fast(950, 2, 16, 1152 * 7 + 100), 2, 16, block_size=1152, max_po=3, max_lpc=0)
    assert run_packed(synth_fast(951, 3, 24, 4608 * 3), 3, 24, block_size=4608, max_po=5, max_lpc=8)
    # a block that is not a whole number of 16-byte groups is refused (the caller widens on the host)
    assert not run_packed(synth_fast(952, 1, 8, 1004 * 3), 1, 8, block_size=1004, max_po=2, max_lpc=4)
    assert run_packed(synth_fast(953, 2, 24, 4096 * 3), 2, 24, pinned=False)


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_pipelined_writer_byte_identical(depth):
    from flac_codec_amd.encode import FlacByteWriter, FlacSampleWriter, Options

    for (ch, bps, n, chunk) in [(2, 24, 4096 * 37 + 1234, 50000), (2, 16, 4096 * 20, 4096 * 2 * 3 + 1),
                                (1, 8, 4096 * 9 + 5, 1 << 20), (4, 20, 4096 * 11 + 17, 33333)]:
        pcm = synth_fast(700 + ch + bps + depth, ch, bps, n)
        opts = Options.best().batch_frames(8).pipeline_depth(depth)
        w = FlacSampleWriter(None, opts, 44100, bps, ch, pcm.size)
        for i in range(0, pcm.size, chunk):
            w.write(pcm[i:i + chunk])
        w.finalize()
        data = w.getvalue()
        w.close()
        rc, ref, _ = orc.encode_stream(orc.options("best"), 44100, bps, ch, pcm, total_known=True)
        assert rc == 0 and data == ref, f"sample writer differs (ch {ch} bps {bps} depth {depth})"
        # FlacByteWriter on the same PCM as little-endian bytes, total unknown
        raw = le_bytes(pcm, (bps + 7) // 8).tobytes()
        bw = FlacByteWriter(None, Options.best().batch_frames(8).pipeline_depth(depth), 44100, bps, ch)
        for i in range(0, len(raw), 77777):
            bw.write(raw[i:i + 77777])
        bw.finalize()
        bdata = bw.getvalue()
        bw.close()
        rc, ref2, _ = orc.encode_stream(orc.options("best"), 44100, bps, ch, pcm, total_known=False)
        assert rc == 0 and bdata == ref2, f"byte writer differs (ch {ch} bps {bps} depth {depth})"


def test_excessive_total_samples_with_batches_in_flight():
    """12 blocks written in batches of 4, three in flight, against a smaller declared total: the error is raised before the
    offending frame is encoded (encode.rs:2006-2011), so behind the header stand exactly the frames in front of it -- the
    oracle's, whose bytes do not depend on the total.  (samples_written in flacenc_writer_stats is set at finalize only:
    the bytes are compared, not the counters.)"""
    from flac_codec_amd import encode as E
    from flac_codec_amd import gpu
    from test_stream_header_unknown_total import header_len

    B = 4096
    pcm = synth_fast(990, 2, 16, B * 12)
    rc, ref, _ = orc.encode_stream(orc.options("default"), 44100, 16, 2, pcm, total_known=True)
    assert rc == 0
    _, offsets, _ = gpu.scan_stream_host(ref)
    starts = [int(v) for v in offsets] + [len(ref)]
    assert len(starts) == 13
    # (total per channel, frames in front of the excess): a batch's first block; mid-batch; a block where the total leaves
    # room for a short last block of 100 samples only
    for total, usable in ((8 * B, 8), (6 * B, 6), (5 * B + 100, 5)):
        for host_pack in (False, True):
            opts = E.Options.default().batch_frames(4).pipeline_depth(3).host_pack(host_pack)
            w = E.FlacSampleWriter(None, opts, 44100, 16, 2, total * 2)
            with pytest.raises(E.ExcessiveTotalSamples):
                w.write(pcm)
            data = w.getvalue()
            w.close()
            rc, hlen = header_len(opts._c_options(), 1, total)
            assert rc == 0
            assert data[hlen:] == ref[starts[0]:starts[usable]], (total, host_pack, len(data) - hlen)


def test_batch_front_end_matches_oracle():
    """flacenc_encode_many: streams of different lengths, more streams than worker threads."""
    from flac_codec_amd.encode import BatchEncoder, Options

    streams = [synth_fast(1200 + i, 2, 16, 4096 * (3 + 5 * i) + 100 * i) for i in range(7)]
    be = BatchEncoder(Options.default().batch_frames(16), threads=3)
    for rep in range(2):   # the second call reuses lanes and output buffers
        outs = be.encode(streams, 44100, 16, 2)
        for s, o in zip(streams, outs):
            rc, ref, _ = orc.encode_stream(orc.options("default"), 44100, 16, 2, s, total_known=True)
            assert rc == 0 and o == ref


@pytest.mark.parametrize("threads", [1, 2, 5])
def test_batch_front_end_more_streams_than_open_slots(threads):
    """flacenc_encode_many keeps at most 64 streams open (submit and finish phases are claimed separately by its
    workers): 70 short streams with one, two and five threads -- the last streams are submitted only after the first
    ones were finished --, every one the oracle's."""
    from flac_codec_amd.encode import BatchEncoder, Options

    streams = [synth_fast(1400 + i, 2, 16, 1152 * (1 + i % 4) + 11 * i) for i in range(70)]
    streams = [s[: s.size - s.size % 2] for s in streams]
    be = BatchEncoder(Options.fast().batch_frames(4), threads=threads)
    outs = be.encode(streams, 44100, 16, 2)
    assert len(outs) == 70
    for i in (0, 1, 33, 63, 64, 65, 69):
        rc, ref, _ = orc.encode_stream(orc.options("fast"), 44100, 16, 2, streams[i], total_known=True)
        assert rc == 0 and outs[i] == ref, i
    refs = {i: orc.encode_stream(orc.options("fast"), 44100, 16, 2, streams[i], total_known=True)[1] for i in range(70)}
    assert all(outs[i] == refs[i] for i in range(70))


def test_many_writers_on_the_shared_md5_engines():
    """More concurrent streams than one engine has lanes, 24-bit (3-byte samples: runs that are no multiple of
    the 64-byte MD5 block), ragged lengths, sleeping waits: every finished stream -- STREAMINFO MD5 included --
    must be the oracle's."""
    import hashlib

    from flac_codec_amd.encode import BatchEncoder, Options

    streams = [synth_fast(1300 + i, 2, 24, 4096 * (2 + (7 * i) % 11) + 37 * i + (i % 3)) for i in range(40)]
    streams = [s[: s.size - s.size % 2] for s in streams]
    be = BatchEncoder(Options.best().batch_frames(8), threads=40)
    outs = be.encode(streams, 48000, 24, 2)
    for s, o in zip(streams, outs):
        rc, ref, _ = orc.encode_stream(orc.options("best"), 48000, 24, 2, s, total_known=True)
        assert rc == 0 and o == ref
        le3 = s.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        assert o[26:42] == hashlib.md5(le3).digest()      # STREAMINFO: 4 + 4 + 18 bytes in front of the MD5
