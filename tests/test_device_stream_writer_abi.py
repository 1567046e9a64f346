"""flacenc_device_stream_writer_plan on the host alone: every refusal with its code, in FlacStreamWriter's order
(the options at `new`; then write's checks, encode.rs:1104-1137: bits per sample outside 1..32, the channel count, the
block size, the subset sample rate, the subset bits per sample), then what flacenc_device_batch_plan refuses for the
shape; and the staging buffer's size."""
import ctypes as C

import pytest

OK, INVALID_ARG, UNSUPPORTED = 0, -140, -151
INVALID_BLOCK_SIZE, INVALID_LPC_ORDER, INVALID_MAX_PARTITIONS, EXCESSIVE_PADDING = -101, -102, -103, -104
INVALID_SAMPLE_RATE, EXCESSIVE_CHANNELS, NON_SUBSET_RATE, NON_SUBSET_BPS = -111, -112, -122, -123


def plan(co, rate=44100, bps=16, channels=2, n=3, max_block=4096, want_bytes=True):
    from flac_codec_amd.encode import _stream_lib

    size = C.c_size_t(12345)
    rc = _stream_lib().flacenc_device_stream_writer_plan(C.byref(co) if co is not None else None, rate, bps, channels, n,
                                                         max_block, C.byref(size) if want_bytes else None)
    if rc != 0:
        assert size.value == 12345   # a refusal writes nothing
    return rc, size.value


def default_options():
    from flac_codec_amd.encode import Options

    return Options.default()._c_options()


@pytest.mark.parametrize("channels,max_block,n,elements", [
    (1, 17, 3, 20),          # 17 elements rounded up to 16 bytes
    (2, 4096, 3, 8192),
    (8, 65535, 2, 524280),   # 65535 * 8 is a multiple of 4 already
    (3, 1, 5, 4),
    (2, 4096, 0, 0),
])
def test_device_bytes(channels, max_block, n, elements):
    assert plan(default_options(), channels=channels, max_block=max_block, n=n) == (OK, 4 * elements * n)
    assert plan(default_options(), channels=channels, max_block=max_block, n=n, want_bytes=False)[0] == OK


def test_refusals_and_their_codes():
    co = default_options()
    assert plan(None)[0] == INVALID_ARG
    # the options (FlacStreamWriter::new takes validated Options); block_size is checked although nothing else uses it
    for field, value, code in [("block_size", 15, INVALID_BLOCK_SIZE), ("block_size", 65536, INVALID_BLOCK_SIZE),
                               ("max_lpc_order", 33, INVALID_LPC_ORDER), ("max_partition_order", 16, INVALID_MAX_PARTITIONS),
                               ("padding", 1 << 24, EXCESSIVE_PADDING)]:
        bad = default_options()
        setattr(bad, field, value)
        assert plan(bad)[0] == code, field
    # block_size is otherwise ignored: any legal value plans the same buffer
    small = default_options()
    small.block_size = 16
    assert plan(small, max_block=65535) == plan(co, max_block=65535) == (OK, 4 * 131072 * 3)   # 131070 rounded up
    # bits per sample outside 1..32, then the channel count, then the block size
    assert plan(co, bps=0)[0] == NON_SUBSET_BPS and plan(co, bps=33)[0] == NON_SUBSET_BPS
    assert plan(co, channels=0)[0] == EXCESSIVE_CHANNELS and plan(co, channels=9)[0] == EXCESSIVE_CHANNELS
    assert plan(co, max_block=0)[0] == INVALID_BLOCK_SIZE and plan(co, max_block=65536)[0] == INVALID_BLOCK_SIZE
    # the subset sample rate: every rate a frame header codes is fine, the others are not
    for rate in (44100, 22051, 12340, 65534, 655340, 254000, 192000, 1):
        assert plan(co, rate=rate)[0] == OK, rate
    for rate in (65535, 655351, 700001):
        assert plan(co, rate=rate)[0] == NON_SUBSET_RATE, rate
    assert plan(co, rate=1 << 20)[0] == INVALID_SAMPLE_RATE
    # the subset bits per sample
    for bps in (8, 12, 16, 20, 24, 32):
        assert plan(co, bps=bps)[0] == OK
    for bps in (1, 7, 15, 17, 28, 31):
        assert plan(co, bps=bps)[0] == NON_SUBSET_BPS, bps
    # the order: an earlier check wins
    bad = default_options()
    bad.max_lpc_order = 33
    assert plan(bad, bps=0, channels=9, max_block=0, rate=65535)[0] == INVALID_LPC_ORDER
    assert plan(co, bps=0, channels=9, max_block=0, rate=65535)[0] == NON_SUBSET_BPS
    assert plan(co, bps=15, channels=9, max_block=0, rate=65535)[0] == EXCESSIVE_CHANNELS
    assert plan(co, bps=15, channels=2, max_block=0, rate=65535)[0] == INVALID_BLOCK_SIZE
    assert plan(co, bps=15, channels=2, max_block=16, rate=65535)[0] == NON_SUBSET_RATE
    assert plan(co, bps=15, channels=2, max_block=16, rate=44100)[0] == NON_SUBSET_BPS
    # what the batch plan refuses for the shape
    assert plan(co, n=1 << 32)[0] == UNSUPPORTED
    # ... and the largest count it takes is answered without building anything of that size
    assert plan(co, n=(1 << 32) - 1) == (OK, 4 * 8192 * ((1 << 32) - 1))


def test_open_runs_the_same_checks_before_it_touches_a_device():
    from flac_codec_amd.encode import _stream_lib

    L = _stream_lib()
    co = default_options()
    h = C.c_void_p(77)
    assert L.flacenc_device_stream_writer_open(C.byref(co), 65535, 16, 2, 3, 4096, None, C.byref(h)) == NON_SUBSET_RATE
    assert h.value is None
    assert L.flacenc_device_stream_writer_open(C.byref(co), 44100, 16, 2, 3, 65536, None, C.byref(h)) == INVALID_BLOCK_SIZE
    assert L.flacenc_device_stream_writer_open(C.byref(co), 44100, 16, 2, 3, 4096, None, None) == INVALID_ARG
    first = (C.c_uint64 * 3)(0, 1 << 36, 0)   # above FrameNumber::MAX_FRAME_NUMBER
    assert L.flacenc_device_stream_writer_open(C.byref(co), 44100, 16, 2, 3, 4096, first, C.byref(h)) == -119
    # the other entry points on NULL
    assert L.flacenc_device_stream_writer_frame_number(None, 0) == 0
    assert L.flacenc_device_stream_writer_write(None, None, None, None, None) == INVALID_ARG
    L.flacenc_device_stream_writer_close(None)
