"""flacgpu_meta_feed_host -- the resumable metadata walk (csrc/kernels/meta_feed_rule.h, the function k_meta_feed runs,
compiled for the host) -- against flacgpu_meta_walk_host on the concatenation, on the CPU: fed in any cuts it must consume
exactly the chain, and give the same info, min_frame, frames_at and refusal.  The Python model
(_container_session_model.MetaFeed) is held to the same answers."""
import ctypes as C
import random

import pytest

import _container_session_model as cm
import _meta_cases as mc

ERR_INVALID_ARG = -1
FRAME = bytes([0xFF, 0xF8, 0x19, 0x08, 0x00]) + bytes(40)   # what follows a chain: never looked at by the walk


def _info_tuple(info):
    return (info.sample_rate, info.channels, info.bits_per_sample, info.min_block, info.max_block, info.total_samples,
            bytes(info.md5), info.frames, info.decoded_samples, info.bad_frames, info.bad_crc16, info.md5_status)


def walk_whole(blob):
    """(rc, info fields, min_frame, frames_at) of flacgpu_meta_walk_host."""
    from flac_codec_amd import _lib

    info, mf, at = _lib.StreamInfo(), C.c_uint32(0xEE), C.c_uint64(0xEE)
    rc = _lib.lib().flacgpu_meta_walk_host(blob, len(blob), C.byref(info), C.byref(mf), C.byref(at))
    return rc, _info_tuple(info), mf.value, at.value


def walk_fed(blob, cuts):
    """The same through flacgpu_meta_feed_host, chunk by chunk (`cuts`: ascending chunk ends, the last len(blob)), with
    the bytes every feed consumed."""
    from flac_codec_amd import _lib

    L = _lib.lib()
    st = _lib.MetaFeedState()
    L.flacgpu_meta_feed_init_host(C.byref(st))
    model = cm.MetaFeed()
    used, at = [], 0
    for c in cuts:
        n = C.c_size_t(0xEE)
        chunk = blob[at:c]
        assert L.flacgpu_meta_feed_host(C.byref(st), chunk if chunk else None, len(chunk), C.byref(n)) == 0
        assert n.value == model.feed(chunk)
        used.append(n.value)
        at = c
    info, mf, fa = _lib.StreamInfo(), C.c_uint32(0xEE), C.c_uint64(0xEE)
    rc = L.flacgpu_meta_feed_result_host(C.byref(st), len(blob), C.byref(info), C.byref(mf), C.byref(fa))
    refused, m_mf, m_f, m_at = model.result(len(blob))
    assert (rc != 0, fa.value) == (refused, m_at) and mf.value == m_mf
    if m_f:
        assert (info.sample_rate, info.channels, info.bits_per_sample) == (m_f["sample_rate"], m_f["channels"], m_f["bits_per_sample"])
    assert C.sizeof(st) == 104 and model.state_bytes() <= 4 + 34 + 34   # whatever the chain's length
    return (rc, _info_tuple(info), mf.value, fa.value), used


def _agrees(blob, cuts, label):
    want = walk_whole(blob)
    got, used = walk_fed(blob, cuts)
    assert got == want, label
    if want[0] == 0:   # accepted: the feeds consumed the chain and nothing else, each its own share
        at, chain = 0, want[3]
        for c, n in zip(cuts, used):
            assert n == max(0, min(c, chain) - at), (label, c)
            at = c
        assert sum(used) == chain, label


def chains():
    si = mc.streaminfo(rate=48000, channels=2, bits=24, min_frame=14)
    seek = bytes(range(36))   # two seek points' worth of bytes: the walk does not read them
    return [
        ("STREAMINFO alone", mc.chain([(0, si)]) + FRAME),
        ("STREAMINFO + SEEKTABLE + PADDING", mc.chain([(0, si), (3, seek), (1, bytes(77))]) + FRAME),
        ("two STREAMINFO blocks: the last wins",
         mc.chain([(0, mc.streaminfo(rate=8000, bits=8, md5=bytes(16))), (1, bytes(3)), (0, si)]) + FRAME),
        ("the second STREAMINFO never whole: the first stays", mc.chain([(0, mc.streaminfo(rate=8000, bits=8)), (0, si)])[:-1]),
        ("a wrong marker", b"fLaX" + mc.chain([(0, si)])[4:] + FRAME),
        ("a type-0 block of length 33", mc.chain([(0, si[:33])]) + bytes(8) + FRAME),
        ("a type-0 block of length 33, then a STREAMINFO", mc.chain([(0, si[:33]), (0, si)]) + FRAME),
        ("no block with the last flag before the input ends", mc.chain([(0, si), (1, bytes(9))], last=False)),
        ("the last flag on a zero-length block", mc.chain([(0, si), (1, b"")]) + FRAME),
        ("max_block 0: unusable", mc.chain([(0, mc.streaminfo(min_block=0, max_block=0))]) + FRAME),
        ("no STREAMINFO at all", mc.chain([(4, b"x" * 50)]) + FRAME),
        ("the metadata ends with the input", mc.chain([(0, si), (4, b"comment")])),
    ]


def test_the_new_symbols_are_exported():
    from flac_codec_amd import _lib

    for name in ("flacgpu_meta_feed_init_host", "flacgpu_meta_feed_host", "flacgpu_meta_feed_result_host",
                 "flacgpu_session_host_open_container", "flacgpu_decoder_session_open_container",
                 "flacgpu_decoder_session_verdict"):
        assert name in _lib.exported_symbols(), name


@pytest.mark.parametrize("label,blob", chains(), ids=[c[0] for c in chains()])
def test_every_single_cut(label, blob):
    _agrees(blob, [len(blob)], f"{label}: whole")
    for cut in range(0, len(blob) + 1):
        _agrees(blob, [cut, len(blob)], f"{label}: cut at {cut}")


def test_seeded_multi_cuts():
    rng = random.Random(20261101)
    cs = chains()
    for k in range(200):
        label, blob = cs[k % len(cs)]
        cuts = cm.multi_cut(rng, len(blob), lo=1, hi=30)
        _agrees(blob, cuts, f"case {k}: {label}")


def test_every_input_of_the_one_shot_walk_cut_at_three_places():
    rng = random.Random(20261102)
    for label, blob in mc.truncations() + mc.edges():
        n = len(blob)
        cuts = sorted(rng.randint(0, n) for _ in range(3)) + [n]
        _agrees(blob, cuts, label)


def test_a_long_block_is_passed_by_count_and_the_session_holds_none_of_it():
    """A 70 000-byte APPLICATION block in 1 KiB pieces: every piece is consumed whole, the state stays its 104 bytes, and
    a host container session fed the same pieces holds no byte while the stream is in its metadata."""
    from flac_codec_amd import _lib

    si = mc.streaminfo()
    blob = mc.chain([(0, si), (2, b"appl" + bytes(range(256)) * 273 + bytes(108)), (1, bytes(10))]) + FRAME
    chain = walk_whole(blob)[3]
    assert chain > 70000
    cuts = list(range(1024, len(blob), 1024)) + [len(blob)]
    _agrees(blob, cuts, "70 000-byte APPLICATION")
    L = _lib.lib()
    h = C.c_void_p()
    assert L.flacgpu_session_host_open_container(1, 1024, C.byref(h)) == 0
    at = 0
    for c in cuts:
        chunk = blob[at:c]
        data = (C.c_void_p * 1)(C.cast(C.c_char_p(chunk), C.c_void_p))
        held, total = (C.c_uint64 * 1)(0xEE), C.c_uint64(0xEE)
        raw = (_lib.RawStream * 1)()
        assert L.flacgpu_session_host_feed(h, data, (C.c_size_t * 1)(len(chunk)), None, None, 0, raw, held, C.byref(total)) == 0
        assert total.value == 0 and (held[0] == 0 or c >= chain) and raw[0].uniform == int(c >= chain), c
        at = c
    L.flacgpu_session_host_close(h)


def test_refusals():
    from flac_codec_amd import _lib

    L = _lib.lib()
    st, n = _lib.MetaFeedState(), C.c_size_t(0)
    L.flacgpu_meta_feed_init_host(C.byref(st))
    assert L.flacgpu_meta_feed_host(None, b"x", 1, C.byref(n)) == ERR_INVALID_ARG
    assert L.flacgpu_meta_feed_host(C.byref(st), None, 1, C.byref(n)) == ERR_INVALID_ARG
    assert L.flacgpu_meta_feed_host(C.byref(st), b"x", 1, None) == ERR_INVALID_ARG
    # a refused stream is sticky: every later byte is consumed and ignored
    assert L.flacgpu_meta_feed_host(C.byref(st), b"fLx", 3, C.byref(n)) == 0 and n.value == 3
    assert L.flacgpu_meta_feed_host(C.byref(st), b"fLaC" + bytes(50), 54, C.byref(n)) == 0 and n.value == 54
    info, mf, at = _lib.StreamInfo(), C.c_uint32(0), C.c_uint64(7)
    assert L.flacgpu_meta_feed_result_host(C.byref(st), 57, C.byref(info), C.byref(mf), C.byref(at)) == ERR_INVALID_ARG
    assert at.value == 0
