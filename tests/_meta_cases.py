"""Inputs for the metadata walk (csrc/kernels/meta_walk.h: one function for the host and for k_meta_walk), shared by
test_device_input_abi.py (the host build against flacgpu_scan_stream_host) and test_gpu_device_input.py (the device
build through flacgpu_decoder_scan_device against flacgpu_decoder_scan).  Every case is (label, bytes)."""
import functools

import _flacsyn as fs
import _foreign_matrix as fm


def streaminfo(min_block=16, max_block=16, min_frame=0, max_frame=0, rate=44100, channels=1, bits=16, total=0,
               md5=bytes(range(16))):
    b = fs.Bits()
    for n, v in ((16, min_block), (16, max_block), (24, min_frame), (24, max_frame), (20, rate), (3, channels - 1),
                 (5, bits - 1), (36, total)):
        b.put(n, v)
    return b.getvalue() + md5


def chain(blocks, last=True):
    """fLaC + the blocks [(type, payload)]; `last`: the final block carries the last-block flag."""
    return b"fLaC" + b"".join(fs.metadata_block(k, p, last and i + 1 == len(blocks)) for i, (k, p) in enumerate(blocks))


def walk(data):
    """The rule in Python: (marker, complete, STREAMINFO bytes or None, frames_at) of `data`."""
    if len(data) < 42 or data[:4] != b"fLaC":
        return False, False, None, 0
    pos, si = 4, None
    while True:
        if pos + 4 > len(data):
            return True, False, si, 0
        head, blen = data[pos], int.from_bytes(data[pos + 1:pos + 4], "big")
        pos += 4
        if pos + blen > len(data):
            return True, False, si, 0
        if head & 0x7F == 0 and blen == 34:
            si = data[pos:pos + 34]
        pos += blen
        if head & 0x80:
            return True, True, si, pos


def small_file():
    """A stream with three metadata blocks, one 16-sample frame; its metadata's length."""
    st = fs.write_stream(8000, 8, [fs.Frame([list(range(16))], [fs.verbatim()])], metadata=[(4, b"vendor--"), (1, bytes(5))])
    return st.blob, walk(st.blob)[3]


@functools.lru_cache(maxsize=1)
def truncations():
    blob, meta = small_file()
    return tuple((f"small file cut at {k}", blob[:k]) for k in range(meta + 3))


@functools.lru_cache(maxsize=1)
def edges():
    frame = fs.write_stream(8000, 8, [fs.Frame([list(range(16))], [fs.verbatim()])]).blob[42:]   # one whole frame
    si = streaminfo()
    out = [
        ("length 41", chain([(0, si)])[:41]),
        ("length 42", chain([(0, si)])),
        ("wrong marker", b"fLaX" + chain([(0, si)])[4:] + frame),
        ("lower-case marker", b"flac" + chain([(0, si)])[4:] + frame),
        ("no last-block flag: the walk runs off the end", chain([(0, si), (1, bytes(9))], last=False)),
        ("no last-block flag, the end inside a block header", chain([(0, si), (1, bytes(9))], last=False) + b"\x01\x00"),
        ("a block passes the end by one byte", chain([(0, si), (1, bytes(100))])[:-1]),
        ("70 KB PADDING behind STREAMINFO", chain([(0, si), (1, bytes(70000)), (4, b"x" * 11)]) + frame),
        ("two STREAMINFO blocks: the second wins",
         chain([(0, streaminfo(rate=8000, bits=8, md5=bytes(16))), (1, bytes(3)), (0, streaminfo(rate=48000, channels=2, bits=24))]) + frame),
        ("second STREAMINFO truncated: the first stays in info",
         chain([(0, streaminfo(rate=8000, bits=8)), (0, streaminfo(rate=48000))])[:-1]),
        ("type 0 with length 33", chain([(0, si[:33])]) + bytes(8) + frame),
        ("type 0 with length 35", chain([(0, si + b"\x00")]) + frame),
        ("type 0 with length 33, then a STREAMINFO", chain([(0, si[:33]), (0, si)]) + frame),
        ("STREAMINFO in the second place", chain([(1, bytes(4)), (0, si)]) + frame),
        ("8 channels", chain([(0, streaminfo(channels=8))]) + frame),
        ("32 bits", chain([(0, streaminfo(bits=32))]) + frame),
        ("4 bits", chain([(0, streaminfo(bits=4))]) + frame),
        ("max_block 0: refused", chain([(0, streaminfo(min_block=0, max_block=0))]) + frame),
        ("max_block 1", chain([(0, streaminfo(min_block=1, max_block=1))]) + frame),
        ("max_block 65535, all ones elsewhere",
         chain([(0, streaminfo(65535, 65535, (1 << 24) - 1, (1 << 24) - 1, (1 << 20) - 1, 8, 32, (1 << 36) - 1, b"\xff" * 16))]) + frame),
        ("metadata ends exactly at len", chain([(0, si), (4, b"comment")])),
        ("metadata ends exactly at len, 42 bytes", chain([(0, si)])),
        ("one byte behind the metadata", chain([(0, si), (4, b"comment")]) + b"\xff"),
        ("the last flag on a zero-length block", chain([(0, si), (1, b"")]) + frame),
        ("empty", b""),
        ("the marker alone", b"fLaC"),
    ]
    return tuple(out)


@functools.lru_cache(maxsize=1)
def foreign():
    """The 133 valid streams of _foreign_matrix.py."""
    return tuple((st.name, st.blob) for st in fm.valid_cases())


def foreign_invalid():
    """Its streams with a malformed frame in the middle: their metadata is as good as any."""
    return tuple((why, st.blob) for why, st in fm.invalid_cases())


def all_cases():
    return foreign() + foreign_invalid() + truncations() + edges()
