"""The per-group rule of k_session_slots (csrc/kernels/session_slots_rule.h) through its host export
flacgpu_session_slots_host, which runs the kernel's per-group code over host memory one "lane" after another: a slot is
the held tail followed by the new chunk, both of any alignment, at a 64-byte boundary, with a zero tail and 64 bytes of
look-ahead.  The expected bytes come from plain concatenation; the output is pre-filled with a canary, so every byte
must be written.  (What the rule READS cannot be asserted here: tools/session_check.cpp runs it under a sanitizer.)
No GPU call."""
import ctypes as C

import numpy as np
import pytest

CANARY = 0xA5
ERR_BUFFER_TOO_SMALL = -5


def _pattern(n, mul, add):
    """distinct neighbouring bytes, never 0: a zero in the output is a zero the rule wrote"""
    return ((np.arange(n) * mul + add) % 251 + 1).astype(np.uint8)


class _Pool:
    """Source bytes at chosen address residues: a 64-byte aligned arena with a pattern of its own."""

    def __init__(self, size, mul, add):
        raw = np.empty(size + 64, dtype=np.uint8)
        off = (-raw.ctypes.data) % 64
        self.a = raw[off:off + size]
        self.a[:] = _pattern(size, mul, add)
        self.base = self.a.ctypes.data

    def at(self, start, n):
        return self.base + start, bytes(self.a[start:start + n])


def _span(L):
    return (L + 64 + 63) & ~63


def _run(slots):
    """slots: [(tail address, tail bytes, chunk address, chunk bytes)] -> the buffer the rule builds; checked against
    the concatenation here."""
    from flac_codec_amd import _lib

    L = _lib.lib()
    tab = (_lib.SessionSlotSrc * max(len(slots), 1))()
    want = bytearray()
    for r, (ta, tb, ca, cb) in zip(tab, slots):
        r.tail, r.tail_len, r.chunk, r.chunk_len = ta, len(tb), ca, len(cb)
        if tb or cb:
            want += tb + cb + bytes(_span(len(tb) + len(cb)) - len(tb) - len(cb))
    if want:
        want += bytes(64)
    size = C.c_uint64(0xDEAD)
    out = np.full(len(want) + 32, CANARY, dtype=np.uint8)
    if want:
        assert L.flacgpu_session_slots_host(tab, len(slots), out.ctypes.data, len(want) - 1, C.byref(size)) == ERR_BUFFER_TOO_SMALL
        assert size.value == len(want) and (out == CANARY).all()
    assert L.flacgpu_session_slots_host(tab, len(slots), out.ctypes.data, len(want), C.byref(size)) == 0
    assert size.value == len(want)
    assert (out[len(want):] == CANARY).all(), "a write past the buffer"
    got = out[:len(want)]
    bad = np.flatnonzero(got != np.frombuffer(bytes(want), dtype=np.uint8))
    assert bad.size == 0, f"first wrong byte at {bad[0]}: {got[bad[0]]:#x}, want {want[bad[0]]:#x}"
    return got


@pytest.mark.parametrize("tail_res", range(16))
def test_the_cube_of_residues_and_short_lengths(tail_res):
    """tail length 0..49 (every residue, with and without whole groups) x tail source residue x chunk source residue
    0..15 x chunk length 0..49: the junction at every byte of a group, from every pair of alignments."""
    tails, chunks = _Pool(256, 7, 3), _Pool(256, 11, 5)
    for chunk_res in range(16):
        slots = []
        for tl in range(50):
            for cl in range(50):
                slots.append(tails.at(64 + tail_res, tl) + chunks.at(80 + chunk_res, cl))
        _run(slots)


def test_empty_tail_empty_chunk_and_both():
    tails, chunks = _Pool(256, 7, 3), _Pool(256, 11, 5)
    assert _run([(0, b"", 0, b"")]).size == 0                       # no slot at all: no byte
    assert _run([]).size == 0
    _run([(0, b"", ) + chunks.at(5, 40)])                           # NULL tail
    _run([tails.at(9, 40) + (0, b"")])                              # NULL chunk
    _run([tails.at(3, 17) + (0, b""), (0, b"", 0, b""), (0, b"") + chunks.at(1, 1), tails.at(0, 1) + (0, b"")])


def test_sources_at_the_ends_of_their_arenas():
    """The last byte of either source is the last byte of its arena, at every residue of the source's start; then the
    first is the arena's first.  (An arena is a 64-byte aligned slice of a numpy block, which may go on behind it: that
    the rule reads no byte outside a source is what tools/session_check.cpp shows, on heap blocks of the exact size.)"""
    for n in range(1, 40):
        tails, chunks = _Pool(192, 7, 3), _Pool(192, 11, 5)
        _run([tails.at(192 - n, n) + chunks.at(192 - (40 - n), 40 - n)])
        _run([tails.at(0, n) + chunks.at(0, 40 - n)])               # and start with them


def test_slots_across_a_block_and_a_workgroup_span():
    """Tails and chunks longer than a 64-byte block and than the 16 KiB a workgroup's 256 lanes of 64-byte blocks span,
    the junction just in front of, at and behind those boundaries; zero tails and look-ahead checked byte for byte."""
    tails, chunks = _Pool(40000, 7, 3), _Pool(40000, 11, 5)
    slots = []
    for tl in (63, 64, 65, 16383, 16384, 16385, 20011):
        for cl in (1, 63, 64, 65, 16400):
            slots.append(tails.at(13, tl) + chunks.at(7, cl))
    got = _run(slots)
    assert got.size % 64 == 0 and not got[-64:].any()
