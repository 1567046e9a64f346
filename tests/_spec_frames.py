"""The raw frame scan with FLACGPU_SCAN_SPECULATIVE -- a frame that no header follows is ended by its own bits (DESIGN.md
4b "A frame's own extent") -- for test_scan_frames_speculative.py (CPU) and test_gpu_speculative_frames.py (GPU) (TEST
INFRASTRUCTURE ONLY): the rule as a Python model, and the inputs both scans are held to it on.

The model takes the candidates and the two end tests of _raw_frames (a later candidate that the CRC-16 precedes, the end
of the input under the same CRC test) and gives a candidate that has neither its own extent: a walk over the frame's
subframes on Python integers that reconstructs no sample.  It shares no code with the C walker (kernels/frame_extent.h)."""
import functools
import re

import numpy as np

import _flacsyn as fs
import _foreign_matrix as fm
import _oracle as orc
import _raw_frames as rf
import _scan_model as sm

SPECULATIVE = 1          # FLACGPU_SCAN_SPECULATIVE, and FLACGPU_FRAME_SPECULATIVE in a record's `reserved`
WINDOW = 1 << 22         # bytes of the input a frame's own extent may take
_NONZERO = re.compile(rb"[^\x00]")


class _NoExtent(Exception):
    pass


class _Bits:
    """MSB-first reader of blob[s : s + window]; a read that would pass the window's last bit raises _NoExtent."""

    def __init__(self, blob, s, window):
        self.blob, self.s, self.limit, self.pos = blob, s, 8 * window, 0

    def skip(self, n):
        if self.pos + n > self.limit:
            raise _NoExtent
        self.pos += n

    def take(self, n):
        at = self.pos
        self.skip(n)
        a, b = self.s + (at >> 3), self.s + ((at + n + 7) >> 3)
        return (int.from_bytes(self.blob[a:b], "big") >> ((b - a) * 8 - (at & 7) - n)) & ((1 << n) - 1)

    def zeros(self):
        """The zeros before the next 1 bit; the 1 is consumed."""
        count = 0
        while self.pos & 7:   # up to the byte boundary, bit by bit
            if self.take(1):
                return count
            count += 1
        m = _NONZERO.search(self.blob, self.s + (self.pos >> 3), self.s + (self.limit >> 3))
        if m is None:
            raise _NoExtent
        whole = m.start() - self.s - (self.pos >> 3)
        lead = 8 - self.blob[m.start()].bit_length()
        self.skip(8 * whole + lead + 1)
        return count + 8 * whole + lead


def extent(blob, s, h):
    """The length in bytes of the frame whose accepted header `h` (_raw_frames.parse) starts at blob[s], by its own bits,
    CRC-16 included and right; None when it has none."""
    r = _Bits(blob, s, min(len(blob) - s, WINDOW))
    n, a, bps = h["block_size"], h["assignment"], h["bits_per_sample"]
    try:
        r.skip(8 * h["header_bytes"])
        for c in range(h["channels"]):
            sbps = bps + ((a, c) in ((8, 1), (9, 0), (10, 1)))
            if r.take(1):
                return None
            kind, wasted = r.take(6), 0
            if r.take(1):
                wasted = r.zeros() + 1
            if wasted >= sbps:
                return None
            eb = sbps - wasted
            if kind == 0:
                r.skip(eb)
                continue
            if kind == 1:
                r.skip(n * eb)
                continue
            if 8 <= kind <= 12:
                order = kind - 8
            elif kind >= 32:
                order = kind - 31
            else:
                return None
            if order > n:
                return None
            r.skip(order * eb)
            if kind >= 32:
                precision = r.take(4) + 1
                if precision == 16:
                    return None
                if r.take(5) & 16:   # a negative shift
                    return None
                r.skip(order * precision)
            method = r.take(2)
            if method > 1:
                return None
            po = r.take(4)
            plen = n >> po
            if plen < order or (plen << po) != n:
                return None
            width = 5 if method else 4
            for part in range(1 << po):
                count = plen - (0 if part else order)
                k = r.take(width)
                if k == (1 << width) - 1:
                    r.skip(count * r.take(5))
                    continue
                for _ in range(count):
                    r.zeros()
                    r.skip(k)
        if r.pos & 7 and r.take(8 - (r.pos & 7)):
            return None
        r.skip(16)
    except _NoExtent:
        return None
    e = r.pos >> 3
    return e if orc.crc16(blob[s:s + e]) == 0 else None


def scan(blob, speculative=True, stream=0, out_offset=0):
    """_raw_frames.scan with the flag: (records, summary); a record ended by its own bits has reserved == 1."""
    if not speculative:
        return rf.scan(blob, stream, out_offset)
    blob = bytes(blob)
    heads = rf.candidates(blob)
    order = sorted(heads)
    frames, cursor, skipped, gaps = [], 0, 0, 0
    for i, s in enumerate(order):
        if s < cursor:
            continue
        h = heads[s]
        lo = s + h["header_bytes"] + 2 + h["channels"]
        ends = [q for q in order[i + 1:] if q >= lo] + ([len(blob)] if len(blob) - s >= 2 else [])
        end = next((q for q in ends if int.from_bytes(blob[q - 2:q], "big") == orc.crc16(blob[s:q - 2])), None)
        own = 0
        if end is None:
            e = extent(blob, s, h)
            if e is None:
                continue
            end, own = s + e, SPECULATIVE
        if s > cursor:
            skipped, gaps = skipped + s - cursor, gaps + 1
        rec = dict(byte_offset=s, out_offset=out_offset, stream=stream, bytes=end - s, status=0, reserved=own)
        rec.update({k: h[k] for k in rf.RECORD_FIELDS if k in h})
        frames.append(rec)
        out_offset += h["block_size"] * h["channels"]
        cursor = end
    if len(blob) > cursor:
        skipped, gaps = skipped + len(blob) - cursor, gaps + 1
    same = {(f["sample_rate"], f["channels"], f["bits_per_sample"]) for f in frames}
    return frames, dict(frames=len(frames), skipped_bytes=skipped, gaps=gaps, uniform=int(len(same) == 1))


class SubsetStream:
    """A valid stream of _foreign_matrix as a raw stream of subset frames.  name; blob; frame_bytes; at (frame starts +
    the end); pcm: per frame an int32 array [n, channels]."""


@functools.lru_cache(maxsize=1)
def subset_matrix():
    """The matrix made subset: every valid stream of _foreign_matrix whose frames all have sample-rate code 0 and a
    sample-size code other than 0, each frame given sample-rate code 9 (44100 Hz: the header keeps its length) and its
    CRC-8 and CRC-16 redone."""
    out = []
    for src in fm.valid_cases():
        if not all(c[2] & 15 == 0 and (c[3] >> 1) & 7 != 0 for c in src.frame_bytes):
            continue
        st = SubsetStream()
        st.name, st.frame_bytes, st.pcm, st.at = src.name, [], [], [0]
        done = 0
        for c, n in zip(src.frame_bytes, src.frame_sizes):
            hb = sm.parse_header(c[:16])[1]
            b = bytearray(c)
            b[2] = (b[2] & 0xF0) | 9
            b[hb - 1] = fs.crc8(bytes(b[:hb - 1]))
            b[-2:] = orc.crc16(bytes(b[:-2])).to_bytes(2, "big")
            assert rf.parse(bytes(b[:16]))["header_bytes"] == hb
            st.frame_bytes.append(bytes(b))
            st.at.append(st.at[-1] + len(b))
            st.pcm.append(np.asarray(src.pcm[done:done + n * src.channels], dtype=np.int32).reshape(n, src.channels))
            done += n * src.channels
        st.blob = b"".join(st.frame_bytes)
        out.append(st)
    return tuple(out)


@functools.lru_cache(maxsize=1)
def alternating():
    """((stream index in subset_matrix(), parity, blob), ...): byte 0 of every frame k with k % 2 == parity set to 0."""
    out = []
    for i, st in enumerate(subset_matrix()):
        for parity in (0, 1):
            b = bytearray(st.blob)
            for k in range(parity, len(st.frame_bytes), 2):
                b[st.at[k]] = 0
            out.append((i, parity, bytes(b)))
    return tuple(out)


def true_frames(st):
    return {(st.at[k], len(c)): k for k, c in enumerate(st.frame_bytes)}
