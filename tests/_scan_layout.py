"""Inputs aimed at the STRUCTURE of the device frame scan (kernels/frame_scan.inc) -- where frames, slots and regions
fall in its 64-byte blocks, its workgroups of WG blocks, k_scan_carry's runs of workgroups and the order of x modulo the
CRC-16 polynomial -- for test_scan_layout_host.py (CPU) and test_gpu_scan_layout.py (GPU) (TEST INFRASTRUCTURE ONLY).

The layout rule (decode_many.hip, SlotLayout::add for scan_impl and scan_raw_impl): a stream with a frame region owns a
SLOT; slot s begins at the previous slot's base + ((len + kSlotTail + 63) & ~63); block0 = base / 64; a block's workgroup is block // WG;
n_wg = ceil(blocks / WG); k_scan_carry's lane t walks per = ceil(n_wg / WG) workgroups.  The region of a regular stream
is the bytes behind its metadata, that of a raw stream the whole input; a stream without a region owns no slot.  WG and
kSlotTail are read from the sources: a change to either re-aims the cases or breaks them (test_scan_layout_host.py
recomputes every aim), never quietly un-aims them.

The frames are mono VERBATIM frames built byte by byte, without _flacsyn's bit writer: header, the subframe header
byte 0x02, the samples' bytes (numpy, values 1..100: never 0, so that a running CRC is never trivially 0, and never
0xFF, so that no candidate is an accident), CRC-16.  A frame is header_bytes + 1 + n * (bits / 8) + 2 bytes long, so
the block size places the next header to the byte.  test_scan_layout_host.py holds the builder to _flacsyn's writer.

With kSlotTail = 64 a slot is at least two blocks (a region block and the tail block), so "a one-block slot" is a slot
whose REGION is one block: cases() places such a region on either side of a workgroup's edge."""
import functools
import hashlib
import os
import re

import numpy as np

import _flacsyn as fs
import _oracle as orc
import _scan_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flac-codec_amd", "csrc")


def _constant(path, pattern):
    with open(os.path.join(CSRC, path)) as f:
        m = re.search(pattern, f.read())
    if m is None:
        raise RuntimeError(f"{path}: no match for {pattern!r}: the scan-layout cases cannot be aimed")
    return int(m.group(1))


WG = _constant(os.path.join("kernels", "types.h"), r"constexpr\s+int\s+WG\s*=\s*(\d+)\s*;")
SLOT_TAIL = _constant("decode_many.hip", r"constexpr\s+uint32_t\s+kSlotTail\s*=\s*(\d+)\s*;")
BLOCK = 64
WGB = WG * BLOCK      # bytes of a workgroup
ORDER = 32767         # the order of x modulo the CRC-16 polynomial
RATE = 44100
LONG_BASE = 1 << 31   # first sample number of a stream with 16-byte headers: a 7-byte coded number


# ---- the layout rule
def region_len(blob, raw):
    if raw:
        return len(blob)
    md = sm.metadata(blob)
    return 0 if md is None else len(blob) - md[0]


class Layout:
    """base[i]: the slot base of stream i (None: no slot); blocks, n_wg, per."""

    def __init__(self, lens):
        self.base, at = [], 0
        for n in lens:
            self.base.append(at if n else None)
            if n:
                at += (n + SLOT_TAIL + 63) & ~63
        self.blocks = at // BLOCK
        self.n_wg = -(-self.blocks // WG)
        self.per = -(-self.n_wg // WG)


def layout(blobs, raw):
    return Layout([region_len(b, raw) for b in blobs])


def where(pos):
    """(workgroup, block in the workgroup, byte in the block) of a byte of the batch buffer."""
    return pos // WGB, pos // BLOCK % WG, pos % BLOCK


def advance_for(blocks, slack=5):
    """A region length after which the next slot begins `blocks` blocks on."""
    n = blocks * BLOCK - SLOT_TAIL - slack
    assert n > 0 and (n + SLOT_TAIL + 63) // 64 == blocks
    return n


# ---- the byte-level builder
def header(n, bits=8, style="fit", number=0, rate=RATE):
    """A frame header.  style "min": the 6-byte minimum (a tabled block size, a one-byte frame number); "six": block-size
    code 6; "fit": block-size code 7 (any n); "long": the 16-byte maximum (blocking bit 1, a 7-byte sample number,
    block-size code 7, rate code 13)."""
    blocking = int(style == "long")
    bcode = {"min": fs.BLOCK_CODES.get(n), "six": 6, "fit": 7, "long": 7}[style]
    assert bcode is not None and 1 <= n <= (256 if bcode == 6 else 65536)
    rcode = 13 if style == "long" else fs.RATE_CODES[rate]
    h = bytes([0xFF, 0xF8 | blocking, bcode << 4 | rcode, fs.BPS_CODES[bits] << 1]) + fs.utf8_number(number)
    if bcode in (6, 7):
        h += (n - 1).to_bytes(bcode - 5, "big")
    if rcode == 13:
        h += rate.to_bytes(2, "big")
    h += bytes([orc.crc8(h)])
    assert style not in ("min", "long") or len(h) == (6 if style == "min" else 16)
    return h


@functools.lru_cache(maxsize=None)
def payload(nbytes, seed):
    """nbytes sample (or filler) bytes, 1..100.  Cached: the long frames' payloads are drawn once per session."""
    return np.random.default_rng(seed).integers(1, 101, size=nbytes, dtype=np.uint8).tobytes()


filler = payload


class Placed:
    """A frame as written: data; n, bits, style, number, header_bytes; samples (int32); kept ("always", or
    "speculative": kept only when a frame may end by its own bits, or "never"); offset (in its region, set by Stream)."""


def frame(n, seed, bits=8, style="fit", number=0, plants=()):
    """plants: ((payload offset, bytes), ...) written over the payload -- whole valid headers that are no frames; the
    CRC-16 covers them."""
    h = header(n, bits, style, number)
    body = bytearray(payload(n * bits // 8, seed))
    for at, p in plants:
        assert 0 <= at and at + len(p) <= len(body)
        body[at:at + len(p)] = p
    body = bytes(body)
    data = h + b"\x02" + body
    fr = Placed()
    fr.data = data + orc.crc16(data).to_bytes(2, "big")
    fr.n, fr.bits, fr.style, fr.number, fr.header_bytes, fr.kept = n, bits, style, number, len(h), "always"
    fr.samples = np.frombuffer(body, dtype=np.int8 if bits == 8 else ">i2").astype(np.int32)
    fr.plants = tuple((len(h) + 1 + at, len(p)) for at, p in plants)   # (offset in the frame, bytes)
    return fr


def overhead(style, number, bits=8):
    """Bytes of a frame that are not samples."""
    return len(header(1, bits, style, number)) + 3


class Stream:
    """One input of a batch.  parts: frames (Placed) and filler (bytes) in order; raw: no metadata in front.  lead: a
    raw stream begins with so many bytes of filler.  Without them the CRC-16 of the region up to any frame's start is 0
    (whole frames with their CRC-16 in front of it) and so is every value the scan compares: a wrong carry, exponent
    or end-CRC multiplied into 0 would not show.  A regular stream cannot have them: its region begins with a frame."""

    def __init__(self, raw, bits=8, style="fit", lead=0):
        self.raw, self.bits, self.style = raw, bits, style
        self.parts, self.frames, self.size, self.samples = [], [], 0, 0
        if raw and lead:
            self.add_filler(lead, 9000 + lead)

    @property
    def number(self):
        """The coded number of the next frame: a frame number, or with 16-byte headers a sample number."""
        return LONG_BASE + self.samples if self.style == "long" else len(self.frames)

    def add(self, n, seed, plants=(), style=None, bits=None):
        fr = frame(n, seed, bits or self.bits, style or self.style, self.number, plants)
        fr.offset = self.size
        self.parts.append(fr.data)
        self.frames.append(fr)
        self.size += len(fr.data)
        self.samples += n
        return fr

    def add_len(self, nbytes, seed, plants=()):
        """A frame of exactly nbytes."""
        width = self.bits // 8
        room = nbytes - overhead(self.style, self.number, self.bits)
        assert room >= width and room % width == 0, (nbytes, room)
        fr = self.add(room // width, seed, plants)
        assert len(fr.data) == nbytes
        return fr

    def add_to(self, offset, seed, plants=()):
        """A frame that ends at this offset of the region."""
        return self.add_len(offset - self.size, seed, plants)

    def fill_to(self, nbytes, seed, step=20000):
        """Frames of about `step` bytes until the region is exactly nbytes long."""
        while self.size < nbytes:
            left = nbytes - self.size
            take = step if left >= 2 * step else left if left <= 65000 else left // 2
            self.add_len(take, seed + len(self.frames))
        assert self.size == nbytes
        return self

    def add_filler(self, nbytes, seed):
        assert self.raw, "only a raw stream has bytes between its frames"
        self.parts.append(filler(nbytes, seed))
        self.size += nbytes

    def cut(self, nbytes):
        """The last nbytes removed: a clean cut inside the last frame."""
        assert self.raw and 0 < nbytes < len(self.frames[-1].data)
        self.parts[-1] = self.parts[-1][:-nbytes]
        self.size -= nbytes
        self.frames[-1].kept = "never"

    @property
    def blob(self):
        region = b"".join(self.parts)
        if self.raw:
            return region
        return stream_head(self.frames, self.bits) + region

    @property
    def pcm(self):
        if not self.frames:
            return np.zeros(0, dtype=np.int32)
        return np.concatenate([f.samples for f in self.frames])


def stream_head(frames, bits, rate=RATE):
    """fLaC and a STREAMINFO with the right totals and MD5: _flacsyn.write_stream's fields."""
    sizes = [f.n for f in frames] or [0]
    coded = [len(f.data) for f in frames] or [0]
    pcm = b"".join(f.samples.astype("<i2" if bits == 16 else np.int8).tobytes() for f in frames)
    v = min(sizes) if frames else 16
    for width, field in ((16, min(max(sizes), 65535) if frames else 16), (24, min(coded)), (24, max(coded)), (20, rate),
                         (3, 0), (5, bits - 1), (36, sum(sizes))):
        v = v << width | field
    si = v.to_bytes(18, "big") + hashlib.md5(pcm).digest()
    return b"fLaC" + fs.metadata_block(0, si, last=True)


def plant(k, style="fit"):
    """A whole valid header that heads no frame."""
    return header(192 + k, 8, style, LONG_BASE + k if style == "long" else k)


# ---- the cases
class Case:
    """name; raw; streams ([Stream]); aims: [(kind, ...)] that test_scan_layout_host.py recomputes from the blobs'
    lengths; item ("a" .. "f"); speculative: the scan flag this case is (also) expected under."""

    def __init__(self, name, item, raw, streams, aims, speculative=False):
        self.name, self.item, self.raw, self.streams, self.aims, self.speculative = name, item, raw, streams, aims, speculative

    @functools.cached_property
    def blobs(self):
        return [s.blob for s in self.streams]

    @functools.cached_property
    def layout(self):
        return layout(self.blobs, self.raw)

    @property
    def nbytes(self):
        return sum(len(b) for b in self.blobs)

    def frame_at(self, i, k):
        """Byte offset of frame k of stream i in the batch buffer."""
        return self.layout.base[i] + self.streams[i].frames[k].offset


def kept_frames(stream, speculative=False):
    ok = ("always", "speculative") if speculative else ("always",)
    return [f for f in stream.frames if f.kept in ok]


def expected_summary(stream, speculative=False):
    """(frames, skipped_bytes, gaps) of the raw rule for what the builder placed."""
    cursor = skipped = gaps = 0
    kept = kept_frames(stream, speculative)
    for f in kept:
        if f.offset > cursor:
            skipped, gaps = skipped + f.offset - cursor, gaps + 1
        cursor = f.offset + len(f.data)
    if stream.size > cursor:
        skipped, gaps = skipped + stream.size - cursor, gaps + 1
    return len(kept), skipped, gaps


def _phase(raw=True):
    """a: a header starts at every byte of a block -- the 6-byte minimum header (frames of 201 bytes: 201 k mod 64 takes
    every value) and the 16-byte one (frames of 65 bytes), whose parse reaches the look-ahead from byte 49 on."""
    short, long_ = Stream(raw, style="min", lead=23), Stream(raw, style="long", lead=41)
    for k in range(64):
        short.add(192, 100 + k)
    for k in range(65):
        long_.add(46, 200 + k)
    aims = [("every phase", 0, 6), ("every phase", 1, 16)]
    return Case("a: block phase", "a", raw, [short, long_], aims)


def _edge_headers(raw):
    """b: 16-byte headers at bytes 48..63 of a workgroup's last block and at byte 0 of a workgroup's first block."""
    lead = Stream(raw, lead=11).fill_to(1000, 300)
    st = Stream(raw, style="long", lead=29)
    base = (1000 + SLOT_TAIL + 63) & ~63
    st.add_to(WGB - 16 - base, 310)           # frame 1 begins 16 bytes before the end of workgroup 0
    st.add_to(2 * WGB - base, 311)            # frame 2 begins with workgroup 2
    st.add_len(1000, 312)
    aims = [("header at", 1, 1, 0, WG - 1, 48), ("header at", 1, 2, 2, 0, 0)]
    return Case(f"b: 16-byte headers at a workgroup's edge ({'raw' if raw else 'regular'})", "b", raw, [lead, st], aims)


def _slot_start_streams(raw):
    s0 = Stream(raw, lead=7).fill_to(advance_for(WG - 1), 320)               # slot 1 begins at block WG - 1
    s1 = Stream(raw, lead=13).fill_to(advance_for(2 * WG - (WG - 1)), 330)   # slot 2 begins at block 2 WG
    # a frame from the slot's first workgroup into the next: an error common to all of a slot's values in one
    # workgroup shows only in a comparison across workgroups
    s2 = Stream(raw, lead=19).fill_to(WGB + 3000, 340)
    return s0, s1, s2


def _slot_starts(raw):
    """b: a slot on a workgroup's last block, the next on a workgroup's first."""
    aims = [("slot at", 1, 0, WG - 1), ("slot at", 2, 2, 0), ("frame spans workgroups", 1, 0),
            ("frame spans workgroups", 2, 0)]
    return Case(f"b: slots on a workgroup's last and first block ({'raw' if raw else 'regular'})", "b", raw,
                list(_slot_start_streams(raw)), aims)


def _no_region_between(raw):
    """e: the same, with a stream that owns no slot in the middle."""
    s0, s1, s2 = _slot_start_streams(raw)
    empty = Stream(raw)   # raw: b""; regular: fLaC and a STREAMINFO, no frame behind them
    aims = [("no slot", 2), ("slot at", 1, 0, WG - 1), ("slot at", 3, 2, 0), ("frame spans workgroups", 3, 0)]
    return Case(f"e: a stream without a region in the middle ({'raw' if raw else 'regular'})", "e", raw,
                [s0, s1, empty, s2], aims)


def _one_block_regions(raw):
    """b: a region of one block whose tail block is a workgroup's last, the next slot on the next workgroup's first
    block; then a region of one block ON a workgroup's last block, its tail the next workgroup's first."""
    s0 = Stream(raw, lead=5).fill_to(advance_for(WG - 2), 350)
    s1 = Stream(raw, style="six", lead=10)
    s1.add_to(64, 351)                                                # a region of 64 bytes: blocks WG - 2, WG - 1
    s2 = Stream(raw, lead=17).fill_to(advance_for(2 * WG - 1), 352)   # from block 0 of workgroup 1 into workgroup 2
    s3 = Stream(raw, style="six", lead=9)
    s3.add_to(64, 353)                                                # block 3 WG - 1, tail: block 0 of workgroup 3
    s4 = Stream(raw, lead=3).fill_to(2000, 354, step=700)             # from block 1 of workgroup 3
    aims = [("slot at", 1, 0, WG - 2), ("region bytes", 1, 64), ("slot at", 2, 1, 0), ("frame spans workgroups", 2, 0),
            ("slot at", 3, 2, WG - 1), ("region bytes", 3, 64), ("slot at", 4, 3, 1)]
    return Case(f"b: one-block regions at a workgroup's edge ({'raw' if raw else 'regular'})", "b", raw,
                [s0, s1, s2, s3, s4], aims)


def _region_ends_with_workgroup(raw):
    """b: a region that ends exactly with a workgroup: its end-CRC is formed by lane 0 of the next from the carry alone."""
    lead = Stream(raw, lead=31).fill_to(700, 360, step=300)
    base = (700 + SLOT_TAIL + 63) & ~63
    s1 = Stream(raw, lead=15).fill_to(2 * WGB - base, 361)
    s2 = Stream(raw, lead=21).fill_to(900, 362, step=400)
    aims = [("region ends with workgroup", 1), ("slot at", 2, 2, 1)]
    return Case(f"b: a region that ends with a workgroup ({'raw' if raw else 'regular'})", "b", raw, [lead, s1, s2], aims)


def _region_lengths(raw):
    """b: region lengths of 0, 1, 2 and 63 modulo 64."""
    streams = [Stream(raw, lead=1 + n % 50).fill_to(n, 370 + n, step=300) for n in (640, 641, 642, 703, 64 * 300, 64 * 300 + 1, 64 * 300 + 63)]
    aims = [("region mod 64", i, r) for i, r in enumerate((0, 1, 2, 63, 0, 1, 63))]
    return Case(f"b: region lengths modulo 64 ({'raw' if raw else 'regular'})", "b", raw, streams, aims)


def _long_frames(raw):
    """b: a frame of 20000 samples, longer than a workgroup; a 16-bit frame of 65535 samples over eight workgroups."""
    s0 = Stream(raw, lead=33)
    s0.add(500, 380)
    s0.add(20000, 381)
    s0.add(700, 382)
    s1 = Stream(raw, bits=16, lead=35)
    s1.add(300, 383)
    s1.add(65535, 384)
    s1.add(200, 385)
    aims = [("frame covers workgroups", 0, 1, 1), ("frame covers workgroups", 1, 1, 8)]
    return Case(f"b: frames longer than a workgroup ({'raw' if raw else 'regular'})", "b", raw, [s0, s1], aims)


def _planted(raw):
    """b: look-alike headers planted on both sides of a workgroup boundary, three and four to a block, in the frame that
    crosses it, and more in front of the next slot; raw: that slot begins with filler, so that its first candidate is not
    at its base."""
    s0 = Stream(raw, lead=27)
    s0.add(1000, 390)
    start = s0.size + overhead("fit", 1) - 2   # the payload of frame 1 begins here
    # 7- to 9-byte plants at batch offsets WGB - 60, - 40, - 20 (block WG - 1) and WGB, + 10, + 30, + 50 (block 0)
    spots = [WGB - 60, WGB - 40, WGB - 20, WGB, WGB + 10, WGB + 30, WGB + 50, 2 * WGB - 9, 2 * WGB + 1]
    plants = tuple((at - start, plant(k, "long" if k % 3 == 2 else "fit")) for k, at in enumerate(spots))
    s0.add(40000, 391, plants)
    s0.add(600, 392, ((100, plant(20)), (300, plant(21)), (500, plant(22))))
    s1 = Stream(raw)
    if raw:
        s1.add_filler(777, 393)
    s1.add(900, 394, ((10, plant(30)),))
    s1.add(400, 395)
    aims = [("plants at", 0, 1, tuple(spots)), ("first candidate not at base", 1)] if raw else \
        [("plants at", 0, 1, tuple(spots))]
    return Case(f"b: planted headers across a workgroup boundary ({'raw' if raw else 'regular'})", "b", raw, [s0, s1], aims)


def _carry_one_region(n_wg):
    """c: one region over the whole batch, of 16-bit frames of 65535 samples: the carry flows through every run."""
    st = Stream(True, bits=16, lead=1001)
    target = (n_wg - 1) * WGB + 5000
    while target - st.size > 65535 * 2 + 20:
        st.add(65535, 400 + len(st.frames) % 4)
    if target - st.size >= 100:   # (less: the batch still ends inside workgroup n_wg - 1)
        st.add_len((target - st.size) & ~1 | (overhead("fit", st.number, 16) & 1), 404)
    return Case(f"c: one region over {n_wg} workgroups", "c", True, [st], [("n_wg", n_wg), ("one region",)])


def _carry_many_regions(n_wg):
    """c: slots that begin in the first workgroup of a run, in the last and in a run's interior, each in the middle of
    its workgroup, so that the region in front of it crosses the boundary in front of it; frames of 60000 bytes and more."""
    per = -(-n_wg // WG)
    runs = -(-n_wg // per)
    starts = {0}
    for r in sorted({1, runs // 2, runs - 2}):
        starts |= {r * per, r * per + per - 1} | ({r * per + 1} if per >= 3 else set())
    starts = sorted(w for w in starts if w < n_wg)
    blocks = [0] + [w * WG + WG // 2 + 3 * i for i, w in enumerate(starts[1:])] + [(n_wg - 1) * WG + 100]
    streams = [Stream(True, lead=50 + i).fill_to(advance_for(b - a, slack=i % 64), 500 + 10 * i, step=60000)
               for i, (a, b) in enumerate(zip(blocks, blocks[1:]))]
    aims = [("n_wg", n_wg), ("slot starts in workgroups", tuple(starts)), ("frames span the run boundaries",)]
    return Case(f"c: many regions over {n_wg} workgroups", "c", True, streams, aims)


CARRY_N_WG = (255, 256, 257, 512, 513, 768, 770)   # per = 1, 1, 2, 2, 3, 3, 4; 257 and 770 leave empty trailing runs


def _order_of_x(raw):
    """d: frames at region offsets 32767, 65534 and 3 * 32767 + 1; frames of 32767 and 65534 bytes; regions of 32767
    and 65534 bytes (the end-CRC with exponent 0).  Raw: filler in front of the first frame, counted as skipped."""
    def lead(st, nbytes, seed):
        if raw:
            st.add_filler(300, seed + 1)
            nbytes -= 300
        st.add_len(nbytes, seed)
        return st

    s0 = lead(Stream(raw), ORDER, 600)
    s0.add_len(ORDER, 601)
    s0.add_len(ORDER + 1, 602)
    s0.add_len(1000, 603)
    s1 = Stream(raw)
    s1.add_len(2 * ORDER, 604)
    s2 = lead(Stream(raw), ORDER, 605)
    s3 = lead(Stream(raw), 30000, 606)
    s3.add_len(2 * ORDER - 30000, 607)
    aims = [("region offsets", 0, (1, 2, 3), (ORDER, 2 * ORDER, 3 * ORDER + 1)), ("frame bytes", 0, 1, ORDER),
            ("frame bytes", 1, 0, 2 * ORDER), ("region bytes", 1, 2 * ORDER), ("region bytes", 2, ORDER),
            ("region bytes", 3, 2 * ORDER)]
    return Case(f"d: the order of x ({'raw' if raw else 'regular'})", "d", raw, [s0, s1, s2, s3], aims)


OWN_LEAD = 45


def _own_extent(cut):
    """f: a last frame across a workgroup boundary that no header follows.  cut: its CRC-16 bytes are cut off -- no test
    is left that could tell the frame from damage, and neither rule keeps it.  Else the input goes on with filler: the
    plain rule passes the frame over, FLACGPU_SCAN_SPECULATIVE ends it by its own bits and keeps it."""
    lead = Stream(True, lead=25).fill_to(900, 700, step=400)
    st = Stream(True, lead=OWN_LEAD)
    st.add(3000, 701)
    fr = st.add(20000, 702)
    if cut:
        st.cut(2)
    else:
        fr.kept = "speculative"
        st.add_filler(1500, 703)
    name = "its CRC-16 cut off" if cut else "filler behind it"
    return Case(f"f: a last frame across a workgroup boundary, {name}", "f", True, [lead, st],
                [("frame spans workgroups", 1, 1)], speculative=True)


@functools.lru_cache(maxsize=1)
def cases():
    out = [_phase()]
    for make in (_edge_headers, _slot_starts, _one_block_regions, _region_ends_with_workgroup, _region_lengths,
                 _long_frames, _planted, _order_of_x, _no_region_between):
        out += [make(True), make(False)]
    for n_wg in CARRY_N_WG:
        out += [_carry_one_region(n_wg), _carry_many_regions(n_wg)]
    out += [_own_extent(True), _own_extent(False)]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


RECORD_FIELDS = ("byte_offset", "number", "out_offset", "stream", "bytes", "block_size", "sample_rate", "channels",
                 "bits_per_sample", "assignment", "blocking", "status", "reserved")   # flacgpu_frame_record


def builder_records(case, speculative=False):
    """The frame records of a raw batch from what the builder placed, as tuples in RECORD_FIELDS order: the streams in
    batch order, out_offset running through the batch."""
    out, at = [], 0
    for i, st in enumerate(case.streams):
        for f in kept_frames(st, speculative):
            out.append((f.offset, f.number, at, i, len(f.data), f.n, RATE, 1, f.bits, 0, int(f.style == "long"), 0,
                        int(f.kept == "speculative")))
            at += f.n
    return out
