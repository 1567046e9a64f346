"""Decoder sessions -- raw frame streams fed chunk by chunk -- for test_session_model.py, test_session_host.py (CPU) and
test_gpu_decoder_session.py (GPU) (TEST INFRASTRUCTURE ONLY): the rule of DESIGN.md 4b "Decoder sessions" as a Python
model over _raw_frames.candidates / parse and _oracle.crc16, stated twice, and the inputs the tests share.

segments() states WHAT comes out: flushes cut the bytes into segments, and a segment's frames are the raw rule's with
one clause added, an end lies at most W bytes behind its candidate.  online() states HOW it comes out feed by feed: a
position is judged once 16 bytes follow it, a candidate is decided once a judged candidate ends it or every position up
to W behind it has been judged, the walk stops at the first undecided one and the bytes from there on are held.  The two
share the candidate test and the CRC and nothing else."""
import functools
import random

import _oracle as orc
import _raw_frames as rf

HEAD = 16   # kHeadBytes: a header is at most 16 bytes


def _fits(buf, s, q):
    return int.from_bytes(buf[q - 2:q], "big") == orc.crc16(buf[s:q - 2])


def _record(h, s, end, stream):
    rec = dict(byte_offset=s, out_offset=0, stream=stream, bytes=end - s, status=0, reserved=0)
    rec.update({k: h[k] for k in rf.RECORD_FIELDS if k in h})
    return rec


def r_w(seg, W):
    """[(start, end, header)] of the rule R_W on one segment: rf.scan's walk with `end - start <= W`."""
    heads = rf.candidates(seg)
    order = sorted(heads)
    out, cursor = [], 0
    for i, s in enumerate(order):
        if s < cursor:
            continue
        h = heads[s]
        lo = s + h["header_bytes"] + 2 + h["channels"]
        ends = [q for q in order[i + 1:] if lo <= q <= s + W] + ([len(seg)] if 2 <= len(seg) - s <= W else [])
        end = next((q for q in ends if _fits(seg, s, q)), None)
        if end is None:
            continue
        out.append((s, end, h))
        cursor = end
    return out


def summary_of(kept, length):
    """(frames, skipped_bytes, gaps) of kept [(start, end), ...] in a byte string of `length`: the maximal runs of bytes
    in no kept frame."""
    at = skipped = gaps = 0
    for s, e in kept:
        if s > at:
            skipped, gaps = skipped + s - at, gaps + 1
        at = e
    if length > at:
        skipped, gaps = skipped + length - at, gaps + 1
    return len(kept), skipped, gaps


def segments(blob, flush_positions, W, stream=0):
    """(records, (frames, skipped_bytes, gaps)) of a whole stream: `flush_positions` are the offsets at which a flush
    was given; the end of the bytes always is one (finish).  byte_offset counts from the stream's first byte;
    out_offset is left 0 (it belongs to a feed)."""
    blob = bytes(blob)
    cuts = sorted({p for p in flush_positions if 0 < p < len(blob)}) + [len(blob)]
    records, a = [], 0
    for b in cuts:
        for s, e, h in r_w(blob[a:b], W):
            records.append(_record(h, a + s, a + e, stream))
        a = b
    return records, summary_of([(r["byte_offset"], r["byte_offset"] + r["bytes"]) for r in records], len(blob))


def raw_links_within(blob, W):
    """Whether the raw rule links no candidate of `blob` (kept or not) to an end more than W bytes away: then R_W is
    the raw rule on it."""
    blob = bytes(blob)
    heads = rf.candidates(blob)
    order = sorted(heads)
    for i, s in enumerate(order):
        h = heads[s]
        lo = s + h["header_bytes"] + 2 + h["channels"]
        ends = [q for q in order[i + 1:] if q >= lo] + ([len(blob)] if len(blob) - s >= 2 else [])
        end = next((q for q in ends if _fits(blob, s, q)), None)
        if end is not None and end - s > W:
            return False
    return True


class Online:
    """One stream of a session, feed by feed."""

    def __init__(self, W, stream=0):
        self.W, self.stream = W, stream
        self.tail, self.base = b"", 0
        self.frames = self.skipped = self.gaps = 0
        self.in_gap = False

    def _skip(self, n):
        if n:
            self.skipped += n
            self.gaps += not self.in_gap
            self.in_gap = True

    def feed(self, chunk, flush=False):
        """The records decided by this feed."""
        buf, W = self.tail + bytes(chunk), self.W
        L = len(buf)
        horizon = L - 1 if flush else L - HEAD   # the last judged position
        heads = {q: h for q, h in rf.candidates(buf).items() if q <= horizon}
        order = sorted(heads)
        out, cursor, hold = [], 0, None
        for i, s in enumerate(order):
            if s < cursor:
                continue
            h = heads[s]
            lo = s + h["header_bytes"] + 2 + h["channels"]
            end = None
            for q in order[i + 1:]:
                if q - s > W:
                    break
                if q >= lo and _fits(buf, s, q):
                    end = q
                    break
            if end is None and flush and 2 <= L - s <= W and _fits(buf, s, L):
                end = L
            if end is None:
                if flush or horizon >= s + W:
                    continue   # it never gets an end: passed over
                hold = s
                break
            self._skip(s - cursor)
            self.frames += 1
            self.in_gap = False
            out.append(_record(h, self.base + s, self.base + end, self.stream))
            cursor = end
        if flush:
            at = L
        else:
            at = max(cursor, min(L if hold is None else hold, max(L - HEAD + 1, 0)))
        self._skip(at - cursor)
        self.tail, self.base = buf[at:], self.base + at
        return out

    def summary(self):
        return self.frames, self.skipped, self.gaps


def online(blob, cuts, flushes, W, stream=0):
    """(records per feed, (frames, skipped_bytes, gaps), the longest held tail): `cuts` are the ascending chunk ends
    (the last is len(blob)), `flushes` the chunk ends given with flush; a finish follows (the last list of records)."""
    blob = bytes(blob)
    st, feeds, at, held = Online(W, stream), [], 0, 0
    for c in cuts:
        feeds.append(st.feed(blob[at:c], c in flushes))
        held = max(held, len(st.tail))
        at = c
    assert at == len(blob)
    feeds.append(st.feed(b"", True))
    return feeds, st.summary(), held


def tuples(records):
    return [rf.record_tuple(r) for r in records]


def with_out_offsets(feed_records):
    """One feed's records (ordered by stream, then position) with out_offset as a feed lays them out: the running sum
    of block_size * channels."""
    out, at = [], 0
    for r in feed_records:
        out.append(dict(r, out_offset=at))
        at += r["block_size"] * r["channels"]
    return out


def multi_cut(rng, st, lo=1, hi=300, flush_rate=0.15):
    """(cuts, flushes) for a built stream: chunks of lo..hi bytes; some chunk ends moved onto a true frame end and
    flushed there, some flushed where they are (a wrong place)."""
    n, cuts, flushes, at = len(st.blob), [], set(), 0
    while at < n:
        at = min(n, at + rng.randint(lo, hi))
        if at < n and rng.random() < flush_rate:
            if rng.random() < 0.7:   # onto the next true frame end
                at = next(e for e in st.at if e >= at)
            flushes.add(at)
        cuts.append(at)
    return cuts, flushes


@functools.lru_cache(maxsize=None)
def lookalike_stream():
    """(blob, at): a header that parses, followed by bytes that hold no sync code and no CRC-16 of it, in front of
    rf.uniform()'s frames: a candidate that never gets an end."""
    st = rf.uniform()
    rng = random.Random(20261022)
    junk = bytes(rng.randrange(0, 0xFF) for _ in range(1500))   # no 0xFF: no candidate inside
    blob = st.frame_bytes[0][:16] + junk + st.blob
    return blob, 16 + len(junk)
