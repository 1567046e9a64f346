"""Container sessions -- regular .flac streams fed chunk by chunk -- for test_meta_feed_host.py,
test_container_session_host.py (CPU) and test_gpu_container_session.py (GPU) (TEST INFRASTRUCTURE ONLY): the rule of
DESIGN.md 4b "Container sessions" a second time, in Python.

MetaFeed is the resumable metadata walk; Online is the rule R_W for regular streams as it comes out feed by feed (a
position is judged once 16 bytes follow it, the frame at the cursor is decided once a judged position ends it or every
position up to W behind it has been judged; lost synchronisation is final).  oneshot() is the plain statement they are
held against: the one-shot regular scan of the concatenation (_scan_model.scan's rule) with `end - start <= W` added.
The two share the header grammar and the CRC and nothing else."""
import _flacsyn as fs
import _oracle as orc
import _raw_frames as rf
import _scan_model as scm

HEAD = 16   # kHeadBytes: a header is at most 16 bytes
INVALID_ARG = -1


def _fits(buf, s, q):
    return q - s >= 2 and int.from_bytes(buf[q - 2:q], "big") == orc.crc16(buf[s:q - 2])


def header_fields(d, info):
    """The record fields of the header at d (which _scan_model.parse_header accepts); rate and sample size are
    STREAMINFO's where the header defers."""
    n, hb, blocking = scm.parse_header(d)
    rcode, assignment, bps_code = d[2] & 15, d[3] >> 4, (d[3] >> 1) & 7
    lead = 8 - (d[4] ^ 0xFF).bit_length()
    number = d[4] & (0x7F >> lead) if lead else d[4]
    for b in d[5:4 + max(lead, 1)]:
        number = number << 6 | (b & 0x3F)
    tail = d[:hb - 1]
    rate = info["sample_rate"] if rcode == 0 else rf.RATE_OF[rcode] if rcode < 12 else tail[-1] * 1000 if rcode == 12 \
        else int.from_bytes(tail[-2:], "big") * (10 if rcode == 14 else 1)
    return dict(block_size=n, blocking=blocking, number=number, sample_rate=rate,
                channels=assignment + 1 if assignment < 8 else 2,
                bits_per_sample=rf.BITS_OF[bps_code] if bps_code else info["bits_per_sample"], assignment=assignment)


def _record(buf, s, end, base, info):
    return dict(header_fields(buf[s:s + HEAD], info), byte_offset=base + s, bytes=end - s)


def streaminfo_fields(si):
    v = int.from_bytes(si[:18], "big")
    return (v >> 88) & 0xFFFFFF, dict(min_block=v >> 128, max_block=(v >> 112) & 0xFFFF, sample_rate=(v >> 44) & 0xFFFFF,
                                      channels=((v >> 41) & 7) + 1, bits_per_sample=((v >> 36) & 31) + 1,
                                      total_samples=v & (2 ** 36 - 1), md5=bytes(si[18:]))


class MetaFeed:
    """The metadata chain byte by byte: nothing is kept of a block but a STREAMINFO's 34 bytes."""

    def __init__(self):
        self.phase, self.got, self.left, self.taken = "marker", b"", 0, 0
        self.si, self.head = None, b""

    def state_bytes(self):
        return len(self.got) + len(self.head) + (34 if self.si else 0)

    def _block_end(self):
        self.phase, self.got = ("done" if self.head[0] & 0x80 else "header"), b""

    def feed(self, chunk):
        """The bytes of `chunk` the walk consumed."""
        if self.phase == "done":
            return 0
        if self.phase == "refused":
            return len(chunk)
        i = 0
        while i < len(chunk) and self.phase != "done":
            if self.phase == "marker":
                if chunk[i] != b"fLaC"[len(self.got)]:
                    self.phase = "refused"
                    return len(chunk)
                self.got += chunk[i:i + 1]
                i += 1
                if len(self.got) == 4:
                    self.phase, self.got = "header", b""
            elif self.phase == "header":
                self.got += chunk[i:i + 1]
                i += 1
                if len(self.got) == 4:
                    self.head, self.left = self.got, int.from_bytes(self.got[1:], "big")
                    self.phase, self.got = ("si" if self.head[0] & 0x7F == 0 and self.left == 34 else "skip"), b""
                    if not self.left:
                        self._block_end()
            elif self.phase == "skip":
                n = min(self.left, len(chunk) - i)
                i, self.left = i + n, self.left - n
                if not self.left:
                    self._block_end()
            else:
                self.got += chunk[i:i + 1]
                i += 1
                if len(self.got) == 34:
                    self.si = self.got
                    self._block_end()
        self.taken += i
        return i

    def result(self, total):
        """(refused, min_frame, STREAMINFO fields or None, frames_at) for the `total` bytes fed, seen as one input: what
        _meta_cases.walk and the usability test give."""
        if self.phase in ("refused", "marker") or total < 42:
            return True, 0, None, 0
        min_frame, f = streaminfo_fields(self.si) if self.si else (0, None)
        if self.phase != "done" or f is None or f["max_block"] < 1:
            return True, min_frame, f, 0
        return False, min_frame, f, self.taken


class Online:
    """One stream of a container session, feed by feed."""

    def __init__(self, W):
        self.W, self.meta = W, MetaFeed()
        self.phase = "meta"   # meta | frames | lost | refused
        self.tail, self.base, self.fed = b"", 0, 0
        self.frames = self.skipped = self.bad_frames = self.samples = 0
        self.info, self.min_frame = None, 0

    def feed(self, chunk, finish=False):
        """The records decided by this feed."""
        chunk = bytes(chunk)
        self.fed += len(chunk)
        out = []
        if self.phase == "meta":
            used = self.meta.feed(chunk)
            if self.meta.phase in ("done", "refused") or finish:
                refused, self.min_frame, self.info, at = self.meta.result(self.meta.taken if self.meta.phase == "done" else self.fed)
                self.phase, self.base = ("refused", 0) if refused else ("frames", at)
            chunk = chunk[used:]
        if self.phase == "frames":
            out = self._frames(self.tail + chunk, finish)
        elif self.phase == "lost":
            self.skipped += len(chunk)
        if self.phase == "refused":
            self.skipped = self.fed
        return out

    def _frames(self, buf, finish):
        L, W = len(buf), self.W
        judged = L if finish else max(L - HEAD + 1, 0)   # the first position not judged yet
        heads = {}
        q = buf.find(b"\xff")
        while 0 <= q < judged:
            h = scm.parse_header(buf[q:q + HEAD])
            if h:
                heads[q] = h
            q = buf.find(b"\xff", q + 1)
        order = sorted(heads)
        out, s, lost = [], 0, False
        while s < L and s < judged:
            if s not in heads:
                lost = True
                break
            _, hb, blocking = heads[s]
            lo = s + max(hb + 2 + self.info["channels"], self.min_frame)
            end = next((q for q in order if lo <= q <= s + W and heads[q][2] == blocking and _fits(buf, s, q)), None)
            if end is None and finish and 2 <= L - s <= W and _fits(buf, s, L):
                end = L
            if end is None:
                if finish or L - HEAD >= s + W:
                    lost = True
                break   # else: held from s
            rec = _record(buf, s, end, self.base, self.info)
            out.append(rec)
            self.samples += rec["block_size"]
            s = end
        self.frames += len(out)
        self.base += s
        if lost:
            self.phase, self.bad_frames, self.skipped, self.tail = "lost", 1, L - s, b""
        else:
            self.tail = buf[s:]
        return out

    def summary(self):
        """(frames, skipped_bytes, gaps, uniform) as flacgpu_raw_stream has them."""
        return self.frames, self.skipped, int(self.skipped > 0), int(self.phase in ("frames", "lost"))


def online(blob, cuts, W):
    """(records per feed with the finish's last, the stream's Online): `cuts` are the ascending chunk ends."""
    st, feeds, at = Online(W), [], 0
    for c in cuts:
        feeds.append(st.feed(blob[at:c]))
        at = c
    feeds.append(st.feed(b"", True))
    return feeds, st


def oneshot(blob, W=None):
    """The one-shot regular scan of the whole input (with `end - start <= W` when W is given):
    (rc, records, bad_frames, samples per channel, STREAMINFO fields or None)."""
    blob = bytes(blob)
    md = scm.metadata(blob)
    if md is None:
        return INVALID_ARG, [], 0, 0, None
    pos, min_frame, f = md
    heads = {q: h for q in range(pos, len(blob)) for h in [scm.parse_header(blob[q:q + HEAD])] if h}
    order = sorted(heads)
    recs, s = [], pos
    while s < len(blob):
        end = None
        if s in heads:
            lo = s + max(heads[s][1] + 2 + f["channels"], min_frame)
            ends = [q for q in order if q >= lo and heads[q][2] == heads[s][2]] + [len(blob)]
            end = next((q for q in ends if (W is None or q - s <= W) and _fits(blob, s, q)), None)
        if end is None:
            return 0, recs, 1, sum(r["block_size"] for r in recs), f
        recs.append(_record(blob, s, end, 0, f))
        s = end
    return 0, recs, 0, sum(r["block_size"] for r in recs), f


def links_within(data, W):
    """Whether the one-shot regular scan of `data` links no frame to an end more than W bytes away: then R_W is the
    one-shot rule on it.  The counterpart of _session_model.raw_links_within."""
    return all(r["bytes"] <= W for r in oneshot(data)[1])


FIELDS = ("byte_offset", "bytes", "block_size", "blocking", "number", "sample_rate", "channels", "bits_per_sample",
          "assignment")


def tuples(records):
    return [tuple(int(r[k]) for k in FIELDS) for r in records]


def multi_cut(rng, n, lo=1, hi=300, one_byte_rate=0.1, idle_rate=0.1):
    """Ascending chunk ends for n bytes: chunks of lo..hi bytes, some of one byte, some empty (an idle feed)."""
    cuts, at = [], 0
    while at < n:
        r = rng.random()
        step = 0 if r < idle_rate else 1 if r < idle_rate + one_byte_rate else rng.randint(lo, hi)
        at = min(n, at + step)
        cuts.append(at)
    return cuts


def crcd(body):
    return body + fs.crc16(body).to_bytes(2, "big")
