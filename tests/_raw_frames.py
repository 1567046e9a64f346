"""Raw frame streams -- bare FLAC frames without fLaC marker or STREAMINFO -- for test_scan_frames_host.py (CPU) and
test_gpu_raw_frames.py (GPU) (TEST INFRASTRUCTURE ONLY): the rule of DESIGN.md 4b "Raw frame streams" as a Python
model, and the hand-built inputs both scans are held to it on, fixed by a seed.

The model states the rule, it does not walk the bytes as the C loop does: it lists the candidates (a header that
_scan_model.parse_header accepts, whose sample-rate and sample-size codes are not 0), gives each its end (the first
later candidate far enough on that the frame's CRC-16 precedes, else the end of the input under the same CRC test) and
walks them with a cursor, passing over a candidate without an end."""
import functools
import random

import _flacsyn as fs
import _foreign_matrix as fm
import _oracle as orc
import _scan_model as sm

RATE_OF = {code: rate for rate, code in fs.RATE_CODES.items()}
BITS_OF = {code: bits for bits, code in fs.BPS_CODES.items()}
RECORD_FIELDS = ("byte_offset", "number", "out_offset", "stream", "bytes", "block_size", "sample_rate", "channels",
                 "bits_per_sample", "assignment", "blocking", "status", "reserved")
# the shapes the mixed stream cycles through: rate, bits, channels, samples
SHAPES = ((8000, 8, 1, 16), (44100, 16, 2, 16), (48000, 24, 3, 33), (96000, 12, 2, 192), (44100, 16, 1, 17),
          (192000, 32, 2, 16))


def parse(d):
    """The fields of the subset frame header at the start of `d` (16 bytes are enough), or None."""
    h = sm.parse_header(d)
    if h is None or d[2] & 15 == 0 or (d[3] >> 1) & 7 == 0:
        return None
    n, hb, blocking = h
    rcode, assignment = d[2] & 15, d[3] >> 4
    lead = 8 - (d[4] ^ 0xFF).bit_length()
    number = d[4] & (0x7F >> lead) if lead else d[4]
    for b in d[5:4 + max(lead, 1)]:
        number = number << 6 | (b & 0x3F)
    tail = d[:hb - 1]   # the rate's own bytes are the last in front of the CRC-8
    rate = RATE_OF[rcode] if rcode < 12 else tail[-1] * 1000 if rcode == 12 else \
        int.from_bytes(tail[-2:], "big") * (10 if rcode == 14 else 1)
    return dict(block_size=n, header_bytes=hb, blocking=blocking, number=number, sample_rate=rate,
                channels=assignment + 1 if assignment < 8 else 2, bits_per_sample=BITS_OF[(d[3] >> 1) & 7],
                assignment=assignment)


def candidates(blob):
    heads, q = {}, blob.find(b"\xff")
    while q >= 0:
        h = parse(blob[q:q + 16])
        if h:
            heads[q] = h
        q = blob.find(b"\xff", q + 1)
    return heads


def scan(blob, stream=0, out_offset=0):
    """(records, summary) of the rule: a list of dicts with RECORD_FIELDS, and dict(frames, skipped_bytes, gaps,
    uniform)."""
    blob = bytes(blob)
    heads = candidates(blob)
    order = sorted(heads)
    frames, cursor, skipped, gaps = [], 0, 0, 0
    for i, s in enumerate(order):
        if s < cursor:
            continue
        h = heads[s]
        lo = s + h["header_bytes"] + 2 + h["channels"]
        ends = [q for q in order[i + 1:] if q >= lo] + ([len(blob)] if len(blob) - s >= 2 else [])
        end = next((q for q in ends if int.from_bytes(blob[q - 2:q], "big") == orc.crc16(blob[s:q - 2])), None)
        if end is None:
            continue   # passed over: the resynchronisation
        if s > cursor:
            skipped, gaps = skipped + s - cursor, gaps + 1
        rec = dict(byte_offset=s, out_offset=out_offset, stream=stream, bytes=end - s, status=0, reserved=0)
        rec.update({k: h[k] for k in RECORD_FIELDS if k in h})
        frames.append(rec)
        out_offset += h["block_size"] * h["channels"]
        cursor = end
    if len(blob) > cursor:
        skipped, gaps = skipped + len(blob) - cursor, gaps + 1
    same = {(f["sample_rate"], f["channels"], f["bits_per_sample"]) for f in frames}
    return frames, dict(frames=len(frames), skipped_bytes=skipped, gaps=gaps, uniform=int(len(same) == 1))


def record_tuple(rec):
    """A record (a model dict or a row of the structured array the library fills) as a tuple of ints."""
    return tuple(int(rec[k]) for k in RECORD_FIELDS)


def summary_tuple(s):
    get = (lambda k: s[k]) if isinstance(s, dict) else (lambda k: getattr(s, k))
    return tuple(int(get(k)) for k in ("frames", "skipped_bytes", "gaps", "uniform"))


class RawStream:
    """blob: the frames back to back; frame_bytes, at (frame starts + the end), pcm: per frame [n][channels] lists;
    shapes: per frame (rate, bits, channels, n); numbers, blockings, assignments, frames (fs.Frame) per frame."""


def _channels(rng, bits, channels, n, amp):
    sub = fs.fixed(2)
    return [fm._predicted(rng, n, min(bits, 24), sub, amp=amp) for _ in range(channels)]


def _subs(chans, bits, assignment, kinds):
    """One subframe per coded channel: "fixed" (order 2, Rice parameters fitted to the coded channel) or "verbatim"."""
    coded = chans
    if assignment == 8:
        coded = [chans[0], [x - y for x, y in zip(*chans)]]
    elif assignment == 9:
        coded = [[x - y for x, y in zip(*chans)], chans[1]]
    elif assignment == 10:
        coded = [[(x + y) >> 1 for x, y in zip(*chans)], [x - y for x, y in zip(*chans)]]
    return [fm.fit_k(v, fs.fixed(2)) if kind == "fixed" else fs.verbatim() for v, kind in zip(coded, kinds)]


def build(shapes, seed, assignments=None, invalid_at=None, blocking=None):
    """A raw stream of one frame per shape.  Stereo frames take left/side, side/right, mid/side and independent in
    turn; the first subframe of every other frame is fixed and the rest verbatim; the first half carries frame numbers
    (blocking 0), the second sample numbers of several bytes (blocking 1): the raw rule does not compare the bit.
    blocking=0 / 1: one bit for all, as a regular stream needs it."""
    rng = random.Random(seed)
    st = RawStream()
    st.frame_bytes, st.pcm, st.shapes, st.numbers, st.blockings, st.assignments = [], [], [], [], [], []
    st.frames = []   # the fs.Frame objects: fs.write_stream makes the regular stream of the same frame bytes of them
    stereo, samples = 0, 0
    for k, (rate, bits, channels, n) in enumerate(shapes):
        chans = _channels(rng, bits, channels, n, amp=3 if bits == 8 else 40 if bits == 12 else 1000)
        assignment = channels - 1
        if channels == 2:
            assignment = (8, 9, 10, 1)[stereo % 4] if assignments is None else assignments[stereo]
            stereo += 1
        kinds = ["fixed" if c == 0 and k & 1 else "verbatim" for c in range(channels)]
        subs = _subs(chans, bits, assignment, kinds)
        if invalid_at == k:
            subs[0] = fs.verbatim(invalid=("type", 2))
        bit = int(k >= len(shapes) // 2) if blocking is None else blocking
        number = (samples + (100000 if blocking is None else 0)) if bit else k
        fr = fs.Frame(chans, subs, assignment=assignment, rcode=fs.RATE_CODES[rate], blocking=bit, number=number)
        st.frames.append(fr)
        st.frame_bytes.append(fs.write_frame(rate, bits, fr, set()))
        st.pcm.append([[ch[i] for ch in chans] for i in range(n)])
        st.shapes.append((rate, bits, channels, n))
        st.numbers.append(number)
        st.blockings.append(bit)
        st.assignments.append(assignment)
        samples += n
    st.blob = b"".join(st.frame_bytes)
    st.at = [0]
    for c in st.frame_bytes:
        st.at.append(st.at[-1] + len(c))
    return st


def expected_records(st, stream=0, out_offset=0):
    """The records of an undamaged built stream, from what the writer was given."""
    out = []
    for k, (rate, bits, channels, n) in enumerate(st.shapes):
        out.append(dict(byte_offset=st.at[k], number=st.numbers[k], out_offset=out_offset, stream=stream,
                        bytes=len(st.frame_bytes[k]), block_size=n, sample_rate=rate, channels=channels,
                        bits_per_sample=bits, assignment=st.assignments[k], blocking=st.blockings[k], status=0,
                        reserved=0))
        out_offset += n * channels
    return out


@functools.lru_cache(maxsize=1)
def mixed():
    """The 12-frame stream: the six shapes twice."""
    return build(SHAPES * 2, 20261018)


@functools.lru_cache(maxsize=1)
def uniform():
    """One shape repeated, block sizes differing: a uniform stream."""
    return build([(44100, 16, 2, n) for n in (16, 192, 33, 16, 17, 192)], 20261019)


UNIFORM_SHAPES = ((8000, 8, 1), (44100, 16, 2), (48000, 24, 3), (96000, 12, 2), (44100, 16, 1), (192000, 32, 2),
                  (16000, 20, 4), (22050, 16, 8), (32000, 24, 2), (88200, 16, 2), (176400, 24, 1), (24000, 8, 2))


@functools.lru_cache(maxsize=1)
def uniform_set():
    """((raw stream, the regular stream of the same frames), ...): twelve uniform streams of five frames of different
    block sizes (4096 among them: more than one pass of a workgroup over a frame), every header subset."""
    out = []
    for k, (rate, bits, channels) in enumerate(UNIFORM_SHAPES):
        raw = build([(rate, bits, channels, n) for n in (16, 192, 33, 4096 if k % 3 == 0 else 576, 17)], 7000 + k, blocking=k & 1)
        regular = fs.write_stream(rate, bits, raw.frames, name=f"uniform-{rate}-{bits}-{channels}")
        assert regular.blob.endswith(raw.blob) and regular.frame_bytes == raw.frame_bytes
        out.append((raw, regular))
    return tuple(out)


def subset_matrix_streams():
    """The valid streams of _foreign_matrix whose every frame header is subset."""
    return [st for st in fm.valid_cases() if all(parse(c[:16]) for c in st.frame_bytes)]


def frame_of(st, pos):
    return next(k for k in range(len(st.frame_bytes)) if st.at[k] <= pos < st.at[k + 1])


def header_bytes(st, k):
    return parse(st.frame_bytes[k][:16])["header_bytes"]


def head_cuts(st):
    return [st.blob[n:] for n in range(1, len(st.frame_bytes[0]) + 1)]


def tail_cuts(st):
    """(bytes of the last frame that remain, blob): every cut inside the last frame."""
    last = st.at[-2]
    return [(n - last, st.blob[:n]) for n in range(last, len(st.blob))]


def flips(st, seed=20261020):
    """(position, blob): one byte flipped (XOR with a seeded non-zero value) at every position."""
    rng = random.Random(seed)
    out = []
    for pos in range(len(st.blob)):
        b = bytearray(st.blob)
        b[pos] ^= rng.randint(1, 255)
        out.append((pos, bytes(b)))
    return out


def non_subset_cases():
    """(label, blob): a frame with sample-rate code 0, and one with sample-size code 0, between subset frames."""
    st = mixed()
    rng = random.Random(5)
    v = [rng.randint(-100, 100) for _ in range(16)]
    out = []
    for label, kw in (("rate code 0", dict(rcode=0)), ("sample-size code 0", dict(rcode=9, bps_code=0))):
        odd = fs.write_frame(44100, 16, fs.Frame([v], [fs.verbatim()], number=3, **kw), set())
        out.append((label, st.blob[:st.at[3]] + odd + st.blob[st.at[3]:]))
    return out


def lookalike_cases():
    """(label, blob): the pure-header regions of _scan_model.damaged_cases(), their metadata prefix removed."""
    out = []
    for label, blob in sm.damaged_cases():
        if label.startswith("look-alikes: "):
            out.append((label, blob[sm.metadata(blob)[0]:]))
    assert len(out) == 9
    return out


@functools.lru_cache(maxsize=1)
def all_cases():
    """((label, blob), ...): every input the host test names, for the device scan to be compared on in one batch."""
    st = mixed()
    out = [("mixed", st.blob), ("uniform", uniform().blob), ("empty", b"")]
    out += [(f"head cut {k + 1}", b) for k, b in enumerate(head_cuts(st))]
    out += [(f"tail cut, {left} bytes of the last frame left", b) for left, b in tail_cuts(st)]
    out += [(f"flip at {pos}", b) for pos, b in flips(st)]
    out += non_subset_cases() + lookalike_cases()
    return tuple(out)
