"""Raw frame streams on a timeline, for test_timeline_host.py (CPU) and test_gpu_timeline.py (GPU) (TEST INFRASTRUCTURE
ONLY): the rule of include/flacenc_gpu.h "raw frame streams on a timeline" as a Python model over record dicts, and the
cases, fixed by seeds.

A case carries its expectation per scan setting (speculative or not): the stream's status and, for a stream with a
timeline, first_sample and the frames that survive as (position, samples, PCM).  The PCM is the writer's own -- what
_raw_frames.build gave _flacsyn.write_frame -- and the survivors are named by the case's author, so the expected tensor
is built by placement alone, independent of any decoder and of the scan."""
import functools
import random

import numpy as np

import _flacsyn as fs
import _raw_frames as rf

OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
PLACED, DROPPED, CONCEALED = 1, 2, 4
RESULT_FIELDS = ("rc", "placed", "dropped", "concealed", "gaps", "first_sample", "timeline_samples", "gap_samples",
                 "concealed_samples")


# ---- the rule
def timeline(records):
    """(result, frames) of the rule for one stream's records (dicts or rows with rf.RECORD_FIELDS), before any decode:
    result is a dict of RESULT_FIELDS, frames a list of (at, flags) per record ((0, 0) for a refused stream)."""
    recs = [{k: int(r[k]) for k in rf.RECORD_FIELDS} for r in records]
    res = dict.fromkeys(RESULT_FIELDS, 0)
    none = [(0, 0)] * len(recs)
    if not recs:
        return dict(res, rc=INVALID_ARG), none
    r0 = recs[0]
    if any((r["sample_rate"], r["channels"], r["bits_per_sample"]) !=
           (r0["sample_rate"], r0["channels"], r0["bits_per_sample"]) for r in recs):
        return dict(res, rc=UNSUPPORTED), none
    if any(r["blocking"] != r0["blocking"] for r in recs):
        return dict(res, rc=UNSUPPORTED), none
    B = r0["block_size"]
    if not r0["blocking"] and (any(r["block_size"] != B for r in recs[:-1]) or recs[-1]["block_size"] > B):
        return dict(res, rc=UNSUPPORTED), none
    pos = [r["number"] if r0["blocking"] else r["number"] * B for r in recs]
    origin = end = pos[0]
    frames = []
    for k, (p, r) in enumerate(zip(pos, recs)):
        if k and p < end:
            res["dropped"] += 1
            frames.append((0, DROPPED))
            continue
        if p > end:
            res["gaps"] += 1
            res["gap_samples"] += p - end
        frames.append((p - origin, PLACED))
        res["placed"] += 1
        end = p + r["block_size"]
    res.update(first_sample=origin, timeline_samples=end - origin)
    return res, frames


def conceal(result, frames, records, statuses):
    """The model's result and frames after a decode whose per-record decode_frames statuses are `statuses`: a list of
    (at, flags, status)."""
    result, out = dict(result), []
    for (at, flags), r, st in zip(frames, records, statuses):
        st = int(st) if flags & PLACED else 0
        if st:
            flags |= CONCEALED
            result["concealed"] += 1
            result["concealed_samples"] += int(r["block_size"])
        out.append((at, flags, st))
    return result, out


def result_tuple(r):
    get = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    return tuple(int(get(k)) for k in RESULT_FIELDS)


# ---- expectations by placement
class Expect:
    """rc; for rc == 0: first_sample, and the surviving frames in the order sent as (position, n, pcm [channels, n] or
    None for a frame that is kept but does not decode).  The walk over them (the rule's step 3) gives the rest."""

    def __init__(self, rc, survivors=()):
        self.rc = rc
        self.pieces, self.hidden = [], []   # (at, pcm) of decoded frames, (at, n) of concealed ones
        self.result = dict.fromkeys(RESULT_FIELDS, 0)
        self.result["rc"] = rc
        if rc:
            return
        origin = end = survivors[0][0]
        for k, (p, n, pcm) in enumerate(survivors):
            if k and p < end:
                self.result["dropped"] += 1
                continue
            if p > end:
                self.result["gaps"] += 1
                self.result["gap_samples"] += p - end
            self.result["placed"] += 1
            if pcm is None:
                self.hidden.append((p - origin, n))
                self.result["concealed"] += 1
                self.result["concealed_samples"] += n
            else:
                assert pcm.shape[1] == n
                self.pieces.append((p - origin, pcm))
            end = p + n
        self.result.update(first_sample=origin, timeline_samples=end - origin)

    @property
    def timeline_samples(self):
        return self.result["timeline_samples"]

    def gap_runs(self):
        """[(first row position, samples)] of the gaps."""
        covered = sorted([(at, p.shape[1]) for at, p in self.pieces] + self.hidden)
        out, end = [], 0
        for at, n in covered:
            if at > end:
                out.append((end, at - end))
            end = at + n
        return out


class Case:
    def __init__(self, label, blob, bits, channels, want, want_speculative=None):
        self.label, self.blob, self.bits, self.channels = label, bytes(blob), bits, channels
        self.want = {False: want, True: want if want_speculative is None else want_speculative}


def expected_rows(cases, speculative, Cp, T):
    """(int32 [n, Cp, T] of the samples, uint8 [n, T] of the mask): what decode_timeline owes for `cases` as one batch."""
    pcm = np.zeros((len(cases), Cp, T), dtype=np.int32)
    mask = np.zeros((len(cases), T), dtype=np.uint8)
    for i, case in enumerate(cases):
        for at, piece in case.want[speculative].pieces:
            pcm[i, :piece.shape[0], at:at + piece.shape[1]] = piece
            mask[i, at:at + piece.shape[1]] = 1
    return pcm, mask


# ---- building blocks
class Sent:
    """One coded frame: its bytes, position on the stream's time axis, samples and PCM [channels, n]."""

    def __init__(self, data, p, n, pcm):
        self.data, self.p, self.n, self.pcm = data, p, n, pcm

    def survivor(self, decodes=True):
        return (self.p, self.n, self.pcm if decodes else None)


def frames_of(rate, bits, channels, sizes, seed, blocking, numbers=None, first=0, odd=None):
    """The frames of a stream of one format as [Sent].  blocking 0: frame numbers first, first + 1, ... (position number
    * sizes[0]); blocking 1: sample numbers, `numbers` or the running sum from `first`.  odd: {frame index: keyword
    arguments of fs.Frame} -- a header that leaves its rate or sample size to a STREAMINFO."""
    st = rf.build([(rate, bits, channels, n) for n in sizes], seed, blocking=blocking)
    out, at = [], first
    for k, fr in enumerate(st.frames):
        number = (numbers[k] if numbers else at) if blocking else first + k
        kw = dict(assignment=fr.assignment, bcode=fr.bcode, rcode=fr.rcode, bps_code=fr.bps_code)
        kw.update((odd or {}).get(k, {}))
        data = fs.write_frame(rate, bits, fs.Frame(fr.pcm, fr.subs, blocking=blocking, number=number, **kw), set())
        out.append(Sent(data, number if blocking else number * sizes[0], fr.n, np.array(fr.pcm, dtype=np.int32)))
        at = number + fr.n if blocking else 0
    return out


def join(sent):
    return b"".join(s.data for s in sent)


def flip(blob, pos, x):
    b = bytearray(blob)
    b[pos] ^= x
    return bytes(b)


FIXED_SIZES = (192,) * 6 + (33,)


@functools.lru_cache(maxsize=1)
def fixed_stream():
    """6 x 192 and a short last 33, 16-bit stereo in all four assignments, frame numbers."""
    return tuple(frames_of(44100, 16, 2, FIXED_SIZES, 9100, 0))


def _whole(label, sent, bits, channels):
    return Case(label, join(sent), bits, channels, Expect(OK, [s.survivor() for s in sent]))


def _without(label, sent, lost, bits=16, channels=2):
    kept = [s for k, s in enumerate(sent) if k not in lost]
    return Case(label, join(kept), bits, channels, Expect(OK, [s.survivor() for s in kept]))


def residue_ladder():
    """Variable blocking, mono, block sizes 16 / 17 / 33 between gaps of 1 and 5 samples: the gaps' first and last row
    positions take every residue modulo 16."""
    sizes = [(17, 16, 33)[k % 3] for k in range(40)]
    numbers, at = [], 70000   # three-byte sample numbers
    for k, n in enumerate(sizes):
        numbers.append(at)
        at += n + (1, 5)[k % 2]
    return frames_of(48000, 16, 1, sizes, 9200, 1, numbers=numbers)


def long_gaps(piece):
    """Variable blocking, stereo, sample numbers from just below 2^32 on: gaps of 4097 samples, of two whole 4-byte
    pieces (one whole 2-byte piece: the gap ends on a piece boundary) and of more than one piece of every element size."""
    sizes = [192, 16, 33, 17, 192]
    gaps = [4097, 2 * (piece // 4), 5, piece + 5]
    numbers, at = [], (1 << 32) - 300
    for k, n in enumerate(sizes):
        numbers.append(at)
        at += n + (gaps[k] if k < len(gaps) else 0)
    return frames_of(44100, 16, 2, sizes, 9300, 1, numbers=numbers)


@functools.lru_cache(maxsize=None)
def cases(piece):
    """Every case, as one batch.  piece: the library's FLACGPU_TIMELINE_PIECE_BYTES."""
    out = []
    fx = list(fixed_stream())
    B = 192
    # 1. whole
    out.append(_whole("fixed: whole", fx, 16, 2))
    # 2. frames cut out
    for j in range(len(fx)):
        out.append(_without(f"fixed: frame {j} cut out", fx, {j}))
    out.append(_without("fixed: frames 2 and 3 cut out", fx, {2, 3}))
    out.append(_without("fixed: all but frame 3 cut out", fx, set(range(7)) - {3}))
    # 3. one byte flipped: in a header (the frame is no candidate: it ends nothing, so the frame in front is lost too
    # unless its own bits end it), and in a body (the frame's CRC-16 fails: no end, passed over)
    at3 = sum(len(s.data) for s in fx[:3])
    lost3 = Expect(OK, [s.survivor() for k, s in enumerate(fx) if k != 3])
    lost23 = Expect(OK, [s.survivor() for k, s in enumerate(fx) if k not in (2, 3)])
    out.append(Case("fixed: a byte of frame 3's header flipped", flip(join(fx), at3 + 2, 0x10), 16, 2, lost23, lost3))
    out.append(Case("fixed: a byte of frame 3's body flipped", flip(join(fx), at3 + len(fx[3].data) // 2, 0x5A), 16, 2,
                    lost3))
    assert lost23.result["gap_samples"] == 2 * B and lost3.result["gap_samples"] == B
    # the other widths, channel counts and block sizes, fixed blocking, one frame lost in the middle
    for k, (rate, bits, channels, n, count) in enumerate(((8000, 8, 1, 16, 5), (48000, 24, 3, 17, 5),
                                                          (192000, 32, 2, 33, 6), (96000, 12, 2, 16, 6),
                                                          (44100, 16, 2, 4096, 3))):
        sent = frames_of(rate, bits, channels, (n,) * count, 9400 + k, 0, first=(0, 130, 20000, 3, 7)[k])
        out.append(_whole(f"fixed {bits}-bit {channels} ch x {n}: whole", sent, bits, channels))
        out.append(_without(f"fixed {bits}-bit {channels} ch x {n}: frame 1 cut out", sent, {1}, bits, channels))
    # 4. variable blocking: sample numbers of several bytes, gaps at every residue, long gaps
    out.append(_whole("variable: gaps of 1 and 5 at every residue", residue_ladder(), 16, 1))
    out.append(_whole("variable: long gaps, numbers across 2^32", long_gaps(piece), 16, 2))
    for k, (bits, channels) in enumerate(((24, 2), (32, 2), (8, 3), (8, 2))):
        sizes = (16, 17, 33, 192)
        numbers = [5000, 5016, 5033 + 1, 5067 + 4097]   # no gap, a gap of 1, a gap of 4097
        sent = frames_of(44100, bits, channels, sizes, 9500 + k, 1, numbers=numbers)
        case = _whole(f"variable {bits}-bit {channels} ch", sent, bits, channels)
        assert (case.want[False].result["gaps"], case.want[False].result["gap_samples"]) == (2, 4098)
        out.append(case)
    # 5. a frame sent twice; two frames swapped
    out.append(Case("fixed: frame 2 sent twice", join(fx[:3] + fx[2:]), 16, 2,
                    Expect(OK, [s.survivor() for s in fx[:3] + fx[2:]])))
    swapped = fx[:2] + [fx[3], fx[2]] + fx[4:]
    out.append(Case("fixed: frames 2 and 3 swapped", join(swapped), 16, 2, Expect(OK, [s.survivor() for s in swapped])))
    assert out[-2].want[False].result["dropped"] == 1 and out[-2].want[False].result["gaps"] == 0
    assert out[-1].want[False].result["dropped"] == 1 and out[-1].want[False].result["gap_samples"] == B
    # 6. refusals
    out.append(Case("refused: mixed blocking", rf.build([(44100, 16, 2, 16)] * 4, 9600).blob, 16, 2, Expect(UNSUPPORTED)))
    out.append(Case("refused: fixed blocking, another block size in the middle",
                    join(frames_of(44100, 16, 2, (192, 33, 192), 9601, 0)), 16, 2, Expect(UNSUPPORTED)))
    out.append(Case("refused: fixed blocking, the last frame larger",
                    join(frames_of(44100, 16, 2, (33, 192), 9602, 0)), 16, 2, Expect(UNSUPPORTED)))
    out.append(Case("refused: frames of different formats", rf.mixed().blob, 32, 3, Expect(UNSUPPORTED)))
    out.append(Case("refused: empty", b"", 16, 0, Expect(INVALID_ARG)))
    for label, blob in rf.non_subset_cases():   # built on the stream of different formats: refused like it
        out.append(Case(f"refused: different formats, {label}", blob, 32, 3, Expect(UNSUPPORTED)))
    # 7. a whole frame that is no candidate, in a stream of one format: the record in front swallows it, does not parse
    # and is concealed; the swallowed frame's time is a gap
    for k, (label, kw) in enumerate((("rate code 0", dict(rcode=0)), ("sample-size code 0", dict(bps_code=0)))):
        sent = frames_of(44100, 16, 1, (16,) * 6, 9700 + k, 0, odd={3: kw})
        want = Expect(OK, [s.survivor(decodes=j != 2) for j, s in enumerate(sent) if j != 3])
        assert (want.result["concealed"], want.result["concealed_samples"], want.result["gap_samples"]) == (1, 16, 16)
        out.append(Case(f"non-subset frame, {label}", join(sent), 16, 1, want))
    # 8. a byte range of a regular file, cut inside a frame at both ends
    sent = frames_of(44100, 16, 2, (192,) * 8, 9800, 0)
    regular = fs.write_stream(44100, 16, rf.build([(44100, 16, 2, 192)] * 8, 9800, blocking=0).frames, name="range")
    assert regular.blob.endswith(join(sent))
    starts = [len(regular.blob) - len(join(sent[k:])) for k in range(8)] + [len(regular.blob)]
    a = starts[1] + 7
    whole = regular.pcm.reshape(-1, 2).T   # [channels, samples] of the whole file
    for label, b, last, last_spec in (("inside frame 6", starts[6] + len(sent[6].data) // 2, 5, 5),
                                      ("two bytes into frame 6", starts[6] + 2, 4, 5)):
        want = [Expect(OK, [s.survivor() for s in sent[2:e + 1]]) for e in (last, last_spec)]
        for w in want:   # the slice of the file's PCM
            lo, n = w.result["first_sample"], w.timeline_samples
            got = expected_rows([Case("", b"", 16, 2, w)], False, 2, n)[0][0]
            assert lo == 2 * 192 and np.array_equal(got, whole[:, lo:lo + n])
        out.append(Case(f"byte range of a file, from inside frame 1 to {label}", regular.blob[a:b], 16, 2, *want))
    return tuple(out)


def layout(case_list):
    """(channels_padded, samples_padded) of the batch: the most channels, and the longest timeline of either setting
    rounded up to 16 samples, so that every row begins on a 16-byte boundary in every element size."""
    T = max(c.want[s].timeline_samples for c in case_list for s in (False, True))
    return max(c.channels for c in case_list if c.want[False].rc == OK), (T + 15) & ~15


def coverage(case_list, piece):
    """What the gaps of the case set cover: per element size the residues modulo 16 of the byte offsets (in a row that
    begins on a 16-byte boundary) at which a gap begins and ends, whether one is longer than a piece, and whether one
    ends exactly on a piece boundary."""
    out = {}
    for es in (1, 2, 3, 4):
        first, last, longer, exact = set(), set(), False, False
        for c in case_list:
            for at, n in c.want[False].gap_runs():
                first.add(at * es % 16)
                last.add((at + n) * es % 16)
                longer |= n * es > piece
                exact |= n * es % piece == 0
        out[es] = (first, last, longer, exact)
    return out


def dump(case_list, speculative, scan):
    """The records of every case (scan(blob, speculative) -> rows with rf.RECORD_FIELDS) as text, for the stand-alone
    program that runs the host rule under sanitizers: a line `n` per stream, then n lines of the 13 fields."""
    lines = []
    for c in case_list:
        recs = scan(c.blob, speculative)
        lines.append(str(len(recs)))
        lines += [" ".join(str(v) for v in rf.record_tuple(r)) for r in recs]
    return "\n".join(lines) + "\n"


def random_records(seed, count):
    """Record lists no scan gives: wrapped and repeated numbers, numbers at the top of 36 bits, mixed shapes."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        blocking = rng.randint(0, 1)
        B = rng.choice((16, 17, 192, 4096))
        recs, number = [], rng.choice((0, 5, (1 << 32) - 2, (1 << 36) - 40))
        for k in range(rng.randint(1, 9)):
            n = B if not blocking or rng.random() < 0.5 else rng.choice((16, 33))
            if rng.random() < 0.08:
                n = rng.choice((B + 1, 7))
            recs.append(dict(byte_offset=100 * k, number=number, out_offset=0, stream=0, bytes=90, block_size=n,
                             sample_rate=44100 if rng.random() > 0.03 else 48000, channels=2, bits_per_sample=16,
                             assignment=1, blocking=blocking if rng.random() > 0.04 else 1 - blocking, status=0,
                             reserved=0))
            step = rng.choice((1, 1, 1, 2, 0, -1, 3)) if not blocking else rng.choice((n, n, n + 5, n - 3, 0, -n, 4097))
            number = max(0, min(number + step, (1 << 36) - 1))
        out.append(recs)
    return out
