"""k_sub64 / k_sub_finish (csrc/kernels/sub64.inc: frames of 5..8 channels, 4096-sample blocks, one workgroup per
subframe) at their word, CRC and placement edges: the cases, and a CPU model of the bit geometry.

geometry() restates the comments at the head of sub64.inc -- where a subframe's image lies in the word grid of the output,
which words it leaves to k_sub_finish, which bytes its CRC share covers and by which power of x the share is multiplied.
self_check() proves the restatement on a frame's bytes: the images tile the frame, the shares XOR to its CRC-16, the
merged edge words are its bytes.  Expected bytes are the oracle's (orc.encode_frame) for the cases the encoder decides
itself, and the host packer's (flacenc_pack_frames, plain C++) for hand-built plans -- sizes the encoder's own decisions
never give (a Rice-coded subframe of 23 .. 250 bits: the reference's shortest is a click in silence, 651 bits).

Every class of reached() is decided by geometry(), never by how a signal was made.  No GPU call in this module."""
import collections
from collections import namedtuple

import numpy as np

import _oracle as orc
from _compare import orc_options_for
from _pcm import synth_fast

B = 4096
CHW = 64 * 17                      # words per slice row of crc16_words_share
POLY = 0x18005
OPTS = dict(max_po=6, max_lpc=12)  # the encoder options of every case (exhaustive, Tukey 0.5)

# frames: [planar int32 [C][B]]; focus: the frames the case is about; group: cases that hold the same case frame at
# another alignment; plans: None, or per frame a list of hand-built subframe specs (hand_frame)
Case = namedtuple("Case", "name cls C bps rate first frames focus group plans")
Sub = namedtuple("Sub", "type bits")
Plan = namedtuple("Plan", "channels sub")
SubGeo = namedtuple("SubGeo", "ch type bits lead w0 nw img_end cov_end len nw4 len3 S padw exp")
Geo = namedtuple("Geo", "begin flen hbytes crc_at subs words")     # words: {word index: [entry names]}


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def geometry(frame_bytes, plan, begin):
    """The images of one frame's subframes as k_sub64 places them, and k_sub_finish's entries per output word."""
    nch = int(plan.channels)
    bits = [int(plan.sub[c].bits) for c in range(nch)]
    flen = len(frame_bytes)
    hbytes = flen - 2 - (sum(bits) + 7) // 8
    crc_at = 8 * (begin + flen - 2)
    subs, words = [], collections.OrderedDict()
    before = 0
    for c in range(nch):
        own = (8 * hbytes if c == 0 else 0) + bits[c]                  # subframe 0 carries the frame header
        gbit = 8 * begin + (0 if c == 0 else 8 * hbytes + before)
        lead, w0 = gbit & 31, gbit >> 5
        nw = (lead + own + 31) // 32
        img_end = 32 * (w0 + nw)
        cov_end = min(img_end, crc_at)                                 # the image's bytes up to the CRC field
        ln = cov_end // 8 - 4 * w0
        nw4 = ln >> 2
        S = (nw4 + CHW - 1) // CHW
        subs.append(SubGeo(c, int(plan.sub[c].type), bits[c], lead, w0, nw, img_end, cov_end, ln, nw4, ln & 3, S, S * CHW - nw4,
                           crc_at - cov_end))
        words.setdefault(w0, []).append("head%d" % c)
        if nw > 1:
            words.setdefault(w0 + nw - 1, []).append("tail%d" % c)
        before += bits[c]
    for k in range(2):
        words.setdefault((begin + flen - 2 + k) >> 2, []).append("crc%d" % k)
    return Geo(begin, flen, hbytes, crc_at, subs, words)


def gf_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a & 0x10000:
            a ^= POLY
    return r


def x_pow(k):
    """x^k mod x^16 + x^15 + x^2 + 1"""
    r, s = 1, 2
    while k:
        if k & 1:
            r = gf_mul(r, s)
        s = gf_mul(s, s)
        k >>= 1
    return r


def self_check(frame_bytes, geo):
    """The model on one frame: images cut from the frame's bit string (zeros outside a subframe's own bits), shares,
    edge words.  Raises AssertionError with the geometry."""
    begin, flen = geo.begin, geo.flen
    total = int.from_bytes(frame_bytes, "big")
    nbits = 8 * flen
    crc, at = 0, 0
    out = bytearray(flen)
    merged = collections.defaultdict(int)
    for s in geo.subs:
        own = (8 * geo.hbytes if s.ch == 0 else 0) + s.bits
        piece = (total >> (nbits - at - own)) & ((1 << own) - 1)
        at += own
        image = (piece << (32 * s.nw - s.lead - own)).to_bytes(4 * s.nw, "big")
        share = gf_mul(orc.crc16(image[: s.len]), x_pow(s.exp))
        assert s.cov_end == s.img_end or not any(image[s.len:]), (s, "bits of the image behind the CRC field's start")
        crc ^= share
        for j in range(s.nw):
            word = int.from_bytes(image[4 * j:4 * j + 4], "big")
            if j in (0, s.nw - 1):
                merged[s.w0 + j] |= word
            else:                                                      # interior: stored by the subframe's own workgroup
                b0 = 4 * (s.w0 + j) - begin
                assert 0 <= b0 and b0 + 4 <= flen and not any(out[b0:b0 + 4]), (s, j, "an interior word outside the frame or written twice")
                out[b0:b0 + 4] = image[4 * j:4 * j + 4]
    assert at == 8 * (flen - 2) - (-(8 * geo.hbytes + sum(s.bits for s in geo.subs)) % 8), "the subframes do not fill the frame"
    assert crc == int.from_bytes(frame_bytes[-2:], "big"), ("the shares do not XOR to the frame's CRC-16", hex(crc), geo.subs)
    for k in range(2):
        p = begin + flen - 2 + k
        merged[p >> 2] |= ((crc >> (8 - 8 * k)) & 0xFF) << (24 - 8 * (p & 3))
    assert set(merged) == set(geo.words)
    for w, v in merged.items():
        for e in range(4):
            p = 4 * w + e - begin
            byte = (v >> (24 - 8 * e)) & 0xFF
            if 0 <= p < flen:
                assert out[p] == 0, (w, e, "an edge word over an interior one")
                out[p] = byte
            else:
                assert byte == 0, (w, e, "an edge word carries bits outside its frame")
    assert bytes(out) == frame_bytes, "interior words + merged edge words are not the frame"


# ---------------------------------------------------------------------------------------------------------------------
# signals
# ---------------------------------------------------------------------------------------------------------------------
def channel(kind, bps, seed):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if kind == "zeros":
        return np.zeros(B, dtype=np.int32)
    if kind == "noise":
        return rng.integers(lo, hi + 1, size=B).astype(np.int32)
    if kind == "synth":
        return synth_fast(seed, 1, bps, B).astype(np.int32)
    if kind == "quiet":
        return rng.integers(-3, 4, size=B).astype(np.int32)
    if kind == "click":
        x = np.zeros(B, dtype=np.int32)
        x[int(rng.integers(0, B))] = hi if seed & 1 else lo
        return x
    if kind == "wasted2":
        return ((synth_fast(seed, 1, bps, B).astype(np.int64) >> 2) << 2).astype(np.int32)
    if kind == "rail":
        return np.full(B, lo, dtype=np.int32)
    if kind.startswith("amp"):                                          # amp125: uniform noise of that amplitude
        a = int(kind[3:])
        return rng.integers(-a, a + 1, size=B).astype(np.int32)
    raise KeyError(kind)


def frame_of(kinds, bps, seed):
    return np.stack([channel(k, bps, seed * 16 + c) for c, k in enumerate(kinds)])


def oracle_options():
    return orc_options_for(B, OPTS["max_po"], OPTS["max_lpc"], True, True)


def oracle_frame(planar, bps, rate, number):
    rc, data, plan = orc.encode_frame(oracle_options(), rate, bps, planar, frame_number=number)
    assert rc == 0
    return data, plan


# ---------------------------------------------------------------------------------------------------------------------
# hand-built plans: ("C", v) CONSTANT v; ("V", kind, seed) VERBATIM; ("F", order, po, v) FIXED of a constant signal v
# (v = 0 for order 0), every partition escaped with 0 bits
# ---------------------------------------------------------------------------------------------------------------------
def hand_bits(spec, bps):
    if spec[0] == "C":
        return 8 + bps
    if spec[0] == "V":
        return 8 + B * bps
    return 8 + spec[1] * bps + 6 + 9 * (1 << spec[2])


def hand_signal(spec, bps):
    if spec[0] == "C":
        return np.full(B, spec[1], dtype=np.int32)
    if spec[0] == "V":
        return channel(spec[1], bps, spec[2])
    return np.full(B, spec[3], dtype=np.int32)


def hand_plans(case):
    """(FramePlan array, SubframePlan array, residual rows) of a hand-built case, in the library's structures."""
    from flac_codec_amd._lib import FramePlan, SubframePlan

    n = len(case.frames)
    plans, subs = (FramePlan * n)(), (SubframePlan * (n * case.C))()
    rows = np.zeros((n, case.C, B), dtype=np.int32)
    for f, specs in enumerate(case.plans):
        plans[f].assignment, plans[f].channels, plans[f].block_size = 0, case.C, B
        plans[f].body_bits = sum(hand_bits(s, case.bps) for s in specs)
        for c, s in enumerate(specs):
            sp = subs[f * case.C + c]
            sp.type = {"C": 0, "V": 1, "F": 2}[s[0]]
            sp.bps, sp.source, sp.bits = case.bps, c, hand_bits(s, case.bps)
            sp.n_partitions, sp.part_len = 1, B
            x = case.frames[f][c]
            if s[0] == "C":
                rows[f, c, 0] = x[0]
            elif s[0] == "V":
                rows[f, c] = x
            else:
                sp.order, sp.partition_order, sp.n_partitions, sp.part_len = s[1], s[2], 1 << s[2], B >> s[2]
                rows[f, c, : s[1]] = x[: s[1]]
                for i in range(1 << s[2]):
                    sp.rice[i], sp.escape_bits[i] = 0xFF, 0
    return plans, subs, rows


_encoded = {}


def encoded(case):
    """[(frame bytes, plan, begin)] of a case: the oracle's frames, or the host packer's for hand-built plans."""
    if case.name not in _encoded:
        out, begin = [], 0
        if case.plans is None:
            for f, planar in enumerate(case.frames):
                data, plan = oracle_frame(planar, case.bps, case.rate, case.first + f)
                out.append((data, plan, begin))
                begin += len(data)
        else:
            from flac_codec_amd.gpu import host_pack_frames

            plans, subs, rows = hand_plans(case)
            data, off = host_pack_frames(case.rate, case.bps, case.C, case.first, len(case.frames), B, plans, subs, rows)
            for f, specs in enumerate(case.plans):
                plan = Plan(case.C, [Sub({"C": 0, "V": 1, "F": 2}[s[0]], hand_bits(s, case.bps)) for s in specs])
                out.append((data[off[f]:off[f + 1]], plan, off[f]))
        _encoded[case.name] = out
    return _encoded[case.name]


def batch_bytes(case):
    enc = encoded(case)
    return b"".join(d for d, _, _ in enc), [b for _, _, b in enc] + [enc[-1][2] + len(enc[-1][0])]


def interleaved(case):
    return np.ascontiguousarray(np.stack(case.frames).transpose(0, 2, 1)).astype(np.int32).reshape(-1)


def geometries(case):
    return [geometry(d, p, b) for d, p, b in encoded(case)]


def describe(case, f):
    g = geometries(case)[f]
    lines = ["%s frame %d: begin %d (& 3 = %d), %d bytes, header %d" % (case.name, f, g.begin, g.begin & 3, g.flen, g.hbytes)]
    lines += ["  " + str(s) for s in g.subs]
    lines += ["  word %d: %s" % (w, " ".join(n)) for w, n in g.words.items()]
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def spacer(C_, bps, rate, number, mod, want, salt=0):
    """A frame of one quiet channel among silent ones whose oracle length is `want` modulo `mod`: seeds in order, the first
    that fits (the length of a Rice-coded channel moves by a few bytes from seed to seed)."""
    for seed in range(600):
        kinds = ["zeros"] * C_
        kinds[(seed + salt) % C_] = "quiet" if seed % 3 else "synth"
        planar = frame_of(kinds, bps, 7000 + 37 * salt + seed)
        data, _ = oracle_frame(planar, bps, rate, number)
        if len(data) % mod == want:
            return planar
    raise AssertionError(("no spacer", C_, bps, mod, want))


def follower(C_, bps, seed):
    return frame_of(["synth", "quiet", "noise", "wasted2", "synth", "click", "synth", "quiet"][:C_], bps, 300 + seed)


def aligned_group(name, cls, kinds, bps, rate=48000, first=0, seed=1):
    """The same case frame at begin & 3 = 0, 1, 2, 3: a spacer picked by its length in front, a non-silent frame behind."""
    C_ = len(kinds)
    x = frame_of(kinds, bps, seed)
    return [Case("%s@%d" % (name, k), cls, C_, bps, rate, first, [spacer(C_, bps, rate, first, 4, k, salt=k), x, follower(C_, bps, seed)],
                 [1], name, None) for k in range(4)]


def run_cases():
    """(a): runs of 2..7 silent channels at the start, in the middle and at the end of a frame, every bps of the list in turn;
    an all-silent frame at every channel count."""
    loud = ("noise", "synth", "quiet", "click", "wasted2", "rail")
    bpss = (4, 8, 12, 16, 20, 24)
    out, i = [], 0
    for C_ in (5, 6, 7, 8):
        per_bps = collections.defaultdict(list)
        for r in range(2, C_):
            for place in ("start", "middle", "end"):
                if place == "middle" and r > C_ - 2:
                    continue
                at = 0 if place == "start" else C_ - r if place == "end" else 1 + (i % (C_ - r - 1))
                kinds = [loud[(i + c) % len(loud)] for c in range(C_)]
                kinds[at:at + r] = ["zeros"] * r
                per_bps[bpss[i % 6]].append(frame_of(kinds, bpss[i % 6], 100 + i))
                i += 1
        for bps in bpss:
            frames = per_bps[bps] + [np.zeros((C_, B), dtype=np.int32), follower(C_, bps, i)]
            out.append(Case("runs_c%d_b%d" % (C_, bps), "a", C_, bps, 48000, 3, frames, list(range(len(frames) - 1)), None, None))
            i += 1
    return out


def crc_row_cases():
    """(d): Rice-coded subframes of 1087, 1088 and 1089 words -- quiet noise of about 8.5 bits per sample, seed after seed
    until a subframe of each size is met (a bounded search: a miss fails reached(), it drops nothing)."""
    out, want = [], {1087, 1088, 1089}
    for seed in range(400):
        if not want:
            break
        amps = ["amp%d" % (124 + (seed + c) % 5) for c in range(6)]
        x = frame_of(amps, 16, 9000 + seed)
        case = Case("rows_seed%d" % seed, "d", 6, 16, 48000, 0, [x, follower(6, 16, seed)], [0], None, None)
        hit = {s.nw4 for s in geometries(case)[0].subs} & want
        if hit:
            want -= hit
            out.append(case)
        else:
            _encoded.pop(case.name, None)
    return out


def power_cases():
    """(g): exponents 8 below, at and 8 above a multiple of 1024 bits -- the size of a quiet last channel moves every
    earlier subframe's exponent; seeds in order until each is met."""
    out, want = [], {1016, 0, 8}
    for seed in range(600):
        if not want:
            break
        x = frame_of(["noise", "zeros", "synth", "zeros", "quiet"], 8, 11000 + seed)
        case = Case("pow_seed%d" % seed, "g", 5, 8, 48000, 0, [x, follower(5, 8, seed)], [0], None, None)
        hit = {s.exp % 1024 for s in geometries(case)[0].subs if s.exp >= 1024} & want
        if hit:
            want -= hit
            out.append(case)
        else:
            _encoded.pop(case.name, None)
    return out


def largest_cases():
    """(f): every channel VERBATIM at 24 bits behind a 14-byte header, channel 0 at lead 24 in a word with (w0 & 3) = 3"""
    out = []
    first, rate = 0xFFFFFFFF0, 12345
    for C_ in (5, 8):
        x = frame_of(["noise"] * C_, 24, 50 + C_)
        out.append(Case("largest_c%d" % C_, "f", C_, 24, rate, first, [spacer(C_, 24, rate, first, 16, 15), x, follower(C_, 24, C_)], [1],
                        None, None))
    return out


def header_cases():
    out = []
    for first in (126, 2046):
        frames = [frame_of(["zeros", "noise", "zeros", "zeros", "synth", "zeros"], 16, first + f) for f in range(4)]
        out.append(Case("header_from_%d" % first, "h", 6, 16, 48000, first, frames, [0, 1, 2, 3], None, None))
    frames = []
    for f in range(65):
        kinds = ["zeros"] * 6
        if f % 16 == 5:
            kinds[f % 6] = "quiet"
        if f in (63, 64):
            kinds[2] = "click"
        frames.append(frame_of(kinds, 16, 400 + f))
    out.append(Case("sixty_five_frames", "h", 6, 16, 48000, 100, frames, list(range(65)), None, None))
    return out


def interior_cases():
    """(e): nw = 1 .. 9 at every (w0 + 1) & 3, from hand-built plans: CONSTANT subframes and FIXED subframes of constant
    signals whose partitions are all escaped with 0 bits (23 .. 250 bits).  Seeded draws; a frame is kept when it reaches
    a pair not reached before."""
    rng = np.random.Generator(np.random.PCG64(0xE5))
    out, missing = [], {(nw, a) for nw in range(1, 10) for a in range(4)}
    for C_, bps in ((5, 16), (6, 8), (7, 24), (8, 12)):
        kept, begin = [], 0
        for _ in range(400):
            if len(kept) == 6 or not missing:
                break
            specs = []
            for c in range(C_):
                t = int(rng.integers(0, 8))
                v = int(rng.integers(-(1 << (bps - 1)), 1 << (bps - 1)))
                if t == 0:
                    specs.append(("C", v))
                else:
                    order = int(rng.integers(0, 5))
                    po = int(rng.integers(0, 5))
                    if hand_bits(("F", order, po, 0), bps) > 260:
                        po = 0
                    specs.append(("F", order, po, v if order else 0))
            plan = Plan(C_, [Sub(0, hand_bits(s, bps)) for s in specs])
            flen = 6 + (sum(s.bits for s in plan.sub) + 7) // 8 + 2
            g = geometry(bytes(flen), plan, begin)
            new = {(s.nw, (s.w0 + 1) & 3) for s in g.subs[1:]} & missing
            if new:
                missing -= new
                kept.append(specs)
                begin += flen
        if kept:
            kept.append([("V", "synth", 77)] + [("C", 1)] * (C_ - 2) + [("V", "noise", 78)])   # CONSTANT beside VERBATIM, both orders
            frames = [np.stack([hand_signal(s, bps) for s in specs]) for specs in kept]
            out.append(Case("interior_c%d_b%d" % (C_, bps), "e", C_, bps, 48000, 0, frames, list(range(len(frames))), None, kept))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        out = run_cases()
        out += aligned_group("one_loud_seven_silent_b4", "c", ["noise"] + ["zeros"] * 7, 4)
        out += aligned_group("five_silent_of_seven_b16", "b", ["synth", "zeros", "zeros", "noise", "zeros", "zeros", "zeros"], 16, seed=2)
        out += aligned_group("all_silent_c6_b24", "b", ["zeros"] * 6, 24, seed=3)
        out += aligned_group("noise17_c5", "d", ["noise"] * 5, 17, seed=4)
        out += aligned_group("noise17_c8", "d", ["noise"] * 8, 17, seed=5)
        out += crc_row_cases() + interior_cases() + largest_cases() + power_cases() + header_cases()
        assert len({c.name for c in out}) == len(out)
        _cases = out
    return _cases


# ---------------------------------------------------------------------------------------------------------------------
# what the matrix reaches
# ---------------------------------------------------------------------------------------------------------------------
REQUIRED = (
    ["a_run_bps%d" % b for b in (4, 8, 12, 16, 20, 24)] + ["a_run_len%d" % r for r in range(2, 8)] +
    ["a_run_start", "a_run_middle", "a_run_end"] + ["a_all_silent_c%d" % c for c in (5, 6, 7, 8)] +
    ["a_nw1_middle", "a_nw1_last", "a_three_records", "a_four_records", "a_tail_head_crc", "a_lead0_unshared",
     "b_crc_one_word", "b_crc_straddles", "b_crc_with_whole_last_subframe", "b_crc_word_shared_with_next_frame",
     "b_nonlast_past_crc", "c_begin_all_four", "c_end_all_four", "c_follower_not_silent"] +
    ["d_S%d" % s for s in range(4)] + ["d_nw4_%d" % v for v in (0, 1, 1087, 1088, 1089, 2177)] +
    ["d_nw4_2176_padw0_c5", "d_nw4_2176_padw0_c8", "d_nw4_2177_c5", "d_nw4_2177_c8"] + ["d_len3_%d_rows" % v for v in range(4)] +
    ["e_nw%d_a%d" % (nw, a) for nw in range(1, 10) for a in range(4)] +
    ["f_all_verbatim24_header14_lead24_w3_c5", "f_all_verbatim24_header14_lead24_w3_c8",
     "g_exp_0", "g_exp_below_1024k", "g_exp_at_1024k", "g_exp_above_1024k", "g_exp_hi_512_up", "g_exp_688000",
     "h_header_grows_1_2", "h_header_grows_2_3", "h_more_than_64_frames"])


def reached(case_list):
    """Counter: class name -> how many subframes (frames, for the per-frame classes) of the matrix reach it."""
    n = collections.Counter()
    groups = collections.defaultdict(lambda: (set(), set()))
    for case in case_list:
        geos = geometries(case)
        enc = encoded(case)
        if len(geos) > 64:
            n["h_more_than_64_frames"] += 1
        for f, g in enumerate(geos):
            C_, subs, last = case.C, g.subs, g.subs[-1]
            types = [s.type for s in subs]
            if f and g.hbytes == geos[f - 1].hbytes + 1:
                n["h_header_grows_%d_%d" % (g.hbytes - 6, g.hbytes - 5)] += 1
            # (a) runs of CONSTANT subframes
            c = 0
            while c < C_:
                if types[c] != orc.SUB_CONSTANT:
                    c += 1
                    continue
                e = c
                while e < C_ and types[e] == orc.SUB_CONSTANT:
                    e += 1
                r = e - c
                if r == C_:
                    n["a_all_silent_c%d" % C_] += 1
                if r >= 2:
                    n["a_run_bps%d" % case.bps] += 1
                    n["a_run_len%d" % r] += 1
                    n["a_run_start" if c == 0 and e < C_ else "a_run_end" if e == C_ and c > 0 else "a_run_middle" if c > 0 else "a_run_all"] += 1
                c = e
            for s in subs[1:]:
                if s.nw == 1:
                    n["a_nw1_last" if s.ch == C_ - 1 else "a_nw1_middle"] += 1
                prev = subs[s.ch - 1]
                if s.lead == 0 and prev.w0 + prev.nw == s.w0 and types[s.ch] == orc.SUB_CONSTANT:
                    n["a_lead0_unshared"] += 1
            for w, names in g.words.items():
                recs = [x for x in names if not x.startswith("crc")]
                if len(recs) == 3:
                    n["a_three_records"] += 1
                if len(recs) >= 4:
                    n["a_four_records"] += 1
                if any(x.startswith("tail") for x in names) and any(x.startswith("head") for x in names) and len(recs) < len(names):
                    n["a_tail_head_crc"] += 1
            # (b) the CRC field
            at = g.begin + g.flen - 2
            n["b_crc_straddles" if at & 3 == 3 else "b_crc_one_word"] += 1
            if last.nw == 1 and at >> 2 == last.w0 and at & 3 != 3:
                n["b_crc_with_whole_last_subframe"] += 1
            if (g.begin + g.flen) & 3 and f + 1 < len(geos):
                n["b_crc_word_shared_with_next_frame"] += 1
            n["b_nonlast_past_crc"] += sum(1 for s in subs[:-1] if s.img_end > g.crc_at)
            # (c) alignment of one and the same case frame
            if case.group and f in case.focus:
                groups[case.group][0].add(g.begin & 3)
                groups[case.group][1].add((g.begin + g.flen) & 3)
                nxt = enc[f + 1][1]
                if any(nxt.sub[k].type != orc.SUB_CONSTANT for k in range(C_)):
                    n["c_follower_not_silent"] += 1
            # (d) CRC rows
            for s in subs:
                n["d_S%d" % s.S] += 1
                if s.nw4 in (0, 1, 1087, 1088, 1089, 2177):
                    n["d_nw4_%d" % s.nw4] += 1
                if s.ch == C_ - 1 and case.bps == 17 and types[s.ch] == orc.SUB_VERBATIM and C_ in (5, 8):
                    if s.nw4 == 2176 and s.padw == 0:
                        n["d_nw4_2176_padw0_c%d" % C_] += 1
                    if s.nw4 == 2177 and s.padw == CHW - 1:
                        n["d_nw4_2177_c%d" % C_] += 1
                if s.S >= 1:
                    n["d_len3_%d_rows" % s.len3] += 1
                # (e) interior stores
                if 1 <= s.nw <= 9:
                    n["e_nw%d_a%d" % (s.nw, (s.w0 + 1) & 3)] += 1
                # (g) the power table
                if s.exp == 0:
                    n["g_exp_0"] += 1
                elif s.exp >= 1024:
                    m = s.exp % 1024
                    n["g_exp_below_1024k" if m == 1016 else "g_exp_at_1024k" if m == 0 else "g_exp_above_1024k" if m == 8 else "g_exp_other"] += 1
                if s.exp >> 10 >= 512:
                    n["g_exp_hi_512_up"] += 1
                if s.exp >= 688000:
                    n["g_exp_688000"] += 1
            # (f) the largest image
            if (case.bps == 24 and all(t == orc.SUB_VERBATIM for t in types) and g.hbytes == 14 and subs[0].lead == 24 and
                    subs[0].w0 & 3 == 3 and C_ in (5, 8)):
                n["f_all_verbatim24_header14_lead24_w3_c%d" % C_] += 1
    n["c_begin_all_four"] = sum(1 for b, _ in groups.values() if b == {0, 1, 2, 3})
    n["c_end_all_four"] = sum(1 for _, e in groups.values() if e == {0, 1, 2, 3})
    return n


def route_inputs(case, knobs=0):
    """tests/test_route_table.py's hook row of a plain encode_device batch of this case"""
    return dict(channels=case.C, bps=case.bps, block=B, order=OPTS["max_lpc"], po=OPTS["max_po"], exhaustive=1, layout=0, aligned=1,
                short_last=0, n_frames=len(case.frames), packed=0, lag_split=4, timing=0, segments=0, knobs=knobs, chunk=-1, two_ranges=0,
                whole_call=1)
