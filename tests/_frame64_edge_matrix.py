"""k_frame64 / wave_subframe (csrc/kernels/pack.inc: frames of 1..4 channels at the five wave block lengths, one wave per
subframe) at their Rice, escape, word and CRC edges: hand-built plans, a builder, and a CPU model of the bit geometry.

A case is a shape (block, channels, bps, the context's max_lpc / mid_side / exhaustive, rate, first frame number) plus
frames: _flacsyn.Frame's, that is PCM and one explicit constant() / verbatim() / fixed() / lpc() spec per subframe.  The
builder derives everything else from that one description: the expected bytes (_flacsyn.write_frame, which uses no
project code), the interleaved PCM and the FramePlan / SubframePlan records flacgpu_pack_plans takes (`bits` counted by
the Python writer), the residual rows flacenc_pack_frames takes (the second reference; test_frame64_edge_matrix_host.py
proves the two agree on every frame), and a geometry record per frame.

geometry() restates the comments and code of wave_subframe / k_frame64: the image starts at frame bit 0 (image word =
frame bit >> 5); per subframe its base bit; per lane its first bit, from the kernel's own sum (partition header when the
lane starts a partition, quotients + cnt (k + 1) or cnt * escape bits); per Rice code its end bit, width k + 1 and
quotient; per frame begin, flen, nw4, (flen - 2) & 3, S, padw, nout, begin & 3.  self_check() proves it on the frame's
bytes: every field, every escaped value and every partition header sits where the record says, with zeros for the
quotients, and the 17-word slice rows of crc16_words_share fold to the frame's CRC-16.

Every class of reached() is decided by the geometry, never by how a signal was made.  The cases of one shape are the
frames of ONE batch (batches()): frame numbers and byte offsets run through it, so a generator is told where its first
frame begins.  No GPU call in this module.

LEFT OUT: the direct instantiations (DIRECT = true: they differ from the planar ones in loads and placing only), the
transposing instantiations (XP) and the handed rows.  flacgpu_pack_plans cannot reach them (it sets no_direct); they stay
with test_gpu_pack.py, test_gpu_decisions.py and test_gpu_hand_over.py."""
import collections
import random
from collections import namedtuple

import numpy as np

import _flacsyn as fs
from _sub64_edge_matrix import gf_mul, x_pow

BLOCKS = (1024, 1152, 2048, 2304, 4096)
HB = 6                                     # frame header bytes of every frame here: coded block and rate, number < 128
Shape = namedtuple("Shape", "block C bps max_lpc mid_side exhaustive rate first")
Case = namedtuple("Case", "name family shape gen")             # gen(begin) -> [fs.Frame] (numbers are set by the batch)
Built = namedtuple("Built", "case frames recs")                 # recs: [FrameRec]
FrameRec = namedtuple("FrameRec", "data begin number subs geo")  # subs: [dict] (plan fields, v, res)
Batch = namedtuple("Batch", "shape built")
PartGeo = namedtuple("PartGeo", "index escaped param hdr_end first_res count end")
SubGeo = namedtuple("SubGeo", "ch type base body0 pos order porder method hb lane_first lane_bits parts code_end code_w code_q code_i "
                              "esc_start esc_w esc_val warm_end")
Geo = namedtuple("Geo", "begin flen hbytes nw4 rem S padw nout r NT SPL MAXO subs")
TYPES = {"constant": 0, "verbatim": 1, "fixed": 2, "lpc": 3}
KIND_OF = {v: k for k, v in TYPES.items()}
SRC_MID, SRC_SIDE = 8, 9


def shape(block, C, bps, max_lpc=16, mid_side=1, exhaustive=1, rate=48000, first=0):
    return Shape(block, C, bps, max_lpc, mid_side, exhaustive, rate, first)


# ---------------------------------------------------------------------------------------------------------------------
# the launch, restated: launch_frame64 (pack.hip) for a batch without Params::inter, and the image its launch gets
# (kernels/shape.h frame_fb_words / frame_fb_words_exhaustive_stereo, pack_impl's choice between them)
# ---------------------------------------------------------------------------------------------------------------------
def launcher(sh):
    """(NT, SPL, MAXO) of k_frame64<NT, SPL, MAXO>"""
    assert sh.C <= 4 and sh.block in BLOCKS and (sh.max_lpc <= 16 or sh.block == 4096)
    if sh.max_lpc > 16:
        return 64 * sh.C, 64, 32               # launch_frame64_deep
    if sh.block == 4096:
        return 64 * sh.C, 64, 16               # launch_frame64_4096
    return 64 * sh.C, sh.block // 64, 16       # launch_frame64_short


def fb_words(C, bps, n):
    return (((16 + 2) * 8 + C * (n * (bps + 1) + 64) + 31) // 32 + 2 + 3) & ~3


def fb_words_exhaustive_stereo(bps, n):
    return (((16 + 2) * 8 + 2 * (n * bps + 64) + 31) // 32 + 2 + 3) & ~3


def image_words(sh):
    words = fb_words(sh.C, sh.bps, sh.block)
    if sh.C == 2 and sh.bps < 32 and sh.exhaustive:
        words = min(words, fb_words_exhaustive_stereo(sh.bps, sh.block))
    return words


def max_body_bits(sh):
    """The most body bits flacgpu_pack_plans takes for a frame of this shape (host/plan_check.cpp): the image under a
    16-byte header, and at most three CRC slice rows: (16 + ceil(body / 8)) >> 2 <= 3 * 17 * NT."""
    image = (image_words(sh) - 2) * 32 - (16 + 2) * 8
    rows = 8 * (4 * 3 * 17 * 64 * sh.C + 3 - 16)
    return min(image, rows)


def max_nw4(sh):
    return (HB + (max_body_bits(sh) + 7) // 8) >> 2


def route_inputs(sh, n_frames, knobs=1, po=6):
    """tests/test_route_table.py's hook row of this shape's batch as flacgpu_pack_plans routes it (no_direct set)"""
    return dict(channels=sh.C, bps=sh.bps, block=sh.block, order=sh.max_lpc, po=po, exhaustive=sh.exhaustive, layout=0, aligned=1,
                short_last=0, n_frames=n_frames, packed=0, lag_split=4, timing=0, segments=0, knobs=knobs, chunk=-1, two_ranges=0,
                whole_call=0)


# ---------------------------------------------------------------------------------------------------------------------
# the builder: one Frame -> bytes, plan fields, residual rows
# ---------------------------------------------------------------------------------------------------------------------
def sub_channels(fr):
    """The subframes' sample sequences and sources (write_frame's arithmetic)"""
    a, ch = fr.assignment, fr.pcm
    if a == 8:
        return [ch[0], [x - y for x, y in zip(*ch)]], [0, SRC_SIDE]
    if a == 9:
        return [[x - y for x, y in zip(*ch)], ch[1]], [SRC_SIDE, 1]
    if a == 10:
        return [[(x + y) >> 1 for x, y in zip(*ch)], [x - y for x, y in zip(*ch)]], [SRC_MID, SRC_SIDE]
    return ch, list(range(len(ch)))


def build_frame(sh, fr, begin):
    feats = set()
    data = fs.write_frame(sh.rate, sh.bps, fr, feats)
    chans, sources = sub_channels(fr)
    subs = []
    for c, (samples, sub) in enumerate(zip(chans, fr.subs)):
        sbps = sh.bps + (1 if sources[c] == SRC_SIDE else 0)
        bw = fs.Bits()
        fs.write_subframe(bw, samples, sbps, sub, set())
        w, order = sub["wasted"], sub["order"]
        v = [s >> w for s in samples]
        coded = sub["kind"] in ("fixed", "lpc")
        coefs = list(sub["coefs"]) if sub["kind"] == "lpc" else fs.FIXED_COEFS[order] if coded else []
        po = sub["porder"] if coded else 0
        d = dict(type=TYPES[sub["kind"]], wasted=w, bps=sbps - w, order=order if coded else 0, precision=sub["precision"],
                 shift=sub["shift"], method=sub["method"] if coded else 0, porder=po, source=sources[c], n_partitions=1 << po,
                 part_len=fr.n >> po, bits=bw.total, coefs=coefs if sub["kind"] == "lpc" else [],
                 rice=[0xFF if isinstance(p, tuple) else p for p in sub["params"]] if coded else [],
                 esc=[p[1] if isinstance(p, tuple) else 0 for p in sub["params"]] if coded else [],
                 v=v, res=fs.residuals(v, order, coefs, sub["shift"]) if coded else [])
        subs.append(d)
    assert len(data) == HB + (sum(d["bits"] for d in subs) + 7) // 8 + 2, "the header is not the six bytes the sizes count on"
    geo = geometry(sh, len(data), subs, begin)
    return FrameRec(data, begin, fr.number, subs, geo)


_batches = {}


def shapes():
    """the shapes of the matrix, in the order their first case appears (nothing is built)"""
    return list(collections.OrderedDict((case.shape, None) for case in case_list()))


def batch_of(sh):
    """The Batch of one shape: its cases in the order of case_list(), every case built where the case before it ended."""
    if sh not in _batches:
        built, begin, number = [], 0, sh.first
        for case in case_list():
            if case.shape != sh:
                continue
            frames = case.gen(begin)
            recs = []
            for fr in frames:
                fr.number, fr.rcode = number, fs.RATE_CODES[sh.rate]      # (the encoder codes the rate in the frame header)
                recs.append(build_frame(sh, fr, begin))
                begin += len(recs[-1].data)
                number += 1
            built.append(Built(case, frames, recs))
        assert number < 128, (sh, number, "a second byte for the frame number")
        _batches[sh] = Batch(sh, built)
    return _batches[sh]


def batches():
    return [batch_of(sh) for sh in shapes()]


def parity_shapes():
    """One shape per block length, channel count and depth -- the first of each in the matrix: its batch also goes through
    the generic packer (whose k_pack holds a subframe of at most 40 + 33 n bits; the row-sized frames of family (d) put a
    whole image's bits into one subframe and stay with k_frame64)."""
    return list({(sh.block, sh.C, sh.max_lpc > 16): sh for sh in reversed(shapes())}.values())[::-1]


def shape_id(sh):
    return "n%d-c%d-b%d-lpc%d%s%s-r%d" % (sh.block, sh.C, sh.bps, sh.max_lpc, "" if sh.exhaustive else "-fast", "" if sh.mid_side else "-lr", sh.rate)


def batch_frames(b):
    return [(bt, i) for bt in b.built for i in range(len(bt.recs))]


def batch_bytes(b):
    recs = [bt.recs[i] for bt, i in batch_frames(b)]
    return b"".join(r.data for r in recs), [r.begin for r in recs] + [recs[-1].begin + len(recs[-1].data)]


def interleaved(b):
    rows = [np.array(bt.frames[i].pcm, dtype=np.int32).T for bt, i in batch_frames(b)]      # [n][C] per frame
    return np.ascontiguousarray(np.concatenate(rows)).reshape(-1)


def plan_arrays(b):
    """(FramePlan array, SubframePlan array, residual rows [frames][C][block]) in the library's structures"""
    from flac_codec_amd._lib import FramePlan, SubframePlan

    sh = b.shape
    fl = batch_frames(b)
    plans, subs = (FramePlan * len(fl))(), (SubframePlan * (len(fl) * sh.C))()
    rows = np.zeros((len(fl), sh.C, sh.block), dtype=np.int32)
    for f, (bt, i) in enumerate(fl):
        fr, rec = bt.frames[i], bt.recs[i]
        plans[f].assignment = fr.assignment if fr.assignment >= 8 else 0
        plans[f].channels, plans[f].block_size = sh.C, sh.block
        plans[f].body_bits = sum(d["bits"] for d in rec.subs)
        for c, d in enumerate(rec.subs):
            sp = subs[f * sh.C + c]
            sp.type, sp.wasted, sp.bps, sp.order = d["type"], d["wasted"], d["bps"], d["order"]
            sp.precision, sp.shift, sp.coding_method, sp.partition_order = d["precision"], d["shift"], d["method"], d["porder"]
            sp.source, sp.n_partitions, sp.part_len, sp.bits = d["source"], d["n_partitions"], d["part_len"], d["bits"]
            for j in range(len(sp.coeffs)):                            # (behind the order: anything -- the kernels read `order` taps)
                sp.coeffs[j] = d["coefs"][j] if j < len(d["coefs"]) else (-1) ** j * (0x12345 + 77 * j) if d["type"] == 3 else 0
            for j, k in enumerate(d["rice"]):
                sp.rice[j], sp.escape_bits[j] = k, d["esc"][j]
            if d["type"] == 0:
                rows[f, c, 0] = d["v"][0]
            elif d["type"] == 1:
                rows[f, c] = d["v"]
            else:                                                      # warm-up samples, then residuals
                rows[f, c, : d["order"]] = d["v"][: d["order"]]
                rows[f, c, d["order"]:] = d["res"]
    return plans, subs, rows


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def zigzag(r):
    return (r << 1) ^ (r >> 63)


def geometry(sh, flen, subs, begin):
    NT, SPL, MAXO = launcher(sh)
    n = sh.block
    out, base = [], 8 * HB
    for c, d in enumerate(subs):
        body0 = base + 8 + d["wasted"]
        bps, order, typ = d["bps"], d["order"], d["type"]
        empty = np.zeros(0, dtype=np.int64)
        if typ == 0:
            out.append(SubGeo(c, typ, base, body0, body0, 0, 0, 0, 0, None, None, [], empty, empty, empty, empty, empty, empty, empty, body0 + bps))
        elif typ == 1:                                                 # lane l streams its SPL samples from body0 + l * SPL * bps
            first = body0 + np.arange(64, dtype=np.int64) * SPL * bps
            out.append(SubGeo(c, typ, base, body0, body0, 0, 0, 0, 0, first, np.full(64, SPL * bps, dtype=np.int64), [], empty, empty,
                              empty, empty, empty, empty, empty, body0))
        else:
            resid_pos = body0 + order * bps + (9 + order * d["precision"] if typ == 3 else 0)
            pos = resid_pos + 6
            method, po = d["method"], d["porder"]
            hb = 5 if method else 4
            lpp = 6 - min(po, 6)                                       # log2(lanes per partition)
            u = zigzag(np.array(d["res"], dtype=np.int64))
            res = np.array(d["res"], dtype=np.int64)
            # the kernel's sum: per lane, its partition header when it starts one + its codes
            kl = np.array([d["rice"][l >> lpp] for l in range(64)], dtype=np.int64)
            el = np.array([d["esc"][l >> lpp] for l in range(64)], dtype=np.int64)
            lane_bits = np.zeros(64, dtype=np.int64)
            for l in range(64):
                lo, hi = max(l * SPL, order) - order, (l + 1) * SPL - order     # the lane's residuals (lane 0: behind the warm-up)
                cnt = SPL - (order if l == 0 else 0)
                assert cnt == hi - lo and cnt >= 0
                head = (l & ((1 << lpp) - 1)) == 0
                rice = kl[l] != 0xFF
                lane_bits[l] = (hb + (0 if rice else 5) if head else 0) + (int((u[lo:hi] >> kl[l]).sum()) + cnt * (kl[l] + 1) if rice else cnt * el[l])
            lane_first = pos + np.concatenate(([0], np.cumsum(lane_bits)[:-1]))
            # the stream's own order: partition by partition
            plen = n >> po
            assert plen == SPL << lpp
            parts, ce, cw, cq, ci, es, ew, ev = [], [], [], [], [], [], [], []
            at, ri = pos, 0
            for p in range(1 << po):
                cnt = plen - order if p == 0 else plen
                k, eb = d["rice"][p], d["esc"][p]
                assert at == lane_first[p << lpp], "a partition does not start where its head lane does"
                if k == 0xFF:
                    hdr_end = at + hb + 5
                    starts = hdr_end + eb * np.arange(cnt, dtype=np.int64)
                    es.append(starts)
                    ew.append(np.full(cnt, eb, dtype=np.int64))
                    ev.append(res[ri:ri + cnt] & ((1 << eb) - 1))
                    end = hdr_end + eb * cnt
                else:
                    hdr_end = at + hb
                    q = u[ri:ri + cnt] >> k
                    ends = hdr_end + np.cumsum(q + k + 1)
                    ce.append(ends)
                    cw.append(np.full(cnt, k + 1, dtype=np.int64))
                    cq.append(q)
                    ci.append(np.arange(ri, ri + cnt, dtype=np.int64))
                    end = int(ends[-1]) if cnt else hdr_end
                parts.append(PartGeo(p, k == 0xFF, eb if k == 0xFF else k, hdr_end, ri, cnt, end))
                at, ri = end, ri + cnt
            assert at == pos + int(lane_bits.sum()) == base + d["bits"], (at, pos, base, d["bits"])
            cat = lambda xs: np.concatenate(xs) if xs else empty
            out.append(SubGeo(c, typ, base, body0, pos, order, po, method, hb, lane_first, lane_bits, parts, cat(ce), cat(cw), cat(cq),
                              cat(ci), cat(es), cat(ew), cat(ev), body0 + order * bps))
        base += d["bits"]
    assert flen == HB + (base - 8 * HB + 7) // 8 + 2
    nw4 = (flen - 2) >> 2
    CHW = 17 * NT
    S = (nw4 + CHW - 1) // CHW
    return Geo(begin, flen, HB, nw4, (flen - 2) & 3, S, S * CHW - nw4, ((begin & 3) + flen + 3) // 4, begin & 3, NT, SPL, MAXO, out)


def frame_bits(data):
    return np.unpackbits(np.frombuffer(data, dtype=np.uint8)).astype(np.int64)


def field_values(bits, start, width):
    """the `width[i]`-bit fields at bit start[i], MSB first"""
    val = np.zeros(len(start), dtype=np.int64)
    for j in range(int(width.max()) if len(width) else 0):
        m = width > j
        val[m] = (val[m] << 1) | bits[start[m] + j]
    return val


def self_check(rec):
    """The model on one frame's bytes.  Raises AssertionError."""
    g, data = rec.geo, rec.data
    bits = frame_bits(data)
    csum = np.concatenate(([0], np.cumsum(bits)))
    for s, d in zip(g.subs, rec.subs):
        tcode = {0: 0, 1: 1, 2: 8 + d["order"], 3: 31 + d["order"]}[s.type]
        assert field_values(bits, np.array([s.base]), np.array([7]))[0] == tcode, (s.ch, "subframe header")
        mask = (1 << d["bps"]) - 1
        if s.type == 1:
            v = np.array(d["v"], dtype=np.int64) & mask
            starts = s.body0 + d["bps"] * np.arange(len(v), dtype=np.int64)
            assert np.array_equal(field_values(bits, starts, np.full(len(v), d["bps"])), v), (s.ch, "verbatim samples")
            assert np.array_equal(starts[:: g.SPL], s.lane_first), (s.ch, "a lane's first bit")
            continue
        if s.type == 0:
            assert field_values(bits, np.array([s.body0]), np.array([d["bps"]]))[0] == d["v"][0] & mask
            continue
        w = np.array(d["v"][: s.order], dtype=np.int64) & mask
        assert np.array_equal(field_values(bits, s.body0 + d["bps"] * np.arange(s.order, dtype=np.int64), np.full(s.order, d["bps"])), w)
        assert field_values(bits, np.array([s.pos - 6]), np.array([6]))[0] == (s.method << 4) | s.porder, (s.ch, "method and order")
        for p in s.parts:
            code = ((31 if s.method else 15) << 5 | p.param) if p.escaped else p.param
            width = s.hb + 5 if p.escaped else s.hb
            assert field_values(bits, np.array([p.hdr_end - width]), np.array([width]))[0] == code, (s.ch, p, "partition header")
        if len(s.code_end):
            k = s.code_w - 1
            u = zigzag(np.array(d["res"], dtype=np.int64))[s.code_i]
            assert np.array_equal(field_values(bits, s.code_end - s.code_w, s.code_w), (1 << k) | (u & ((1 << k) - 1))), (s.ch, "a Rice field")
            stop = s.code_end - s.code_w
            assert not np.any(csum[stop] - csum[stop - s.code_q]), (s.ch, "a set bit where a quotient's zeros lie")
        if len(s.esc_start):
            m = s.esc_w > 0
            assert np.array_equal(field_values(bits, s.esc_start[m], s.esc_w[m]), s.esc_val[m]), (s.ch, "an escaped residual")
    # ---- the CRC-16 from the slice rows of crc16_words_share<NT, S>, then the <= 3 bytes behind the whole words
    body = data[:-2]
    crc = 0
    if g.S:
        CHW = 17 * g.NT
        words = bytes(4 * g.padw) + body[: 4 * g.nw4]
        assert len(words) == 4 * g.S * CHW
        for t in range(g.NT):
            acc = 0
            for c in range(g.S):                                       # Horner in x^(544 NT) over the lane's chains
                sl = (c * g.NT + t) * 68
                acc = gf_mul(acc, x_pow(544 * g.NT)) ^ fs.crc16(words[sl:sl + 68])
            crc ^= gf_mul(acc, x_pow(544 * (g.NT - 1 - t)))
    for b in body[4 * g.nw4:]:
        crc = ((crc << 8) & 0xFFFF) ^ fs._T16[(crc >> 8) ^ b]          # crc16_tail: the byte-wise table
    assert len(body) - 4 * g.nw4 == g.rem
    assert crc == int.from_bytes(data[-2:], "big"), ("the slice rows do not fold to the frame's CRC-16", g.NT, g.S, g.padw)


def field_class(end, w):
    """where put_end's field of w bits ending at bit `end` lies: wholly in word W - 1, straddling, wholly in word W"""
    r = end & 31
    return "prev" if r == 0 else "straddle" if r < w else "in"


def locate(rec, byte):
    """The geometry's description of frame byte `byte`: subframe, lane, code, class."""
    g, bit = rec.geo, 8 * byte
    if byte >= g.flen - 2:
        return "the CRC-16 (nw4 %d, rem %d, S %d, padw %d)" % (g.nw4, g.rem, g.S, g.padw)
    if bit < 8 * g.hbytes:
        return "the frame header"
    s = [x for x in g.subs if x.base <= bit + 7][-1]
    text = "subframe %d (%s, base bit %d)" % (s.ch, KIND_OF[s.type], s.base)
    if s.lane_first is None or bit + 7 < s.lane_first[0]:
        return text + ", its header, warm-up or parameters"
    lane = int(np.searchsorted(s.lane_first, bit + 7, side="right")) - 1
    text += ", lane %d (first bit %d)" % (lane, s.lane_first[lane])
    if len(s.code_end):
        i = int(np.searchsorted(s.code_end, bit, side="right"))
        if i < len(s.code_end) and s.code_end[i] - s.code_w[i] - s.code_q[i] <= bit + 7:
            text += ", residual %d: Rice field of %d bits ending at bit %d (%s), quotient %d" % (
                s.code_i[i], s.code_w[i], s.code_end[i], field_class(int(s.code_end[i]), int(s.code_w[i])), s.code_q[i])
    for p in s.parts:
        if p.hdr_end - s.hb - (5 if p.escaped else 0) <= bit + 7 and bit < p.end:
            text += ", partition %d (%s %d)" % (p.index, "escaped" if p.escaped else "Rice", p.param)
    return text


def describe(b, f, byte):
    bt, i = batch_frames(b)[f]
    rec = bt.recs[i]
    g = rec.geo
    return ("%s frame %d (batch frame %d): begin %d (& 3 = %d), %d bytes, nw4 %d, rem %d, S %d, padw %d, nout %d, k_frame64<%d,%d,%d>; "
            "byte %d is %s" % (bt.case.name, i, f, g.begin, g.r, g.flen, g.nw4, g.rem, g.S, g.padw, g.nout, g.NT, g.SPL, g.MAXO, byte,
                               locate(rec, byte) if byte >= 0 else "past the shorter of the two"))


# ---------------------------------------------------------------------------------------------------------------------
# signals and specs
# ---------------------------------------------------------------------------------------------------------------------
def rails(bits):
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def walk(rng, n, bits, step=3, start=0):
    """a bounded random walk of `bits`-bit samples"""
    lo, hi = rails(bits)
    x, out = start, []
    for _ in range(n):
        x = min(hi, max(lo, x + rng.randint(-step, step)))
        out.append(x)
    return out


def noise(rng, n, bits):
    lo, hi = rails(bits)
    return [rng.randint(lo, hi) for _ in range(n)]


def unzig(u):
    return u >> 1 if not u & 1 else -((u + 1) >> 1)


def rice_cost(us, k):
    return int((us >> k).sum()) + (k + 1) * len(us)


def auto_params(res, n, order, po, method, escape_every=0, widen=0):
    """A caller's choice per partition: the cheapest Rice parameter, or the escape where that is cheaper (always for every
    `escape_every`-th partition, `widen` bits wider than needed)."""
    kmax = 30 if method else 14
    plen, at, out = n >> po, 0, []
    for p in range(1 << po):
        cnt = plen - order if p == 0 else plen
        chunk = np.array(res[at:at + cnt], dtype=np.int64)
        at += cnt
        us = zigzag(chunk)
        need = max([0] + [int(r).bit_length() + 1 if r >= 0 else int(-r - 1).bit_length() + 1 for r in (chunk.min(initial=0), chunk.max(initial=0))])
        if not len(chunk) or not chunk.any():
            need = 0
        k = min(range(kmax + 1), key=lambda kk: rice_cost(us, kk))
        if (escape_every and p % escape_every == escape_every - 1) or 5 + need * cnt < rice_cost(us, k):
            out.append(("escape", min(31, need + widen)))
        else:
            out.append(k)
    return out


def residuals_of(v, sub):
    coefs = list(sub["coefs"]) if sub["kind"] == "lpc" else fs.FIXED_COEFS[sub["order"]]
    return fs.residuals([s >> sub["wasted"] for s in v], sub["order"], coefs, sub["shift"])


def with_auto(v, sub, **kw):
    """the spec with its partition parameters chosen from the residuals"""
    sub = dict(sub)
    sub["params"] = tuple(auto_params(residuals_of(v, sub), len(v), sub["order"], sub["porder"], sub["method"], **kw))
    return sub


def unit_coefs(rng, order, shift=10, spread=3):
    """coefficients summing to 2^shift: a constant level predicts itself; the taps behind the first are small"""
    c = [rng.randint(-spread, spread) for _ in range(order)]
    c[0] += (1 << shift) - sum(c)
    return c


def quiet(C, n):
    return [[0] * n for _ in range(C)]


def frame(pcm, subs, assignment=None):
    return fs.Frame(pcm, subs, assignment=assignment)


def filler(sh, rng, kind="fixed"):
    """A non-silent frame of the shape: FIXED 1 on a random walk in every channel (independent assignment)."""
    n = sh.block
    pcm = [walk(rng, n, sh.bps, 2, rng.randint(-5, 5)) for _ in range(sh.C)]
    return frame(pcm, [with_auto(ch, fs.fixed(1, porder=3)) for ch in pcm])


def sized(sh, flen, seed=0, pad=3):
    """A frame of exactly `flen` bytes: channel 0 FIXED 0 with ONE k = 0 partition, where a residual of value v costs
    zigzag(v) + 1 bits, the other channels CONSTANT 0."""
    n, C = sh.block, sh.C
    others = (C - 1) * (8 + sh.bps)
    body = 8 * (flen - 2 - HB) - pad
    total_u = body - others - (8 + 6 + 4) - n
    if total_u < 0:                                                    # too short for a coded channel: all CONSTANT (flen must fit)
        assert flen == HB + (C * (8 + sh.bps) + 7) // 8 + 2, (flen, "no frame of this shape has this length")
        return frame([[seed % 3 - 1] * n for _ in range(C)], [fs.constant() for _ in range(C)])
    umax = (1 << sh.bps) - 1
    x = [0] * n
    at, step = (17 * seed + 5) % n, 61 if n % 61 else 67
    while total_u:
        assert x[at] == 0, "more bits than the block's samples can cost"
        u = min(umax, total_u)
        x[at] = unzig(u)
        total_u -= u
        at = (at + step) % n
    return frame([x] + quiet(C - 1, n), [fs.fixed(0, params=(0,))] + [fs.constant() for _ in range(C - 1)])


def smallest_len(sh):
    return HB + (sh.C * (8 + sh.bps) + 7) // 8 + 2


def shortest_coded_len(sh):
    """the shortest frame sized() makes with a coded channel: every residual 0, one bit each"""
    return HB + ((sh.C - 1) * (8 + sh.bps) + 8 + 6 + 4 + sh.block + 7) // 8 + 2


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def spread(sh, rng, subs_pcm):
    """a frame of the shape's C channels from a list of (samples, spec): the list is repeated / cut to C channels"""
    items = [subs_pcm[c % len(subs_pcm)] for c in range(sh.C)]
    return frame([x for x, _ in items], [s for _, s in items])


def frames_of(sh, items):
    """(samples, spec) items, C to a frame in their order (the last frame filled up with the first items)"""
    return [spread(sh, None, (items + items)[i:i + sh.C]) for i in range(0, len(items), sh.C)]


def a_phase_items(sh, rng):
    """(a): FIXED 0, eight partitions, every code of an odd length (or of 16 + 1): 32 codes in a row end at all 32 phases"""
    n, bps = sh.block, sh.bps
    assert bps >= 16
    def part(k, cnt):
        if k == 0:
            return [unzig(2 * rng.randint(0, 1)) for _ in range(cnt)]                       # 1 or 3 bits
        if k in (1, 7, 15):
            return [unzig((1 << k) + rng.randrange(1 << k)) for _ in range(cnt)]            # quotient 1: 3, 9, 17 bits
        return [unzig(rng.randrange(1 << min(k, bps - 1))) for _ in range(cnt)]             # quotient 0: 15, 25, 31, 4 bits
    out = []
    # (k = 24 and 30 cost 25 and 31 bits a sample: quiet partitions beside them keep the frame inside its image)
    for method, ks in ((0, (0, 1, 7, 14, 14, 7, 1, 0)), (1, (15, 24, 30, 3, 0, 0, 0, 0)), (0, (14, 0, 7, 1, 1, 14, 0, 7)), (1, (0, 30, 0, 3, 15, 0, 24, 0))):
        x = [v for k in ks for v in part(k, n // 8)]
        out.append((x, fs.fixed(0, method=method, porder=3, params=ks)))
    return out


def a_quotient_items(sh, rng):
    """(a): k = 0 quotients 0 .. 65 and >= 1000, long ones at the lane, partition and warm-up edges"""
    n, SPL = sh.block, sh.block // 64
    x = [0] * n
    for i, u in enumerate((1, 31, 32, 33, 63, 64, 65, 1000, 1999, 2, 64, 64)):
        x[7 * SPL + 1 + i] = unzig(u)
    x[4 * SPL - 1] = unzig(200)            # the last sample of lane 3
    x[4 * SPL] = unzig(300)                # ... and the first of lane 4
    x[9 * SPL] = unzig(1200)               # the first sample of lane 9
    x[n // 4] = unzig(700)                 # the first sample of partition 1
    x[n - 1] = unzig(1500)                 # the last code of the subframe
    y = [0] + [600] * (n - 1)              # FIXED 1: the first residual behind the warm-up is 600 (quotient 1200)
    z = [5, 5] + [5 + 40] + [5 + 80] * (n - 3)     # FIXED 2: residuals 40, 0 - 40 + ... behind two warm-up samples
    return [(x, fs.fixed(0, porder=2, params=(0, 0, 0, 0))), (y, fs.fixed(1, params=(0,))), (z, fs.fixed(2, porder=1, params=(0, 1)))]


def b_partition_items(sh, rng):
    """(b): partition orders 0 .. 6, FIXED 2 and LPC of the largest order the instantiation takes, auto parameters"""
    n = sh.block
    NT, SPL, MAXO = launcher(sh)
    out = []
    for po in range(7):
        x = walk(rng, n, sh.bps, 4)
        out.append((x, with_auto(x, fs.fixed(2, porder=po, method=po & 1))))
    orders = [16] + ([17, 31, 32] if MAXO == 32 else [])
    for order in orders:
        for head in ("rice", "escape"):
            x = walk(rng, n, sh.bps, 2, 100)
            sub = with_auto(x, fs.lpc(order, 12, 10, unit_coefs(rng, order), porder=6))
            if head == "escape":                                     # (an empty first partition's escape is a header and nothing else)
                res = residuals_of(x, sub)[: SPL - order] if order < SPL else []
                need = max([0] + [abs(r).bit_length() + 1 for r in res])
                sub["params"] = (("escape", need),) + sub["params"][1:]
            elif isinstance(sub["params"][0], tuple):
                sub["params"] = (3,) + sub["params"][1:]
            out.append((x, sub))
    return out


def b_alternating_items(sh, rng):
    """(b): Rice and escaped partitions alternating at orders 6 and 5, both phases, both coding methods; every other
    escape one bit wider than its residuals need"""
    n = sh.block
    out = []
    for po, method in ((6, 0), (5, 1)):
        for phase in (0, 1):
            x = walk(rng, n, sh.bps, 6)
            sub = fs.fixed(1, porder=po, method=method)
            res = residuals_of(x, sub)
            auto = auto_params(res, n, 1, po, method)
            esc = auto_params(res, n, 1, po, method, escape_every=1)
            wide = auto_params(res, n, 1, po, method, escape_every=1, widen=1)
            forced = [a if not isinstance(a, tuple) else 2 for a in auto]
            sub["params"] = tuple((wide if p & 2 else esc)[p] if (p + phase) & 1 else forced[p] for p in range(1 << po))
            out.append((x, sub))
    return out


def solve_target(coefs, target, bits):
    """history h (most recent first) and sample x, all of `bits` bits, with x - sum(coefs[j] * h[j]) == target (shift 0)"""
    lo, hi = rails(bits)
    rem, h = -target, []
    for c in coefs:
        t = max(lo, min(hi, (2 * rem + abs(c)) // (2 * abs(c)) * (1 if c > 0 else -1)))      # rem / c to the nearest: x stays small
        h.append(t)
        rem -= c * t
    x = target + sum(c * t for c, t in zip(coefs, h))
    assert lo <= x <= hi, (coefs, target, bits)
    return h, x


def b_escape_width_items(sh, rng):
    """(b): escape widths 0, 1, 2, 17, bps + 1 and 31, each holding its lowest and highest value; width 0 beside Rice"""
    n, bps = sh.block, sh.bps
    plen = n // 8
    out = []
    # FIXED 0: the residual is the sample
    x = [0] * n
    widths = [0, None, 1, 2, None, 0, bps, None]
    for p, wd in enumerate(widths):
        for i in range(plen):
            at = p * plen + i
            if wd is None:
                x[at] = rng.randint(-2, 2)
            elif wd:
                x[at] = rng.randint(*rails(wd))
        if wd:
            x[p * plen + 3], x[p * plen + plen - 2] = rails(wd)
    out.append((x, fs.fixed(0, porder=3, params=tuple(1 if wd is None else ("escape", wd) for wd in widths))))
    # LPC with shift 0: x[i] - sum(c h) hits the ends of 17, bps + 1 and 31 bits
    for method, coefs, prec, targets in ((0, [64], 8, [17, bps + 1]), (1, [-16384, -16384], 15, [31, 31])):
        order = len(coefs)
        x = [0] * n
        params = []
        for p in range(8):
            wd = targets[(p // 2) % len(targets)] if p & 1 else None
            if wd is None:
                params.append(0 if p & 2 else ("escape", 0))
                continue
            params.append(("escape", wd))
            for j, t in enumerate(rails(wd)):
                at = p * plen + 10 + 20 * j
                h, xv = solve_target(coefs, t, bps)
                for q, hv in enumerate(h):
                    x[at - 1 - q] = hv
                x[at] = xv
        out.append((x, fs.lpc(order, prec, 0, coefs, method=method, porder=3, params=tuple(params))))
    return out


def c_fixed_items(sh, rng):
    """(c): FIXED 0 .. 4 with the warm-up at both rails; FIXED 4 on alternating rails in one partition, escaped"""
    n, bps = sh.block, sh.bps
    lo, hi = rails(bps)
    out = []
    for order in range(5):
        for first in (lo, hi):
            other = hi if first == lo else lo
            x = [(first, other)[i & 1] for i in range(order)] + [other if order & 1 else first] * (n - order)
            if order == 0:
                x = walk(rng, n, bps, 3)
            out.append((x, with_auto(x, fs.fixed(order, porder=4, method=order & 1))))
    plen = n // 16
    x = [0] * n
    for i in range(plen):
        x[5 * plen + i] = (lo, hi)[i & 1]
    out.append((x, with_auto(x, fs.fixed(4, porder=4, method=1))))
    return out


def c_lpc_items(sh, rng):
    """(c): LPC orders 1, 2, 3, 15, 16; every precision with both ends of its coefficient range; shifts 0 and 15"""
    n, bps = sh.block, sh.bps
    out = []
    for order in (1, 2, 3, 15, 16):
        x = walk(rng, n, bps, 3, -50)
        out.append((x, with_auto(x, fs.lpc(order, 13, 10, unit_coefs(rng, order), porder=5, method=order & 1))))
    for prec in range(1, 16):
        lo, hi = rails(prec)
        shift = (0, 15, 7)[prec % 3]
        x, level = [], 0
        for i in range(n):                                          # long level runs: both taps see the same value
            if i % (n // 4) == n // 8:
                level = rng.randint(-90, 90)
            x.append(level)
        out.append((x, with_auto(x, fs.lpc(2, prec, shift, [hi, lo], porder=6, method=prec & 1))))
    return out


def c_unit_items(sh, rng, sbits):
    """(c): unit predictors on levels near the rails of a `sbits`-bit subframe: eight taps of one sign before the others
    undo them, so the prediction's partial sums need 40 bits and more while the residual stays small"""
    n = sh.block
    NT, SPL, MAXO = launcher(sh)
    out = []
    for order, level in ((16, 1), (MAXO, 0)):
        lo, hi = rails(sbits)
        half = order // 2
        coefs = [16383] * half + [-16383] * (order - half - 1)
        coefs.append((1 << 14) - sum(coefs))
        assert -16384 <= coefs[-1] <= 16383 and sum(coefs) == 1 << 14
        x = [hi - rng.randint(0, 3) if level else lo + rng.randint(0, 3) for _ in range(n)]
        run, top = 0, 0
        for a, c in zip(x[order - 1::-1], coefs):
            run += a * c
            top = max(top, abs(run))
        assert top >= 1 << 39, "no partial sum of the prediction needs 40 bits"
        out.append((x, with_auto(x, fs.lpc(order, 15, 14, coefs, porder=2, method=1))))
    return out


def c_wasted_items(sh, rng):
    """(c): wasted bits 1, 2 and width - 1 on the four kinds"""
    n, bps = sh.block, sh.bps
    out = []
    for w in (1, 2, bps - 1):
        eb = bps - w
        lo, hi = rails(eb)
        up = lambda v: [s << w for s in v]
        odd = lambda v: [s | 1 if eb > 1 else s for s in v]            # (so that no more bits are wasted than stated)
        out.append((up([hi | 1 if eb > 1 else -1] * n), fs.constant(wasted=w)))
        v = odd(noise(rng, n, eb))
        out.append((up(v), fs.verbatim(wasted=w)))
        v = odd(walk(rng, n, eb, 2))
        out.append((up(v), with_auto(up(v), fs.fixed(min(2, eb), wasted=w, porder=3))))
        coefs, prec, shift = ([1], 2, 0) if eb == 1 else (unit_coefs(rng, 4, 6, 2), 9, 6)
        out.append((up(v), with_auto(up(v), fs.lpc(len(coefs), prec, shift, coefs, wasted=w, porder=3, method=1))))
    return out


def c_kind_rotation(sh, rng):
    """(c): each of the four kinds on each wave position"""
    n, bps = sh.block, sh.bps
    def item(kind):
        if kind == 0:
            return ([rng.randint(*rails(bps))] * n, fs.constant())
        if kind == 1:
            return (noise(rng, n, bps), fs.verbatim())
        x = walk(rng, n, bps, 3 if bps > 8 else 1)                     # (narrow samples: a quiet walk, or the frame outgrows its image)
        if kind == 2:
            return (x, with_auto(x, fs.fixed(3 if bps > 8 else 1, porder=2)))
        return (x, with_auto(x, fs.lpc(5, 11, 9, unit_coefs(rng, 5, 9, 3 if bps > 8 else 0), porder=4, method=1)))
    frames = []
    for rot in range(4):
        items = [item((c + rot) % 4) for c in range(sh.C)]
        frames.append(frame([x for x, _ in items], [s for _, s in items]))
    return frames


def c_stereo_frames(sh, rng):
    """(c): sources L, R, MID, SIDE under assignments 8, 9, 10 -- each kind on the side and on the mid channel, the side
    channel at both ends of its bps + 1 bits, MID with wasted bits"""
    n, bps = sh.block, sh.bps
    lo, hi = rails(bps)
    frames = []
    def coded(v, kind, **kw):
        if kind == 2:
            return with_auto(v, fs.fixed(2, porder=3, **kw))
        return with_auto(v, fs.lpc(4, 10, 8, unit_coefs(rng, 4, 8), porder=4, method=1, **kw))
    for a in (8, 9, 10):
        for kind in range(4):                                          # the kind of the SIDE subframe; the other one rotates
            L = walk(rng, n, bps - 1, 3)
            if kind == 0:
                R = [l - hi // 4 for l in L]
            elif kind == 1:                                            # (the kept channel stays quiet: the frame must fit the image)
                N = noise(rng, n, max(2, bps - 4))
                if a == 8:
                    R = [l - 2 * v for l, v in zip(L, N)]
                elif a == 9:
                    L, R = [l + 2 * v for l, v in zip(L, N)], L
                else:
                    L, R = [l + v for l, v in zip(L, N)], [l - v for l, v in zip(L, N)]
                L[5], R[5], L[n - 7], R[n - 7] = hi, lo, lo, hi          # side = 2^bps - 1 and -(2^bps - 1)
            else:
                R = [l - s for l, s in zip(L, walk(rng, n, bps - 2, 2))]
                if kind == 2:
                    L[0], R[0], L[1], R[1] = hi, lo, lo, hi              # the side's warm-up at both ends
            fr = fs.Frame([L, R], [None, None], assignment=a)
            chans, _ = sub_channels(fr)
            side_at = fs.SIDE_OF[a]
            other_kind = (kind + 1 + a) % 4
            other = chans[1 - side_at]
            if (other_kind == 0 and len(set(other)) > 1) or (other_kind == 1 and kind == 1):
                other_kind = 2
            mk = lambda v, kd: fs.constant() if kd == 0 else fs.verbatim() if kd == 1 else coded(v, kd)
            subs = [None, None]
            subs[side_at] = mk(chans[side_at], kind)
            subs[1 - side_at] = mk(other, other_kind)
            fr.subs = subs
            frames.append(fr)
    # each kind on the MID channel (the side CONSTANT but for the last): L = m + t, R = m - t
    for kind in range(4):
        if kind == 0:
            t = walk(rng, n, bps - 2, 2)
            L, R = [hi // 4 + v for v in t], [hi // 4 - v for v in t]
        elif kind == 1:
            m = noise(rng, n, bps - 1)
            L, R = [v + 1 for v in m], [v - 1 for v in m]
        else:
            m = walk(rng, n, bps - 2, 3)
            L, R = [v + 3 for v in m], [v - 3 for v in m]
        fr = fs.Frame([L, R], [None, None], assignment=10)
        mid, side = sub_channels(fr)[0]
        fr.subs = [fs.constant() if kind == 0 else fs.verbatim() if kind == 1 else coded(mid, kind),
                   fs.constant() if len(set(side)) == 1 else coded(side, 2)]
        frames.append(fr)
    # MID with wasted bits: L = R = 4 w, so mid = 4 w and the kernel shifts L + R by wasted + 1
    for w, kind in ((2, 2), (1, 3), (3, 1), (2, 0)):
        v = [s | 1 for s in walk(rng, n, bps - w - 1, 2)] if kind else [5] * n
        L = [s << w for s in v]
        fr = fs.Frame([L, list(L)], [None, None], assignment=10)
        mid = sub_channels(fr)[0][0]
        fr.subs = [fs.constant(wasted=w) if kind == 0 else fs.verbatim(wasted=w) if kind == 1 else coded(mid, kind, wasted=w), fs.constant()]
        frames.append(fr)
    # independent L / R on the stereo context
    x, y = walk(rng, n, bps, 3), noise(rng, n, bps)
    frames.append(frame([x, y], [with_auto(x, fs.fixed(1, porder=6)), fs.verbatim()]))
    return frames


def d_row_sizes(sh):
    """(d): the nw4 this shape's image admits of CHW - 1 .. 2 CHW + 1, and the largest it admits"""
    CHW = 17 * 64 * sh.C
    top = max_nw4(sh)
    return [(name, w) for name, w in (("chw-1", CHW - 1), ("chw", CHW), ("chw+1", CHW + 1), ("2chw-1", 2 * CHW - 1), ("2chw", 2 * CHW),
                                      ("2chw+1", 2 * CHW + 1)) if w <= top] + [("max", top)]


def d_row_frames(sh):
    frames = []
    for i, (name, w) in enumerate(d_row_sizes(sh)):
        if name == "max":                                              # one bit more and flacgpu_pack_plans refuses the plan
            body = max_body_bits(sh)
            flen = HB + (body + 7) // 8 + 2
            frames.append(sized(sh, flen, seed=i, pad=8 * ((body + 7) // 8) - body))
        else:
            frames.append(sized(sh, 4 * w + (i & 3) + 2, seed=i, pad=i % 8))
    return frames


def d_rem_frames(sh):
    """(d): (flen - 2) & 3 in 0 .. 3 for S = 1, 2, 3"""
    CHW = 17 * 64 * sh.C
    return [sized(sh, 4 * ((S - 1) * CHW + 200 + 9 * rem) + rem + 2, seed=S + rem, pad=rem) for S in (1, 2, 3) for rem in range(4)]


def e_alignment_frames(sh, rng, begin):
    """(e): one focus frame at all 16 (begin & 3, (begin + flen) & 3), a non-silent frame on either side"""
    frames = []
    base = shortest_coded_len(sh) + 40
    at = begin
    for b in range(4):
        for e in range(4):
            gap = base + ((b - (at + base)) & 3)                       # the spacer ends where the focus must begin
            frames.append(sized(sh, gap, seed=len(frames)))
            at += gap
            flen = base + 24 + ((e - (at + base + 24)) & 3)
            frames.append(sized(sh, flen, seed=len(frames) + 1))
            at += flen
    frames.append(filler(sh, rng))
    return frames


def e_turn_frames(sh, begin):
    """(e): frames under 16 bytes (C = 1, 8 bits: the smallest is 10) and of 16 .. 31; nout a multiple of 4 NT and that
    plus one; the last frame of the batch"""
    NT = 64 * sh.C
    frames, at = [], begin
    for seed in (0, 1):                                                # all CONSTANT: 10 .. 25 bytes
        frames.append(sized(sh, smallest_len(sh), seed=seed))
        at += smallest_len(sh)
    for extra in (0, 1):                                               # nout = ((begin & 3) + flen + 3) >> 2
        flen = 4 * (4 * NT + extra) - 3 - (at & 3) + 1                 # ... the least flen with that nout
        if 8 * (flen - 2 - HB) <= max_body_bits(sh):
            frames.append(sized(sh, flen, seed=extra))
            assert ((at & 3) + flen + 3) // 4 == 4 * NT + extra
            at += flen
    frames.append(sized(sh, shortest_coded_len(sh) + 21, seed=3))
    return frames


def gen_items(sh, seed, maker):
    return lambda begin: frames_of(sh, maker(sh, random.Random(seed)))


_cases = None


def case_list():
    global _cases
    if _cases is not None:
        return _cases
    out = []
    tag = lambda sh: ("_deep" if sh.max_lpc > 16 else "") + ("" if sh.exhaustive else "_fast") + ("" if sh.mid_side else "_lr") + ("" if sh.rate == 48000 else "_r%d" % sh.rate)
    add = lambda name, fam, sh, gen: out.append(Case("%s_n%d_c%d_b%d%s" % (name, sh.block, sh.C, sh.bps, tag(sh)), fam, sh, gen))
    seed = 0
    for n in BLOCKS:
        for C in (1, 2, 3, 4):
            for deep in ((0, 1) if n == 4096 else (0,)):
                seed += 1
                sh = shape(n, C, 16, max_lpc=32 if deep else 16)
                if C <= 2:                                             # (a) and (b): every block length, one and two waves
                    add("rice_phases", "a", sh, gen_items(sh, seed, a_phase_items))
                    add("rice_quotients", "a", sh, gen_items(sh, seed, a_quotient_items))
                    add("partitions", "b", sh, gen_items(sh, seed, b_partition_items))
                    add("alternating", "b", sh, gen_items(sh, seed, b_alternating_items))
                    add("escape_widths", "b", sh, gen_items(sh, seed, b_escape_width_items))
                else:
                    add("partitions", "b", sh, gen_items(sh, seed, b_partition_items))
                add("kinds", "c", sh, (lambda sh, seed: lambda begin: c_kind_rotation(sh, random.Random(seed)))(sh, seed))
                add("turns", "e", sh, (lambda sh: lambda begin: e_turn_frames(sh, begin))(sh))
    # (c) predictors and sources
    for sh in (shape(4096, 1, 16), shape(1152, 2, 16, exhaustive=0), shape(2048, 3, 16), shape(1024, 4, 16), shape(2304, 1, 16)):
        add("fixed_rails", "c", sh, gen_items(sh, 101, c_fixed_items))
        add("lpc_params", "c", sh, gen_items(sh, 102, c_lpc_items))
        add("wasted", "c", sh, gen_items(sh, 103, c_wasted_items))
    for sh in (shape(2048, 1, 24), shape(4096, 2, 24)):                # 17 and bps + 1 = 25 are two widths here
        add("escape_widths", "b", sh, gen_items(sh, 109, b_escape_width_items))
    for sh in (shape(4096, 1, 25), shape(4096, 1, 25, max_lpc=32), shape(2304, 3, 25), shape(1024, 4, 25)):
        add("unit_rails", "c", sh, (lambda sh: lambda begin: frames_of(sh, c_unit_items(sh, random.Random(104), sh.bps)))(sh))
        add("fixed_rails", "c", sh, gen_items(sh, 105, c_fixed_items))
    for sh in (shape(4096, 2, 24), shape(4096, 2, 24, exhaustive=0), shape(1152, 2, 16), shape(2048, 2, 8, mid_side=0), shape(4096, 2, 16, max_lpc=32)):
        add("stereo_sources", "c", sh, (lambda sh: lambda begin: c_stereo_frames(sh, random.Random(106)))(sh))
    for sh in (shape(1024, 2, 4), shape(1152, 3, 8), shape(2048, 4, 12), shape(2304, 1, 20), shape(1024, 3, 17), shape(2048, 1, 24),
               shape(1024, 1, 8)):
        add("kinds", "c", sh, (lambda sh: lambda begin: c_kind_rotation(sh, random.Random(107)))(sh))
        add("turns", "e", sh, (lambda sh: lambda begin: e_turn_frames(sh, begin))(sh))
    # (d) CRC rows: the widest narrow samples, so that the image is as large as the shape's gets
    for n in BLOCKS:
        for C in (1, 2, 3, 4):
            sh = shape(n, C, 24 if C == 2 else 25, rate=44100)
            add("crc_rows", "d", sh, (lambda sh: lambda begin: d_row_frames(sh))(sh))
            if n == 4096:
                add("crc_rem", "d", sh, (lambda sh: lambda begin: d_rem_frames(sh))(sh))
    sh = shape(4096, 2, 24, exhaustive=0, rate=44100)                  # the other stereo image
    add("crc_rows", "d", sh, (lambda sh: lambda begin: d_row_frames(sh))(sh))
    # (e) copy-out
    for sh in (shape(1024, 1, 8, rate=44100), shape(4096, 2, 16, rate=44100), shape(2304, 4, 16, rate=44100)):
        add("alignment", "e", sh, (lambda sh: lambda begin: e_alignment_frames(sh, random.Random(108), begin))(sh))
    assert len({c.name for c in out}) == len(out)
    _cases = out
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what the matrix reaches
# ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 8, 15, 16, 25, 31)
QUOTIENTS = (0, 1, 31, 32, 33, 63, 64, 65)
LONG = 64                                  # a "long" quotient: at least two whole words of zeros


def required():
    req = ["a_w%d_end%d" % (w, p) for w in WIDTHS for p in range(32)]
    req += ["a_w%d_%s" % (w, c) for w in WIDTHS for c in ("prev", "straddle", "in") if not (w == 1 and c == "straddle")]
    req += ["a_q%d_k0" % q for q in QUOTIENTS] + ["a_q1000_k0", "a_words_untouched_between_fields"]
    req += ["a_long_last_of_lane", "a_long_first_of_lane", "a_long_first_of_partition", "a_long_first_behind_warmup"]
    req += ["a_khdr%d_%s" % (hb, c) for hb in (4, 5) for c in ("prev", "straddle", "in")]
    req += ["b_po%d_n%d" % (po, n) for po in range(7) for n in BLOCKS]
    req += ["b_order0_n%d" % n for n in BLOCKS] + ["b_order16_maxo16_n%d" % n for n in BLOCKS]
    req += ["b_empty_first_rice", "b_empty_first_escaped", "b_two_in_first_1152"] + ["b_deep_order%d_po6" % o for o in (17, 31, 32)]
    req += ["b_alt_po%d_%s_first" % (po, k) for po in (6, 5) for k in ("rice", "escape")]
    req += ["b_rice_then_escape_in_one_word", "b_escape_then_rice_in_one_word"]
    req += ["b_esc_w%s_%s" % (w, e) for w in ("1", "2", "17", "31", "bps1") for e in ("lo", "hi")] + ["b_esc_w0", "b_esc_w0_beside_rice"]
    req += ["b_esc_code_m0", "b_esc_code_m1", "b_esc_wider_than_needed", "b_esc_bps1_is_not_17_lo", "b_esc_bps1_is_not_17_hi"]
    req += ["c_fixed0"] + ["c_fixed%d_warm_%s" % (o, e) for o in range(1, 5) for e in ("lo", "hi")] + ["c_fixed4_alternating_rails_escaped"]
    req += ["c_lpc_order%d" % o for o in (1, 2, 3, 15, 16, 17, 31, 32)]
    req += ["c_prec%d_%s" % (p, e) for p in range(1, 16) for e in ("lo", "hi")] + ["c_shift0", "c_shift15", "c_unit_sum40_w25", "c_unit_sum40_deep"]
    req += ["c_wasted%s_%s" % (w, k) for w in ("1", "2", "max") for k in TYPES]
    req += ["c_src_%s" % s for s in ("L", "R", "MID", "SIDE")] + ["c_assign%d" % a for a in (8, 9, 10)] + ["c_side_lo", "c_side_hi", "c_mid_wasted"]
    req += ["c_%s_on_%s" % (k, s) for k in TYPES for s in ("side", "mid")]
    req += ["c_ch%d_%s_wave%d" % (C, k, w) for C in (3, 4) for k in TYPES for w in range(C)]
    req += ["c_bps%d" % b for b in (8, 12, 16, 20, 24, 4, 17, 25)]
    for n in BLOCKS:
        for C in (1, 2, 3, 4):
            req += ["d_nt%d_n%d_%s" % (64 * C, n, name) for name, _ in d_row_sizes(shape(n, C, 24 if C == 2 else 25))]
    req += ["d_nt128_fast_stereo_image_max"]
    req += ["d_nt%d_S%d_rem%d" % (64 * C, S, rem) for C in (1, 2, 3, 4) for S in (1, 2, 3) for rem in range(4)]
    req += ["d_smallest_c%d" % C for C in (1, 2, 3, 4)]
    req += ["e_begin%d_end%d" % (b, e) for b in range(4) for e in range(4)] + ["e_under_16_bytes", "e_16_to_31_bytes", "e_last_of_batch"]
    req += ["e_second_turn_nt%d" % nt for nt in (64, 128, 192, 256)]
    req += ["e_nout_4nt_nt%d" % nt for nt in (64, 128, 192, 256)] + ["e_nout_4nt_plus1_nt%d" % nt for nt in (64, 128, 192, 256)]
    req += ["i_%d_%d_%d" % (64 * C, spl, maxo) for C in (1, 2, 3, 4) for spl, maxo in ((16, 16), (18, 16), (32, 16), (36, 16), (64, 16), (64, 32))]
    return req


REQUIRED = required()


def reached(batch_list):
    """Counter: class name -> how often the matrix reaches it (codes, partitions, subframes or frames)."""
    n = collections.Counter()
    for b in batch_list:
        sh = b.shape
        fl = batch_frames(b)
        for f, (bt, i) in enumerate(fl):
            fr, rec = bt.frames[i], bt.recs[i]
            g = rec.geo
            n["i_%d_%d_%d" % (g.NT, g.SPL, g.MAXO)] += 1
            n["c_bps%d" % sh.bps] += 1
            types = [s.type for s in g.subs]
            # ---- (d) CRC rows, (e) copy-out
            CHW = 17 * g.NT
            for name, w in d_row_sizes(sh):
                if g.nw4 == w and (name != "max" or sum(d["bits"] for d in rec.subs) == max_body_bits(sh)):
                    n["d_nt%d_n%d_%s" % (g.NT, sh.block, name)] += 1
                    if name == "max" and sh.C == 2 and not sh.exhaustive:
                        n["d_nt128_fast_stereo_image_max"] += 1
            if g.S:
                n["d_nt%d_S%d_rem%d" % (g.NT, g.S, g.rem)] += 1
            if all(t == 0 for t in types):
                n["d_smallest_c%d" % sh.C] += 1
            loud = lambda k: 0 <= k < len(fl) and any(s.type for s in fl[k][0].recs[fl[k][1]].geo.subs)
            if loud(f - 1) and loud(f + 1) and loud(f):
                n["e_begin%d_end%d" % (g.begin & 3, (g.begin + g.flen) & 3)] += 1
            n["e_under_16_bytes" if g.flen < 16 else "e_16_to_31_bytes" if g.flen < 32 else "e_32_bytes_up"] += 1
            if g.nout > 4 * g.NT:
                n["e_second_turn_nt%d" % g.NT] += 1
            if g.nout % (4 * g.NT) == 0:
                n["e_nout_4nt_nt%d" % g.NT] += 1
            if g.nout % (4 * g.NT) == 1 and g.nout > 1:
                n["e_nout_4nt_plus1_nt%d" % g.NT] += 1
            if f + 1 == len(fl):
                n["e_last_of_batch"] += 1
            if fr.assignment >= 8:
                n["c_assign%d" % fr.assignment] += 1
            for s, d in zip(g.subs, rec.subs):
                kind = KIND_OF[s.type]
                sbps = d["bps"] + d["wasted"]
                lo, hi = rails(d["bps"])
                # ---- (c) sources, kinds, wasted bits
                if sh.C == 2:
                    n["c_src_%s" % {0: "L", 1: "R", SRC_MID: "MID", SRC_SIDE: "SIDE"}[d["source"]]] += 1
                    if d["source"] == SRC_SIDE:
                        n["c_%s_on_side" % kind] += 1
                        full = [v << d["wasted"] for v in d["v"]]
                        n["c_side_lo"] += min(full) == -(1 << sh.bps) + 1
                        n["c_side_hi"] += max(full) == (1 << sh.bps) - 1
                    if d["source"] == SRC_MID:
                        n["c_%s_on_mid" % kind] += 1
                        n["c_mid_wasted"] += d["wasted"] > 0
                if sh.C >= 3:
                    n["c_ch%d_%s_wave%d" % (sh.C, kind, s.ch)] += 1
                if d["wasted"]:
                    n["c_wasted%s_%s" % ("max" if d["bps"] == 1 else d["wasted"], kind)] += 1
                if s.type < 2:
                    continue
                # ---- (b) partitions and warm-up, (c) predictors
                n["b_po%d_n%d" % (s.porder, sh.block)] += 1
                if s.order == 0:
                    n["b_order0_n%d" % sh.block] += 1
                    n["c_fixed0"] += 1
                if s.order == 16 and g.MAXO == 16:
                    n["b_order16_maxo16_n%d" % sh.block] += 1
                first = s.parts[0]
                if len(s.parts) == 64 and first.count == 0:
                    n["b_empty_first_escaped" if first.escaped else "b_empty_first_rice"] += 1
                if len(s.parts) == 64 and first.count == 2 and sh.block == 1152:
                    n["b_two_in_first_1152"] += 1
                if g.MAXO == 32 and s.porder == 6 and s.order in (17, 31, 32):
                    n["b_deep_order%d_po6" % s.order] += 1
                warm = d["v"][: s.order]
                if s.type == 2 and s.order:
                    n["c_fixed%d_warm_lo" % s.order] += lo in warm
                    n["c_fixed%d_warm_hi" % s.order] += hi in warm
                if s.type == 3:
                    n["c_lpc_order%d" % s.order] += 1
                    plo, phi = rails(d["precision"])
                    n["c_prec%d_lo" % d["precision"]] += min(d["coefs"]) == plo
                    n["c_prec%d_hi" % d["precision"]] += max(d["coefs"]) == phi
                    n["c_shift%d" % d["shift"]] += 1
                    top, best = 0, 0
                    for at in range(s.order, min(len(d["v"]), s.order + 64)):
                        run = 0
                        for a, c in zip(d["v"][at - 1::-1], d["coefs"]):
                            run += a * c
                            top = max(top, abs(run))
                    if top >= 1 << 39 and max(abs(r) for r in d["res"]) < 1 << 12:
                        n["c_unit_sum40_deep" if s.order > 16 else "c_unit_sum40_w25" if sbps == 25 else "c_unit_sum40_narrower"] += 1
                kinds = [p.escaped for p in s.parts]
                if len(kinds) >= 32 and all(a != b_ for a, b_ in zip(kinds, kinds[1:])):
                    n["b_alt_po%d_%s_first" % (s.porder, "escape" if kinds[0] else "rice")] += 1
                res = d["res"]
                for j, p in enumerate(s.parts):
                    n["a_khdr%d_%s" % (s.hb, field_class(p.hdr_end - (5 if p.escaped else 0), s.hb))] += 1
                    if j and p.escaped != s.parts[j - 1].escaped and s.parts[j - 1].end & 31:
                        n["b_escape_then_rice_in_one_word" if s.parts[j - 1].escaped else "b_rice_then_escape_in_one_word"] += 1
                    if not p.escaped:
                        continue
                    n["b_esc_code_m%d" % s.method] += 1
                    chunk = res[p.first_res:p.first_res + p.count]
                    if p.param == 0:
                        n["b_esc_w0"] += 1
                        if (j and not s.parts[j - 1].escaped) or (j + 1 < len(s.parts) and not s.parts[j + 1].escaped):
                            n["b_esc_w0_beside_rice"] += 1
                        continue
                    elo, ehi = rails(p.param)
                    names = [str(p.param)] if p.param in (1, 2, 17, 31) else []
                    names += ["bps1"] if p.param == sh.bps + 1 else []
                    for nm in names:
                        n["b_esc_w%s_lo" % nm] += elo in chunk
                        n["b_esc_w%s_hi" % nm] += ehi in chunk
                    if p.param == sh.bps + 1 != 17:
                        n["b_esc_bps1_is_not_17_lo"] += elo in chunk
                        n["b_esc_bps1_is_not_17_hi"] += ehi in chunk
                    if chunk and elo // 2 <= min(chunk) and max(chunk) <= ehi // 2:
                        n["b_esc_wider_than_needed"] += 1
                    if s.type == 2 and s.order == 4 and p.param >= sbps + 4 and any(abs(r) >= 1 << (sbps + 2) for r in chunk):
                        n["c_fixed4_alternating_rails_escaped"] += 1
                # ---- (a) Rice fields
                if not len(s.code_end):
                    continue
                for w in WIDTHS:
                    m = s.code_w == w
                    if not m.any():
                        continue
                    ph = np.bincount(s.code_end[m] & 31, minlength=32)
                    for p_ in range(32):
                        n["a_w%d_end%d" % (w, p_)] += int(ph[p_])
                    r = s.code_end[m] & 31
                    n["a_w%d_prev" % w] += int((r == 0).sum())
                    n["a_w%d_straddle" % w] += int(((r > 0) & (r < w)).sum())
                    n["a_w%d_in" % w] += int((r >= w).sum())
                k0 = s.code_w == 1
                for q in QUOTIENTS:
                    n["a_q%d_k0" % q] += int((s.code_q[k0] == q).sum())
                n["a_q1000_k0"] += int((s.code_q[k0] >= 1000).sum())
                start = s.code_end - s.code_w - s.code_q                   # where the code's zeros begin: the field before ends here
                n["a_words_untouched_between_fields"] += int((((s.code_end - s.code_w) >> 5) - ((start + 31) >> 5) >= 1).sum())
                sample = s.code_i + s.order                                # the residual's sample index in the block
                long_ = s.code_q >= LONG
                e, lane = sample % g.SPL, sample // g.SPL
                n["a_long_last_of_lane"] += int((long_ & (e == g.SPL - 1) & (lane < 63)).sum())
                n["a_long_first_of_lane"] += int((long_ & (e == 0) & (lane > 0)).sum())
                plen = sh.block >> s.porder
                n["a_long_first_of_partition"] += int((long_ & (sample % plen == 0) & (sample > 0)).sum())
                n["a_long_first_behind_warmup"] += int((long_ & (s.code_i == 0)).sum()) if s.order else 0
    return n
