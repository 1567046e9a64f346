"""A FLAC stream writer driven by explicit syntax choices (TEST INFRASTRUCTURE ONLY).

The caller gives the PCM and every syntax decision: header codes, channel assignment, subframe kind, predictor,
wasted bits, Rice method, partition order and every partition's parameter.  The writer analyses nothing.  It forms
each residual as `sample - prediction` in Python integers, so the PCM is the decoder's correct answer by construction,
and it asserts what the format needs (partition lengths, 32-bit residuals, escape and sample widths).  `invalid=`
on a subframe writes a deliberately malformed one.  Uses no project code: int arithmetic, hashlib, numpy for arrays.

    sub = lpc(order, precision, shift, coefs, wasted=0, method=0, porder=0, params=[k | ("escape", bits), ...])
    fr = Frame(pcm=[[...], [...]], subs=[sub, sub], assignment=10, bcode=6, rcode=0, bps_code=0, blocking=0, number=0)
    st = write_stream(rate, bps, [fr, ...], md5="right", metadata=[(1, bytes(10))])
    st.blob, st.pcm (interleaved int32), st.features, st.md5_status, st.n_frames, st.valid
"""
import hashlib

import numpy as np

BLOCK_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
               16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10,
              96000: 11}
BPS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}
FIXED_COEFS = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]]
SIDE_OF = {8: 1, 9: 0, 10: 1}   # channel assignment -> the subframe that carries the side channel
SIDE_NAME = {8: "left", 9: "right", 10: "mid"}


def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    t = []
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


class Bits:
    """MSB-first bit writer."""

    def __init__(self):
        self.chunks, self.acc, self.n, self.total = [], 0, 0, 0

    def put(self, n, v):
        assert 0 <= v < (1 << n), (n, v)
        self.acc = (self.acc << n) | v
        self.n += n
        self.total += n
        if self.n >= 2048:
            self._flush()

    def signed(self, n, v):
        assert n == 0 and v == 0 or -(1 << (n - 1)) <= v < (1 << (n - 1)), f"{v} does not fit {n} bits"
        self.put(n, v & ((1 << n) - 1))

    def _flush(self):
        keep = self.n & 7
        whole = self.n - keep
        if whole:
            self.chunks.append((self.acc >> keep).to_bytes(whole // 8, "big"))
            self.acc &= (1 << keep) - 1
            self.n = keep

    def getvalue(self):
        if self.n & 7:
            self.put(8 - (self.n & 7), 0)
        self._flush()
        return b"".join(self.chunks)


def utf8_number(v):
    """The frame header's coded number: 1..7 bytes, up to 36 bits."""
    assert 0 <= v < (1 << 36)
    if v < 0x80:
        return bytes([v])
    for nbytes in range(2, 8):
        if v < (1 << (5 * nbytes + 1)):
            break
    out = [((0xFF << (8 - nbytes)) & 0xFF) | (v >> (6 * (nbytes - 1)))]
    for i in range(nbytes - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


def _sub(kind, order=0, **kw):
    d = dict(kind=kind, order=order, precision=0, shift=0, coefs=(), wasted=0, method=0, porder=0, params=(0,),
             invalid=None)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


def constant(**kw):
    return _sub("constant", **kw)


def verbatim(**kw):
    return _sub("verbatim", **kw)


def fixed(order, **kw):
    assert 0 <= order <= 4
    return _sub("fixed", order, **kw)


def lpc(order, precision, shift, coefs, **kw):
    assert 1 <= order <= 32 and len(coefs) == order
    return _sub("lpc", order, precision=precision, shift=shift, coefs=tuple(int(c) for c in coefs), **kw)


class Frame:
    def __init__(self, pcm, subs, assignment=None, bcode=None, rcode=0, bps_code=None, blocking=0, number=0):
        self.pcm = [[int(v) for v in ch] for ch in pcm]   # [channel][n], the true PCM
        self.n = len(self.pcm[0])
        assert all(len(ch) == self.n for ch in self.pcm) and 1 <= self.n <= 65536
        self.subs = subs
        self.assignment = len(self.pcm) - 1 if assignment is None else assignment
        self.bcode, self.rcode, self.bps_code = bcode, rcode, bps_code
        self.blocking, self.number = blocking, number


def residuals(v, order, coefs, shift):
    """sample - prediction for v[order:], FLAC's predictor: sum(coefs[j] * v[i-1-j]) >> shift."""
    out = []
    if order == 0:
        return list(v)
    rc = coefs[::-1]
    for i in range(order, len(v)):
        w = v[i - order:i]
        s = 0
        for a, b in zip(w, rc):
            s += a * b
        out.append(v[i] - (s >> shift))
    return out


def _write_residual_section(bw, res, n, order, sub, feats):
    method, po, params, invalid = sub["method"], sub["porder"], sub["params"], sub["invalid"]
    hb, esc = (5, 31) if method else (4, 15)
    bw.put(2, 2 if invalid == "method2" else method)
    bw.put(4, po)
    plen = n >> po
    if invalid in ("porder_nodiv", "order_gt_plen"):
        # no legal layout exists: one parameter, then every residual
        assert (plen << po) != n if invalid == "porder_nodiv" else plen < order
        k = params[0]
        bw.put(hb, k)
        for r in res:
            u = 2 * r if r >= 0 else -2 * r - 1
            bw.put((u >> k) + 1 + k, (1 << k) | (u & ((1 << k) - 1)))
        return
    assert (plen << po) == n, "the partition length must divide the block"
    assert plen >= order, "partition 0 must hold the warm-up samples"
    assert len(params) == 1 << po, (len(params), po)
    feats.add(("porder", n, po) if po else ("porder", 0))
    kinds = []
    at = 0
    for part, prm in enumerate(params):
        cnt = plen - order if part == 0 else plen
        chunk = res[at:at + cnt]
        at += cnt
        if isinstance(prm, tuple):
            assert prm[0] == "escape" and 0 <= prm[1] <= 31
            bits = prm[1]
            bw.put(hb, esc)
            bw.put(5, bits)
            for r in chunk:
                bw.signed(bits, r)   # asserts that the escaped value fits its width
            feats.add(("escape_bits", bits))
            kinds.append("escape")
        else:
            k = prm
            assert 0 <= k < esc
            bw.put(hb, k)
            mask = (1 << k) - 1
            run33 = 0
            for r in chunk:
                u = 2 * r if r >= 0 else -2 * r - 1
                q = u >> k
                length = q + 1 + k
                bw.put(length, (1 << k) | (u & mask))
                if length in (31, 32, 33, 64, 65):
                    feats.add(("rice_code_bits", length))
                if q >= 1000:
                    feats.add(("rice_quotient", "thousands"))
                elif q >= 100:
                    feats.add(("rice_quotient", "hundreds"))
                run33 = run33 + 1 if (length == 33 and k + q == 32) else 0
                if run33 == 64:   # k + quotient == 32 at every bit phase of a 64-bit register
                    feats.add(("rice33_every_phase", k))
            feats.add(("rice2_k" if method else "rice_k", k))
            kinds.append("rice")
        if part == 1 and plen == order:
            feats.add(("empty_partition0", kinds[1]))
    assert at == len(res)
    if len(kinds) >= 4 and all(a != b for a, b in zip(kinds, kinds[1:])):
        feats.add(("alternating_partitions", method))


def write_subframe(bw, samples, sbps, sub, feats):
    """One subframe of `samples` (Python ints of `sbps` bits)."""
    kind, order, wasted, invalid = sub["kind"], sub["order"], sub["wasted"], sub["invalid"]
    n = len(samples)
    bw.put(1, 0)
    if isinstance(invalid, tuple):   # ("type", code): a reserved subframe type
        bw.put(6, invalid[1])
    else:
        bw.put(6, {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[kind])
    if invalid == "wasted_ge_bps":
        bw.put(1, 1)
        bw.put(sbps, 1)   # unary: wasted = sbps
        for _ in samples:
            bw.put(1, 0)
        return
    assert 0 <= wasted < sbps
    if wasted:
        bw.put(1, 1)
        bw.put(wasted, 1)
        assert all(s & ((1 << wasted) - 1) == 0 for s in samples), "wasted bits must be zero"
        feats.add(("wasted", kind, "bps-1" if wasted == sbps - 1 else wasted))
    else:
        bw.put(1, 0)
    eb = sbps - wasted
    v = [s >> wasted for s in samples]
    lo, hi = -(1 << (eb - 1)), (1 << (eb - 1)) - 1
    assert all(lo <= s <= hi for s in v), f"a sample does not fit {eb} bits"
    if kind == "constant":
        assert all(s == v[0] for s in v)
        bw.signed(eb, v[0])
        feats.add(("kind", "constant"))
        return
    if kind == "verbatim" or isinstance(invalid, tuple):
        for s in v:
            bw.signed(eb, s)
        feats.add(("kind", "verbatim"))
        return
    assert order <= n
    for s in v[:order]:
        bw.signed(eb, s)
    if kind == "lpc":
        prec, shift, coefs = sub["precision"], sub["shift"], list(sub["coefs"])
        assert 1 <= prec <= 15 and 0 <= shift <= 15
        bw.put(4, 15 if invalid == "prec15" else prec - 1)
        bw.signed(5, -1 if invalid == "neg_shift" else shift)
        for c in coefs:
            bw.signed(prec, c)
        feats.add(("lpc_order", order))
        feats.add(("lpc_precision", prec))
        feats.add(("lpc_shift", shift))
        if min(coefs) == -(1 << (prec - 1)):
            feats.add(("lpc_coef", "lowest"))
        if max(coefs) == (1 << (prec - 1)) - 1:
            feats.add(("lpc_coef", "highest"))
    else:
        shift, coefs = 0, FIXED_COEFS[order]
        feats.add(("fixed_order", order))
    if n - order <= 1:
        feats.add(("residuals", kind, n - order))
    res = residuals(v, order, coefs, shift)
    assert all(-(1 << 31) <= r < (1 << 31) for r in res), "a residual does not fit 32 signed bits"
    if kind == "lpc" and order == 32 and n > 32:   # how wide the prediction's running sum gets (first residual)
        run, top = 0, 0
        for a, c in zip(v[31::-1], coefs):
            run += a * c
            top = max(top, abs(run))
        if top >= 1 << 48:
            feats.add(("lpc_sum_bits", "49+"))
    _write_residual_section(bw, res, n, order, sub, feats)


def write_frame(rate, bps, fr, feats):
    n, nch, a = fr.n, len(fr.pcm), fr.assignment
    assert 0 <= a <= 10 and (a + 1 == nch if a < 8 else nch == 2)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    assert all(lo <= s <= hi for ch in fr.pcm for s in ch), f"a sample does not fit {bps} bits"
    bcode = BLOCK_CODES.get(n, 6 if n <= 256 else 7) if fr.bcode is None else fr.bcode
    assert (bcode in (6, 7) and n <= (256 if bcode == 6 else 65536)) or BLOCK_CODES.get(n) == bcode
    rcode = fr.rcode
    assert rcode in (0, 12, 13, 14) or RATE_CODES.get(rate) == rcode
    bps_code = BPS_CODES.get(bps, 0) if fr.bps_code is None else fr.bps_code
    assert bps_code == 0 or BPS_CODES.get(bps) == bps_code
    bw = Bits()
    bw.put(14, 0x3FFE)
    bw.put(1, 0)
    bw.put(1, fr.blocking)
    bw.put(4, bcode)
    bw.put(4, rcode)
    bw.put(4, a)
    bw.put(3, bps_code)
    bw.put(1, 0)
    num = utf8_number(fr.number)
    for b in num:
        bw.put(8, b)
    if bcode == 6:
        bw.put(8, n - 1)
    elif bcode == 7:
        bw.put(16, n - 1)
    if rcode == 12:
        assert rate % 1000 == 0 and rate // 1000 < 256
        bw.put(8, rate // 1000)
    elif rcode == 13:
        bw.put(16, rate)
    elif rcode == 14:
        assert rate % 10 == 0
        bw.put(16, rate // 10)
    header = bw.getvalue()
    bw.put(8, crc8(header))
    feats.update({("blocking", fr.blocking), ("bcode", bcode), ("rcode", rcode), ("bps_code", bps_code),
                  ("number_bytes", len(num)), ("channels", nch), ("assignment", a)})
    if fr.bcode in (6, 7):   # an explicit choice of "block size in the header"
        feats.add(("bcode_n", bcode, n))
    chans = fr.pcm
    if a == 8:
        chans = [chans[0], [x - y for x, y in zip(*chans)]]
    elif a == 9:
        chans = [[x - y for x, y in zip(*chans)], chans[1]]
    elif a == 10:
        chans = [[(x + y) >> 1 for x, y in zip(*chans)], [x - y for x, y in zip(*chans)]]
        side = chans[1]
        if any(s < 0 for s in side):
            feats.add(("mid_side", "negative_side"))
        feats.update(("mid_side", "odd_sum" if s & 1 else "even_sum") for s in side)
    for c, (samples, sub) in enumerate(zip(chans, fr.subs)):
        is_side = a >= 8 and SIDE_OF[a] == c
        sbps = bps + (1 if is_side else 0)
        if is_side:
            feats.add(("side_bps", SIDE_NAME[a], sbps))
            if min(samples) == -(1 << bps) + 1 or max(samples) == (1 << bps) - 1:
                feats.add(("side_full_width", SIDE_NAME[a], sbps))
            if sbps == 33 and sub["invalid"] is None:
                feats.add(("side33", SIDE_NAME[a]))
                feats.add(("side33_kind", sub["kind"]))
            if sub["wasted"]:
                feats.add(("wasted_on_side", sbps))
        if sub["wasted"] and bps == 32:
            feats.add(("wasted_at_32",))
        write_subframe(bw, samples, sbps, sub, feats)
    body = bw.getvalue()
    return body + crc16(body).to_bytes(2, "big")


class Stream:
    pass


def le_bytes(pcm, bps):
    """Interleaved samples as ceil(bps / 8)-byte little-endian values: what the MD5 covers."""
    w = (bps + 7) // 8
    a = np.asarray(pcm, dtype=np.int64).astype("<i8")
    return a.view(np.uint8).reshape(-1, 8)[:, :w].tobytes()


def metadata_block(kind, payload, last=False):
    return bytes([(0x80 if last else 0) | kind]) + len(payload).to_bytes(3, "big") + payload


def write_stream(rate, bps, frames, md5="right", metadata=(), min_block=None, max_block=None, min_frame="exact",
                 max_frame="exact", total="exact", name=""):
    """frames: [Frame]; metadata: [(block type, payload)] written behind STREAMINFO; md5: right | zero | wrong;
    min_frame / max_frame / total: "exact" or 0 (unknown)."""
    assert 4 <= bps <= 32 and frames
    nch = len(frames[0].pcm)
    assert 1 <= nch <= 8 and all(len(f.pcm) == nch for f in frames)
    feats = set()
    coded = [write_frame(rate, bps, f, feats) for f in frames]
    valid = all(s["invalid"] is None for f in frames for s in f.subs)
    pcm = np.array([[ch[i] for ch in f.pcm] for f in frames for i in range(f.n)], dtype=np.int64).reshape(-1)
    digest = hashlib.md5(le_bytes(pcm, bps)).digest()
    stored = {"right": digest, "zero": bytes(16), "wrong": bytes([digest[0] ^ 1]) + digest[1:]}[md5]
    sizes = [f.n for f in frames]
    si = Bits()
    si.put(16, min(sizes) if min_block is None else min_block)
    si.put(16, min(max(sizes), 65535) if max_block is None else max_block)
    si.put(24, min(len(c) for c in coded) if min_frame == "exact" else 0)
    si.put(24, max(len(c) for c in coded) if max_frame == "exact" else 0)
    si.put(20, rate)
    si.put(3, nch - 1)
    si.put(5, bps - 1)
    si.put(36, sum(sizes) if total == "exact" else 0)
    blocks = [(0, si.getvalue() + stored)] + list(metadata)
    st = Stream()
    st.blob = b"fLaC" + b"".join(metadata_block(k, p, i + 1 == len(blocks)) for i, (k, p) in enumerate(blocks))
    st.blob += b"".join(coded)
    feats.update({("stream_bps", bps), ("md5", md5), ("min_frame", min_frame), ("total_samples", total)})
    feats.update(("metadata", k) for k, _ in metadata)
    st.frame_bytes, st.frame_sizes = coded, sizes
    st.pcm = pcm.astype(np.int32)
    st.bps, st.channels, st.rate, st.name = bps, nch, rate, name
    st.n_frames = len(frames)
    st.md5_status = {"right": 1, "zero": 2, "wrong": 0}[md5]
    st.digest = digest
    st.valid = valid
    st.features = feats if valid else set()
    st.coded_samples = sum(sizes) * nch
    return st
