"""The matrix of hand-built FLAC streams behind test_flacsyn_oracle.py (CPU) and test_gpu_decode_foreign.py (GPU):
legal syntax that this project's encoder never writes, each case at the smallest shape where its path can go wrong.
Built from _flacsyn alone.  What is chosen here (signals, Rice parameters that keep the codes short) is the matrix's
choice; the writer only writes it down and checks it.

valid_cases() -> [Stream], invalid_cases() -> [(reason, Stream)]; both cached and never modified by a test."""
import functools
import random

import _flacsyn as fs

LO = {b: -(1 << (b - 1)) for b in range(1, 34)}
HI = {b: (1 << (b - 1)) - 1 for b in range(1, 34)}


def synth(rng, n, eb, order=0, coefs=(), shift=0, amp=40, warm=None):
    """n samples of eb bits that the predictor follows up to a residual of about +-amp (clamped to the width)."""
    lo, hi = LO[eb], HI[eb]
    v = [min(hi, max(lo, rng.randint(-4 * amp, 4 * amp))) for _ in range(order)] if warm is None else list(warm)
    rc = list(coefs)[::-1]
    for i in range(order, n):
        s = 0
        for a, b in zip(v[i - order:i], rc):
            s += a * b
        v.append(min(hi, max(lo, (s >> shift) + rng.randint(-amp, amp))))
    return v[:n]


def part_residuals(v, sub):
    """The residuals of each partition."""
    order, po = sub["order"], sub["porder"]
    coefs = sub["coefs"] if sub["kind"] == "lpc" else fs.FIXED_COEFS[order]
    res = fs.residuals([s >> sub["wasted"] for s in v], order, list(coefs), sub["shift"])
    plen = len(v) >> po
    out, at = [], 0
    for part in range(1 << po):
        cnt = plen - order if part == 0 else plen
        out.append(res[at:at + cnt])
        at += cnt
    return out


def fit_k(v, sub):
    """One Rice parameter per partition, near log2 of the partition's mean |residual| (the matrix's choice)."""
    out = []
    for chunk in part_residuals(v, sub):
        mean = sum(abs(r) for r in chunk) // max(len(chunk), 1)
        out.append(min(mean.bit_length(), 30 if sub["method"] else 14))
    sub["params"] = tuple(out)
    return sub


def small_coefs(rng, order, precision=12, shift=10):
    """Coefficients whose absolute sum stays near 2^shift: the prediction keeps the signal's scale."""
    top = max(1, (1 << shift) // order)
    top = min(top, fs_hi(precision))
    return [rng.randint(-top, top) for _ in range(order)]


def fs_hi(precision):
    return (1 << (precision - 1)) - 1


class Builder:
    def __init__(self):
        self.streams = []

    def mono(self, name, bps, items, rate=44100, blocking=1, **kw):
        """One stream of one-channel frames; items: [(samples, sub)]; sample numbers (or frame numbers) run on."""
        frames, at = [], 0
        for k, (v, sub) in enumerate(items):
            frames.append(fs.Frame([v], [sub], blocking=blocking, number=at if blocking else k))
            at += len(v)
        return self.add(name, rate, bps, frames, **kw)

    def add(self, name, rate, bps, frames, **kw):
        st = fs.write_stream(rate, bps, frames, name=name, **kw)
        self.streams.append(st)
        return st


def _lpc_sub(rng, order, precision=12, shift=10, **kw):
    return fs.lpc(order, precision, shift, small_coefs(rng, order, precision, shift), **kw)


def _unit_lpc(rng, order, **kw):
    """An LPC predictor whose coefficients sum to 2^shift: a constant level predicts itself."""
    c = small_coefs(rng, order, 13, 10)
    c[0] += (1 << 10) - sum(c)
    return fs.lpc(order, 13, 10, c, **kw)


def _predicted(rng, n, bps, sub, amp=40):
    eb = bps - sub["wasted"]
    coefs = sub["coefs"] if sub["kind"] == "lpc" else fs.FIXED_COEFS[sub["order"]]
    v = synth(rng, n, eb, sub["order"], coefs, sub["shift"], amp)
    return [s << sub["wasted"] for s in v]


def _kinds(b, rng):
    items = []
    for n in (1, 16, 192, 4096):
        items.append(([-1234] * n, fs.constant()))
        items.append(([rng.randint(-32768, 32767) for _ in range(n)], fs.verbatim()))
    b.mono("constant+verbatim", 16, items)
    for order in range(5):
        items = []
        for n in sorted({max(order, 1), order + 1, 16, 192} | ({4096} if order == 4 else set())):
            sub = fs.fixed(order)
            v = _predicted(rng, n, 16, sub)
            items.append((v, fit_k(v, sub)))
        b.mono(f"fixed{order}", 16, items)
    for order in range(1, 33):
        sizes = {order, order + 1, 192}
        if order <= 16:
            sizes.add(16)
        if order in (7, 8, 31, 32):   # store_ring writes 16 bytes at a time: a multiple of 4 next to one that is not
            sizes.add(4096)
        items = []
        for n in sorted(sizes):
            sub = _lpc_sub(rng, order)
            v = _predicted(rng, n, 16, sub)
            items.append((v, fit_k(v, sub)))
        b.mono(f"lpc{order}", 16, items)


def _lpc_params(b, rng):
    items = []
    for p in range(1, 16):   # both ends of the coefficient range; shift p - 1 makes them -1 and almost +1
        sub = fs.lpc(2, p, max(p - 1, 0), [fs_hi(p), LO[p]])
        v = _predicted(rng, 16, 16, sub)
        items.append((v, fit_k(v, sub)))
    b.mono("lpc-precisions", 16, items)
    items = []
    for s in range(16):
        c = min(1 << s, fs_hi(15))
        sub = fs.lpc(2, 15, s, [c, -(c // 2)])
        v = _predicted(rng, 16, 16, sub)
        items.append((v, fit_k(v, sub)))
    b.mono("lpc-shifts", 16, items)
    # 32-bit input near full scale, order 32, precision 15: the partial sums of the prediction need 50 bits
    sub = fs.lpc(32, 15, 15, [fs_hi(15)] * 17 + [-fs_hi(15)] * 15, method=1)
    # (the coefficients sum to 2^15, so a level near full scale predicts itself and the residuals stay small)
    items = []
    for n, level in ((192, HI[32]), (4096, LO[32])):
        v = [level - (2 * (level > 0) - 1) * rng.randint(0, 2000) for _ in range(n)]
        items.append((v, fit_k(v, dict(sub))))
    st = b.mono("lpc-50-bit-sum", 32, items)
    assert ("lpc_sum_bits", "49+") in st.features


def _residual_coding(b, rng):
    items = []
    for k in range(15):
        v = [rng.randint(-(1 << k), 1 << k) for _ in range(16)]
        items.append((v, fs.fixed(0, method=0, params=(k,))))
    b.mono("rice-k", 16, items)
    items = []
    for k in range(31):
        v = [rng.randint(-(1 << k), 1 << k) for _ in range(16)]
        items.append((v, fs.fixed(0, method=1, params=(k,))))
    b.mono("rice2-k", 32, items)
    items = []
    for bits in (0, 1, 2, 17, 31):
        for method in (0, 1):
            lim = (1 << (bits - 1)) if bits else 0
            v = [rng.randint(-lim, max(lim - 1, 0)) for _ in range(16)]
            if bits:
                v[3], v[9] = -lim, lim - 1
            items.append((v, fs.fixed(0, method=method, params=(("escape", bits),))))
    b.mono("escape-widths", 32, items)
    for n, top in ((16, 4), (4096, 12)):
        items = []
        for po in range(top + 1):
            sub = fs.fixed(1 if (n >> po) >= 1 else 0, porder=po, method=po & 1)
            v = _predicted(rng, n, 16, sub, amp=300)
            items.append((v, fit_k(v, sub)))
        b.mono(f"partition-orders-{n}", 16, items)
    items = []
    for order in (0, 1):   # partition length 1; with order 1 the first partition is empty
        sub = fs.fixed(order, porder=15)
        v = _predicted(rng, 32768, 8, sub, amp=3)
        items.append((v, fit_k(v, sub)))
    b.mono("partition-order-15", 8, items)
    # partition 0 empty (plen == order), then Rice / escaped partitions; Rice and escape alternating
    items = []
    for order, kind in ((4, "fixed"), (8, "lpc"), (2, "fixed")):
        for first in ("rice", "escape"):
            for method in (0, 1):
                n, po = order * 8, 3
                sub = fs.fixed(order, porder=po, method=method) if kind == "fixed" else \
                    _lpc_sub(rng, order, porder=po, method=method)
                v = [rng.randint(-100, 100) for _ in range(n)]   # residuals of at most 16 x 100: 12 bits
                ks = list(fit_k(v, sub)["params"])
                for part in range(8):
                    if (part % 2 == 1) == (first == "escape"):
                        ks[part] = ("escape", 17)
                sub["params"] = tuple(ks)
                items.append((v, sub))
    st = b.mono("empty-partition-0+alternating", 16, items)
    # Rice codes of exactly 31, 32, 33, 64 and 65 bits, and quotients of hundreds and thousands of zeros at k = 0
    v = []
    for length in (31, 32, 33, 64, 65, 32, 33, 31, 65, 64):
        u = length - 1   # k = 0: quotient + stop bit
        v += [(u >> 1) if u % 2 == 0 else -((u + 1) >> 1), rng.randint(-2, 2)]
    v += [150, -150, 1, 1500, -1501, 0, 2047, -2048, 777, -333, 0, 0]
    assert len(v) == 32
    items = [(v, fs.fixed(0, params=(0,))), (v[::-1], fs.fixed(0, method=1, params=(0,)))]
    # ... and with a remainder: k = 2, quotients 28..30 and 61..62
    w = []
    for length in (31, 32, 33, 64, 65):
        u = ((length - 3) << 2) | rng.randint(0, 3)
        w += [(u >> 1) if u % 2 == 0 else -((u + 1) >> 1)] * 2 + [rng.randint(-8, 8)]
    items.append((w + [0], fs.fixed(0, params=(2,))))
    b.mono("long-rice-codes", 16, items)
    # k + quotient == 32 (a 33-bit code) at every bit phase of the reader's 64-bit register: runs of 33-bit codes
    # move the phase by one bit per code.  The r04 bug's shape (a code whose last bit falls outside a refill of an
    # empty register), made on purpose for every alignment of either decoder's buffer.
    items = []
    for k, method in ((28, 1), (30, 1), (14, 0), (2, 0)):
        q = 32 - k
        v = []
        for i in range(192):
            u = (q << k) | rng.getrandbits(k)
            v.append((u >> 1) if u % 2 == 0 else -((u + 1) >> 1))
        items.append((v, fs.fixed(0, method=method, params=(k,))))
    b.mono("33-bit-codes-every-phase", 32, items)


def _wasted(b, rng):
    items = []
    for w in (1, 2, 15):
        items.append(([-3 << w if w < 15 else LO[16]] * 16, fs.constant(wasted=w)))
        eb = 16 - w
        items.append(([rng.randint(LO[eb], HI[eb]) << w for _ in range(16)], fs.verbatim(wasted=w)))
        for sub in (fs.fixed(2, wasted=w), _lpc_sub(rng, 5, wasted=w), fs.fixed(0, wasted=w)):
            v = _predicted(rng, 192, 16, sub)
            items.append((v, fit_k(v, sub)))
    b.mono("wasted-16", 16, items)
    items = []
    for w in (1, 8, 31):
        eb = 32 - w
        items.append(([rng.randint(LO[eb], HI[eb]) << w for _ in range(16)], fs.verbatim(wasted=w)))
        sub = fs.fixed(1, wasted=w, method=1)
        v = _predicted(rng, 16, 32, sub, amp=1 << min(eb - 1, 20))
        items.append((v, fit_k(v, sub)))
        items.append(([HI[eb] << w] * 16, fs.constant(wasted=w)))
    b.mono("wasted-32", 32, items)


def stereo_from_side(rng, side, bps):
    """left, right of `bps` bits with left - right == side."""
    left = []
    for s in side:
        a, z = (LO[bps] + s, HI[bps]) if s >= 0 else (LO[bps], HI[bps] + s)
        left.append(rng.randint(a, z))
    return left, [x - s for x, s in zip(left, side)]


def _stereo(b, rng):
    for bps in (8, 12, 16, 20, 24, 32):
        sb = bps + 1
        frames, at = [], 0
        for a in (8, 9, 10):
            side_at = fs.SIDE_OF[a]
            specs = []
            # anti-phase full scale: the side needs all bps + 1 bits; CONSTANT and VERBATIM
            specs.append(([HI[sb]] * 16, fs.constant()))
            specs.append(([LO[sb] + 1] * 16, fs.constant()))
            v = [rng.randint(LO[sb] + 1, HI[sb]) for _ in range(16)]
            v[0], v[5], v[6], v[7] = HI[sb], LO[sb] + 1, 1 - (1 << (bps - 1)), (1 << (bps - 1))
            specs.append((v, fs.verbatim()))
            # FIXED and LPC at both ends of the side's range, warm-up samples included: a level that predicts
            # itself (the LPC coefficients sum to 2^shift) minus a little noise, so that the residuals stay small
            for k, (sub, n) in enumerate(((fs.fixed(1, method=1), 16), (fs.fixed(4, method=1), 192),
                                          (fs.fixed(2, method=1), 2), (_unit_lpc(rng, 3, method=1), 16),
                                          (_unit_lpc(rng, 32, method=1), 192),
                                          (_unit_lpc(rng, 9, method=1, porder=2), 64))):
                level, sign = (HI[sb], 1) if (k + a) % 2 else (LO[sb] + 1, -1)
                v = [level - sign * rng.randint(0, 1 << max(bps - 8, 1)) for _ in range(n)]
                v[0] = level
                specs.append((v, sub))
            # wasted bits on the side channel
            v = [rng.randint(LO[sb - 1] + 1, HI[sb - 1]) << 1 for _ in range(16)]
            v[2] = HI[sb - 1] << 1
            specs.append((v, fs.verbatim(wasted=1)))
            sub = fs.fixed(2, wasted=3, method=1)
            v = _predicted(rng, 16, sb, sub, amp=1 << (bps - 5))
            specs.append((v, fit_k(v, sub)))
            for side, sub in specs:
                # left - right never reaches -2^bps, the lowest value of bps + 1 bits
                side = [x + (1 << sub["wasted"]) if x == LO[sb] else x for x in side]
                if sub["kind"] in ("fixed", "lpc"):
                    fit_k(side, sub)
                left, right = stereo_from_side(rng, side, bps)
                subs = [fs.verbatim(), fs.verbatim()]
                subs[side_at] = sub
                frames.append(fs.Frame([left, right], subs, assignment=a, blocking=1, number=at))
                at += len(side)
        b.add(f"stereo-{bps}", 48000, bps, frames)
    # mid/side with odd and even sums and negative sides, small values, every kind for the mid channel too
    frames = []
    for k, (subm, subs) in enumerate(((fs.fixed(1), fs.fixed(0)), (fs.verbatim(), fs.fixed(1)))):
        left = [rng.randint(-50, 50) for _ in range(16)]
        right = [rng.randint(-50, 50) for _ in range(16)]
        mid = [(x + y) >> 1 for x, y in zip(left, right)]
        side = [x - y for x, y in zip(left, right)]
        frames.append(fs.Frame([left, right], [fit_k(mid, subm) if subm["kind"] != "verbatim" else subm,
                                               fit_k(side, subs)], assignment=10, number=k))
    b.add("mid-side-parity", 44100, 16, frames)


def _channels_and_widths(b, rng):
    for nch in range(1, 9):
        frames = []
        for k, n in enumerate((16, 192)):
            pcm, subs = [], []
            for c in range(nch):
                sub = [fs.fixed(2), fs.verbatim(), _lpc_sub(rng, 6), fs.constant()][(c + k) % 4]
                v = [77 * c - 300] * n if sub["kind"] == "constant" else _predicted(rng, n, 16, sub)
                pcm.append(v)
                subs.append(sub if sub["kind"] in ("constant", "verbatim") else fit_k(v, sub))
            frames.append(fs.Frame(pcm, subs, number=k, bcode=6 if n == 16 else 1))
        b.add(f"channels-{nch}", 48000, 16, frames, min_block=192, max_block=192)
    for bps in (4, 10, 17, 31):   # widths only STREAMINFO can state: bps code 0
        frames = []
        for k in range(2):
            pcm, subs = [], []
            for c in range(2):
                sub = [fs.fixed(1, method=1), _lpc_sub(rng, 4, method=1), fs.verbatim()][(c + k) % 3]
                v = [rng.randint(LO[bps], HI[bps]) for _ in range(16)] if sub["kind"] == "verbatim" else \
                    _predicted(rng, 16, bps, sub, amp=max(1, 1 << (bps - 4)))
                v[0] = LO[bps] if k else HI[bps]
                pcm.append(v)
                subs.append(sub if sub["kind"] == "verbatim" else fit_k(v, sub))
            frames.append(fs.Frame(pcm, subs, number=k, bps_code=0))
        b.add(f"width-{bps}", 32000, bps, frames)
        # ... and decorrelated
        side = [rng.randint(LO[bps + 1] + 1, HI[bps + 1]) for _ in range(16)]
        left, right = stereo_from_side(rng, side, bps)
        b.add(f"width-{bps}-mid-side", 32000, bps,
              [fs.Frame([left, right], [fs.verbatim(), fs.verbatim()], assignment=10, bps_code=0)])


def _headers(b, rng):
    for n, code in sorted((n, c) for n, c in fs.BLOCK_CODES.items()):
        v = [rng.randint(-100, 100) for _ in range(16)]
        frames = [fs.Frame([[5] * n], [fs.constant()], bcode=code, number=0),
                  fs.Frame([v], [fs.verbatim()], number=1)]   # a short last frame
        b.add(f"bcode-{code}", 44100, 16, frames, min_block=n, max_block=n)
    for code, n in ((6, 1), (6, 256), (7, 257), (7, 65535), (7, 256), (6, 192), (7, 4096)):
        v = [rng.randint(-2000, 2000) for _ in range(n)]
        b.add(f"bcode-{code}-n{n}", 44100, 16, [fs.Frame([v], [fs.verbatim()], bcode=code)])
    for rate, code in sorted(fs.RATE_CODES.items()):
        b.add(f"rcode-{code}", rate, 16, [fs.Frame([[1, -2, 3]], [fs.verbatim()], rcode=code),
                                          fs.Frame([[9]], [fs.constant()], rcode=0, number=1)])
    for rate, code in ((48000, 12), (255000, 12), (44100, 13), (65535, 13), (1, 13), (44100, 14), (655350, 14)):
        b.add(f"rcode-{code}-{rate}", rate, 16, [fs.Frame([[1, -2, 3]], [fs.verbatim()], rcode=code),
                                                 fs.Frame([[4, 5, 6]], [fs.verbatim()], rcode=code, number=1)])
    # coded numbers of 1..7 bytes; the stream need not start at 0
    for nbytes, last in enumerate((0x7F, 0x7FF, 0xFFFF, 0x1FFFFF, 0x3FFFFFF, 0x7FFFFFFF, 0xFFFFFFFFF), start=1):
        blocking = 1 if nbytes == 7 else 0   # 36 bits: a sample number
        frames = [fs.Frame([[k, -k, 7]], [fs.verbatim()], blocking=blocking,
                           number=last - (6 - 3 * k if blocking else 2 - k)) for k in range(3)]
        st = b.add(f"number-{nbytes}-bytes", 8000, 16, frames)
        assert ("number_bytes", nbytes) in st.features
    # variable block size with matching sample numbers; fixed block size with a last frame of one sample
    items = []
    for n in (16, 4096, 1, 577, 192):
        sub = fs.fixed(2) if n > 2 else fs.verbatim()
        v = _predicted(rng, n, 16, sub) if n > 2 else [rng.randint(-9, 9) for _ in range(n)]
        items.append((v, fit_k(v, sub) if n > 2 else sub))
    b.mono("variable-block-size", 16, items, blocking=1)
    items = []
    for n in (192, 192, 1):
        sub = fs.fixed(1) if n > 1 else fs.verbatim()
        v = _predicted(rng, n, 16, sub) if n > 1 else [-7]
        items.append((v, fit_k(v, sub) if n > 1 else sub))
    b.mono("fixed-block-last-1", 16, items, blocking=0, min_block=192, max_block=192)


def _stream_level(b, rng):
    def frames():
        out = []
        for k in range(3):
            sub = fs.fixed(2)
            v = _predicted(rng, 192, 16, sub)
            out.append(fs.Frame([v, v[::-1]], [fit_k(v, sub), fs.verbatim()], number=k))
        return out

    seektable = b"".join(s.to_bytes(8, "big") + o.to_bytes(8, "big") + n.to_bytes(2, "big")
                         for s, o, n in ((0, 0, 192), (192, 700, 192), ((1 << 64) - 1, 0, 0)))
    vendor = b"hand-built"
    comment = len(vendor).to_bytes(4, "little") + vendor + (1).to_bytes(4, "little") + \
        (7).to_bytes(4, "little") + b"TITLE=x"
    variants = {"padding": [(1, bytes(100))], "application": [(2, b"test" + bytes(range(40)))],
                "seektable": [(3, seektable)], "vorbis-comment": [(4, comment)],
                "all-blocks": [(3, seektable), (2, b"abcd\xff\xf8\xc9\x08"), (4, comment), (1, bytes(7))],
                "empty-padding": [(1, b"")]}
    for name, md in variants.items():
        b.add(f"metadata-{name}", 44100, 16, frames(), metadata=md)
    b.add("min-frame-unknown", 44100, 16, frames(), min_frame=0, max_frame=0)
    b.add("total-samples-unknown", 44100, 16, frames(), total=0)
    b.add("md5-zero", 44100, 16, frames(), md5="zero")
    b.add("md5-wrong", 44100, 16, frames(), md5="wrong")
    b.add("all-unknown", 44100, 24, [fs.Frame([[1 << 20, -(1 << 22)]], [fs.verbatim()])], md5="zero", total=0,
          min_frame=0, max_frame=0)


@functools.lru_cache(maxsize=1)
def valid_cases():
    rng = random.Random(20240817)
    b = Builder()
    for part in (_kinds, _lpc_params, _residual_coding, _wasted, _stereo, _channels_and_widths, _headers,
                 _stream_level):
        part(b, rng)
    assert all(s.valid for s in b.streams)
    return tuple(b.streams)


INVALID = [
    ("negative LPC shift", dict(invalid="neg_shift"), "lpc"),
    ("precision code 15", dict(invalid="prec15"), "lpc"),
    ("reserved subframe type 2", dict(invalid=("type", 2)), "verbatim"),
    ("reserved subframe type 7", dict(invalid=("type", 7)), "verbatim"),
    ("reserved subframe type 13", dict(invalid=("type", 13)), "verbatim"),
    ("reserved subframe type 31", dict(invalid=("type", 31)), "verbatim"),
    ("wasted >= bps", dict(invalid="wasted_ge_bps"), "verbatim"),
    ("partition order does not divide n", dict(invalid="porder_nodiv", porder=3, params=(4,)), "fixed"),
    ("order larger than the partition length", dict(invalid="order_gt_plen", porder=3, params=(4,)), "lpc"),
    ("residual coding method 2", dict(invalid="method2", params=(4,)), "fixed"),
]


@functools.lru_cache(maxsize=1)
def invalid_cases():
    """One malformed frame between two valid frames of the same stream."""
    rng = random.Random(77)
    out = []
    for reason, kw, kind in INVALID:
        n = 100 if kw.get("invalid") == "porder_nodiv" else 16   # 100 is no multiple of 8; 16 >> 3 < order 8
        frames = []
        for k in range(3):
            if k != 1:
                sub = fs.fixed(2)
                v = _predicted(rng, 192, 16, sub)
                frames.append(fs.Frame([v], [fit_k(v, sub)], number=k))
                continue
            if kind == "lpc":
                sub = fs.lpc(8, 12, 10, small_coefs(rng, 8), **kw)
            elif kind == "fixed":
                sub = fs.fixed(2, **kw)
            else:
                sub = fs.verbatim(**kw)
            v = _predicted(rng, n, 16, sub, amp=12) if kind != "verbatim" else [rng.randint(-99, 99) for _ in range(n)]
            frames.append(fs.Frame([v], [sub], number=k))
        st = fs.write_stream(44100, 16, frames, name=reason)
        assert not st.valid
        out.append((reason, st))
    return tuple(out)
