"""A plain Python restatement of the frame analysis rule (TEST INFRASTRUCTURE ONLY).

parse_frame walks one FLAC frame bit by bit and returns what flacgpu_analyze_frame_host / flacgpu_decoder_analyze must
record for it: the frame fields, one record per subframe with the field names of flacgpu_subframe_plan, and the rows
as Python integers (so a 33-bit side channel is exact).  It uses no project code and no device.  The tests are the
decoder's: a frame is refused (None) when a pad bit is set, the type is reserved, wasted >= width, order > n,
precision code 15, a negative shift, method > 1, a partition length below the order or not dividing n, a read past
the frame's end, non-zero padding, or anything but 16 bits left behind the padding.
"""
from types import SimpleNamespace

SUB_CONSTANT, SUB_VERBATIM, SUB_FIXED, SUB_LPC = 0, 1, 2, 3
SRC_MID, SRC_SIDE = 8, 9
AN_WIDE, AN_PARTS_CLIPPED = 1, 2
MAX_PARTITIONS = 64
BLOCK_OF_CODE = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608}
BPS_OF_CODE = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


class Refused(Exception):
    pass


class Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "big")
        self.total = 8 * len(data)
        self.pos = 0

    def get(self, n):
        if self.pos + n > self.total:
            raise Refused("read past the end")
        self.pos += n
        return (self.v >> (self.total - self.pos)) & ((1 << n) - 1)

    def signed(self, n):
        u = self.get(n)
        return u - (1 << n) if n and u >> (n - 1) else u

    def zeros(self):
        q = 0
        while not self.get(1):
            q += 1
        return q


def _crc(data, poly, width):
    top, mask, c = 1 << (width - 1), (1 << width) - 1, 0
    for b in data:
        c ^= b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
    return c


def source_of(acode, c):
    if acode < 8:
        return c
    return {8: (0, SRC_SIDE), 9: (SRC_SIDE, 1), 10: (SRC_MID, SRC_SIDE)}[acode][c]


def parse_header(r, data):
    """The frame header at the reader's position 0; returns (n, acode, bps_code, header_bytes)."""
    if r.get(14) != 0x3FFE or r.get(1):
        raise Refused("sync")
    r.get(1)
    bcode, rcode, acode, bps_code = r.get(4), r.get(4), r.get(4), r.get(3)
    if r.get(1) or acode > 10 or bcode == 0 or rcode == 15 or bps_code == 3:
        raise Refused("reserved header value")
    ones = 0
    while ones < 8 and r.get(1):
        ones += 1
    if ones == 1 or ones > 7:
        raise Refused("coded number")
    r.get(7 - ones)
    for _ in range(max(ones - 1, 0)):
        if r.get(2) != 2:
            raise Refused("coded number")
        r.get(6)
    if bcode == 6:
        n = r.get(8) + 1
    elif bcode == 7:
        n = r.get(16) + 1
    else:
        n = BLOCK_OF_CODE.get(bcode) or 256 << (bcode - 8)
    if rcode == 12:
        r.get(8)
    elif rcode in (13, 14):
        r.get(16)
    hb = r.pos // 8
    if r.get(8) != _crc(data[:hb], 0x07, 8):
        raise Refused("CRC-8")
    return n, acode, bps_code, hb + 1


def _subframe(r, n, sbps, acode, c):
    at = r.pos
    if r.get(1):
        raise Refused("pad bit")
    t = r.get(6)
    wasted = r.zeros() + 1 if r.get(1) else 0
    if wasted >= sbps:
        raise Refused("wasted >= width")
    eb = sbps - wasted
    s = SimpleNamespace(type=0, wasted=wasted, bps=eb, order=0, precision=0, shift=0, coding_method=0, partition_order=0,
                        source=source_of(acode, c), flags=AN_WIDE if sbps > 32 else 0, n_partitions=0, part_len=0,
                        bits=0, coeffs=[0] * 32, rice=[0] * MAX_PARTITIONS, escape_bits=[0] * MAX_PARTITIONS,
                        all_params=[])
    if t == 0:
        s.type, row = SUB_CONSTANT, [r.signed(eb)]
    elif t == 1:
        s.type, row = SUB_VERBATIM, [r.signed(eb) for _ in range(n)]
    elif 8 <= t <= 12 or t >= 32:
        lpc = t >= 32
        s.type, s.order = (SUB_LPC, t - 31) if lpc else (SUB_FIXED, t - 8)
        if s.order > n:
            raise Refused("order > n")
        row = [r.signed(eb) for _ in range(s.order)]
        if lpc:
            s.precision = r.get(4) + 1
            shift = r.signed(5)
            if s.precision == 16 or shift < 0:
                raise Refused("precision / shift")
            s.shift = shift
            for j in range(s.order):
                s.coeffs[j] = r.signed(s.precision)
        s.coding_method = r.get(2)
        if s.coding_method > 1:
            raise Refused("method")
        hb, esc = (5, 31) if s.coding_method else (4, 15)
        po = r.get(4)
        plen = n >> po
        if plen < s.order or (plen << po) != n:
            raise Refused("partition order")
        s.partition_order, s.n_partitions, s.part_len = po, 1 << po, plen
        if (1 << po) > MAX_PARTITIONS:
            s.flags |= AN_PARTS_CLIPPED
        for part in range(1 << po):
            count = plen - (s.order if part == 0 else 0)
            k = r.get(hb)
            if k == esc:
                w = r.get(5)
                s.all_params.append(("escape", w))
                if part < MAX_PARTITIONS:
                    s.rice[part], s.escape_bits[part] = 0xFF, w
                row += [r.signed(w) for _ in range(count)]
            else:
                s.all_params.append(k)
                if part < MAX_PARTITIONS:
                    s.rice[part] = k
                for _ in range(count):
                    u = (r.zeros() << k) | (r.get(k) if k else 0)
                    row.append((u >> 1) ^ -(u & 1))
    else:
        raise Refused("reserved subframe type")
    s.bits = r.pos - at
    return s, row


def parse_frame(data, streaminfo_bps=0):
    """data: the frame, header .. CRC-16.  Returns None for a frame that does not parse, else a namespace: n, acode
    (as coded), assignment (0 for independent channels, as the encoder's plans hold it), channels, header_bytes,
    body_bits, crc_ok, subs (records) and rows (lists of Python ints: n per FIXED / LPC / VERBATIM row, 1 per CONSTANT)."""
    data = bytes(data)
    r = Bits(data)
    try:
        n, acode, bps_code, hb = parse_header(r, data)
        bps = BPS_OF_CODE.get(bps_code, streaminfo_bps)
        if not 4 <= bps <= 32:
            raise Refused("no sample size")
        channels = acode + 1 if acode < 8 else 2
        side = {8: 1, 9: 0, 10: 1}.get(acode)
        subs, rows = [], []
        for c in range(channels):
            s, row = _subframe(r, n, bps + (1 if c == side else 0), acode, c)
            subs.append(s)
            rows.append(row)
        body = r.pos - 8 * hb
        if r.pos & 7 and r.get(8 - (r.pos & 7)):
            raise Refused("padding")
        if r.pos + 16 != r.total:
            raise Refused("frame end")
    except Refused:
        return None
    return SimpleNamespace(n=n, acode=acode, assignment=acode if acode >= 8 else 0, channels=channels, header_bytes=hb,
                           body_bits=body, block_size=n & 0xFFFF, crc_ok=_crc(data, 0x8005, 16) == 0, subs=subs, rows=rows)


RECORD_FIELDS = ("type", "wasted", "bps", "order", "precision", "shift", "coding_method", "partition_order", "source",
                 "n_partitions", "part_len", "bits")


def assert_records_equal(got_frame, got_subs, model, where=""):
    """got_frame: an ANALYSIS_FRAME_DTYPE record, got_subs: its SUBFRAME_DTYPE records; every field against the model,
    the unused array entries (which must be 0) included."""
    assert int(got_frame["status"]) & 1 == 0, f"{where} status {got_frame['status']}"
    plan = got_frame["plan"]
    for name, want in (("block_size", model.n), ("header_bytes", model.header_bytes), ("assignment_code", model.acode)):
        assert int(got_frame[name]) == want, f"{where} {name}: {got_frame[name]} != {want}"
    for name, want in (("assignment", model.assignment), ("channels", model.channels), ("block_size", model.block_size),
                       ("body_bits", model.body_bits)):
        assert int(plan[name]) == want, f"{where} plan.{name}: {plan[name]} != {want}"
    assert len(got_subs) == model.channels, f"{where} subframe count"
    for c, (g, m) in enumerate(zip(got_subs, model.subs)):
        for name in RECORD_FIELDS:
            assert int(g[name]) == getattr(m, name), f"{where} ch{c} {name}: {g[name]} != {getattr(m, name)}"
        assert list(g["reserved"]) == [m.flags, 0, 0], f"{where} ch{c} flags {list(g['reserved'])} != {m.flags}"
        assert list(g["coeffs"]) == m.coeffs, f"{where} ch{c} coeffs"
        assert list(g["rice"]) == m.rice, f"{where} ch{c} rice {list(g['rice'])} != {m.rice}"
        assert list(g["escape_bits"]) == m.escape_bits, f"{where} ch{c} escape_bits"


def assert_rows_equal(row_of, model, where="", wide_low32=True):
    """row_of(c): the row of channel c, at least n elements.  int32 rows hold the low 32 bits of a wide value
    (wide_low32); int64 rows are exact.  A CONSTANT row is defined at [0] alone."""
    for c, want in enumerate(model.rows):
        got = [int(v) for v in row_of(c)[:len(want)]]
        if wide_low32 and model.subs[c].flags & AN_WIDE:
            want = [((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31) for v in want]
        assert got == want, f"{where} ch{c} row differs at {[i for i, (a, b) in enumerate(zip(got, want)) if a != b][:5]}"
