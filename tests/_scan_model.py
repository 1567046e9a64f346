"""The frame scan of DESIGN.md 4b ("The scan finds the host scan's frames, for any bytes") as a Python model, and the
damaged streams the decoders' scans are held to it on (TEST INFRASTRUCTURE ONLY).

The model states the rule, it does not walk the bytes as the C loop does: it lists every position where a valid frame
header starts, and a frame's end is the first listed position far enough on, with the frame's blocking bit, whose two
preceding bytes are the CRC-16 of the frame so far.  The header grammar is _flacsyn.write_frame's, read backwards."""
import functools
import random

import _flacsyn as fs
import _foreign_matrix as fm
import _oracle as orc

INVALID_ARG = -1   # FLACGPU_ERR_INVALID_ARG
BLOCK_SIZE_OF = {code: n for n, code in fs.BLOCK_CODES.items()}
STREAMINFO_FIELDS = ["sample_rate", "channels", "bits_per_sample", "min_block", "max_block", "total_samples", "md5"]


def parse_header(d):
    """(block size, header bytes, blocking bit) of the frame header at the start of `d`, or None."""
    if len(d) < 4 or d[0] != 0xFF or d[1] & 0xFE != 0xF8:   # 14 sync bits, a reserved 0
        return None
    bcode, rcode, assignment, bps_code = d[2] >> 4, d[2] & 15, d[3] >> 4, (d[3] >> 1) & 7
    if bcode == 0 or rcode == 15 or assignment > 10 or bps_code == 3 or d[3] & 1:
        return None
    lead = 8 - (d[4] ^ 0xFF).bit_length() if len(d) > 4 else 1   # leading ones of the coded number's first byte
    if lead in (1, 8):
        return None
    k = 4 + max(lead, 1)
    if any(b & 0xC0 != 0x80 for b in d[5:k]):
        return None
    extra = {6: 1, 7: 2}.get(bcode, 0)
    n = BLOCK_SIZE_OF[bcode] if not extra else int.from_bytes(d[k:k + extra], "big") + 1
    k += extra + {12: 1, 13: 2, 14: 2}.get(rcode, 0)
    if k >= len(d) or orc.crc8(d[:k]) != d[k]:   # (k >= len: the header does not fit what is left of the stream)
        return None
    return n, k + 1, d[1] & 1


def metadata(blob):
    """None when the stream is refused, else (first frame byte, min_frame, STREAMINFO fields)."""
    if len(blob) < 42 or blob[:4] != b"fLaC":
        return None
    pos, si = 4, None
    while True:
        if pos + 4 > len(blob):
            return None
        last, kind, size = blob[pos] >> 7, blob[pos] & 0x7F, int.from_bytes(blob[pos + 1:pos + 4], "big")
        pos += 4
        if pos + size > len(blob):
            return None
        if kind == 0 and size == 34:
            si = blob[pos:pos + 34]
        pos += size
        if last:
            break
    if si is None:
        return None
    v = int.from_bytes(si[:18], "big")   # 16 + 16 + 24 + 24 + 20 + 3 + 5 + 36 bits
    f = dict(min_block=v >> 128, max_block=(v >> 112) & 0xFFFF, sample_rate=(v >> 44) & 0xFFFFF,
             channels=((v >> 41) & 7) + 1, bits_per_sample=((v >> 36) & 31) + 1, total_samples=v & (2 ** 36 - 1),
             md5=bytes(si[18:]))
    if f["max_block"] < 1:
        return None
    return pos, (v >> 88) & 0xFFFFFF, f


def scan(blob):
    """(rc, frame starts, block sizes, bad_frames, samples per channel) of the rule."""
    md = metadata(blob)
    if md is None:
        return INVALID_ARG, [], [], 0, 0
    pos, min_frame, f = md
    heads = {q: h for q in range(pos, len(blob)) for h in [parse_header(blob[q:q + 16])] if h}
    starts, sizes, s = [], [], pos
    while s < len(blob):
        if s not in heads:
            return 0, starts, sizes, 1, sum(sizes)
        n, hb, blocking = heads[s]
        lo = s + max(hb + 2 + f["channels"], min_frame)
        ends = [q for q in sorted(heads) if q >= lo and heads[q][2] == blocking] + [len(blob)]
        end = next((q for q in ends if int.from_bytes(blob[q - 2:q], "big") == orc.crc16(blob[s:q - 2])), None)
        if end is None:   # lost synchronisation: nothing from s on is kept
            return 0, starts, sizes, 1, sum(sizes)
        starts.append(s)
        sizes.append(n)
        s = end
    return 0, starts, sizes, 0, sum(sizes)


def header(n=192, blocking=0, number=0, bcode=None, rcode=9, assignment=0, bps_code=4):
    """A valid frame header and nothing else: what the scan takes for a frame start."""
    bcode = fs.BLOCK_CODES.get(n, 6 if n <= 256 else 7) if bcode is None else bcode
    h = bytes([0xFF, 0xF8 | blocking, bcode << 4 | rcode, assignment << 4 | bps_code << 1]) + fs.utf8_number(number)
    h += (n - 1).to_bytes(bcode - 5, "big") if bcode in (6, 7) else b""
    return h + bytes([fs.crc8(h)])


DAMAGED_FROM = ["fixed2", "lpc8", "stereo-16", "channels-3", "metadata-all-blocks", "variable-block-size",
                "number-7-bytes", "min-frame-unknown", "fixed-block-last-1", "rice-k"]


@functools.lru_cache(maxsize=1)
def damaged_cases():
    """((label, blob), ...): about 300 damaged versions of ten matrix streams, fixed by the seed."""
    rng = random.Random(20261018)
    by_name = {s.name: s for s in fm.valid_cases()}
    out = []
    for name in DAMAGED_FROM:
        st = by_name[name]
        first = len(st.blob) - sum(len(c) for c in st.frame_bytes)
        at = [first]
        for c in st.frame_bytes:
            at.append(at[-1] + len(c))
        nf = len(st.frame_bytes)

        def flip(pos):
            b = bytearray(st.blob)
            b[pos] ^= rng.randint(1, 255)
            return bytes(b)

        for _ in range(4):
            k = rng.randrange(nf)
            hb = parse_header(st.frame_bytes[k])[1]
            out.append((f"{name}: body byte of frame {k}", flip(rng.randrange(at[k] + hb, at[k + 1] - 2))))
            out.append((f"{name}: header byte of frame {k}", flip(rng.randrange(at[k], at[k] + hb))))
            out.append((f"{name}: CRC-16 byte of frame {k}", flip(at[k + 1] - 1 - rng.randrange(2))))
        k = rng.randrange(nf)
        out.append((f"{name}: frame {k} twice", st.blob[:at[k + 1]] + st.frame_bytes[k] + st.blob[at[k + 1]:]))
        for _ in range(3):
            k = rng.randrange(nf + 1)
            junk = bytes(rng.choice((0xFF, 0xF8, rng.randrange(256))) for _ in range(rng.randint(1, 40)))
            out.append((f"{name}: {len(junk)} garbage bytes before frame {k}", st.blob[:at[k]] + junk + st.blob[at[k]:]))
        out.append((f"{name}: no frame region", st.blob[:first]))
    st = by_name["rice-k"]
    last = len(st.blob) - len(st.frame_bytes[-1])
    out += [(f"rice-k: truncated to {n} bytes", st.blob[:n]) for n in range(last + 1, len(st.blob))]
    st = by_name["metadata-all-blocks"]
    first = len(st.blob) - sum(len(c) for c in st.frame_bytes)
    cuts = set(range(38, 52)) | set(rng.sample(range(52, first), 26))
    pos = 4
    while pos < first:   # around every block's header
        cuts |= {pos - 1, pos, pos + 3, pos + 4}
        pos += 4 + int.from_bytes(st.blob[pos + 1:pos + 4], "big")
    out += [(f"metadata-all-blocks: truncated to {n} bytes", st.blob[:n]) for n in sorted(cuts)]
    # regions made of nothing but valid headers (FF F8 ..): every one is a candidate, few or none link
    meta = by_name["fixed2"].blob[:len(by_name["fixed2"].blob) - sum(len(c) for c in by_name["fixed2"].frame_bytes)]
    same = header() * 40
    mixed = b"".join(header(n=rng.choice((16, 192, 4096, 300)), blocking=k & 1, number=k) for k in range(40))

    def crcd(b):
        return b + fs.crc16(b).to_bytes(2, "big")

    chain = b""   # headers that DO link: each followed by its CRC-16 and enough bytes for the minimum distance
    for k in range(6):
        chain += crcd(header(number=k) + bytes([0xFF, 0xF8]) * 3)
    # a CRC-16 that fits in front of a header with the OTHER blocking bit does not end the frame; the next one does
    other = crcd(crcd(header() + bytes(8)) + header(blocking=1, number=1) + bytes(8)) + crcd(header(number=2) + bytes(8))
    for label, region in (("one header 40 times", same), ("a linking header with the other blocking bit", other), ("40 headers, both blocking bits", mixed),
                          ("headers that link by CRC-16", chain), ("linked headers, then unlinked", chain + same),
                          ("headers, the last two bytes the CRC-16 of all", crcd(same)),
                          ("FF F8 pairs without a CRC-8", bytes([0xFF, 0xF8]) * 60),
                          ("a header cut short", header()[:5]), ("one header alone", header())):
        out.append((f"look-alikes: {label}", meta + region))
    return tuple(out)
