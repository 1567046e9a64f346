// spec_end.inc -- FLACGPU_SCAN_SPECULATIVE on the device: a raw candidate that no header ends gets its own extent
// (DESIGN.md 4b "A frame's own extent").  Included inside decode_many.hip's anonymous namespace, after decode.inc (the
// BitReader), frame_scan.inc (ScanParams, the CRC algebra) and kernels/frame_extent.h (the walk, shared with the host).

// frame_extent's bit source: decode.inc's BitReader on the batch buffer, positions relative to the candidate.  Reads
// are clamped at `cap` = the slot's end - 4 (ManyFrame::cap): behind the input lies the slot's zero tail, the reader
// never leaves it, and a walk into it ends at the window test.
struct SpecBits {
    BitReader r;
    const uint32_t *words;
    uint64_t start, cap;
    __device__ __forceinline__ uint32_t pos() const { return r.pos(); }
    // set the reader down again at the byte, skip the odd bits: O(1) whatever the distance
    __device__ __forceinline__ void seek(uint32_t bit) {
        r.init(words, start + (bit >> 3), cap, bit & ~7u);
        r.skip(bit & 7u);
    }
    __device__ __forceinline__ uint32_t get(uint32_t n) { return r.get(n); }
    __device__ __forceinline__ uint32_t zeros(uint32_t limit) { return r.unary1(limit); }
    __device__ __forceinline__ void rice(uint32_t k, uint32_t limit) { r.rice(k, 1u << k, limit); }
};

// K_r3: lane per candidate, behind K_r2 and only under the flag.  A candidate with a link leaves at once; one without
// walks its subframes (frame_extent: at most 2^25 bits and 8 x 65535 Rice codes) and tests the CRC-16 of [s, e) by the
// scan's prefix identity A(e) == A(s): P(e) from the block prefix as K_s3 forms it, advanced over e mod 64 bytes -- the
// frame is not read a second time.  spec_len[i] = e - s, 0: none.
__global__ void __launch_bounds__(64) k_spec_end(ScanParams p, uint32_t *__restrict__ spec_len) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= p.n_cand) return;
    spec_len[i] = 0;
    if (p.link[i] != LINK_NONE) return;
    const uint32_t s = p.cand_slot[i];
    const ScanSlot sl = p.slots[s];
    const uint64_t slot_end = s + 1 < p.n_slots ? p.slots[s + 1].base : p.n_blocks * 64;
    const uint64_t pos = p.cand_pos[i];
    const uint32_t info = p.cand_info[i];
    const uint32_t b3 = p.bytes[pos + 3];
    const uint32_t bcode = (b3 >> 1) & 7u;   // 1, 2, 4, 5, 6, 7 -> 8, 12, 16, 20, 24, 32 (0 and 3 are no candidates)
    const uint32_t bps = bcode == 7 ? 32u : bcode < 3 ? 4u + 4u * bcode : 4u * bcode;
    const uint64_t left = sl.base + sl.len - pos;
    SpecBits bits;
    bits.words = reinterpret_cast<const uint32_t *>(p.bytes);
    bits.start = pos;
    bits.cap = slot_end - 4;
    const uint32_t len = frame_extent(bits, (info >> 16) & 0xFFu, (info & 0xFFFFu) + 1u, b3 >> 4, bps,
                                      left < kFrameExtentWindow ? left : kFrameExtentWindow);
    if (!len) return;
    const uint64_t e = pos + len;   // <= the slot's region end: block b lies inside the slot
    const uint64_t b = e / 64, wg_first = b / WG * WG;
    uint32_t P = p.plocal[b];
    if (sl.block0 < wg_first) P ^= gf_mulmod(p.wg_carry[b / WG], kCrcW.w[b - wg_first]);
    if (crc_normalise(crc16_bytes(P, p.bytes + b * 64, (uint32_t)(e % 64)), e - sl.base) == p.cand_crc[i]) spec_len[i] = len;
}
