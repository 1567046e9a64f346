// frame_scan.inc -- frame discovery on the device for the batch decoder (decode_many.hip).
// Included inside decode_many.hip's anonymous namespace, after crc16.inc.
//
// The batch buffer holds one SLOT per stream: the stream's frame region (the bytes behind its metadata), 64-byte
// aligned, followed by at least 64 zero bytes.  A BLOCK is 64 bytes of it; the slots tile the blocks.  The scan finds
// the same frames as flacgpu_decode_stream's host scan, for any bytes (DESIGN.md "Frame discovery on the device"):
//   K_s1 k_scan_blocks   lane per block: candidate bitmap (a valid frame header starts here) + the block's CRC-16 +
//                        the workgroup's segmented CRC scan (a segment = one slot) and candidate count
//   K_s2 k_scan_carry    one workgroup: carries of the CRC scan and candidate offsets across workgroups
//   K_s3 k_scan_emit     lane per block: P64 = CRC-16 of the slot's bytes before the block; one record per candidate,
//                        in offset order, holding the header's fields and A = P x^(-8 q) (below)
//   K_s4 k_link          lane per candidate s: the first later candidate q that ends frame s (distance, blocking bit,
//                        CRC(s, q) == 0), or the slot's end, or none
// Raw frame streams (no metadata: a slot is the whole input; DESIGN.md "Raw frame streams") run the same kernels with two
// of their own: K_r1 k_scan_subset behind K_s1 drops the candidates that leave their sample rate or sample size to a
// STREAMINFO, and K_r2 k_link_raw stands in for K_s4 with the raw end rule.  K_s2 and K_s3 (P64, A, slot_pend) are shared.
// With init 0 and no final XOR, bytes [q-2, q) are the CRC-16 of [s, q-2) exactly when CRC(s, q) == 0, and
// CRC(s, q) = P(q) ^ P(s) x^(8 (q - s)) mod P with P(k) = CRC-16 of the region's bytes [0, k).  x is invertible mod P,
// so CRC(s, q) == 0 exactly when A(q) == A(s) with A(k) = P(k) x^(-8 k): one comparison per tested pair.

struct ScanSlot {        // one stream's frame region in the batch buffer
    uint64_t base;       // byte offset of the region (a multiple of 64)
    uint64_t len;        // region bytes (> 0)
    uint64_t block0;     // base / 64
    uint32_t channels;   // STREAMINFO
    uint32_t min_frame;  // STREAMINFO (0: unknown)
};
struct ScanParams {
    const uint8_t *bytes;        // the batch buffer
    const ScanSlot *slots;
    uint32_t n_slots;
    uint64_t n_blocks;           // blocks of the batch buffer (the slots tile them)
    // K_s1 -> K_s2 / K_s3
    uint64_t *mask;              // [n_blocks] candidate bitmap
    uint16_t *plocal;            // [n_blocks] CRC of the slot's bytes from max(slot start, workgroup start) to the block
    uint32_t *wg_cnt;            // [n_wg] candidates in the workgroup
    uint32_t *wg_tail;           // [n_wg] CRC of the workgroup's last segment (bit 16: a slot starts in the workgroup)
    // K_s2 -> K_s3
    uint32_t *wg_off;            // [n_wg + 1] exclusive prefix of wg_cnt (+ the total)
    uint16_t *wg_carry;          // [n_wg] P of the slot of the workgroup's first block at the workgroup's start
    // K_s3 -> K_s4 / host
    uint64_t *cand_pos;          // [n_cand] byte offset in the batch buffer, ascending
    uint32_t *cand_info;         // [n_cand] (n - 1) | header_bytes << 16 | blocking << 24
    uint32_t *cand_crc;          // [n_cand] A at the candidate
    uint32_t *cand_slot;         // [n_cand]
    uint32_t *slot_cand0;        // [n_slots] index of the slot's first candidate
    uint32_t *slot_pend;         // [n_slots] A at the region's end
    int32_t *link;               // [n_cand] next frame's candidate, LINK_END, LINK_NONE
    uint32_t n_cand;
};
constexpr int32_t LINK_END = -2;    // the frame ends with the stream
constexpr int32_t LINK_NONE = -1;   // no end: the scan loses synchronisation here

// x^(2^i) mod P, i < 15.  x has order 32767 modulo P = (x + 1)(x^15 + x + 1) (a primitive trinomial times x + 1), so
// every power of x reduces to an exponent below 2^15.
struct XPow2 {
    uint16_t w[15];
    constexpr XPow2() : w() {
        uint32_t v = 2;
        for (int i = 0; i < 15; i++) {
            w[i] = (uint16_t)v;
            v = gf_mulmod_c(v, v);
        }
    }
};
__constant__ XPow2 kXPow2 = XPow2();
// x^e mod P, e < 32767
__device__ __forceinline__ uint32_t gf_xpow(uint32_t e) {
    uint32_t r = 1;
#pragma unroll
    for (int i = 0; i < 15; i++)
        if ((e >> i) & 1u) r = gf_mulmod(r, kXPow2.w[i]);
    return r;
}
// x^(8 nbytes) mod P
__device__ __forceinline__ uint32_t gf_xpow_bytes(uint64_t nbytes) {
    return gf_xpow((uint32_t)((nbytes % 32767u) * 8u % 32767u));
}
// A(k) = P(k) x^(-8 k) mod P
__device__ __forceinline__ uint32_t crc_normalise(uint32_t P, uint64_t k) {
    const uint32_t e = (uint32_t)((k % 32767u) * 8u % 32767u);
    return gf_mulmod(P, gf_xpow(e ? 32767u - e : 0u));
}
// the CRC continued over n (< 64) bytes, one table step per byte
__device__ __forceinline__ uint32_t crc16_bytes(uint32_t crc, const uint8_t *p, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) crc = ((crc << 8) & 0xFFFFu) ^ kCrcT.t[0][((crc >> 8) ^ p[i]) & 0xFFu];
    return crc;
}

// host_parse_header (host/flac_stream.cpp) on the device: FrameHeader::parse (stream.rs:214-240) + CRC-8, every read
// bounded by `avail` = bytes left in the stream.
struct ScanHead {
    uint32_t n, header_bytes, blocking;
};
__device__ __forceinline__ bool scan_parse_header(const uint8_t *d, uint64_t avail64, ScanHead &h) {
    const uint32_t avail = avail64 > 64 ? 64u : (uint32_t)avail64;   // a header is at most 16 bytes
    if (avail < 6 || d[0] != 0xFF || (d[1] & 0xFE) != 0xF8) return false;
    h.blocking = d[1] & 1;
    const uint32_t bcode = d[2] >> 4, rcode = d[2] & 15;
    const uint32_t acode = d[3] >> 4, bps_code = (d[3] >> 1) & 7;
    if ((d[3] & 1) || acode > 10 || bcode == 0 || rcode == 15 || bps_code == 3) return false;
    uint32_t k = 4;
    {   // UTF-8 like number
        const uint32_t b0 = d[k];
        uint32_t ones = 0;
        while (ones < 8 && (b0 & (0x80u >> ones))) ones++;
        if (ones == 1 || ones > 7) return false;
        const uint32_t extra = ones ? ones - 1 : 0;
        if (k + 1 + extra > avail) return false;
        for (uint32_t i = 1; i <= extra; i++)
            if ((d[k + i] & 0xC0) != 0x80) return false;
        k += 1 + extra;
    }
    switch (bcode) {
    case 1: h.n = 192; break;
    case 2: h.n = 576; break;
    case 3: h.n = 1152; break;
    case 4: h.n = 2304; break;
    case 5: h.n = 4608; break;
    case 6:
        if (k + 1 > avail) return false;
        h.n = d[k] + 1u;
        k += 1;
        break;
    case 7:
        if (k + 2 > avail) return false;
        h.n = ((uint32_t)d[k] << 8 | d[k + 1]) + 1u;
        k += 2;
        break;
    default: h.n = 256u << (bcode - 8); break;
    }
    if (rcode == 12) k += 1;
    else if (rcode == 13 || rcode == 14) k += 2;
    if (k + 1 > avail) return false;
    uint32_t crc = 0;   // CRC-8, poly x^8 + x^2 + x + 1 (crc.rs:99-128)
    for (uint32_t i = 0; i < k; i++) {
        crc ^= d[i];
        for (int b = 0; b < 8; b++) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1) & 0xFF;
    }
    if (crc != d[k]) return false;
    h.header_bytes = k + 1;
    return true;
}

// the slot that holds block b (slots ascending, tiling the blocks)
__device__ __forceinline__ uint32_t slot_of_block(const ScanSlot *slots, uint32_t n, uint64_t b) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (slots[mid].block0 <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ void load_crc_tables(uint16_t (*T)[256], uint32_t tid) {
    uint32_t c = tid << 8;
    for (int k = 0; k < 4; k++) {   // T[k][b] = CRC state after byte b followed by k zero bytes
        for (int b = 0; b < 8; b++) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
        T[k][tid] = (uint16_t)c;
    }
}

// K_s1: lane per block.  The candidate filter (0xFF, then 0xF8 | blocking) runs on the 16-byte loads in registers;
// the rare positions that pass it are parsed from memory.
__global__ void __launch_bounds__(WG) k_scan_blocks(ScanParams p) {
    __shared__ uint16_t T[4][256];
    __shared__ uint32_t sv[WG];
    __shared__ uint32_t sf[WG];
    __shared__ uint32_t scnt[WG / 64];
    const uint32_t tid = threadIdx.x;
    load_crc_tables(T, tid);
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * WG + tid;
    const bool live = b < p.n_blocks;
    uint32_t crc = 0, start = 0, cnt = 0;
    if (live) {
        const uint32_t s = slot_of_block(p.slots, p.n_slots, b);
        const ScanSlot sl = p.slots[s];
        start = b == sl.block0;
        const uint64_t rel = (b - sl.block0) * 64;   // region offset of the block
        // 64 bytes + 16 of look-ahead (the slot's zero tail keeps them inside the slot)
        uint32_t w[20];
        const uint4 *src = reinterpret_cast<const uint4 *>(p.bytes + b * 64);
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uint4 v = src[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
        uint64_t m = 0;
        if (rel < sl.len) {
#pragma unroll
            for (int j = 0; j < 64; j++) {
                const uint32_t b0 = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                const uint32_t b1 = (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu;
                m |= (uint64_t)(b0 == 0xFFu && (b1 & 0xFEu) == 0xF8u) << j;
            }
            const uint64_t here = sl.len - rel;   // region bytes from the block's start
            if (here < 64) m &= (1ull << here) - 1;
            uint64_t t = m;
            while (t) {
                const uint32_t j = (uint32_t)__builtin_ctzll(t);
                t &= t - 1;
                ScanHead h;
                if (!scan_parse_header(p.bytes + b * 64 + j, here - j, h)) m &= ~(1ull << j);
            }
        }
        p.mask[b] = m;
        cnt = (uint32_t)__builtin_popcountll(m);
#pragma unroll
        for (int i = 0; i < 16; i++) {   // the k_crc step (pack.inc): four bytes of a little-endian dword
            const uint32_t v = w[i];
            crc = T[3][((crc >> 8) ^ v) & 0xFF] ^ T[2][(crc ^ (v >> 8)) & 0xFF] ^ T[1][(v >> 16) & 0xFF] ^ T[0][v >> 24];
        }
    }
    // segmented inclusive scan of the block CRCs over the workgroup: I_t = start_t ? c_t : I_(t-1) x^512 ^ c_t
    uint32_t v = crc, f = start;
    sv[tid] = v;
    sf[tid] = f;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < WG; d <<= 1) {
        uint32_t lv = 0, lf = 0;
        if (tid >= d) { lv = sv[tid - d]; lf = sf[tid - d]; }
        __syncthreads();
        if (tid >= d && !f) {
            v = gf_mulmod_t(lv, kCrcW.w[d], T) ^ v;
            f = lf;
        }
        sv[tid] = v;
        sf[tid] = f;
        __syncthreads();
    }
    if (live) p.plocal[b] = (uint16_t)((start || tid == 0) ? 0u : sv[tid - 1]);
    // candidates in the workgroup
    uint32_t c = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((tid & 63) == 0) scnt[tid >> 6] = c;
    __syncthreads();
    if (tid == WG - 1) {
        p.wg_cnt[blockIdx.x] = scnt[0] + scnt[1] + scnt[2] + scnt[3];
        p.wg_tail[blockIdx.x] = sv[WG - 1] | (sf[WG - 1] ? 0x10000u : 0u);
    }
}

// K_s2: one workgroup.  Lane t takes a contiguous run of workgroups: a serial segmented scan inside the run, the runs
// combined with a Hillis-Steele scan in LDS, then the run is walked again to write the carries and offsets.
__global__ void __launch_bounds__(WG) k_scan_carry(ScanParams p, uint32_t n_wg) {
    __shared__ uint16_t T[4][256];
    __shared__ uint32_t sv[WG], sf[WG], sc[WG];
    const uint32_t tid = threadIdx.x;
    load_crc_tables(T, tid);
    __syncthreads();
    const uint32_t per = (n_wg + WG - 1) / WG;
    const uint32_t w0 = min(n_wg, tid * per), w1 = min(n_wg, w0 + per);
    const uint32_t xwg = kCrcW.w[WG];   // x^(512 WG): one workgroup's blocks
    // run aggregate: CRC of the run's last segment, whether a slot starts in the run, candidates
    uint32_t v = 0, f = 0, cnt = 0;
    for (uint32_t w = w0; w < w1; w++) {
        const uint32_t t = p.wg_tail[w];
        v = (t & 0x10000u) ? (t & 0xFFFFu) : (gf_mulmod_t(v, xwg, T) ^ (t & 0xFFFFu));
        f |= t >> 16;
        cnt += p.wg_cnt[w];
    }
    sv[tid] = v;
    sf[tid] = f;
    sc[tid] = cnt;
    __syncthreads();
    for (uint32_t d = 1; d < WG; d <<= 1) {
        uint32_t lv = 0, lf = 0, lc = 0;
        if (tid >= d) { lv = sv[tid - d]; lf = sf[tid - d]; lc = sc[tid - d]; }
        __syncthreads();
        if (tid >= d) {
            // the right-hand window holds runs tid-d+1 .. tid: (w1 of tid) - (w0 of tid-d+1) workgroups
            const uint32_t span = w1 - min(n_wg, (tid - d + 1) * per);
            if (!f) v = gf_mulmod(lv, gf_xpow_bytes((uint64_t)span * WG * 64)) ^ v;
            f |= lf;
            cnt += lc;
        }
        sv[tid] = v;
        sf[tid] = f;
        sc[tid] = cnt;
        __syncthreads();
    }
    // exclusive values of the run
    uint32_t carry = tid ? sv[tid - 1] : 0u;
    uint32_t off = tid ? sc[tid - 1] : 0u;
    for (uint32_t w = w0; w < w1; w++) {
        p.wg_carry[w] = (uint16_t)carry;
        p.wg_off[w] = off;
        const uint32_t t = p.wg_tail[w];
        carry = (t & 0x10000u) ? (t & 0xFFFFu) : (gf_mulmod_t(carry, xwg, T) ^ (t & 0xFFFFu));
        off += p.wg_cnt[w];
    }
    if (tid == WG - 1) p.wg_off[n_wg] = sc[WG - 1];
}

// K_s3: lane per block.  P64 of the block, then one record per candidate (offset order: workgroup offset + the
// lanes before it in the workgroup + the bits below it in its mask).
__global__ void __launch_bounds__(WG) k_scan_emit(ScanParams p) {
    __shared__ uint32_t scnt[WG];
    const uint32_t tid = threadIdx.x;
    const uint64_t b = (uint64_t)blockIdx.x * WG + tid;
    const bool live = b < p.n_blocks;
    uint64_t m = live ? p.mask[b] : 0;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
    scnt[tid] = cnt;
    __syncthreads();
    for (uint32_t d = 1; d < WG; d <<= 1) {
        const uint32_t l = tid >= d ? scnt[tid - d] : 0u;
        __syncthreads();
        scnt[tid] += l;
        __syncthreads();
    }
    if (!live) return;
    uint32_t idx = p.wg_off[blockIdx.x] + scnt[tid] - cnt;
    const uint32_t s = slot_of_block(p.slots, p.n_slots, b);
    const ScanSlot sl = p.slots[s];
    const uint64_t wg_first = (uint64_t)blockIdx.x * WG;
    uint32_t P = p.plocal[b];
    if (sl.block0 < wg_first)   // the slot began before this workgroup: add the carry, moved up to this block
        P ^= gf_mulmod(p.wg_carry[blockIdx.x], kCrcW.w[b - wg_first]);
    const uint64_t rel = (b - sl.block0) * 64;
    const uint8_t *blk = p.bytes + b * 64;
    if (b == sl.block0) p.slot_cand0[s] = idx;
    if (rel <= sl.len && sl.len - rel < 64)
        p.slot_pend[s] = crc_normalise(crc16_bytes(P, blk, (uint32_t)(sl.len - rel)), sl.len);
    while (m) {
        const uint32_t j = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        ScanHead h;
        scan_parse_header(blk + j, sl.len - rel - j, h);   // accepted by K_s1
        p.cand_pos[idx] = b * 64 + j;
        p.cand_info[idx] = (h.n - 1u) | h.header_bytes << 16 | h.blocking << 24;
        p.cand_crc[idx] = crc_normalise(crc16_bytes(P, blk, j), rel + j);
        p.cand_slot[idx] = s;
        idx++;
    }
}

// K_s4: lane per candidate.  The host scan's rule: frame s ends at the first q >= s + max(header_bytes + 2 + channels,
// min_frame) where a header with the same blocking bit starts and bytes [q-2, q) are the CRC-16 of [s, q-2); failing
// that, with the stream when its last two bytes are that CRC; failing that, nowhere.
__global__ void __launch_bounds__(WG) k_link(ScanParams p) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= p.n_cand) return;
    const uint32_t s = p.cand_slot[i];
    const ScanSlot sl = p.slots[s];
    const uint32_t end = s + 1 < p.n_slots ? p.slot_cand0[s + 1] : p.n_cand;
    const uint64_t pos = p.cand_pos[i];
    const uint32_t info = p.cand_info[i];
    const uint32_t blocking = info >> 24, hb = (info >> 16) & 0xFFu;
    const uint64_t min_len = max(hb + 2u + sl.channels, sl.min_frame);
    const uint32_t A = p.cand_crc[i];
    int32_t link = LINK_NONE;
    for (uint32_t j = i + 1; j < end; j++) {
        if (p.cand_crc[j] != A || (p.cand_info[j] >> 24) != blocking || p.cand_pos[j] - pos < min_len) continue;
        link = (int32_t)j;
        break;
    }
    if (link == LINK_NONE && sl.base + sl.len - pos >= 2 && p.slot_pend[s] == A) link = LINK_END;
    p.link[i] = link;
}

// ---- raw frame streams ----
// K_r1: lane per block, behind K_s1 and in front of K_s2.  A raw stream's frame must say its own sample rate and sample
// size (FrameHeader::read_subset, stream.rs:672, 1161): candidates whose codes for either are 0 leave the bitmap, and
// the workgroup's candidates are counted again.  A candidate has at least 6 bytes of its stream behind it (K_s1).
__global__ void __launch_bounds__(WG) k_scan_subset(ScanParams p) {
    __shared__ uint32_t scnt[WG / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t b = (uint64_t)blockIdx.x * WG + tid;
    uint32_t cnt = 0;
    if (b < p.n_blocks) {
        uint64_t m = p.mask[b], t = m;
        const uint8_t *blk = p.bytes + b * 64;
        while (t) {
            const uint32_t j = (uint32_t)__builtin_ctzll(t);
            t &= t - 1;
            if ((blk[j + 2] & 15u) == 0 || ((blk[j + 3] >> 1) & 7u) == 0) m &= ~(1ull << j);
        }
        p.mask[b] = m;
        cnt = (uint32_t)__builtin_popcountll(m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0) scnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == WG - 1) p.wg_cnt[blockIdx.x] = scnt[0] + scnt[1] + scnt[2] + scnt[3];
}

// K_r2: lane per candidate.  The raw end rule: frame s ends at the first later candidate q >= s + header_bytes + 2 +
// channels(s) with CRC(s, q) == 0 -- the channels are those of s's own assignment code (byte 3 of its header), the
// blocking bit of q is not compared and there is no minimum frame size: every frame stands alone --; failing that, with
// the input when its last two bytes are that CRC; failing that, nowhere (the host walk passes such a candidate over).
__global__ void __launch_bounds__(WG) k_link_raw(ScanParams p) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= p.n_cand) return;
    const uint32_t s = p.cand_slot[i];
    const ScanSlot sl = p.slots[s];
    const uint32_t end = s + 1 < p.n_slots ? p.slot_cand0[s + 1] : p.n_cand;
    const uint64_t pos = p.cand_pos[i];
    const uint32_t hb = (p.cand_info[i] >> 16) & 0xFFu;
    const uint32_t acode = p.bytes[pos + 3] >> 4;
    const uint64_t min_len = hb + 2u + (acode < 8 ? acode + 1u : 2u);
    const uint32_t A = p.cand_crc[i];
    int32_t link = LINK_NONE;
    for (uint32_t j = i + 1; j < end; j++) {
        if (p.cand_crc[j] != A || p.cand_pos[j] - pos < min_len) continue;
        link = (int32_t)j;
        break;
    }
    if (link == LINK_NONE && sl.base + sl.len - pos >= 2 && p.slot_pend[s] == A) link = LINK_END;
    p.link[i] = link;
}
