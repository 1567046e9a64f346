// decode.inc -- frame decoder + verifier.
// Part of flacenc_gpu.hip (one translation unit; included inside its anonymous namespace).

// ---------------------------------------------------------------------------------
// Frame decoder + verifier (SURVEY.md 8(f) N3): the reference's read_frame / read_subframes /
// read_subframe / read_residuals / predict (decode.rs:1388-1436, 1494-1856) for frames whose
// byte offsets are known (everything this encoder produces).  Rice decoding and LPC synthesis
// are sequential inside a subframe, so ONE LANE decodes ONE SUBFRAME: the parallelism is across
// the thousands of frames of a batch times their channels.  A subframe's start is only known
// once the previous one has been parsed; the lanes take the encoder's own subframe lengths
// (SubPlan::bits) as the CLAIM and prove it: each lane must end exactly where the next one was
// told to start, the first starts where the frame header ends and the last ends at the padding
// before the CRC-16 -- so the frame is known to parse front to back the way a sequential
// decoder would, without any lane waiting for another.  What keeps a lane fast:
//   * the bit reader is a 64-bit shift register refilled with aligned, byte-swapped dwords, the
//     next dword always in flight (one load per 32 consumed bits instead of ten byte loads per
//     sample);
//   * the last MAXO decoded samples and the coefficients live in registers: the synthesis loop is
//     unrolled MAXO times so that the history index rotates statically (no register shifting, no
//     re-reading of just-written global memory); MAXO is picked per launch from the encoder's
//     maximum LPC order, and every lane of a wave runs the same instruction stream at the same
//     sample index whatever the orders of its subframes are (coefficients beyond the order are
//     zero), so partition headers come up for all lanes at once;
//   * k_decode writes the subframes as they are coded; k_decode_finish (one workgroup per
//     frame, coalesced) undoes the stereo decorrelation and compares with the expected PCM.
// Output: planar PCM [frame][channel][ldb].
// verify_counts[0] frames with a header / structure error, [2] frames whose PCM differs from the
// reference buffer (when given), [3] differing samples; verify_counts[4 + frame] = the frame's
// channel-assignment code, | 0x100 when one of its lanes found an error (nothing to finish).
// ---------------------------------------------------------------------------------
struct BitReader {
    const uint32_t *words;  // the packed buffer as dwords
    uint32_t widx, wmax;    // next dword to request / last dword that may be read
    uint64_t buf;           // unread bits, left-aligned
    uint32_t cnt;           // valid bits in buf
    uint32_t next;          // the prefetched dword, as loaded: swapping it on arrival would make
                            // the load synchronous
    uint32_t loaded;        // bits ever put into buf, + the start position: pos = loaded - cnt
                            // (positions are relative to the frame start: 32 bits are enough)
    // start reading at byte `byte_off` of the buffer, which is bit `rel` of the frame
    __device__ __forceinline__ void init(const uint32_t *w, uint64_t byte_off, uint64_t cap_bytes, uint32_t rel) {
        words = w;
        wmax = (uint32_t)(cap_bytes / 4);
        widx = (uint32_t)(byte_off >> 2);
        const uint32_t skip = (uint32_t)(byte_off & 3) * 8;
        const uint32_t first = __builtin_bswap32(words[widx]);
        widx = min(widx + 1, wmax);
        buf = ((uint64_t)first << 32) << skip;
        cnt = 32 - skip;
        loaded = rel - skip + 32;
        next = words[widx];
        widx = min(widx + 1, wmax);
        refill();
    }
    // Afterwards cnt >= 32 (>= 33 unless the register was empty).  Lanes of a wave need their refills at different times, so the wave
    // runs this body at nearly every call: the fewer call sites on the per-sample path, the fewer
    // waits for the dword requested at the previous one.
    __device__ __forceinline__ void refill() {
        if (cnt <= 32) {
            buf |= (uint64_t)__builtin_bswap32(next) << (32 - cnt);
            cnt += 32;
            loaded += 32;
            next = words[widx];
            widx = min(widx + 1, wmax);
        }
    }
    __device__ __forceinline__ uint32_t pos() const { return loaded - cnt; }
    __device__ __forceinline__ void skip(uint32_t n) {  // n <= cnt
        buf <<= n;
        cnt -= n;
    }
    __device__ __forceinline__ uint32_t peek(uint32_t n) const {  // n in 0..32, n <= cnt
        return (uint32_t)((buf >> 1) >> (63 - n));
    }
    __device__ __forceinline__ uint32_t get(uint32_t n) {  // n in 0..32
        refill();
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
    __device__ __forceinline__ int32_t get_signed(uint32_t n) {  // n in 0..32
        refill();
        const int32_t v = (int32_t)(((int64_t)buf >> 1) >> (63 - n));
        skip(n);
        return n ? v : 0;
    }
    // a signed value of 1..33 bits: the 33rd is what a side channel of 32-bit stereo adds
    __device__ __forceinline__ int64_t get_wide(uint32_t n) {
        if (n <= 32) return get_signed(n);
        const int64_t top = get_signed(n - 32);
        return top * 4294967296ll + get(32);
    }
    // zeros before the next 1 bit; `limit`: bit position that ends the frame
    __device__ __forceinline__ uint32_t unary1(uint32_t limit) {
        uint32_t q = 0;
        for (;;) {
            refill();
            const uint32_t hi = (uint32_t)(buf >> 32);
            if (hi) {
                const uint32_t z = (uint32_t)__builtin_clz(hi);
                skip(z + 1);
                return q + z;
            }
            q += 32;
            skip(32);
            if (pos() > limit) return q;  // corrupt stream guard
        }
    }
    // One Rice code with parameter k (<= 30): quotient in unary, a 1, k remainder bits.  One
    // refill covers every code of up to 32 bits (thr = 2^k: the stop bit is early enough in the top 32
    // bits); longer ones take the general route.  (Until r04 the fast route took 33-bit codes as well, on
    // the strength of "cnt >= 33 after refill()" -- which fails when the previous code ended exactly at the
    // register's last bit: cnt == 0 refills to 32, and the code's last bit -- the sign of the residual --
    // was read as zero.  It takes k + quotient = 32, e.g. 32-bit samples at k = 28 with a residual of
    // four times the partition's mean; found by the r04 random sweep, seed 1264.)
    __device__ __forceinline__ uint32_t rice(uint32_t k, uint32_t thr, uint32_t limit) {
        refill();
        const uint32_t hi = (uint32_t)(buf >> 32);
        if (hi >= thr) {
            const uint32_t z = (uint32_t)__builtin_clz(hi);
            buf <<= z + 1;
            const uint32_t u = (z << k) | __builtin_amdgcn_ubfe((uint32_t)(buf >> 32), 32 - k, k);
            buf <<= k;
            cnt -= z + 1 + k;
            return u;
        }
        const uint32_t qn = unary1(limit);
        return (qn << k) | get(k);
    }
};

// One subframe with residuals: partitions, Rice / escape codes, synthesis (read_residuals,
// decode.rs:1800-1856, fused with predict, decode.rs:1738-1752).  Sample i lives in ring slot
// i % MAXO, so every lane of a wave is at the same sample index at the same instruction whatever
// its predictor order is: partition boundaries (multiples of the partition length) then come at
// the same step for all lanes and their header path runs once, not once per lane.
// On entry h[j] = sample j for j < order; coef[j] = 0 for j >= order.
struct ResidualWalk {
    uint32_t order, n, part, parts, plen;
    uint32_t left, esc_left;  // residuals left in the current partition: Rice coded / escaped
    uint32_t k, thr, ebits, hb, esc, shift, wasted, end_bit;
    bool fail;
};
// h[0..CNT) << wasted to dst[0..CNT), 16 bytes at a time (turns start at multiples of MAXO)
template <int MAXO>
__device__ __forceinline__ void store_ring(const int32_t (&h)[MAXO], int32_t *__restrict__ dst, uint32_t wasted,
                                           uint32_t count) {
    if (count >= (uint32_t)MAXO) {
        static_assert(MAXO % 4 == 0, "16-byte stores");
#pragma unroll
        for (int q = 0; q < MAXO; q += 4)
            *reinterpret_cast<int4 *>(dst + q) =
                make_int4((int32_t)((uint32_t)h[q] << wasted), (int32_t)((uint32_t)h[q + 1] << wasted),
                          (int32_t)((uint32_t)h[q + 2] << wasted), (int32_t)((uint32_t)h[q + 3] << wasted));
    } else {
#pragma unroll
        for (int q = 0; q < MAXO; q++)
            if ((uint32_t)q < count) dst[q] = (int32_t)((uint32_t)h[q] << wasted);
    }
}
__device__ __forceinline__ int32_t rice_residual(BitReader &r, ResidualWalk &w) {
    const uint32_t u = r.rice(w.k, w.thr, w.end_bit);
    w.left--;
    return (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
}
// Steps T..MAXO-1 of the turn of the history ring that starts at sample `base` (a template
// recursion rather than a loop: the ring index has to be a compile-time constant for h[] to stay
// in registers).  The per-sample path has ONE test (w.left): the range test (the first turn holds
// the warm-up samples, the last one may be short), failure, partition headers and escaped
// partitions all hide behind it.
template <int MAXO, int T>
__device__ __forceinline__ void synth_steps(BitReader &r, const int32_t (&coef)[MAXO], int32_t (&h)[MAXO],
                                            ResidualWalk &w, uint32_t base) {
    if constexpr (T < MAXO) {
        const uint32_t i = base + T;
        int32_t res = 0;
        bool live = true;
        if (w.left == 0) {
            // everything that is not "one more Rice code of this partition": samples outside
            // [order, n) (left is 0 before the first and after the last partition), a failed
            // subframe (left stays 0), partition headers, escaped partitions
            if (i < w.order || i >= w.n || w.fail) {
                live = false;
            } else {
                while (w.left == 0 && w.esc_left == 0) {  // next partition header
                    if (w.part == w.parts || r.pos() > w.end_bit) {
                        w.fail = true;
                        break;
                    }
                    const uint32_t cnt = w.plen - (w.part == 0 ? w.order : 0u);
                    w.part++;
                    w.k = r.get(w.hb);
                    if (w.k == w.esc) {
                        w.ebits = r.get(5);
                        w.esc_left = cnt;
                    } else {
                        w.thr = 1u << w.k;   // k <= 30 (31 is the escape code)
                        w.left = cnt;
                    }
                }
                if (w.fail) {
                    live = false;
                } else if (w.left == 0) {
                    res = r.get_signed(w.ebits);
                    w.esc_left--;
                } else {
                    res = rice_residual(r, w);
                }
            }
        } else {
            res = rice_residual(r, w);
        }
        // two chains up to order 16: a lone wave has issue slots to spare, not latency (together
        // with the single test above: -4 % at MAXO = 12); MAXO = 32 keeps one chain (registers)
        long long s0 = 0, s1 = 0;
        if constexpr (MAXO <= 16) {
#pragma unroll
            for (int j = 0; j < MAXO; j += 2) {
                s0 += (long long)h[(T - 1 - j + 2 * MAXO) % MAXO] * (long long)coef[j];
                s1 += (long long)h[(T - 2 - j + 2 * MAXO) % MAXO] * (long long)coef[j + 1];
            }
        } else {
#pragma unroll
            for (int j = 0; j < MAXO; j++) s0 += (long long)h[(T - 1 - j + 2 * MAXO) % MAXO] * (long long)coef[j];
        }
        const int32_t v = res + (int32_t)((s0 + s1) >> w.shift);
        h[T] = live ? v : h[T];
        synth_steps<MAXO, T + 1>(r, coef, h, w, base);
    }
}

template <int MAXO>
__device__ __forceinline__ bool decode_residuals(BitReader &r, const int32_t (&coef)[MAXO], int32_t (&h)[MAXO],
                                                 uint32_t order, uint32_t shift, uint32_t wasted, uint32_t n,
                                                 int32_t *__restrict__ x, uint32_t end_bit) {
    const uint32_t method = r.get(2);
    if (method > 1) return false;
    ResidualWalk w;
    w.hb = method ? 5u : 4u;
    w.esc = method ? 31u : 15u;
    const uint32_t po = r.get(4);
    w.plen = n >> po;
    w.parts = 1u << po;
    if (w.plen < order || (w.plen << po) != n) return false;
    w.order = order; w.n = n; w.part = 0; w.left = 0; w.esc_left = 0; w.k = 0; w.thr = 1; w.ebits = 0;
    w.shift = shift; w.wasted = wasted; w.end_bit = end_bit; w.fail = false;
    for (uint32_t base = 0; base < n && !w.fail; base += MAXO) {
        synth_steps<MAXO, 0>(r, coef, h, w, base);
        store_ring<MAXO>(h, x + base, wasted, n - base);  // the ring is also the output buffer
    }
    if (w.fail) return false;
    while (w.part < w.parts && w.left == 0 && w.esc_left == 0) {  // partitions without residuals have headers too
        const uint32_t cnt = w.plen - (w.part == 0 ? order : 0u);
        w.part++;
        if (r.get(w.hb) == w.esc) {
            r.get(5);
            w.esc_left = cnt;
        } else {
            w.left = cnt;
        }
    }
    return w.part == w.parts && w.left == 0 && w.esc_left == 0 && r.pos() <= end_bit;
}

// FrameHeader::parse (stream.rs:214-240) + CRC-8; returns false on a malformed header.  blocking:
// the blocking-strategy bit (1: the coded number is a sample number, stream.rs:1219-1262).
struct FrameHead {
    uint32_t n, bps_code, acode, rcode, blocking;
};
__device__ __forceinline__ bool parse_frame_header(BitReader &r, const uint8_t *bytes, uint64_t start_byte,
                                                   FrameHead &h) {
    bool bad = false;
    if (r.get(14) != 0x3FFE) bad = true;   // sync 0b11111111111110
    if (r.get(1)) bad = true;              // reserved
    h.blocking = r.get(1);
    const uint32_t bcode = r.get(4);
    h.rcode = r.get(4);
    h.acode = r.get(4);
    h.bps_code = r.get(3);
    if (r.get(1)) bad = true;              // reserved
    {   // frame / sample number (UTF-8 like), stream.rs:1244-1262
        uint32_t ones = 0;
        while (ones < 8 && r.get(1)) ones++;
        if (ones == 0) r.get(7);
        else if (ones == 1 || ones > 7) bad = true;
        else {
            r.get(7 - ones);
            for (uint32_t i = 1; i < ones; i++) {
                if (r.get(2) != 2) bad = true;
                r.get(6);
            }
        }
    }
    switch (bcode) {
    case 1: h.n = 192; break;
    case 2: h.n = 576; break;
    case 3: h.n = 1152; break;
    case 4: h.n = 2304; break;
    case 5: h.n = 4608; break;
    case 6: h.n = r.get(8) + 1; break;
    case 7: h.n = r.get(16) + 1; break;
    case 0: h.n = 0; bad = true; break;
    default: h.n = 256u << (bcode - 8); break;
    }
    if (h.rcode == 12) r.get(8);
    else if (h.rcode == 13 || h.rcode == 14) r.get(16);
    else if (h.rcode == 15) bad = true;
    {   // CRC-8 over the header
        const uint32_t hb1 = r.pos() >> 3;
        uint32_t crc = 0;
        for (uint32_t i = 0; i < hb1; i++) {
            crc ^= bytes[start_byte + i];
            for (int b = 0; b < 8; b++) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1) & 0xFF;
        }
        if (r.get(8) != crc) bad = true;
    }
    if (h.acode > 10) bad = true;
    return !bad;
}
__device__ __forceinline__ uint32_t bps_of_code(uint32_t code, uint32_t streaminfo_bps) {
    const uint32_t bps_tab[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    return code ? bps_tab[code] : streaminfo_bps;
}

// The body of a 33-bit subframe: the side channel of 32-bit stereo, which the reference reads as i64
// (read_subframe::<33, R, i64>, decode.rs:1520-1628).  Rare, so plain rather than fast: no ring in
// registers.  The last 32 samples -- all a predictor can ask for -- wait in x[] as coded (before the
// wasted-bits shift), their low words there and their 33rd bits in `hi` (bit j: sample i-1-j); a
// sample that leaves the window is FINISHED in place:
//   mid == nullptr  left/side, side/right: x[i] = the low word of the side.  The finish kernels
//                   form left - side / side + right modulo 2^32, and the true result fits 32 bits.
//   mid != nullptr  mid/side needs all 33 bits of the side (side >> 1), so the lane that has both
//                   rows undoes the decorrelation itself (decode.rs:1598-1602): mid[i] becomes left,
//                   x[i] right, and the caller records the frame as two independent channels.
__device__ __forceinline__ int64_t wide_sample(int32_t lo, uint32_t bit32) {
    return (int64_t)(((uint64_t)(0u - (bit32 & 1u)) << 32) | (uint32_t)lo);
}
__device__ __forceinline__ void wide_finish(int32_t *x, int32_t *mid, uint32_t i, int64_t coded, uint32_t wasted) {
    const int64_t s = (int64_t)((uint64_t)coded << wasted);
    if (mid) {
        const int64_t sum = (int64_t)mid[i] * 2 + (s & 1);
        mid[i] = (int32_t)((sum + s) >> 1);
        x[i] = (int32_t)((sum - s) >> 1);
    } else {
        x[i] = (int32_t)s;
    }
}
__device__ __forceinline__ bool decode_subframe_wide(BitReader &r, uint32_t type, uint32_t wasted, uint32_t n,
                                                     int32_t *x, uint32_t end_bit, int32_t *mid) {
    const uint32_t eb = 33 - wasted;
    if (type == 0) {  // CONSTANT
        const int64_t v = r.get_wide(eb);
        for (uint32_t i = 0; i < n; i++) wide_finish(x, mid, i, v, wasted);
        return true;
    }
    if (type == 1) {  // VERBATIM
        for (uint32_t i = 0; i < n; i++) {
            wide_finish(x, mid, i, r.get_wide(eb), wasted);
            if (r.pos() > end_bit) return false;
        }
        return true;
    }
    if (!((type >= 8 && type <= 12) || type >= 32)) return false;
    const bool lpc = type >= 32;
    const uint32_t order = lpc ? type - 31 : type - 8;
    if (order > n) return false;
    uint32_t hi = 0;
    for (uint32_t i = 0; i < order; i++) {  // warm-up
        const int64_t v = r.get_wide(eb);
        x[i] = (int32_t)v;
        hi = (hi << 1) | ((uint32_t)(v >> 32) & 1u);
        if (r.pos() > end_bit) return false;
    }
    int32_t coef[32];
    uint32_t shift = 0;
    if (lpc) {
        const uint32_t prec = r.get(4) + 1;
        const int32_t sh = r.get_signed(5);
        if (prec == 16 || sh < 0) return false;
        shift = (uint32_t)sh;
#pragma unroll
        for (int j = 0; j < 32; j++) {
            coef[j] = 0;
            if ((uint32_t)j < order) coef[j] = r.get_signed(prec);
        }
    } else {
        const int32_t fc[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
#pragma unroll
        for (int j = 0; j < 32; j++) coef[j] = j < 4 ? fc[order][j] : 0;
    }
    const uint32_t method = r.get(2);
    if (method > 1) return false;
    const uint32_t hb = method ? 5u : 4u, esc = method ? 31u : 15u;
    const uint32_t po = r.get(4);
    const uint32_t plen = n >> po;
    if (plen < order || (plen << po) != n) return false;
    uint32_t i = order;
    for (uint32_t part = 0; part < (1u << po); part++) {
        const uint32_t k = r.get(hb);
        const bool escaped = k == esc;
        const uint32_t ebits = escaped ? r.get(5) : 0u;
        for (uint32_t cnt = plen - (part ? 0u : order); cnt; cnt--, i++) {
            if (r.pos() > end_bit) return false;
            int32_t res;
            if (escaped) {
                res = r.get_signed(ebits);
            } else {
                const uint32_t u = r.rice(k, 1u << k, end_bit);
                res = (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
            }
            int64_t s = 0;
#pragma unroll
            for (int j = 0; j < 32; j++)
                if ((uint32_t)j < order) s += (int64_t)coef[j] * wide_sample(x[i - 1 - j], hi >> j);
            const int64_t v = res + (s >> shift);
            if (i >= 32) wide_finish(x, mid, i - 32, wide_sample(x[i - 32], hi >> 31), wasted);
            x[i] = (int32_t)v;
            hi = (hi << 1) | ((uint32_t)(v >> 32) & 1u);
        }
    }
    for (uint32_t j = n > 32 ? n - 32 : 0; j < n; j++) wide_finish(x, mid, j, wide_sample(x[j], hi >> (n - 1 - j)), wasted);
    return r.pos() <= end_bit;
}

// One subframe (read_subframe, decode.rs:1635-1752) at the reader's position: header, wasted bits,
// CONSTANT / VERBATIM / FIXED / LPC body; n samples to x[].  Returns false when it does not parse.
// sbps == 33 goes to decode_subframe_wide; `mid` (then only): the mid channel's row of a mid/side frame.
template <int MAXO>
__device__ __forceinline__ bool decode_subframe(BitReader &r, uint32_t sbps, uint32_t n, int32_t *__restrict__ x,
                                                uint32_t end_bit, int32_t *mid = nullptr) {
    bool bad = false;
    // SubframeHeader, stream.rs:1375-1388
    if (r.get(1)) bad = true;
    const uint32_t type = r.get(6);
    uint32_t wasted = 0;
    if (r.get(1)) wasted = r.unary1(end_bit) + 1;
    const uint32_t eb = sbps - wasted;
    if (wasted >= sbps) {
        bad = true;
    } else if (sbps > 32) {
        if (bad || !decode_subframe_wide(r, type, wasted, n, x, end_bit, mid)) bad = true;
    } else if (type == 0) {  // CONSTANT
        const int32_t v = (int32_t)((uint32_t)r.get_signed(eb) << wasted);
        for (uint32_t i = 0; i < n; i++) x[i] = v;
    } else if (type == 1) {  // VERBATIM
        for (uint32_t i = 0; i < n; i++) {
            x[i] = (int32_t)((uint32_t)r.get_signed(eb) << wasted);
            if (r.pos() > end_bit) { bad = true; break; }
        }
    } else if ((type >= 8 && type <= 12) || type >= 32) {
        // FIXED (decode.rs:1683-1702) is LPC with binomial coefficients and shift 0
        const bool lpc = type >= 32;
        const uint32_t order = lpc ? type - 31 : type - 8;
        if (order > n || order > (uint32_t)MAXO) {
            bad = true;
        } else {
            int32_t h[MAXO], coef[MAXO];
#pragma unroll
            for (int j = 0; j < MAXO; j++) h[j] = 0;
#pragma unroll 1
            for (uint32_t i = 0; i < order; i++) {  // warm-up: sample i sits in ring slot i
                const int32_t v = r.get_signed(eb);
#pragma unroll
                for (int j = 0; j < MAXO; j++) h[j] = (uint32_t)j == i ? v : h[j];
            }
            uint32_t shift = 0;
            if (lpc) {  // decode.rs:1704-1736
                const uint32_t prec = r.get(4) + 1;
                if (prec == 16) bad = true;
                const int32_t sh = r.get_signed(5);
                if (sh < 0) bad = true;
                shift = (uint32_t)sh & 31;
#pragma unroll
                for (int j = 0; j < MAXO; j++) {
                    coef[j] = 0;
                    if ((uint32_t)j < order) coef[j] = r.get_signed(prec);
                }
            } else {
                const int32_t fc[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
#pragma unroll
                for (int j = 0; j < MAXO; j++) coef[j] = j < 4 ? fc[order][j] : 0;
            }
            if (!bad && !decode_residuals<MAXO>(r, coef, h, order, shift, wasted, n, x, end_bit)) bad = true;
        }
    } else {
        bad = true;
    }
    return !bad;
}
__device__ __forceinline__ uint32_t subframe_bps(uint32_t bps, uint32_t acode, uint32_t c) {
    // the side channel carries one more bit (decode.rs:1520-1628)
    return bps + (((acode == 8 && c == 1) || (acode == 9 && c == 0) || (acode == 10 && c == 1)) ? 1u : 0u);
}
// mid/side at 32 bits: the lane that decodes the 33-bit side also undoes the decorrelation (decode_subframe_wide),
// and the frame goes to the finish kernel as two independent channels
__device__ __forceinline__ bool wide_mid_side(uint32_t bps, uint32_t acode) { return bps == 32 && acode == 10; }

// Verifier of this encoder's own output: one lane per SUBFRAME, starting where the plan says.
template <int MAXO>
__global__ void __launch_bounds__(64) k_decode(Params p, PackParams q, int32_t *__restrict__ out,
                                               uint32_t *verify_counts) {
    const uint32_t unit = blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= p.n_frames * p.channels) return;
    const uint32_t frame = unit / p.channels, c = unit % p.channels;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(q.out_words);
    const uint64_t start_byte = q.frame_off[frame];
    const uint32_t end_bit = (uint32_t)(q.frame_off[frame + 1] - start_byte) * 8;  // positions: frame-relative
    BitReader r;
    r.init(q.out_words, start_byte, q.cap_bytes, 0);
    FrameHead fh;
    bool bad = !parse_frame_header(r, bytes, start_byte, fh);   // every lane of the frame reads it
    const uint32_t n = fh.n, acode = fh.acode;
    const uint32_t bps = bps_of_code(fh.bps_code, p.bps);
    const uint32_t nch = acode < 8 ? acode + 1 : 2;
    if (n != frame_len(p, frame) || bps != p.bps || nch != p.channels || fh.blocking) bad = true;
    // not this encoder's output (it keeps 32-bit stereo independent), and no lane here holds both rows
    if (wide_mid_side(bps, acode)) bad = true;
    // Where this subframe is said to start and end.  The chain is closed below: subframe 0 starts
    // where the header ends, every subframe must end exactly where the next one is said to start,
    // and the last one where the padding + CRC-16 begin -- which is what a decoder walking the
    // frame front to back would have found.
    const SubPlan *plans = p.out_plan + (size_t)frame * p.channels;
    uint64_t start64 = r.pos();
    for (uint32_t k = 0; k < c; k++) start64 += plans[k].bits;
    const uint64_t stop64 = start64 + plans[c].bits;
    if (stop64 > end_bit) bad = true;
    const uint32_t start = (uint32_t)start64, stop = (uint32_t)stop64;
    if (c > 0 && !bad) {
        r.init(q.out_words, start_byte + (start >> 3), q.cap_bytes, start & ~7u);
        r.skip(start & 7);
    }
    int32_t *__restrict__ x = out + ((size_t)frame * p.channels + c) * p.ldb;
    if (!bad && !decode_subframe<MAXO>(r, subframe_bps(bps, acode, c), n, x, end_bit)) bad = true;
    if (!bad) {
        if (r.pos() != stop) bad = true;
        // byte alignment + CRC-16 must end the frame exactly
        if (c + 1 == nch && ((stop + 7) & ~7u) + 16 != end_bit) bad = true;
    }
    const uint32_t code = (bad ? 0x100u : 0u) | (c == 0 ? acode : 0u);
    if (code) atomicOr(&verify_counts[4 + frame], code);
}

// Stand-alone decoder (any FLAC stream whose frame starts a scan has found): one lane per FRAME
// walks its subframes front to back (read_frame / read_subframes, decode.rs:1388-1436, 1494-1633);
// frames run in parallel.  frame_n[f]: the block size the scan read from the header.
struct DecodeParams {
    const uint32_t *words;        // the stream's bytes as dwords
    const uint64_t *frame_off;    // [n_frames + 1] byte offsets of the frames
    const uint32_t *frame_n;      // [n_frames] samples per channel
    uint64_t cap_bytes;
    uint32_t n_frames, channels, bps, ldb;
};
template <int MAXO>
__global__ void __launch_bounds__(64) k_decode_frames(DecodeParams p, int32_t *__restrict__ out,
                                                      uint32_t *verify_counts) {
    const uint32_t frame = blockIdx.x * blockDim.x + threadIdx.x;
    if (frame >= p.n_frames) return;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(p.words);
    const uint64_t start_byte = p.frame_off[frame];
    const uint32_t end_bit = (uint32_t)(p.frame_off[frame + 1] - start_byte) * 8;
    BitReader r;
    r.init(p.words, start_byte, p.cap_bytes, 0);
    FrameHead fh;
    bool bad = !parse_frame_header(r, bytes, start_byte, fh);
    const uint32_t n = fh.n, acode = fh.acode;
    const uint32_t bps = bps_of_code(fh.bps_code, p.bps);
    const uint32_t nch = acode < 8 ? acode + 1 : 2;
    if (n != p.frame_n[frame] || n > p.ldb || bps != p.bps || nch != p.channels) bad = true;
    for (uint32_t c = 0; c < nch && !bad; c++) {
        int32_t *__restrict__ x = out + ((size_t)frame * p.channels + c) * p.ldb;
        int32_t *mid = (c == 1 && wide_mid_side(bps, acode)) ? x - p.ldb : nullptr;
        if (!decode_subframe<MAXO>(r, subframe_bps(bps, acode, c), n, x, end_bit, mid)) bad = true;
    }
    // zero padding to a byte, then the CRC-16 ends the frame exactly
    if (!bad && ((r.pos() + 7) & ~7u) + 16 != end_bit) bad = true;
    if (!bad && (r.pos() & 7) && r.get(8 - (r.pos() & 7)) != 0) bad = true;
    verify_counts[4 + frame] = (bad ? 0x100u : 0u) | (wide_mid_side(bps, acode) ? 1u : acode);
}

// Undo the stereo decorrelation (decode.rs:1520-1628) and compare with the expected PCM: one
// workgroup per frame, coalesced.
// (frame_n != nullptr: per-frame lengths of a foreign stream instead of frame_len(p, frame))
__global__ void __launch_bounds__(WG) k_decode_finish(Params p, int32_t *__restrict__ out,
                                                      const int32_t *__restrict__ expect,
                                                      uint32_t *verify_counts, const uint32_t *frame_n) {
    __shared__ uint64_t scratch[4];
    const uint32_t frame = blockIdx.x;
    const uint32_t code = verify_counts[4 + frame], acode = code & 0xFFu;
    if (code & 0x100u) {  // one of the frame's subframes (or its header) did not parse
        if (threadIdx.x == 0) atomicAdd(&verify_counts[0], 1u);
        return;
    }
    const uint32_t n = frame_n ? frame_n[frame] : frame_len(p, frame);
    int32_t *rows = out + (size_t)frame * p.channels * p.ldb;
    const int32_t *e = expect ? expect + (size_t)frame * p.channels * p.ldb : nullptr;
    uint32_t diff = 0;
    if (acode >= 8) {
        int32_t *c0 = rows, *c1 = rows + p.ldb;
        for (uint32_t i = threadIdx.x; i < n; i += WG) {
            const long long a = c0[i], b = c1[i];
            long long l, rr;
            if (acode == 8) { l = a; rr = a - b; }
            else if (acode == 9) { l = a + b; rr = b; }
            else {
                const long long sum = a * 2 + ((b < 0 ? -b : b) & 1);
                l = (sum + b) >> 1;
                rr = (sum - b) >> 1;
            }
            c0[i] = (int32_t)l;
            c1[i] = (int32_t)rr;
            if (e) diff += ((int32_t)l != e[i]) + ((int32_t)rr != e[p.ldb + i]);
        }
    } else if (e) {
        for (uint32_t c = 0; c < p.channels; c++)
            for (uint32_t i = threadIdx.x; i < n; i += WG) diff += rows[(size_t)c * p.ldb + i] != e[(size_t)c * p.ldb + i];
    }
    if (!e) return;
    const uint64_t total = block_sum_u64(diff, scratch);
    if (threadIdx.x == 0 && total) {
        atomicAdd(&verify_counts[2], 1u);
        atomicAdd(&verify_counts[3], (uint32_t)total);
    }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
