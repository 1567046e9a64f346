// session.inc -- the kernels of the decoder sessions (DESIGN.md 4b "Decoder sessions"): raw frame streams that arrive
// chunk by chunk; behind them the two of a container session (whole .flac files; "Container sessions").  Included inside
// decode_many.hip's anonymous namespace, after frame_scan.inc (ScanSlot, ScanParams, slot_of_block), gather.inc
// (kHeadBytes, DevSource), kernels/session_slots_rule.h and kernels/meta_feed_rule.h.  No kernel here has LDS, atomics or
// scratch:
//   K_n1 k_session_slots  lane per 16-byte group of the batch buffer: slot = the stream's held tail (in the session's
//                         other batch buffer) followed by its new chunk, zero tails and look-ahead included
//   K_n2 k_link_session   lane per candidate: the raw end rule bounded by W = max_frame_bytes, with "not decided yet"

// K_n1: lane per destination 16-byte group; consecutive lanes store consecutive groups, one uint4 each.  Every byte of
// the n_groups groups is written, as k_gather_slots does: the buffer is reused and never cleared as a whole.  What is
// loaded, and the junction of tail and chunk inside one group: kernels/session_slots_rule.h.
__global__ void __launch_bounds__(WG) k_session_slots(uint8_t *__restrict__ bytes, const ScanSlot *__restrict__ slots,
                                                       const SessionSrc *__restrict__ src, uint32_t n_slots,
                                                       uint64_t n_blocks, uint64_t n_groups) {
    const uint64_t g = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (g >= n_groups) return;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    const uint64_t b = g / 4;
    if (b < n_blocks) {
        const uint32_t s = slot_of_block(slots, n_slots, b);
        v = session_group(src[s], g * 16 - slots[s].base);
    }
    reinterpret_cast<uint4 *>(bytes)[g] = v;
}

// what a session says about a slot, beside ScanSlot (whose layout the scan kernels keep)
struct SessionSlot {
    uint32_t final;   // 1: the stream is flushed with this feed -- the slot's end is an end of input
    uint32_t W;       // max_frame_bytes: no frame is longer
};
constexpr int32_t LINK_HOLD = -3;   // not decided yet: the walk stops here and the bytes from here on are held

// K_n2: lane per candidate s of a slot of L bytes.  k_link_raw's rule with two changes.  An end e must have e - s <= W.
// And in a slot that is not final only the positions q <= L - kHeadBytes are candidates yet (a header may need the 16
// bytes from q on): s itself behind that is LINK_HOLD; a later candidate behind that ends nothing; the slot's end ends
// nothing; and s without an end is passed over (LINK_NONE) only when every position up to s + W has been judged,
// L - kHeadBytes >= s + W, else it is LINK_HOLD.  A final slot: LINK_END as k_link_raw, within W.
__global__ void __launch_bounds__(WG) k_link_session(ScanParams p, const SessionSlot *__restrict__ info) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= p.n_cand) return;
    const uint32_t s = p.cand_slot[i];
    const ScanSlot sl = p.slots[s];
    const SessionSlot si = info[s];
    const uint32_t end = s + 1 < p.n_slots ? p.slot_cand0[s + 1] : p.n_cand;
    const uint64_t pos = p.cand_pos[i];
    // the first byte behind the judged positions
    const uint64_t judged = si.final ? sl.base + sl.len : sl.base + (sl.len >= kHeadBytes ? sl.len - kHeadBytes + 1 : 0);
    if (pos >= judged) {
        p.link[i] = LINK_HOLD;
        return;
    }
    const uint32_t hb = (p.cand_info[i] >> 16) & 0xFFu;
    const uint32_t acode = p.bytes[pos + 3] >> 4;
    const uint64_t min_len = hb + 2u + (acode < 8 ? acode + 1u : 2u);
    const uint32_t A = p.cand_crc[i];
    int32_t link = LINK_NONE;
    for (uint32_t j = i + 1; j < end; j++) {
        const uint64_t q = p.cand_pos[j];
        if (q >= judged || q - pos > si.W) break;   // ascending: nothing behind it can end s either
        if (p.cand_crc[j] != A || q - pos < min_len) continue;
        link = (int32_t)j;
        break;
    }
    if (link == LINK_NONE) {
        const uint64_t left = sl.base + sl.len - pos;
        if (si.final) {
            if (left >= 2 && left <= si.W && p.slot_pend[s] == A) link = LINK_END;
        } else if (left < (uint64_t)si.W + kHeadBytes) {
            link = LINK_HOLD;
        }
    }
    p.link[i] = link;
}

// ---- container sessions (DESIGN.md 4b "Container sessions"): regular .flac streams chunk by chunk ----
//   K_n3 k_link_container  lane per candidate: k_link's rule bounded by W, with "not decided yet"
//   K_n4 k_meta_feed       lane per stream: the resumable metadata walk over a chunk where it lies
// Neither has LDS, atomics or scratch.

// K_n3: lane per candidate s of a slot of L bytes, whose candidates are the regular scan's (K_s1: every header that
// parses).  k_link's rule -- the first later candidate q >= s + max(header_bytes + 2 + channels, min_frame), channels and
// min_frame the slot's (STREAMINFO's), with s's blocking bit and CRC(s, q) == 0 -- with k_link_session's three changes:
// q - s <= W; in a slot that is not final only the positions q <= L - kHeadBytes are judged (s behind that: LINK_HOLD, a
// later candidate behind that ends nothing, the slot's end ends nothing) and s without an end is LINK_NONE only once
// L - kHeadBytes >= s + W, else LINK_HOLD; a final slot's end is an end of input (LINK_END, within W).
__global__ void __launch_bounds__(WG) k_link_container(ScanParams p, const SessionSlot *__restrict__ info) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= p.n_cand) return;
    const uint32_t s = p.cand_slot[i];
    const ScanSlot sl = p.slots[s];
    const SessionSlot si = info[s];
    const uint32_t end = s + 1 < p.n_slots ? p.slot_cand0[s + 1] : p.n_cand;
    const uint64_t pos = p.cand_pos[i];
    const uint64_t judged = si.final ? sl.base + sl.len : sl.base + (sl.len >= kHeadBytes ? sl.len - kHeadBytes + 1 : 0);
    if (pos >= judged) {
        p.link[i] = LINK_HOLD;
        return;
    }
    const uint32_t ci = p.cand_info[i];
    const uint32_t blocking = ci >> 24, hb = (ci >> 16) & 0xFFu;
    const uint64_t min_len = max(hb + 2u + sl.channels, sl.min_frame);
    const uint32_t A = p.cand_crc[i];
    int32_t link = LINK_NONE;
    for (uint32_t j = i + 1; j < end; j++) {
        const uint64_t q = p.cand_pos[j];
        if (q >= judged || q - pos > si.W) break;   // ascending: nothing behind it can end s either
        if (p.cand_crc[j] != A || (p.cand_info[j] >> 24) != blocking || q - pos < min_len) continue;
        link = (int32_t)j;
        break;
    }
    if (link == LINK_NONE) {
        const uint64_t left = sl.base + sl.len - pos;
        if (si.final) {
            if (left >= 2 && left <= si.W && p.slot_pend[s] == A) link = LINK_END;
        } else if (left < (uint64_t)si.W + kHeadBytes) {
            link = LINK_HOLD;
        }
    }
    p.link[i] = link;
}

// K_n4: lane per stream that is still in its metadata.  state[i] is the stream's walk so far; the lane runs meta_feed
// (kernels/meta_feed_rule.h) over the stream's chunk and leaves the state and the count of consumed bytes.  A serial
// walk of a few dependent byte loads per block -- a block that is no STREAMINFO is passed by count -- and the streams
// run side by side.  Reads bytes of [data, data + len) alone; a null pointer or a zero length reads nothing.
__global__ void __launch_bounds__(64) k_meta_feed(const DevSource *__restrict__ src, uint32_t n, MetaFeed *state,
                                                  uint64_t *__restrict__ consumed) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    // on the row itself: its byte arrays are indexed by the walk's own counts, which a copy in registers cannot be
    consumed[i] = src[i].len ? meta_feed(state[i], src[i].data, src[i].len) : 0;
}
