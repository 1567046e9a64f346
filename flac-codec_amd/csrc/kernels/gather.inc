// gather.inc -- the batch decoder's second front door (DESIGN.md 4b "Device-resident input"): streams that already lie
// in device memory.  Included inside decode_many.hip's anonymous namespace, after frame_scan.inc (ScanSlot,
// slot_of_block), kernels/meta_walk.h and kernels/byte_shift.h.  Three kernels, none with LDS, atomics or scratch:
//   K_g1 k_meta_walk     lane per stream: the metadata chain of a regular stream, walked where it lies (meta_walk)
//   K_g2 k_gather_slots  lane per 16-byte group of the batch buffer: builds the slots from the sources, zero tails and
//                        look-ahead included -- the device's stand-in for the host door's staging copy and upload
//   K_g3 k_cand_heads    lane per candidate of a raw scan: the 16 bytes at the candidate, for the host walk's records

// one stream as the caller handed it over
struct DevSource {
    const uint8_t *data;   // device memory, any alignment; null: no bytes
    uint64_t len;
};

// K_g1: lane per stream.  A serial walk of a few dependent byte loads per metadata block; the batch's streams run
// side by side.  Reads bytes of [data, data + len) alone (meta_walk).
__global__ void __launch_bounds__(64) k_meta_walk(const DevSource *__restrict__ src, uint32_t n, MetaRecord *__restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    meta_walk(src[i].data, src[i].len, out[i]);
}

// pick4, shift_group, keep_bytes: kernels/byte_shift.h (shared with k_place_runs)

// K_g2: lane per destination 16-byte group; consecutive lanes store consecutive groups, one uint4 each.  `src[s]` is
// the first byte of slot s's region in the caller's memory.  Every byte of the n_groups groups is written: the region's
// bytes, zeros from the region's end to the next slot's base, and zeros in the look-ahead behind the last slot (the
// groups from block n_blocks on) -- the buffer is reused between scans and never cleared as a whole.
// What is loaded: with p = src + (the group's offset in the region) and a = p mod 16, the aligned 16-byte group at
// p - a, which holds the region's byte p; and, when a != 0 and the region reaches it, the aligned group behind it,
// which holds the region's byte p + 16 - a.  So the kernel loads only aligned 16-byte groups that contain at least one
// byte of [src, src + len): such a group cannot leave the page of that byte, and a group that lies wholly outside the
// region is never read.  A destination group behind the region's end loads nothing.
__global__ void __launch_bounds__(WG) k_gather_slots(uint8_t *__restrict__ bytes, const ScanSlot *__restrict__ slots,
                                                      const uint8_t *const *__restrict__ src, uint32_t n_slots,
                                                      uint64_t n_blocks, uint64_t n_groups) {
    const uint64_t g = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (g >= n_groups) return;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    const uint64_t b = g / 4;
    if (b < n_blocks) {
        const uint32_t s = slot_of_block(slots, n_slots, b);
        const uint64_t rel = g * 16 - slots[s].base, len = slots[s].len;
        if (rel < len) {
            const uint8_t *p = src[s] + rel;
            const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
            const uint4 *grp = reinterpret_cast<const uint4 *>(p - a);
            const uint4 lo = grp[0];   // holds p, a byte of the region
            uint4 hi = make_uint4(0u, 0u, 0u, 0u);
            if (a && rel + (16u - a) < len) hi = grp[1];   // holds p + 16 - a, a byte of the region
            v = shift_group(lo, hi, a);
            const int64_t left = len - rel >= 16 ? 16 : (int64_t)(len - rel);   // region bytes in this group
            v.x = keep_bytes(v.x, left);
            v.y = keep_bytes(v.y, left - 4);
            v.z = keep_bytes(v.z, left - 8);
            v.w = keep_bytes(v.w, left - 12);
        }
    }
    reinterpret_cast<uint4 *>(bytes)[g] = v;
}

// K_g3: lane per candidate.  head[c] = the 16 bytes at cand_pos[c]: a frame header is at most kMaxHeaderBytes = 16 bytes
// (2 sync, 2 codes, a number of at most 7, a block size of at most 2, a sample rate of at most 2, the CRC-8 --
// scan_parse_header's header_bytes), and the host walk reads nothing of a kept frame but its header.  Loaded as the five
// aligned dwords from cand_pos & ~3: at most 19 bytes behind the candidate, inside the slot's zero tail.
constexpr uint32_t kMaxHeaderBytes = 2 + 2 + 7 + 2 + 2 + 1;
constexpr uint32_t kHeadBytes = 16;
static_assert(kMaxHeaderBytes <= kHeadBytes, "a candidate's head holds its whole header");
__global__ void __launch_bounds__(WG) k_cand_heads(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ cand_pos,
                                                    uint32_t n_cand, uint4 *__restrict__ head) {
    const uint32_t c = blockIdx.x * WG + threadIdx.x;
    if (c >= n_cand) return;
    const uint64_t pos = cand_pos[c];
    const uint32_t *w = reinterpret_cast<const uint32_t *>(bytes + (pos & ~(uint64_t)3));
    const uint32_t r = (uint32_t)(pos & 3u);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    uint4 v;
    v.x = __builtin_amdgcn_alignbyte(w1, w0, r);
    v.y = __builtin_amdgcn_alignbyte(w2, w1, r);
    v.z = __builtin_amdgcn_alignbyte(w3, w2, r);
    v.w = __builtin_amdgcn_alignbyte(w4, w3, r);
    head[c] = v;
}
