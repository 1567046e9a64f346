// meta_feed_rule.h -- meta_walk (kernels/meta_walk.h) in a resumable form: the metadata chain of a FLAC stream taken
// chunk by chunk, cut anywhere (DESIGN.md 4b "Container sessions").  One set of functions for the host
// (flacgpu_meta_feed_host, the host container session) and the device (k_meta_feed, kernels/session.inc: chunks that
// already lie in device memory), so that the rule is tested without a GPU.  The state is a few words and two STREAMINFO
// images, whatever the chain's length: a block that is not a STREAMINFO is passed by count, never buffered.
// meta_feed reads bytes of [chunk, chunk + len) alone, one at a time, and none of a block it passes over.
// meta_feed_record turns a state into the MetaRecord meta_walk gives for the concatenation of everything fed.
#ifndef FLACGPU_META_FEED_RULE_H
#define FLACGPU_META_FEED_RULE_H
#include "meta_walk.h"

constexpr uint32_t MF_MARKER = 0;    // inside the fLaC marker: `have` of its 4 bytes matched
constexpr uint32_t MF_HEADER = 1;    // inside a block header: `have` of its 4 bytes are in `head`
constexpr uint32_t MF_SKIP = 2;      // inside a block that is passed over: `left` bytes of it to come
constexpr uint32_t MF_SI = 3;        // inside a STREAMINFO block: `have` of its 34 bytes are in `cur`
constexpr uint32_t MF_DONE = 4;      // the block with the last flag is complete: `taken` is frames_at
constexpr uint32_t MF_REFUSED = 5;   // a wrong marker: sticky

struct MetaFeed {                     // 104 bytes
    uint32_t phase;                   // MF_*
    uint32_t have;
    uint64_t left;
    uint64_t taken;                   // bytes of the chain consumed since the stream's first byte
    uint32_t status;                  // META_HAVE_SI: `si` holds a whole STREAMINFO (the last one seen whole)
    uint8_t head[4];
    uint8_t si[kStreamInfoBytes];
    uint8_t cur[kStreamInfoBytes];    // the STREAMINFO block under way: it wins only once it is whole, as in meta_walk
    uint8_t pad[4];
};
static_assert(sizeof(MetaFeed) == 104, "MetaFeed is a table row shared by the device and the host");

FLACGPU_MW void meta_feed_init(MetaFeed &m) {
    m.phase = MF_MARKER;
    m.have = 0;
    m.left = m.taken = 0;
    m.status = 0;
    for (uint32_t i = 0; i < 4; i++) m.head[i] = m.pad[i] = 0;
    for (uint32_t i = 0; i < kStreamInfoBytes; i++) m.si[i] = m.cur[i] = 0;
}

// the block under way is complete: the walk is through behind the one with the last flag
FLACGPU_MW void meta_feed_block_end(MetaFeed &m) {
    m.phase = (m.head[0] & 0x80u) ? MF_DONE : MF_HEADER;
    m.have = 0;
}

// One chunk.  Returns the bytes of it the walk consumed: all of them while the chain goes on (and of a refused stream,
// whose bytes are ignored), those up to the end of the block with the last flag when it ends in this chunk, 0 when the
// chain was through already.
FLACGPU_MW uint64_t meta_feed(MetaFeed &m, const uint8_t *chunk, uint64_t len) {
    if (m.phase == MF_DONE || !chunk) return 0;
    if (m.phase == MF_REFUSED) return len;
    uint64_t i = 0;
    while (i < len && m.phase != MF_DONE) {
        if (m.phase == MF_MARKER) {
            const uint8_t want = m.have == 0 ? 'f' : m.have == 1 ? 'L' : m.have == 2 ? 'a' : 'C';
            if (chunk[i] != want) {
                m.phase = MF_REFUSED;
                return len;
            }
            i++;
            if (++m.have == 4) {
                m.phase = MF_HEADER;
                m.have = 0;
            }
        } else if (m.phase == MF_HEADER) {
            m.head[m.have] = chunk[i++];
            if (++m.have < 4) continue;
            m.left = (uint64_t)m.head[1] << 16 | (uint64_t)m.head[2] << 8 | m.head[3];
            m.have = 0;
            m.phase = (m.head[0] & 0x7Fu) == 0 && m.left == kStreamInfoBytes ? MF_SI : MF_SKIP;
            if (!m.left) meta_feed_block_end(m);
        } else if (m.phase == MF_SKIP) {
            const uint64_t n = len - i < m.left ? len - i : m.left;
            i += n;
            m.left -= n;
            if (!m.left) meta_feed_block_end(m);
        } else {   // MF_SI
            m.cur[m.have] = chunk[i++];
            if (++m.have < kStreamInfoBytes) continue;
            for (uint32_t k = 0; k < kStreamInfoBytes; k++) m.si[k] = m.cur[k];
            m.status |= META_HAVE_SI;
            m.left = 0;
            meta_feed_block_end(m);
        }
    }
    m.taken += i;
    return i;
}

// meta_walk's record for the `total` bytes fed so far, seen as a whole input
FLACGPU_MW void meta_feed_record(const MetaFeed &m, uint64_t total, MetaRecord &r) {
    r.status = r.reserved = 0;
    r.frames_at = 0;
    for (uint32_t i = 0; i < kStreamInfoBytes; i++) r.si[i] = 0;
    for (uint32_t i = 0; i < 6; i++) r.pad[i] = 0;
    if (m.phase == MF_REFUSED || m.phase == MF_MARKER || total < 42) return;
    r.status = META_MARKER | (m.status & META_HAVE_SI);
    if (m.status & META_HAVE_SI)
        for (uint32_t i = 0; i < kStreamInfoBytes; i++) r.si[i] = m.si[i];
    if (m.phase == MF_DONE) {
        r.status |= META_COMPLETE;
        r.frames_at = m.taken;
    }
}
#endif
