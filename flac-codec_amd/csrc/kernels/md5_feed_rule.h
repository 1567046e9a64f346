// md5_feed_rule.h -- the rule of the resumable MD5 chains (kernels/md5_chain.inc, md5_chain.hip; DESIGN.md 4c "Sessions"):
// how a piece of int32 samples, appended to a chain that already holds up to 63 buffered message bytes, becomes 64-byte
// blocks, what stays in the buffer, and the padding.  One set of functions for the device (k_md5_chain, k_md5_chain_final)
// and the host (flacgpu_md5_feed_host, flacgpu_md5_final_host), so that the rule is tested without a GPU.  Compiles as
// plain C++ too (the stand-alone sanitizer program of tests/test_md5_chain_host.py).
//   * A chain is {h[4], len, buf[64]}: the state after every whole block so far, the message bytes so far, and the
//     fill = len % 64 bytes behind the last whole block.
//   * One feed of `count` samples of `width` bytes sees the VIRTUAL STRING  V = buf[0, fill) || sample bytes, T = fill +
//     count * width bytes long, whose byte 0 is the first byte of the chain's open block.  Byte b (< width) of sample e
//     -- bits [8b, 8b + 8) of the int32, which is the mask of k_md5_many -- stands at V[fill + e * width + b]: that one
//     line is where width 3 splits a sample across words and blocks, and where the buffered bytes shift everything behind
//     them (md5_feed_scatter).
//   * V is taken in WINDOWS of MD5_STAGE_BYTES (a multiple of 64): window r is V[r * STAGE, min((r + 1) * STAGE, T)).  The
//     samples that own a byte of a window are [md5_feed_first, md5_feed_end); each puts the bytes it owns INSIDE the
//     window there and no other (a sample on a window's edge is looked at for both windows).  The whole 64-byte blocks of a
//     window are hashed in order; only the last window can end with T % 64 bytes over, and those are the new buffer.
//   * Padding (md5_chain_final): 0x80, zeros to 56 mod 64, the bit length as 64 little-endian bits -- one block when
//     fill < 56, else two -- built word by word from the buffer with constant indices (md5_pad_word), and the chain is back
//     at its initial state.
#ifndef FLACGPU_MD5_FEED_RULE_H
#define FLACGPU_MD5_FEED_RULE_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLACGPU_MD5_HD __host__ __device__
#else
#define FLACGPU_MD5_HD
#endif

constexpr uint32_t MD5_STAGE_BYTES = 1024;   // a window: 16 blocks (flacgpu_md5_stage_bytes)

struct alignas(8) Md5Chain {
    uint32_t h[4];
    uint64_t len;       // message bytes so far
    uint8_t buf[64];    // the first len % 64 hold the bytes behind the last whole block
};
static_assert(sizeof(Md5Chain) == 88, "Md5Chain is the 88-byte flacgpu_md5_state");

FLACGPU_MD5_HD inline void md5_chain_init(Md5Chain &c) {
    c.h[0] = 0x67452301u; c.h[1] = 0xefcdab89u; c.h[2] = 0x98badcfeu; c.h[3] = 0x10325476u;
    c.len = 0;
}

// ---- one block (RFC 1321): md5_block's arithmetic (kernels/decode_many.inc), a copy so that that file stays as it is ----
struct Md5RuleConsts {
    uint32_t k[64];
    constexpr Md5RuleConsts() : k() {
        const uint32_t t[64] = {
            0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
            0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
            0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
            0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
            0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
            0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
            0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
            0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
        for (int i = 0; i < 64; i++) k[i] = t[i];
    }
};
constexpr Md5RuleConsts kMd5Rule = Md5RuleConsts();
FLACGPU_MD5_HD inline void md5_rule_block(uint32_t (&s)[4], const uint32_t (&m)[16]) {
    constexpr int R[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        uint32_t f;
        int g;
        if (i < 16) { f = (b & c) | (~b & d); g = i; }
        else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
        else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
        else { f = c ^ (b | ~d); g = (7 * i) & 15; }
        const uint32_t t = a + f + kMd5Rule.k[i] + m[g];
        const int r = R[i >> 4][i & 3];
        a = d;
        d = c;
        c = b;
        b = b + ((t << r) | (t >> (32 - r)));
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d;
}

// ---- the virtual string ----
FLACGPU_MD5_HD inline uint32_t md5_feed_fill(uint64_t len) { return (uint32_t)(len & 63u); }
// the first sample that owns a byte of V[lo, ...), and the end of the samples that own a byte of V[..., hi)
FLACGPU_MD5_HD inline uint64_t md5_feed_first(uint64_t lo, uint32_t fill, uint32_t width) {
    return lo <= fill ? 0 : (lo - fill) / width;
}
FLACGPU_MD5_HD inline uint64_t md5_feed_end(uint64_t hi, uint32_t fill, uint32_t width, uint64_t count) {
    const uint64_t e = hi <= fill ? 0 : (hi - fill + width - 1) / width;
    return e < count ? e : count;
}
// sample e (value v) into the window V[lo, lo + len) that `win` holds: its bytes inside the window, no other
FLACGPU_MD5_HD inline void md5_feed_scatter(uint8_t *win, uint64_t lo, uint32_t len, uint32_t fill, uint32_t width,
                                            uint64_t e, uint32_t v) {
    const uint64_t pos = fill + e * width;
#pragma unroll
    for (uint32_t b = 0; b < 4u; b++) {
        const uint64_t p = pos + b;
        if (b < width && p >= lo && p - lo < len) win[p - lo] = (uint8_t)(v >> (8u * b));
    }
}

// ---- the padding ----
// word k of the block that holds the 0x80: w is word k of the buffer, fill (< 64) its valid bytes
FLACGPU_MD5_HD inline uint32_t md5_pad_word(uint32_t w, uint32_t k, uint32_t fill) {
    if (4u * k + 4u <= fill) return w;
    if (4u * k > fill) return 0u;
    const uint32_t keep = fill - 4u * k;   // 0..3 bytes of the word are data
    return (w & ((1u << (8u * keep)) - 1u)) | (0x80u << (8u * keep));
}
// digest = MD5 of everything fed; the chain goes back to its initial state.  bufw: the buffer as 16 little-endian words.
FLACGPU_MD5_HD inline void md5_chain_final(uint32_t (&h)[4], uint64_t len, const uint32_t (&bufw)[16], uint32_t (&digest)[4]) {
    const uint32_t fill = md5_feed_fill(len);
    const uint64_t bits = len * 8u;
    uint32_t m[16];
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) m[k] = md5_pad_word(bufw[k], k, fill);
    if (fill >= 56u) {   // no room for the length: it goes into a block of its own
        md5_rule_block(h, m);
#pragma unroll
        for (uint32_t k = 0; k < 14u; k++) m[k] = 0u;
    }
    m[14] = (uint32_t)bits;
    m[15] = (uint32_t)(bits >> 32);
    md5_rule_block(h, m);
#pragma unroll
    for (int k = 0; k < 4; k++) digest[k] = h[k];
}

// ---- the host's pass: window after window as k_md5_chain takes them, one "lane" after another ----
inline void md5_feed_host(Md5Chain &c, const int32_t *samples, uint64_t count, uint32_t width) {
    if (!count) return;
    const uint32_t fill = md5_feed_fill(c.len);
    const uint64_t T = fill + count * width;
    uint8_t win[MD5_STAGE_BYTES];
    for (uint64_t lo = 0; lo < T; lo += MD5_STAGE_BYTES) {
        const uint32_t len = (uint32_t)(T - lo < MD5_STAGE_BYTES ? T - lo : MD5_STAGE_BYTES);
        if (!lo) memcpy(win, c.buf, fill);
        const uint64_t e1 = md5_feed_end(lo + len, fill, width, count);
        for (uint64_t e = md5_feed_first(lo, fill, width); e < e1; e++)
            md5_feed_scatter(win, lo, len, fill, width, e, (uint32_t)samples[e]);
        const uint32_t blocks = len / 64u;
        for (uint32_t b = 0; b < blocks; b++) {
            uint32_t m[16];
            memcpy(m, win + 64u * b, 64);
            md5_rule_block(c.h, m);
        }
        if (len % 64u) memcpy(c.buf, win + 64u * blocks, len % 64u);   // (the last window only)
    }
    c.len += count * width;
}
inline void md5_final_host(Md5Chain &c, uint8_t md5[16]) {
    uint32_t bufw[16] = {0}, digest[4];
    memcpy(bufw, c.buf, md5_feed_fill(c.len));
    md5_chain_final(c.h, c.len, bufw, digest);
    memcpy(md5, digest, 16);
    md5_chain_init(c);
}
#endif
