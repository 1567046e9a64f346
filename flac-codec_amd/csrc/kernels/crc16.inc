// crc16.inc -- GF(2) algebra of the CRC-16 (poly 0x8005, MSB first, init 0; crc.rs:142-188): products mod P,
// the x^(512 k) / x^(544 k) weight tables and the slicing-by-4 tables.  Shared by the frame kernels (pack.inc) and
// the stand-alone decoder's frame scan (frame_scan.inc); included inside the includer's anonymous namespace.
__device__ __forceinline__ uint32_t gf_mulmod(uint32_t a, uint32_t b) {  // a*b mod P over GF(2)
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1) & 0xFFFF;
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
// the same with the slicing tables at hand (T[k][b] = b x^(16 + 8 k) mod P, in LDS): the 31-bit carry-less product first
// (sixteen masked XORs), then its high half reduced by two lookups -- about half the instructions of the bit-serial loop
// above, which every lane of the frame kernels ran two to four times per subframe
__device__ __forceinline__ uint32_t gf_mulmod_t(uint32_t a, uint32_t b, const uint16_t (*T)[256]) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) p ^= (uint32_t)(-(int32_t)((b >> i) & 1u)) & (a << i);
    const uint32_t h = p >> 16;   // 15 bits: h x^16 = (h >> 8) x^24 + (h & 255) x^16
    return (p & 0xFFFFu) ^ T[1][h >> 8] ^ T[0][h & 0xFFu];
}
constexpr uint32_t gf_mulmod_c(uint32_t a, uint32_t b) {  // compile-time a*b mod P over GF(2)
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1) & 0xFFFF;
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
// W[k] = x^(512 k) mod P: weight of a 64-byte slice that is followed by k more slices
struct CrcWeights {
    uint16_t w[WG + 1];
    constexpr CrcWeights() : w() {
        uint32_t x512 = 0x100;
        for (int i = 0; i < 6; i++) x512 = gf_mulmod_c(x512, x512);
        uint32_t v = 1;
        for (int k = 0; k <= WG; k++) {
            w[k] = (uint16_t)v;
            v = gf_mulmod_c(v, x512);
        }
    }
};
__constant__ CrcWeights kCrcW = CrcWeights();

// W17[k] = x^(544 k) mod P: weight of a 68-byte slice that is followed by k more slices
struct CrcWeights17 {
    uint16_t w[512 + 1];
    constexpr CrcWeights17() : w() {
        uint32_t x32 = 0x100;                       // x^8
        x32 = gf_mulmod_c(x32, x32);                // x^16
        x32 = gf_mulmod_c(x32, x32);                // x^32
        uint32_t x544 = 1;
        for (int i = 0; i < 17; i++) x544 = gf_mulmod_c(x544, x32);
        uint32_t v = 1;
        for (int k = 0; k <= 512; k++) {
            w[k] = (uint16_t)v;
            v = gf_mulmod_c(v, x544);
        }
    }
};
__constant__ CrcWeights17 kCrcW17 = CrcWeights17();
// slicing-by-4 tables of the CRC-16: T[k][b] = CRC state after byte b followed by k zero bytes
struct CrcTables {
    uint16_t t[4][256];
    constexpr CrcTables() : t() {
        for (int b = 0; b < 256; b++) {
            uint32_t c = (uint32_t)b << 8;
            for (int k = 0; k < 4; k++) {
                for (int i = 0; i < 8; i++) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
                t[k][b] = (uint16_t)c;
            }
        }
    }
};
__constant__ __attribute__((aligned(16))) CrcTables kCrcT = CrcTables();
