// byte_shift.h -- 16 bytes at any byte offset of two aligned 16-byte groups, in registers: what k_gather_slots
// (kernels/gather.inc) and k_place_runs (kernels/place.inc, through kernels/place_rule.h) share.  For .hip translation
// units (uint4).  On the device the odd bytes come from v_alignbyte; the host pass of a translation unit (the copy rule
// of place_rule.h run over host memory) gets the same dword from a 64-bit shift.
#ifndef FLACGPU_BYTE_SHIFT_H
#define FLACGPU_BYTE_SHIFT_H
#include <hip/hip_runtime.h>

#include <stdint.h>

// the low dword of (hi:lo) >> 8 r, r < 4
__host__ __device__ __forceinline__ uint32_t align_byte(uint32_t hi, uint32_t lo, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (r & 3u)));
#endif
}
// 16 bytes, as four little-endian dwords, from the eight dwords w at byte offset a (< 16)
__host__ __device__ __forceinline__ uint32_t pick4(uint32_t q, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
}
// the 16 bytes at byte offset a (< 16) of the 32 bytes lo, hi, as four little-endian dwords.  Dword q + k is taken by
// selects and the odd bytes by v_alignbyte: no register is indexed by a lane's value, so nothing goes to scratch.
__host__ __device__ __forceinline__ uint4 shift_group(const uint4 lo, const uint4 hi, uint32_t a) {
    const uint32_t q = a >> 2, r = a & 3u;
    const uint32_t t0 = pick4(q, lo.x, lo.y, lo.z, lo.w), t1 = pick4(q, lo.y, lo.z, lo.w, hi.x);
    const uint32_t t2 = pick4(q, lo.z, lo.w, hi.x, hi.y), t3 = pick4(q, lo.w, hi.x, hi.y, hi.z);
    const uint32_t t4 = pick4(q, hi.x, hi.y, hi.z, hi.w);
    uint4 v;
    v.x = align_byte(t1, t0, r);
    v.y = align_byte(t2, t1, r);
    v.z = align_byte(t3, t2, r);
    v.w = align_byte(t4, t3, r);
    return v;
}
// the low `keep` (0 .. 4) bytes of a dword
__host__ __device__ __forceinline__ uint32_t keep_bytes(uint32_t v, int64_t keep) {
    return keep >= 4 ? v : keep <= 0 ? 0u : v & ((1u << (8 * (uint32_t)keep)) - 1u);
}
#endif
