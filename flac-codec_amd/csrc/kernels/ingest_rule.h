// ingest_rule.h -- one element of a caller's tensor (int32, int16, packed 24-bit or float32) -> the bps-bit sample the encoder reads:
// the exact inverse of sample_bits (kernels/decode_many.inc).  One function for the device (k_ingest, kernels/ingest.inc)
// and the host (flacenc_ingest_sample, host/device_batch.cpp), so that the rule is tested without a GPU.
//   lo = -2^(bps - 1), hi = 2^(bps - 1) - 1; every result lies in [lo, hi]: the analysis kernels never see a sample that
//   does not fit bps bits.
//   F32  v = x * 2^(bps - 1) (a power of two: the product is exact, or it overflows to +-inf), rounded to the nearest
//        integer, ties to even, then clamped -- on the float side, where bps == 32 and +-inf are defined: a rounded value
//        >= 2^(bps - 1) is above hi (it is an integer), one below -2^(bps - 1) is below lo.  NaN gives 0.
//   I16  x >> (16 - bps), an arithmetic shift (bps <= 16; the callers refuse anything else before a sample is looked at).
//   S24  sign_extend24(x) >> (24 - bps), an arithmetic shift (bps <= 24; refused above like I16).  Bits 24-31 of raw are
//        ignored: the kernel hands over a dword that may hold the next element's first byte.
//   I32  x clamped to [lo, hi].
// *altered = 1 when the element was clamped, was NaN or (I16, S24) had non-zero bits below the ones kept; else 0.
#ifndef FLACGPU_INGEST_RULE_H
#define FLACGPU_INGEST_RULE_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLACGPU_HD __host__ __device__
#else
#define FLACGPU_HD
#endif

constexpr uint32_t INGEST_I32 = 0, INGEST_I16 = 1, INGEST_F32 = 2, INGEST_S24 = 24;   // FLACGPU_SAMPLE_*

// raw: the element's bits in the low end of a dword (I16: the low half; S24: the low 24 bits).  1 <= bps <= 32; I16
// needs bps <= 16, S24 bps <= 24.
FLACGPU_HD inline int32_t ingest_sample(uint32_t sample_type, uint32_t raw, uint32_t bps, int *altered) {
    *altered = 0;
    if (sample_type == INGEST_F32) {
        float x, scale;
        const uint32_t scale_bits = (127u + bps - 1u) << 23;   // 2^(bps - 1)
        __builtin_memcpy(&x, &raw, 4);
        __builtin_memcpy(&scale, &scale_bits, 4);
        if (x != x) {
            *altered = 1;
            return 0;
        }
        const float r = rintf(x * scale);   // nearest, ties to even (the default rounding mode on both sides)
        if (r >= scale) {
            *altered = 1;
            return (int32_t)(((uint32_t)1 << (bps - 1u)) - 1u);
        }
        if (r < -scale) {
            *altered = 1;
            return (int32_t)(0u - ((uint32_t)1 << (bps - 1u)));
        }
        return (int32_t)r;   // an integer in [-2^31, 2^31): exact
    }
    if (sample_type == INGEST_I16) {
        const int32_t x = (int16_t)(uint16_t)raw;
        const uint32_t drop = (16u - bps) & 15u;
        *altered = (raw & ((1u << drop) - 1u)) != 0;
        return x >> drop;
    }
    if (sample_type == INGEST_S24) {
        const int32_t x = (int32_t)(raw << 8) >> 8;
        const uint32_t drop = (24u - bps) & 31u;
        *altered = (raw & ((1u << drop) - 1u)) != 0;
        return x >> drop;
    }
    const int32_t x = (int32_t)raw;
    if (bps >= 32) return x;
    const int32_t hi = (int32_t)(((uint32_t)1 << (bps - 1u)) - 1u), lo = -hi - 1;
    if (x > hi) {
        *altered = 1;
        return hi;
    }
    if (x < lo) {
        *altered = 1;
        return lo;
    }
    return x;
}
#endif
