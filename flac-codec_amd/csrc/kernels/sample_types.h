// sample_types.h -- what the host code knows about an element type (FLACGPU_SAMPLE_*) of flacgpu_out_format: one place
// for the batch decoder (decode_many.hip), the ingest pass (ingest.hip) and the device batch plan (host/device_batch.cpp).
#ifndef FLACGPU_SAMPLE_TYPES_H
#define FLACGPU_SAMPLE_TYPES_H
#include <stddef.h>
#include <stdint.h>

#include "flacenc_gpu.h"

constexpr bool sample_type_known(uint32_t t) { return t <= FLACGPU_SAMPLE_F32 || t == FLACGPU_SAMPLE_S24; }
// bytes per element; S24 elements are packed: element e starts at byte 3 * e
constexpr size_t sample_type_bytes(uint32_t t) { return t == FLACGPU_SAMPLE_I16 ? 2 : t == FLACGPU_SAMPLE_S24 ? 3 : 4; }
// what a buffer of such elements must be aligned to: the element size, and nothing for the packed 3-byte elements
constexpr size_t sample_type_align(uint32_t t) { return t == FLACGPU_SAMPLE_S24 ? 1 : sample_type_bytes(t); }
// the most bits per sample the type holds without loss of the top bits (I16, S24); 0: any width
constexpr uint32_t sample_type_max_bits(uint32_t t) { return t == FLACGPU_SAMPLE_I16 ? 16 : t == FLACGPU_SAMPLE_S24 ? 24 : 0; }
constexpr const char *sample_type_name(uint32_t t) {
    return t == FLACGPU_SAMPLE_I32   ? "int32"
           : t == FLACGPU_SAMPLE_I16 ? "int16"
           : t == FLACGPU_SAMPLE_F32 ? "float32"
           : t == FLACGPU_SAMPLE_S24 ? "packed 24-bit"
                                     : "unknown";
}
#endif
