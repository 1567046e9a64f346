// plan_check.cpp -- check_plans(): see plan_check.h.  Plain C++ (no HIP headers).
#include "plan_check.h"

#include <stddef.h>

namespace flacenc_route {

namespace {
// k_sub64's four CRC rows hold the largest subframe image its launch admits (lead bits, header and guard words included)
static_assert((sub64_max_sub_bits(25u) + 128u + 64u) / 32u <= frame_crc_max_words(64u, 4u), "k_sub64: S <= 4");

PlanFault fault(uint32_t frame, uint32_t subframe, const char *field) {
    PlanFault f;
    f.bad = true;
    f.frame = frame;
    f.subframe = subframe;
    f.field = field;
    return f;
}
}  // namespace

PlanFault check_plans(const RouteContext &c, const Route &r, uint32_t n_frames, uint32_t last_len, uint64_t out_cap,
                      const flacgpu_frame_plan *plans, const flacgpu_subframe_plan *subs) {
    const uint32_t C_ = c.channels, B = c.block_size;
    const uint32_t max_po = c.max_partition_order < (uint32_t)MAXP ? c.max_partition_order : (uint32_t)MAXP;
    const uint32_t max_lpc = c.max_lpc_order < 32u ? c.max_lpc_order : 32u;
    // (launch_frame64, pack.hip: frames of 5..8 independent channels with edge records go subframe by subframe)
    const bool by_subframe = c.has_edges && B == FN && C_ >= 5 && !c.stereo4 && c.max_lpc_order <= 16;
    const uint32_t image_bits = frame_fb_max_body_bits(frame_image_words(c));
    const uint32_t crc_words = frame_crc_max_words(64u * C_);
    uint64_t total = 0;
    for (uint32_t f = 0; f < n_frames; f++) {
        const flacgpu_frame_plan &fp = plans[f];
        const uint32_t n = f + 1 == n_frames ? last_len : B;
        const bool fast = f < r.fast_pack;
        if (fp.channels != C_) return fault(f, C_, "channels");
        if (fp.block_size != n) return fault(f, C_, "block_size");
        const uint32_t a = fp.assignment;
        if (c.stereo4 ? !(a == FLACGPU_ASSIGN_INDEPENDENT || a == FLACGPU_ASSIGN_LEFT_SIDE || a == FLACGPU_ASSIGN_SIDE_RIGHT ||
                          a == FLACGPU_ASSIGN_MID_SIDE)
                      : a != FLACGPU_ASSIGN_INDEPENDENT)
            return fault(f, C_, "assignment");
        uint64_t body = 0;
        for (uint32_t s = 0; s < C_; s++) {
            const flacgpu_subframe_plan &sp = subs[(size_t)f * C_ + s];
            if (sp.type > FLACGPU_SUB_LPC) return fault(f, s, "type");
            const uint32_t src = sp.source;
            if (c.stereo4 ? !(src <= 1u || src == FLACGPU_SRC_MID || src == FLACGPU_SRC_SIDE) : src >= c.ncand) return fault(f, s, "source");
            const uint32_t width = c.bps + ((c.stereo4 && src == FLACGPU_SRC_SIDE) ? 1u : 0u);
            if (sp.wasted >= width) return fault(f, s, "wasted");
            if ((uint32_t)sp.bps + sp.wasted != width) return fault(f, s, "bps");   // (the width left behind the wasted bits)
            if (sp.type == FLACGPU_SUB_FIXED || sp.type == FLACGPU_SUB_LPC) {
                if (sp.type == FLACGPU_SUB_FIXED ? sp.order > 4u : (sp.order < 1u || sp.order > max_lpc)) return fault(f, s, "order");
                if (sp.type == FLACGPU_SUB_LPC) {
                    if (sp.precision < 1u || sp.precision > 15u) return fault(f, s, "precision");
                    if (sp.shift > 15u) return fault(f, s, "shift");
                    const int32_t lim = (int32_t)1 << (sp.precision - 1u);
                    for (uint32_t j = 0; j < sp.order; j++)
                        if (sp.coeffs[j] < -lim || sp.coeffs[j] >= lim) return fault(f, s, "coeffs");
                }
                if (sp.coding_method > 1u) return fault(f, s, "coding_method");
                if (sp.partition_order > max_po) return fault(f, s, "partition_order");
                if (sp.n_partitions != 1u << sp.partition_order) return fault(f, s, "n_partitions");
                if ((uint64_t)sp.part_len << sp.partition_order != n) return fault(f, s, "part_len");
                if (sp.order > sp.part_len) return fault(f, s, "order");   // the first partition holds the warm-up
                const uint32_t kmax = sp.coding_method ? 30u : 14u;
                for (uint32_t i = 0; i < sp.n_partitions; i++) {
                    if (sp.rice[i] == 0xFFu) {
                        if (sp.escape_bits[i] > 31u) return fault(f, s, "escape_bits");
                    } else if (sp.rice[i] > kmax) {
                        return fault(f, s, "rice");
                    }
                }
            }
            // a subframe's own bit string: k_sub64's image, k_pack's LDS string
            if (fast ? (by_subframe && sp.bits > sub64_max_sub_bits(c.bps)) : sp.bits > pack_max_sub_bits(n)) return fault(f, s, "bits");
            body += sp.bits;
        }
        if (body != fp.body_bits) return fault(f, C_, "body_bits");
        const uint64_t bytes = 16u + (body + 7u) / 8u;   // the longest header; without the CRC-16
        if (fast && !by_subframe) {   // k_frame64: the whole frame in one image, its CRC-16 in at most three slice rows
            if (body > image_bits) return fault(f, C_, "body_bits over the image");
            if (bytes / 4u > crc_words) return fault(f, C_, "body_bits over the CRC rows");
        }
        total += bytes + 2u;
    }
    if (total > out_cap) return fault(n_frames - 1u, C_, "total bytes");
    return PlanFault();
}

}  // namespace flacenc_route

// Test hook (tests/test_plan_check_host.py, tests/test_frame64_edge_matrix_host.py; not in the public header, needs no
// device): check_plans (plan_check.h) for the batch of one route row, as flacgpu_pack_plans asks it.  out_cap: bytes of the
// output buffer.  Returns 0 and leaves `out` alone when no field offends; else 1 with out[3] = frame, subframe, the image
// words of the shape, and the field's name in `field` (cut to cap - 1 characters).
extern "C" int flacenc_check_plans_row(const int32_t *in, uint64_t out_cap, const flacgpu_frame_plan *plans,
                                       const flacgpu_subframe_plan *subs, uint32_t *out, char *field, size_t cap) {
    using namespace flacenc_route;
    RouteContext c;
    RouteBatch b;
    route_row(in, c, b);
    const PlanFault f = check_plans(c, plan_route(c, b), b.n_frames, b.last_len, out_cap, plans, subs);
    if (!f.bad) return 0;
    out[0] = f.frame;
    out[1] = f.subframe;
    out[2] = frame_image_words(c);
    if (field && cap) {
        size_t i = 0;
        for (; f.field[i] && i + 1 < cap; i++) field[i] = f.field[i];
        field[i] = 0;
    }
    return 1;
}
