// decode_many.hip -- batch decoder: many FLAC streams in one call, metadata parsed by flacgpu_decode_stream's parser
// (host/flac_stream.cpp), frames found and decoded, samples hashed (MD5) on the device (include/flacenc_gpu.h "batch decoder").
// One of the translation units of libflacenc_amd.so (gfx950 only).  Kernels: kernels/frame_scan.inc (frame discovery)
// and kernels/decode_many.inc (decode, CRC-16, finish, MD5); the subframe decoder is decode.inc's, unchanged.  Streams
// that already lie in device memory come in through kernels/gather.inc (DESIGN.md 4b "Device-resident input").
#include "kernels/types.h"
#include "kernels/sample_types.h"
#include "kernels/frame_extent.h"
#include "kernels/frame_analysis.h"
#include "kernels/meta_walk.h"
#include "kernels/meta_feed_rule.h"
#include "kernels/byte_shift.h"
#include "kernels/session_slots_rule.h"
#include "flac_stream.h"
#include "session_rule.h"
#include "container_rule.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

namespace {
#include "kernels/common.inc"
#include "kernels/decode.inc"
#include "kernels/crc16.inc"
#include "kernels/frame_scan.inc"
#include "kernels/spec_end.inc"
#include "kernels/gather.inc"
#include "kernels/session.inc"
#include "kernels/decode_many.inc"
#include "kernels/analyze_many.inc"

constexpr uint32_t kSlotTail = 64;   // zero bytes behind every stream's region (at least)
// k_scan_blocks reads 16 bytes of look-ahead behind a block, and k_scan_emit (slot_pend) and k_spec_end (the CRC test of
// an extent that ends with the region) take the prefix of the block that holds the region's END: with a tail of at
// least one block that block lies inside the stream's own slot, its prefix covers the slot's bytes alone, and the
// bit reader's cap (the slot's end - 4) lies in zeros.
static_assert(kSlotTail >= 64, "the block behind a region's last byte must belong to the region's slot");
// k_cand_heads reads five aligned dwords from the last dword boundary at or before a candidate, and a candidate is a
// byte of its region: at most kHeadBytes + 3 bytes behind the region's last byte, inside the slot's tail
static_assert(kSlotTail >= kHeadBytes + 4, "a candidate's head lies inside its slot");

// Where a scan's bytes lie.  Host memory goes through the pinned staging and one upload (the first door); device memory
// of the decoder's device is gathered into the slot buffer by k_gather_slots, and the little the host has to see of it
// -- the metadata of a regular stream, the headers of a raw stream's candidates -- comes down as small tables.
struct ScanInput {
    const uint8_t *const *data;   // [n_streams]
    bool device;
};

// a buffer that only grows: device memory, or pinned host memory
template <bool PINNED> struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;
    void release() { (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    int ensure(size_t bytes) {
        if (bytes <= cap) return FLACGPU_OK;
        const size_t want = std::max(bytes, cap + cap / 2);
        release();
        if (PINNED) HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
        else HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return FLACGPU_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    ~GrowBuf() { release(); }
};
using DevBuf = GrowBuf<false>;
}  // namespace

struct flacgpu_decoder {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev = nullptr;   // the device door's wait for the caller's stream: created by the first device scan
    GrowBuf<true> staging;   // pinned: the batch buffer on its way up (host scans alone)
    DevBuf dev_src, meta, gather_src, cand_head;   // device scans alone: sources, metadata records, regions, headers
    uint64_t slot_bytes = 0;   // bytes of `bytes` the last scan defined: its slots and the look-ahead; 0: no slot
    DevBuf bytes, slots, mask, plocal, wg_cnt, wg_tail, wg_off, wg_carry;
    DevBuf cand_pos, cand_info, cand_crc, cand_slot, slot_cand0, slot_pend, link;
    DevBuf spec_len;   // FLACGPU_SCAN_SPECULATIVE alone: allocated by the first scan that asks for it
    DevBuf frames, scratch, codes, counts, jobs, digest, out_stage;
    DevBuf md5_stage, pad_out, pad_streams;   // decode_as: interleaved int32 for the MD5, padded layout tables
    DevBuf win_frames, win_desc;              // decode_windows: the selected frames (d->frames stays the scan's)
    DevBuf tl_runs, tl_mask;                  // decode_timeline: the fill runs; the mask on its way to host memory
    // the scanned batch
    bool scanned = false;
    std::vector<flacgpu_decoded_stream> res;
    std::vector<int32_t> slot_of;          // stream -> slot, -1: no frame region on the device
    std::vector<uint32_t> slot_stream;     // slot -> stream
    std::vector<ManyFrame> frame_tab;
    uint32_t n_slots = 0;
    uint64_t total = 0, scratch_total = 0;
    // decode_windows' index of frame_tab: slot s owns frames [slot_frame0[s], slot_frame0[s + 1]); frame_first is a
    // frame's first sample per channel in its stream
    std::vector<uint32_t> slot_frame0;
    std::vector<uint64_t> frame_first;
    // a raw scan (flacgpu_decoder_scan_frames): every kept frame's record, the streams' summaries, and decode_frames' own
    // frame table -- every kept frame with `out` = the record's out_offset and `slot` = the frame's index, so that the
    // frame kernels' per-slot counts come out per frame.  frame_tab holds the frames of the uniform streams alone.
    bool raw = false;
    std::vector<flacgpu_frame_record> records;
    std::vector<flacgpu_raw_stream> raw_streams;
    std::vector<ManyFrame> raw_tab;   // uploaded to raw_frames by the first decode_frames of the scan
    bool raw_tab_uploaded = false;
    DevBuf raw_frames;
    // flacgpu_decoder_analyze: the scan's frame table with the analysis' own offsets, uploaded by the first call of a scan
    DevBuf an_frames;
    bool an_tab_uploaded = false;
    uint64_t raw_elements = 0, raw_scratch = 0;
    bool session = false;   // owned by a flacgpu_decoder_session: the scan calls and destroy are refused
    // a container session's decoder: decode / decode_as hash into the session's MD5 chains (decode_impl), not k_md5_many
    struct flacgpu_decoder_session *container = nullptr;
    // the last device_scan, seconds: from its start to the end of its first synchronisation (the candidate count), and
    // from there to the end of its second (the candidates); read by a session's flacgpu_decoder_session_last_feed_timing
    double scan_sync_s[2] = {0, 0};
};

namespace {
// A scan's slots in the batch buffer: one per stream with a frame region, 64-byte aligned, a zero tail behind each.
struct SlotLayout {
    std::vector<ScanSlot> slots;
    std::vector<size_t> region_at;       // first byte of the frame region in the caller's buffer
    std::vector<uint32_t> slot_stream;   // slot -> stream
    uint64_t at = 0;                     // the end of the last slot
    // the new slot's index
    uint32_t add(uint32_t stream, size_t region, uint64_t len, uint32_t channels, uint32_t min_frame) {
        ScanSlot s{};
        s.base = at;
        s.len = len;
        s.block0 = at / 64;
        s.channels = channels;
        s.min_frame = min_frame;
        slots.push_back(s);
        region_at.push_back(region);
        slot_stream.push_back(stream);
        at += (len + kSlotTail + 63) & ~(uint64_t)63;
        return (uint32_t)slots.size() - 1;
    }
    uint64_t end_of(uint32_t s) const { return s + 1 < slots.size() ? slots[s + 1].base : at; }
};

// What a device scan leaves on the host: the candidates' positions, records and links, and every slot's first candidate.
// spec (raw, under FLACGPU_SCAN_SPECULATIVE; else empty): the own extents of the candidates without a link (k_spec_end),
// 0: none.  heads (device input of a raw scan; else empty): the 16 bytes at every candidate (k_cand_heads).
struct Candidates {
    std::vector<uint64_t> pos;
    std::vector<uint32_t> info, cand0, spec;
    std::vector<int32_t> link;
    std::vector<uint8_t> heads;
    uint32_t n = 0;
    uint32_t end_of(uint32_t s) const { return s + 1 < cand0.size() ? cand0[s + 1] : n; }
};

// A decoder session's feed (kernels/session.inc): every slot is built by k_session_slots from `srcs` (device addresses),
// and the links are made under `info`; both tables have one entry per slot and go up into the two buffers.
struct SessionFill {
    const SessionSrc *srcs;
    const SessionSlot *info;
    DevBuf *src_tab, *info_tab;
};

// The rule that links a scan's candidates: k_link (regular streams), k_link_raw (raw frame streams), and the two of a
// session's feed, k_link_session (raw) and k_link_container (regular).  The raw rules take the candidates with a sample
// rate and a sample size of their own (k_scan_subset); a feed's slots come from its SessionFill.
enum class LinkRule { Regular, Raw, Session, Container };

// The device half of a scan: fills every slot (zero tails, 64 bytes of look-ahead) -- host input in one upload, device
// input with k_gather_slots, a session's feed (`fill`, given with its two rules and no other; `in` is not looked at) with
// k_session_slots -- and runs the scan kernels; the candidates come down into `c`, with the extents and the headers the
// caller asks for.
int device_scan(flacgpu_decoder *d, const ScanInput &in, const SlotLayout &lay, LinkRule rule, bool want_spec,
                bool want_heads, Candidates &c, const SessionFill *fill = nullptr) {
    const bool raw = rule == LinkRule::Raw || rule == LinkRule::Session;
    const std::vector<ScanSlot> &slots = lay.slots;
    const uint64_t at = lay.at;
    const uint32_t S = (uint32_t)slots.size();
    const uint8_t *const *data = in.data;
    const auto t_begin = std::chrono::steady_clock::now();   // (scan_sync_s: three clock reads a scan)
    const std::string who = fill ? std::string("flacgpu_decoder_session_feed")
                                 : std::string(raw ? "flacgpu_decoder_scan_frames" : "flacgpu_decoder_scan") + (in.device ? "_device" : "");
    // the bit reader indexes dwords with 32 bits
    if (at + 64 > ((uint64_t)1 << 34)) {
        g_last_error = who + ": the batch's frames exceed 16 GiB";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    const uint64_t n_blocks = at / 64;
    const uint64_t n_wg64 = (n_blocks + WG - 1) / WG;
    if (n_wg64 > 0xFFFFFFFFull) return FLACGPU_ERR_UNSUPPORTED;
    const uint32_t n_wg = (uint32_t)n_wg64;
    const size_t buf_bytes = at + 64;
    uint8_t *stg = nullptr;
    std::vector<const uint8_t *> srcs;   // device input: every region's first byte
    if (fill) {
        if (int rc = fill->src_tab->ensure(sizeof(SessionSrc) * S)) return rc;
        if (int rc = fill->info_tab->ensure(sizeof(SessionSlot) * S)) return rc;
    } else if (in.device) {
        try {
            srcs.resize(S);
        } catch (const std::bad_alloc &) {
            g_last_error = who + ": out of host memory";
            return FLACGPU_ERR_UNSUPPORTED;
        }
        for (uint32_t s = 0; s < S; s++) srcs[s] = data[lay.slot_stream[s]] + lay.region_at[s];
        if (int rc = d->gather_src.ensure(sizeof(const uint8_t *) * S)) return rc;
    } else {
        // ---- one upload: every region into the pinned staging, zero tails, 64 bytes of look-ahead
        if (int rc = d->staging.ensure(buf_bytes)) return rc;
        stg = d->staging.as<uint8_t>();
        for (uint32_t s = 0; s < S; s++) {
            const uint64_t b = slots[s].base, l = slots[s].len;
            const uint64_t e = s + 1 < S ? slots[s + 1].base : buf_bytes;   // the last: the look-ahead too
            memcpy(stg + b, data[lay.slot_stream[s]] + lay.region_at[s], l);
            memset(stg + b + l, 0, e - b - l);
        }
    }
    if (int rc = d->bytes.ensure(buf_bytes)) return rc;
    if (int rc = d->slots.ensure(sizeof(ScanSlot) * S)) return rc;
    if (int rc = d->mask.ensure(8 * n_blocks)) return rc;
    if (int rc = d->plocal.ensure(2 * n_blocks)) return rc;
    if (int rc = d->wg_cnt.ensure(4 * n_wg)) return rc;
    if (int rc = d->wg_tail.ensure(4 * n_wg)) return rc;
    if (int rc = d->wg_off.ensure(4 * (n_wg + 1))) return rc;
    if (int rc = d->wg_carry.ensure(2 * n_wg)) return rc;
    if (int rc = d->slot_cand0.ensure(4 * S)) return rc;
    if (int rc = d->slot_pend.ensure(4 * S)) return rc;
    d->slot_bytes = buf_bytes;
    if (!fill && !in.device) HIP_TRY(hipMemcpyAsync(d->bytes.p, stg, buf_bytes, hipMemcpyHostToDevice, d->st));
    HIP_TRY(hipMemcpyAsync(d->slots.p, slots.data(), sizeof(ScanSlot) * S, hipMemcpyHostToDevice, d->st));
    if (fill) {   // tail and chunk into every slot: every byte of [0, buf_bytes), a lane per 16-byte group
        HIP_TRY(hipMemcpyAsync(fill->src_tab->p, fill->srcs, sizeof(SessionSrc) * S, hipMemcpyHostToDevice, d->st));
        HIP_TRY(hipMemcpyAsync(fill->info_tab->p, fill->info, sizeof(SessionSlot) * S, hipMemcpyHostToDevice, d->st));
        const uint64_t n_groups = buf_bytes / 16;
        hipLaunchKernelGGL(k_session_slots, dim3((uint32_t)((n_groups + WG - 1) / WG)), dim3(WG), 0, d->st,
                           d->bytes.as<uint8_t>(), d->slots.as<const ScanSlot>(), fill->src_tab->as<const SessionSrc>(), S,
                           n_blocks, n_groups);
    } else if (in.device) {   // the gather: every byte of [0, buf_bytes), a lane per 16-byte group
        HIP_TRY(hipMemcpyAsync(d->gather_src.p, srcs.data(), sizeof(const uint8_t *) * S, hipMemcpyHostToDevice, d->st));
        const uint64_t n_groups = buf_bytes / 16;   // buf_bytes is a multiple of 64, at most 2^34: the grid fits
        hipLaunchKernelGGL(k_gather_slots, dim3((uint32_t)((n_groups + WG - 1) / WG)), dim3(WG), 0, d->st,
                           d->bytes.as<uint8_t>(), d->slots.as<const ScanSlot>(), d->gather_src.as<const uint8_t *const>(),
                           S, n_blocks, n_groups);
    }
    ScanParams p{};
    p.bytes = d->bytes.as<uint8_t>();
    p.slots = d->slots.as<ScanSlot>();
    p.n_slots = S;
    p.n_blocks = n_blocks;
    p.mask = d->mask.as<uint64_t>();
    p.plocal = d->plocal.as<uint16_t>();
    p.wg_cnt = d->wg_cnt.as<uint32_t>();
    p.wg_tail = d->wg_tail.as<uint32_t>();
    p.wg_off = d->wg_off.as<uint32_t>();
    p.wg_carry = d->wg_carry.as<uint16_t>();
    p.slot_cand0 = d->slot_cand0.as<uint32_t>();
    p.slot_pend = d->slot_pend.as<uint32_t>();
    hipLaunchKernelGGL(k_scan_blocks, dim3(n_wg), dim3(WG), 0, d->st, p);
    if (raw) hipLaunchKernelGGL(k_scan_subset, dim3(n_wg), dim3(WG), 0, d->st, p);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(WG), 0, d->st, p, n_wg);
    HIP_TRY(hipGetLastError());
    uint32_t n_cand = 0;
    HIP_TRY(hipMemcpyAsync(&n_cand, d->wg_off.as<uint32_t>() + n_wg, 4, hipMemcpyDeviceToHost, d->st));
    HIP_TRY(hipStreamSynchronize(d->st));
    const auto t_count = std::chrono::steady_clock::now();
    const size_t nc = std::max<uint32_t>(n_cand, 1);
    if (int rc = d->cand_pos.ensure(8 * nc)) return rc;
    if (int rc = d->cand_info.ensure(4 * nc)) return rc;
    if (int rc = d->cand_crc.ensure(4 * nc)) return rc;
    if (int rc = d->cand_slot.ensure(4 * nc)) return rc;
    if (int rc = d->link.ensure(4 * nc)) return rc;
    if (want_spec)
        if (int rc = d->spec_len.ensure(4 * nc)) return rc;
    if (want_heads)
        if (int rc = d->cand_head.ensure(kHeadBytes * nc)) return rc;
    p.cand_pos = d->cand_pos.as<uint64_t>();
    p.cand_info = d->cand_info.as<uint32_t>();
    p.cand_crc = d->cand_crc.as<uint32_t>();
    p.cand_slot = d->cand_slot.as<uint32_t>();
    p.link = d->link.as<int32_t>();
    p.n_cand = n_cand;
    hipLaunchKernelGGL(k_scan_emit, dim3(n_wg), dim3(WG), 0, d->st, p);
    const dim3 link_grid((n_cand + WG - 1) / WG);
    if (n_cand && rule == LinkRule::Container)
        hipLaunchKernelGGL(k_link_container, link_grid, dim3(WG), 0, d->st, p, fill->info_tab->as<const SessionSlot>());
    else if (n_cand && rule == LinkRule::Session)
        hipLaunchKernelGGL(k_link_session, link_grid, dim3(WG), 0, d->st, p, fill->info_tab->as<const SessionSlot>());
    else if (n_cand && rule == LinkRule::Raw) hipLaunchKernelGGL(k_link_raw, link_grid, dim3(WG), 0, d->st, p);
    else if (n_cand) hipLaunchKernelGGL(k_link, link_grid, dim3(WG), 0, d->st, p);
    if (n_cand && want_spec)
        hipLaunchKernelGGL(k_spec_end, dim3((n_cand + 63) / 64), dim3(64), 0, d->st, p, d->spec_len.as<uint32_t>());
    if (n_cand && want_heads)
        hipLaunchKernelGGL(k_cand_heads, dim3((n_cand + WG - 1) / WG), dim3(WG), 0, d->st, p.bytes, p.cand_pos, n_cand,
                           d->cand_head.as<uint4>());
    HIP_TRY(hipGetLastError());
    try {
        c.pos.resize(n_cand);
        c.info.resize(n_cand);
        c.link.resize(n_cand);
        c.cand0.resize(S);
        if (want_spec) c.spec.resize(n_cand);
        if (want_heads) c.heads.resize(kHeadBytes * (size_t)n_cand);
    } catch (const std::bad_alloc &) {
        g_last_error = who + ": out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (n_cand) {
        HIP_TRY(hipMemcpyAsync(c.pos.data(), p.cand_pos, 8 * (size_t)n_cand, hipMemcpyDeviceToHost, d->st));
        HIP_TRY(hipMemcpyAsync(c.info.data(), p.cand_info, 4 * (size_t)n_cand, hipMemcpyDeviceToHost, d->st));
        HIP_TRY(hipMemcpyAsync(c.link.data(), p.link, 4 * (size_t)n_cand, hipMemcpyDeviceToHost, d->st));
        if (want_spec)   // with the links, in the same submission
            HIP_TRY(hipMemcpyAsync(c.spec.data(), d->spec_len.p, 4 * (size_t)n_cand, hipMemcpyDeviceToHost, d->st));
        if (want_heads)
            HIP_TRY(hipMemcpyAsync(c.heads.data(), d->cand_head.p, kHeadBytes * (size_t)n_cand, hipMemcpyDeviceToHost, d->st));
    }
    HIP_TRY(hipMemcpyAsync(c.cand0.data(), p.slot_cand0, 4 * (size_t)S, hipMemcpyDeviceToHost, d->st));
    HIP_TRY(hipStreamSynchronize(d->st));
    d->scan_sync_s[0] = std::chrono::duration<double>(t_count - t_begin).count();
    d->scan_sync_s[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_count).count();
    c.n = n_cand;
    return FLACGPU_OK;
}

// The metadata of device input: k_meta_walk's record of every stream, on the host.  A null pointer or a zero length
// is handed to the kernel as no bytes, and is not dereferenced.
int device_meta_walk(flacgpu_decoder *d, const uint8_t *const *data, const size_t *len, uint32_t n,
                     std::vector<MetaRecord> &meta) {
    std::vector<DevSource> src;
    try {
        src.resize(n);
        meta.resize(n);
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_scan_device: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (!n) return FLACGPU_OK;
    for (uint32_t i = 0; i < n; i++) src[i] = data[i] && len[i] ? DevSource{data[i], len[i]} : DevSource{nullptr, 0};
    if (int rc = d->dev_src.ensure(sizeof(DevSource) * n)) return rc;
    if (int rc = d->meta.ensure(sizeof(MetaRecord) * n)) return rc;
    HIP_TRY(hipMemcpyAsync(d->dev_src.p, src.data(), sizeof(DevSource) * n, hipMemcpyHostToDevice, d->st));
    hipLaunchKernelGGL(k_meta_walk, dim3((n + 63) / 64), dim3(64), 0, d->st, d->dev_src.as<const DevSource>(), n,
                       d->meta.as<MetaRecord>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(meta.data(), d->meta.p, sizeof(MetaRecord) * n, hipMemcpyDeviceToHost, d->st));
    HIP_TRY(hipStreamSynchronize(d->st));
    return FLACGPU_OK;
}

// The end of both scans: the frame table onto the device, the batch's sizes and its slots' streams into the handle.
int finish_scan(flacgpu_decoder *d, SlotLayout &lay, uint64_t total, uint64_t scratch_total) {
    d->an_tab_uploaded = false;
    if (!d->frame_tab.empty()) {
        if (int rc = d->frames.ensure(sizeof(ManyFrame) * d->frame_tab.size())) return rc;
        HIP_TRY(hipMemcpyAsync(d->frames.p, d->frame_tab.data(), sizeof(ManyFrame) * d->frame_tab.size(),
                               hipMemcpyHostToDevice, d->st));
        HIP_TRY(hipStreamSynchronize(d->st));   // frame_tab may change before the copy is done otherwise
    }
    d->total = total;
    d->scratch_total = scratch_total;
    d->slot_stream.swap(lay.slot_stream);
    return FLACGPU_OK;
}

// The running sizes of a scan's two layouts: decode_frames' (every kept frame of a raw scan) and the regular batch
// calls' (every stream of a regular scan, the uniform streams of a raw one).
struct RawTotals {
    uint64_t elements = 0, raw_scratch = 0, total = 0, scratch_total = 0;
};

// Where candidate k of a slot that ends at slot_end ends by its link
flacenc::RawEnd end_by_link(const Candidates &c, size_t k, uint64_t slot_end) {
    const int32_t link = c.link[k];
    if (link == LINK_HOLD) return flacenc::RawEnd{flacenc::kRawHold, false};
    if (link == LINK_NONE) return flacenc::RawEnd{flacenc::kRawNone, false};
    return flacenc::RawEnd{link == LINK_END ? slot_end : c.pos[link], false};
}

// The chain walk (regular_walk, host/raw_walk.h) over slot s, whose positions below `judged` are judged, along the links
// the device left (k_link, or a feed's k_link_container with its LINK_HOLD): every kept frame joins frame_tab with
// STREAMINFO's channels and sample size, `out` counted in samples per channel from *samples on (lay_out_regular makes
// it absolute).  A frame without an end is not taken, and nothing behind it.
flacenc::RegularWalk walk_regular_slot(flacgpu_decoder *d, const Candidates &c, const SlotLayout &lay, uint32_t s,
                                       uint64_t judged, const flacgpu_stream_info &info, uint64_t *samples) {
    const ScanSlot &sl = lay.slots[s];
    const uint64_t slot_end = sl.base + sl.len;
    return flacenc::regular_walk(
        c.pos.data(), c.cand0[s], c.end_of(s), sl.base, slot_end, judged,
        [&](size_t k, uint64_t) { return end_by_link(c, k, slot_end); },
        [&](size_t k, uint64_t at, uint64_t end) {
            ManyFrame f{};
            f.start = at;
            f.end = end;
            f.cap = lay.end_of(s) - 4;
            f.n = (c.info[k] & 0xFFFFu) + 1u;
            f.slot = s;
            f.channels = info.channels;
            f.bps = info.bits_per_sample;
            f.out = *samples;
            d->frame_tab.push_back(f);
            *samples += f.n;
        });
}

// The regular batch's output layout: the streams one after another, interleaved; every frame's place in it and in the
// planar scratch.
RawTotals lay_out_regular(flacgpu_decoder *d, const SlotLayout &lay) {
    RawTotals tot;
    for (flacgpu_decoded_stream &r : d->res) {
        r.out_offset = tot.total;
        if (r.rc == FLACGPU_OK) tot.total += r.info.decoded_samples * r.info.channels;
    }
    for (ManyFrame &f : d->frame_tab) {
        f.out = d->res[lay.slot_stream[f.slot]].out_offset + f.out * f.channels;
        f.scratch = tot.scratch_total;
        tot.scratch_total += (uint64_t)f.channels * ((f.n + 3u) & ~3u);
    }
    return tot;
}

int scan_impl(flacgpu_decoder *d, const ScanInput &in, const size_t *len, uint32_t n) {
    const uint8_t *const *data = in.data;
    d->res.assign(n, flacgpu_decoded_stream{});
    d->slot_of.assign(n, -1);
    d->frame_tab.clear();
    d->slot_bytes = 0;
    std::vector<MetaRecord> meta;   // device input: the walk was done where the bytes lie
    if (in.device)
        if (int rc = device_meta_walk(d, data, len, n, meta)) return rc;
    // ---- host: metadata, slot layout
    SlotLayout lay;
    for (uint32_t i = 0; i < n; i++) {
        flacgpu_decoded_stream &r = d->res[i];
        uint32_t min_frame = 0;
        size_t pos = 0;
        const char *why = in.device ? flacenc::metadata_of_record(meta[i], &r.info, &min_frame, &pos)
                                    : flacenc::parse_metadata(data ? data[i] : nullptr, len ? len[i] : 0, &r.info, &min_frame, &pos);
        r.rc = why ? FLACGPU_ERR_INVALID_ARG : FLACGPU_OK;
        if (r.rc != FLACGPU_OK || pos >= len[i]) continue;   // no frame region: 0 frames, nothing bad
        d->slot_of[i] = (int32_t)lay.add(i, pos, len[i] - pos, r.info.channels, min_frame);
    }
    const uint32_t S = (uint32_t)lay.slots.size();
    d->n_slots = S;
    if (S) {
        Candidates c;
        if (int rc = device_scan(d, in, lay, LinkRule::Regular, false, false, c)) return rc;
        // ---- host walk: the chain from each region's first byte to its end (the host scan's lost-sync rule)
        for (uint32_t s = 0; s < S; s++) {
            flacgpu_stream_info &info = d->res[lay.slot_stream[s]].info;
            const size_t first = d->frame_tab.size();
            uint64_t samples = 0;
            const uint64_t slot_end = lay.slots[s].base + lay.slots[s].len;
            if (walk_regular_slot(d, c, lay, s, slot_end, info, &samples).lost) info.bad_frames = 1;
            info.frames = (uint32_t)(d->frame_tab.size() - first);
            info.decoded_samples = samples;
        }
    }
    const RawTotals tot = lay_out_regular(d, lay);
    return finish_scan(d, lay, tot.total, tot.scratch_total);
}

// A kept frame [at, end) of stream i (positions in the batch buffer; slot_end: the end of its slot): its record, with
// byte_offset as given, and its entry in decode_frames' table.  The header was accepted by K_s1: n, header_bytes and the
// blocking bit come from its candidate record, the rest from the header's bytes `head` (header_bytes <= kHeadBytes).
void keep_raw_frame(flacgpu_decoder *d, uint32_t i, uint64_t at, uint64_t end, uint64_t slot_end, uint64_t byte_offset,
                    uint32_t cinfo, const uint8_t *head, bool own, RawTotals &tot) {
    flacenc::HostFrameInfo h;
    h.n = (cinfo & 0xFFFFu) + 1u;
    h.header_bytes = (cinfo >> 16) & 0xFFu;
    h.blocking = cinfo >> 24;
    h.acode = head[3] >> 4;
    h.bps_code = (head[3] >> 1) & 7;
    flacenc::host_frame_fields(head, h);
    const flacgpu_frame_record f = flacenc::raw_frame_record(h, i, byte_offset, end - at, tot.elements, own);
    ManyFrame m{};
    m.start = at;
    m.end = end;
    m.cap = slot_end - 4;
    m.scratch = tot.raw_scratch;
    m.out = tot.elements;
    m.n = h.n;
    m.slot = (uint32_t)d->records.size();   // the frame kernels count per slot: per frame here
    m.channels = h.channels;
    m.bps = h.bits_per_sample;
    d->records.push_back(f);
    d->raw_tab.push_back(m);
    tot.elements += (uint64_t)h.n * h.channels;
    tot.raw_scratch += (uint64_t)h.channels * ((h.n + 3u) & ~3u);
}

// Stream i's place in the regular batch calls, from its `count` records from `first` on (slot s): a uniform stream joins
// frame_tab and the uniform streams' layout, any other is absent from those calls.
void join_regular(flacgpu_decoder *d, uint32_t i, int32_t s, size_t first, size_t count, bool uniform, RawTotals &tot) {
    flacgpu_decoded_stream &r = d->res[i];
    r.out_offset = tot.total;
    if (!uniform) {
        r.rc = count ? FLACGPU_ERR_UNSUPPORTED : FLACGPU_ERR_INVALID_ARG;
        return;
    }
    const flacgpu_frame_record &f0 = d->records[first];
    r.info.sample_rate = f0.sample_rate;
    r.info.channels = f0.channels;
    r.info.bits_per_sample = f0.bits_per_sample;
    r.info.min_block = r.info.max_block = f0.block_size;
    r.info.frames = (uint32_t)count;
    for (size_t k = first; k < first + count; k++) {
        const flacgpu_frame_record &f = d->records[k];
        r.info.min_block = std::min(r.info.min_block, f.block_size);
        r.info.max_block = std::max(r.info.max_block, f.block_size);
        ManyFrame m = d->raw_tab[k];
        m.slot = (uint32_t)s;
        m.out = tot.total + r.info.decoded_samples * f.channels;
        m.scratch = tot.scratch_total;
        tot.scratch_total += (uint64_t)m.channels * ((m.n + 3u) & ~3u);
        d->frame_tab.push_back(m);
        r.info.decoded_samples += f.block_size;
    }
    tot.total += r.info.decoded_samples * r.info.channels;
}

// The raw walk (host/raw_walk.h) over slot s's candidates, their ends answered from the tables the device left: the
// link (k_link_raw, or a session's k_link_session with its LINK_HOLD), and for a candidate without one its own extent
// where the scan asked for extents (c.spec).  Positions are the batch buffer's.
template <class Keep>
flacenc::RawWalk walk_slot(const Candidates &c, const ScanSlot &sl, uint32_t s, Keep keep, flacenc::SessionCount *count = nullptr) {
    const uint64_t slot_end = sl.base + sl.len;
    return flacenc::raw_walk(
        c.pos.data(), c.cand0[s], c.end_of(s), sl.base, slot_end,
        [&](size_t k, uint64_t at) {
            if (c.link[k] == LINK_NONE && !c.spec.empty() && c.spec[k]) return flacenc::RawEnd{at + c.spec[k], true};
            return end_by_link(c, k, slot_end);
        },
        keep, count);
}

// The end of a raw scan and of a session's feed (`who`): the frame kernels index frames with 31 bits; the sizes of
// decode_frames' layout; finish_scan.
int finish_raw_scan(flacgpu_decoder *d, SlotLayout &lay, const RawTotals &tot, const char *who) {
    if (d->raw_tab.size() > 0x7FFFFFFFull) {
        g_last_error = std::string(who) + ": more than 2^31 - 1 frames";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    d->raw_elements = tot.elements;
    d->raw_scratch = tot.raw_scratch;
    return finish_scan(d, lay, tot.total, tot.scratch_total);
}

// flacgpu_decoder_scan_frames behind its argument checks: a slot is a whole input, the device finds the candidates and
// their ends by the raw rule, and the host walks them with a cursor (DESIGN.md "Raw frame streams").  Under
// FLACGPU_SCAN_SPECULATIVE a candidate without a link ends where its own extent does, if it has one.
int scan_raw_impl(flacgpu_decoder *d, const ScanInput &in, const size_t *len, uint32_t n, uint32_t flags) {
    const uint8_t *const *data = in.data;
    const bool spec = flags & FLACGPU_SCAN_SPECULATIVE;
    d->slot_bytes = 0;
    SlotLayout lay;
    Candidates c;   // heads (device input): the candidates' headers
    try {   // no exception crosses the C ABI
        d->res.assign(n, flacgpu_decoded_stream{});
        d->slot_of.assign(n, -1);
        d->frame_tab.clear();
        d->records.clear();
        d->raw_streams.assign(n, flacgpu_raw_stream{});
        for (uint32_t i = 0; i < n; i++) {
            if (!data[i] || !len[i]) continue;   // nothing to scan: no kept frame
            d->slot_of[i] = (int32_t)lay.add(i, 0, len[i], 0, 0);
        }
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_scan_frames: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    const uint32_t S = (uint32_t)lay.slots.size();
    d->n_slots = S;
    if (S)
        if (int rc = device_scan(d, in, lay, LinkRule::Raw, spec, in.device, c)) return rc;
    const uint32_t n_cand = c.n;
    // ---- host walk, stream by stream: the candidates in ascending order, those below the cursor ignored, one without
    // an end passed over, one with an end kept and the cursor moved to that end.  A kept frame's record is read from
    // its own header: in the staging copy of the bytes, or (device input) in the downloaded table of headers.
    std::vector<ManyFrame> &all = d->raw_tab;   // decode_frames' table
    all.clear();
    d->raw_tab_uploaded = false;
    const uint8_t *stg = d->staging.as<const uint8_t>();
    RawTotals tot;
    try {
        d->records.reserve(n_cand);   // a kept frame is a candidate
        all.reserve(n_cand);
        d->frame_tab.reserve(n_cand);
        for (uint32_t i = 0; i < n; i++) {
            flacgpu_raw_stream &sum = d->raw_streams[i];
            const size_t first = d->records.size();
            const int32_t s = d->slot_of[i];
            if (s >= 0) {
                const ScanSlot &sl = lay.slots[s];
                walk_slot(c, sl, (uint32_t)s, [&](size_t k, uint64_t at, uint64_t end, bool own) {
                    const uint8_t *head = in.device ? c.heads.data() + kHeadBytes * k : stg + at;
                    keep_raw_frame(d, i, at, end, lay.end_of((uint32_t)s), at - sl.base, c.info[k], head, own, tot);
                });
            }
            const size_t count = d->records.size() - first;
            flacenc::summarise_raw_frames(d->records.data() + first, count, len[i], sum);
            sum.first_frame = first;
            join_regular(d, i, s, first, count, sum.uniform, tot);
        }
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_scan_frames: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    return finish_raw_scan(d, lay, tot, "flacgpu_decoder_scan_frames");
}
}  // namespace

// A decoder session (include/flacenc_gpu.h "sessions that take raw frame streams chunk by chunk"; DESIGN.md 4b "Decoder
// sessions").  The decoder's batch buffer and `other` take turns: a feed builds its slots in the one while the held tails
// still lie in the other.
struct flacgpu_decoder_session {
    struct Stream {
        uint64_t base = 0;   // offset of the first held byte from the stream's first byte
        uint64_t held = 0;   // bytes not decided yet
        uint64_t at = 0;     // where they lie in the decoder's batch buffer
        flacenc::SessionCount count;
    };
    flacgpu_decoder *d = nullptr;
    std::vector<Stream> streams;
    uint32_t W = 0;
    uint64_t fed = 0;
    bool finished = false, dead = false;   // dead: a call failed half way; every further call is refused
    flacgpu_session_timing timing{};       // of the last feed or finish
    DevBuf other, chunks, src_tab, info_tab;
    // ---- a container session (DESIGN.md 4b "Container sessions"): regular .flac streams, MD5 across feeds ----
    struct Container : flacenc::ContainerStream {   // the rule's state (host/container_rule.h), and the device session's own
        // cumulative, as the one-shot decode counts them: lost synchronisation, and what the hashing decode of every
        // feed found
        uint32_t bad_frames = 0, bad_crc16 = 0;
        bool in_feed = false;        // the last feed decided frames for this stream
        bool broken = false;         // such a feed was never hashed: the chain says nothing
    };
    bool container = false;
    std::vector<Container> cs;
    flacgpu_md5_chains *chains = nullptr;   // one per stream
    bool hashed = true;           // the last feed's samples are in the chains (or it decided none)
    bool verdict_given = false;
    bool meta_on_device = false;  // meta_tab holds every stream's `meta` as it stands here
    bool meta_fresh = false;      // k_meta_feed ran in the feed under way: its table is this feed's result
    DevBuf meta_tab, meta_src, meta_used;
};

namespace {
// What the feeds of the two device sessions share (session_step, container_step).  The feed's slots and the decoder's
// new per-stream tables are built here, in locals: a call refused before commit_and_scan has touched neither the session
// nor its decoder, whose last feed can still be decoded; a failure behind it leaves the session dead.
struct SessionFeed {
    using Clock = std::chrono::steady_clock;
    flacgpu_decoder_session *ses;
    const uint8_t *tails;   // the buffer the held tails lie in: the decoder's batch buffer, `other` from the commit on
    SlotLayout lay;
    Candidates c;
    std::vector<SessionSrc> srcs;
    std::vector<SessionSlot> info;
    std::vector<flacgpu_decoded_stream> res;
    std::vector<int32_t> slot_of;
    std::vector<flacgpu_raw_stream> raw_streams;
    Clock::time_point t0, t1, t2;

    explicit SessionFeed(flacgpu_decoder_session *s) : ses(s), tails(s->d->bytes.as<const uint8_t>()) {}
    void begin(uint32_t n) {
        res.assign(n, flacgpu_decoded_stream{});
        slot_of.assign(n, -1);
        raw_streams.assign(n, flacgpu_raw_stream{});
    }
    // stream i's slot: its held tail, then the `fresh` new bytes at `chunk` (a DEVICE address)
    void add(uint32_t i, const flacgpu_decoder_session::Stream &st, const uint8_t *chunk, uint64_t fresh, bool final,
             uint32_t channels, uint32_t min_frame) {
        slot_of[i] = (int32_t)lay.add(i, 0, st.held + fresh, channels, min_frame);
        srcs.push_back(SessionSrc{reinterpret_cast<uint64_t>(tails + st.at), st.held,
                                  fresh ? reinterpret_cast<uint64_t>(chunk) : 0, fresh});
        info.push_back(SessionSlot{final ? 1u : 0u, ses->W});
    }
    // device_scan's limit, before anything has changed
    int refused() const {
        if (lay.at + 64 <= ((uint64_t)1 << 34)) return FLACGPU_OK;
        g_last_error = "flacgpu_decoder_session_feed: the feed's slots exceed 16 GiB";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    // The commit point (nothing here up to the scan allocates), and the scan under `rule`
    int commit_and_scan(LinkRule rule, bool want_heads) {
        flacgpu_decoder *d = ses->d;
        const uint32_t S = (uint32_t)lay.slots.size();
        d->scanned = d->raw = false;
        d->res.swap(res);
        d->slot_of.swap(slot_of);
        d->raw_streams.swap(raw_streams);
        d->frame_tab.clear();
        d->records.clear();
        d->raw_tab.clear();
        d->raw_tab_uploaded = false;
        d->n_slots = S;
        d->slot_bytes = 0;
        ses->dead = true;   // until the feed is through: a failure from here on leaves the tails in neither buffer for certain
        std::swap(d->bytes.p, ses->other.p);
        std::swap(d->bytes.cap, ses->other.cap);
        t0 = Clock::now();
        d->scan_sync_s[0] = d->scan_sync_s[1] = 0;   // what a feed without a slot reports
        if (S) {
            const SessionFill fill{srcs.data(), info.data(), &ses->src_tab, &ses->info_tab};
            if (int rc = device_scan(d, ScanInput{nullptr, true}, lay, rule, false, want_heads, c, &fill)) return rc;
        }
        t1 = Clock::now();
        return FLACGPU_OK;
    }
    void walked() { t2 = Clock::now(); }
    // the feed is through, its frame table on the device
    void done() {
        const auto ms = [](Clock::duration v) { return std::chrono::duration<double, std::milli>(v).count(); };
        flacgpu_session_timing &t = ses->timing;
        t.to_first_sync_ms = ses->d->scan_sync_s[0] * 1e3;
        t.to_second_sync_ms = ses->d->scan_sync_s[1] * 1e3;
        t.scan_rest_ms = ms(t1 - t0) - t.to_first_sync_ms - t.to_second_sync_ms;
        t.walk_ms = ms(t2 - t1);
        t.table_upload_ms = ms(Clock::now() - t2);
        ses->dead = false;
    }
};

// One feed behind its argument checks (finish: no bytes, every stream flushed).  chunk[i]: DEVICE address of stream i's
// new bytes (null: none), len[i] their count.  The slots are tail + chunk, built and scanned on the device; the host
// walks the links as scan_raw_impl does, stops at the first LINK_HOLD and keeps the session's counts.
int session_step(flacgpu_decoder_session *ses, const uint8_t *const *chunk, const uint64_t *len, const uint8_t *flush,
                 bool finish) {
    flacgpu_decoder *d = ses->d;
    const uint32_t n = (uint32_t)ses->streams.size();
    SessionFeed feed(ses);
    try {
        feed.begin(n);
        for (uint32_t i = 0; i < n; i++) {
            const flacgpu_decoder_session::Stream &st = ses->streams[i];
            const uint64_t fresh = chunk && chunk[i] ? len[i] : 0;
            if (st.held + fresh)   // else nothing held, nothing new
                feed.add(i, st, fresh ? chunk[i] : nullptr, fresh, finish || (flush && flush[i]), 0, 0);
        }
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_session_feed: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (int rc = feed.refused()) return rc;
    if (int rc = feed.commit_and_scan(LinkRule::Session, true)) return rc;
    const SlotLayout &lay = feed.lay;
    const Candidates &c = feed.c;
    RawTotals tot;
    try {
        d->records.reserve(c.n);
        d->raw_tab.reserve(c.n);
        d->frame_tab.reserve(c.n);
        for (uint32_t i = 0; i < n; i++) {
            flacgpu_decoder_session::Stream &st = ses->streams[i];
            const size_t first = d->records.size();
            const int32_t s = d->slot_of[i];
            if (s >= 0) {
                const ScanSlot &sl = lay.slots[s];
                const flacenc::RawWalk w = walk_slot(
                    c, sl, (uint32_t)s,
                    [&](size_t k, uint64_t at, uint64_t end, bool) {
                        keep_raw_frame(d, i, at, end, lay.end_of((uint32_t)s), st.base + (at - sl.base), c.info[k],
                                       c.heads.data() + kHeadBytes * k, false, tot);
                    },
                    &st.count);
                const uint64_t h = flacenc::session_hold(w, sl.base, sl.len, feed.info[s].final, st.count);
                st.base += h - sl.base;
                st.held = sl.base + sl.len - h;
                st.at = h;
            }
            const size_t count = d->records.size() - first;
            flacgpu_raw_stream &sum = d->raw_streams[i];
            sum = flacenc::session_summary(st.count, first, d->records.data() + first, count);
            join_regular(d, i, s, first, count, sum.uniform, tot);
        }
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_session_feed: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    feed.walked();
    if (int rc = finish_raw_scan(d, feed.lay, tot, "flacgpu_decoder_session_feed")) return rc;
    feed.done();
    return FLACGPU_OK;
}

// The metadata walk of one feed of a container session (kernels/meta_feed_rule.h): meta[i] is stream i's walk behind this
// feed's bytes, used[i] how many of them belong to the metadata.  Host chunks (door 0) are walked here; device chunks
// (door 1) by k_meta_feed where they lie -- the state table stays in device memory from feed to feed, goes up only when a
// host feed has changed it, and comes down with the counts.  Nothing of the session changes but that table and its flag.
int container_meta(flacgpu_decoder_session *ses, int door, const uint8_t *const *data, const size_t *len,
                   std::vector<MetaFeed> &meta, std::vector<uint64_t> &used) {
    flacgpu_decoder *d = ses->d;
    const uint32_t n = (uint32_t)ses->cs.size();
    std::vector<DevSource> src;
    bool any = false;
    ses->meta_fresh = false;
    try {
        meta.resize(n);
        used.assign(n, 0);
        src.assign(n, DevSource{nullptr, 0});
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_session_feed: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    for (uint32_t i = 0; i < n; i++) {
        meta[i] = ses->cs[i].meta;
        if (door == 2 || ses->cs[i].phase != flacenc::CS_META || !data[i] || !len[i]) continue;
        any = true;
        if (door == 0) used[i] = meta_feed(meta[i], data[i], len[i]);
        else src[i] = DevSource{data[i], len[i]};
    }
    if (!any) return FLACGPU_OK;
    if (door == 0) {
        ses->meta_on_device = false;
        return FLACGPU_OK;
    }
    if (int rc = ses->meta_tab.ensure(sizeof(MetaFeed) * n)) return rc;
    if (int rc = ses->meta_src.ensure(sizeof(DevSource) * n)) return rc;
    if (int rc = ses->meta_used.ensure(8 * (size_t)n)) return rc;
    if (!ses->meta_on_device)
        HIP_TRY(hipMemcpyAsync(ses->meta_tab.p, meta.data(), sizeof(MetaFeed) * n, hipMemcpyHostToDevice, d->st));
    ses->meta_on_device = false;   // until the table and this feed's result are known to agree
    HIP_TRY(hipMemcpyAsync(ses->meta_src.p, src.data(), sizeof(DevSource) * n, hipMemcpyHostToDevice, d->st));
    hipLaunchKernelGGL(k_meta_feed, dim3((n + 63) / 64), dim3(64), 0, d->st, ses->meta_src.as<const DevSource>(), n,
                       ses->meta_tab.as<MetaFeed>(), ses->meta_used.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(meta.data(), ses->meta_tab.p, sizeof(MetaFeed) * n, hipMemcpyDeviceToHost, d->st));
    HIP_TRY(hipMemcpyAsync(used.data(), ses->meta_used.p, 8 * (size_t)n, hipMemcpyDeviceToHost, d->st));
    HIP_TRY(hipStreamSynchronize(d->st));
    ses->meta_fresh = true;
    return FLACGPU_OK;
}

// One feed of a container session behind its argument checks and container_meta (finish: no bytes, the input ends).
// chunk[i]: DEVICE address of what stream i was fed behind its metadata (null: none), len[i] the count; fed_now[i]: all
// the bytes it was fed.  The rule of a stream is host/container_rule.h's; a stream in its frame phase gets a slot of
// tail + chunk with STREAMINFO's channels and min_frame, the device finds the regular scan's candidates and links them by
// the rule (k_link_container), and the host follows the chain from the cursor as scan_impl follows k_link's.  The
// decoder is left as scan_impl leaves it, for the batch "every STREAMINFO with the frames decided now".
int container_step(flacgpu_decoder_session *ses, const uint8_t *const *chunk, const uint64_t *len, const uint64_t *fed_now,
                   const std::vector<MetaFeed> &meta, bool finish) {
    using Ses = flacgpu_decoder_session;
    flacgpu_decoder *d = ses->d;
    const uint32_t n = (uint32_t)ses->streams.size();
    SessionFeed feed(ses);
    std::vector<Ses::Stream> streams;   // the session's own state in copies, swapped in at the commit
    std::vector<Ses::Container> cs;
    try {
        feed.begin(n);
        streams = ses->streams;
        cs = ses->cs;
        for (uint32_t i = 0; i < n; i++) {
            Ses::Container &k = cs[i];
            Ses::Stream &st = streams[i];
            if (!ses->hashed && k.in_feed) k.broken = true;   // the feed before decided frames that were never hashed
            k.in_feed = false;
            flacenc::container_begin(k, meta[i], fed_now[i], finish, &st.base);
            const uint64_t fresh = chunk && chunk[i] ? len[i] : 0;
            if (k.phase == flacenc::CS_FRAMES && st.held + fresh)
                feed.add(i, st, fresh ? chunk[i] : nullptr, fresh, finish, k.info.channels, k.min_frame);
        }
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_session_feed: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (int rc = feed.refused()) return rc;
    ses->streams.swap(streams);
    ses->cs.swap(cs);
    if (int rc = feed.commit_and_scan(LinkRule::Container, false)) return rc;
    const SlotLayout &lay = feed.lay;
    try {
        d->frame_tab.reserve(feed.c.n);
        for (uint32_t i = 0; i < n; i++) {
            Ses::Container &k = ses->cs[i];
            Ses::Stream &st = ses->streams[i];
            const size_t first = d->frame_tab.size();
            const int32_t s = d->slot_of[i];
            uint64_t samples = 0;
            if (s >= 0) {
                const ScanSlot &sl = lay.slots[s];
                const flacenc::RegularWalk w = walk_regular_slot(d, feed.c, lay, (uint32_t)s,
                                                                 flacenc::session_judged(sl.base, sl.len, finish), k.info, &samples);
                k.bad_frames += w.lost;
                st.base += w.cursor - sl.base;
                st.held = flacenc::container_end(k, w, sl.base + sl.len, d->frame_tab.size() - first, samples);
                st.at = w.cursor;
            }
            const size_t F = d->frame_tab.size() - first;
            k.in_feed = F != 0;
            if (F) {
                flacgpu_decoded_stream &r = d->res[i];
                r.rc = FLACGPU_OK;
                r.info = k.info;
                r.info.frames = (uint32_t)F;
                r.info.decoded_samples = samples;
                r.info.md5_status = 3;   // the MD5 is the session's, across feeds
            } else {
                d->res[i].rc = FLACGPU_ERR_INVALID_ARG;
            }
            d->raw_streams[i] = flacenc::container_summary(k, first);
        }
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_session_feed: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (d->frame_tab.size() > 0x7FFFFFFFull) {
        g_last_error = "flacgpu_decoder_session_feed: more than 2^31 - 1 frames";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    const RawTotals tot = lay_out_regular(d, lay);
    feed.walked();
    d->raw_elements = tot.total;
    d->raw_scratch = 0;
    if (int rc = finish_scan(d, feed.lay, tot.total, tot.scratch_total)) return rc;
    ses->hashed = d->frame_tab.empty();
    feed.done();
    return FLACGPU_OK;
}

// The frame kernels over one frame table, for every decode call: K_d1 decodes each frame into planar scratch, K_d2 tests
// its CRC-16, and the finish kernel that the caller launches behind them counts the frames that did not parse.
// counts[2 k] / counts[2 k + 1]: the frames of pair k that did not parse / whose CRC-16 is wrong, where k is the table's
// `slot` -- a slot of the scan, a frame or a window.  A table without frames launches nothing; a call without pairs
// still owns a pair, so that counts.p is memory a kernel may be handed.
struct FramePass {
    flacgpu_decoder *d;
    const ManyFrame *frames = nullptr;   // device memory
    uint32_t F = 0;
    size_t pairs = 0;

    // scratch (of scratch_elems samples), codes and counts are there, and the counts are zero on the decoder's stream
    int open(const ManyFrame *table, uint32_t n_frames, uint64_t scratch_elems, size_t n_pairs) {
        frames = table;
        F = n_frames;
        pairs = n_pairs;
        const size_t count_bytes = 8 * std::max<size_t>(pairs, 1);
        if (int rc = d->counts.ensure(count_bytes)) return rc;
        if (F) {
            if (int rc = d->scratch.ensure(4 * scratch_elems)) return rc;
            if (int rc = d->codes.ensure(4 * (size_t)F)) return rc;
        }
        HIP_TRY(hipMemsetAsync(d->counts.p, 0, count_bytes, d->st));
        return FLACGPU_OK;
    }
    // K_d1, a lane per frame in waves of 32 lanes (every lane reads and writes cache lines of its own: decode.hip's
    // launch_decode measured 32 against 64, 16 and 8), and K_d2
    void launch() const {
        if (!F) return;
        const uint32_t lanes = 32;
        hipLaunchKernelGGL(k_decode_many<32>, dim3((F + lanes - 1) / lanes), dim3(lanes), 0, d->st,
                           d->bytes.as<const uint32_t>(), frames, F, d->scratch.as<int32_t>(), d->codes.as<uint32_t>());
        hipLaunchKernelGGL(k_frame_crc, dim3(F), dim3(64), 0, d->st, d->bytes.as<const uint8_t>(), frames,
                           d->counts.as<uint32_t>());
    }
    // The pairs on their way into `counts`, behind everything launched so far: read them after the caller's
    // synchronisation.  No exception crosses the C ABI; the kernels are waited for before a refusal returns.
    int fetch(std::vector<uint32_t> &counts, const char *who) const {
        try {
            counts.resize(2 * pairs);
        } catch (const std::bad_alloc &) {
            (void)hipStreamSynchronize(d->st);
            g_last_error = std::string(who) + ": out of host memory";
            return FLACGPU_ERR_UNSUPPORTED;
        }
        if (pairs) HIP_TRY(hipMemcpyAsync(counts.data(), d->counts.p, 8 * pairs, hipMemcpyDeviceToHost, d->st));
        return FLACGPU_OK;
    }
};
// bit 0: the frame of this pair did not parse; bit 1: its CRC-16 is wrong (a pair that counts one frame)
inline uint32_t pair_status(const std::vector<uint32_t> &counts, size_t k) {
    return (counts[2 * k] ? 1u : 0u) | (counts[2 * k + 1] ? 2u : 0u);
}

// Where a call's kernels write: the caller's buffer when that is device memory, else a buffer of the decoder's, which
// `download` sends to the caller's behind the kernels.  An output without bytes is never staged.
struct OutStage {
    void *out = nullptr, *dst = nullptr;
    size_t bytes = 0;
    bool staged = false;
    int open(DevBuf &stage, void *out_, size_t bytes_, bool to_device) {
        out = dst = out_;
        bytes = bytes_;
        staged = !to_device && bytes;
        if (!staged) return FLACGPU_OK;
        if (int rc = stage.ensure(bytes)) return rc;
        dst = stage.p;
        return FLACGPU_OK;
    }
    int download(hipStream_t st) const {
        if (staged) HIP_TRY(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, st));
        return FLACGPU_OK;
    }
};

// f(std::integral_constant<uint32_t, DT_*>{}) for the FLACGPU_SAMPLE_* value `dtype` (a validated one)
template <class F> void with_dtype(uint32_t dtype, F f) {
    if (dtype == FLACGPU_SAMPLE_I16) f(std::integral_constant<uint32_t, DT_I16>{});
    else if (dtype == FLACGPU_SAMPLE_F32) f(std::integral_constant<uint32_t, DT_F32>{});
    else if (dtype == FLACGPU_SAMPLE_S24) f(std::integral_constant<uint32_t, DT_S24>{});
    else f(std::integral_constant<uint32_t, DT_I32>{});
}

int refuse_rows(const char *who, uint64_t rows) {
    if (rows <= 0x7FFFFFFFull) return FLACGPU_OK;
    g_last_error = std::string(who) + ": more than 2^31 - 1 padded rows";
    return FLACGPU_ERR_UNSUPPORTED;
}

// ---- what the three plans refuse alike: `who` is the call, the differing words are the caller's ----
// `what` ("stream 3", "window 3") with `detail` ("2 channels, 100 samples") does not fit the padded batch
int refuse_fit(const std::string &who, const std::string &what, const std::string &detail) {
    g_last_error = who + ": " + what + " (" + detail + ") does not fit channels_padded x samples_padded";
    return FLACGPU_ERR_INVALID_ARG;
}
// a stream of `bps` bits per sample does not go into `dtype`
bool too_wide(uint32_t dtype, uint32_t bps) { return sample_type_max_bits(dtype) && bps > sample_type_max_bits(dtype); }
int refuse_bits(const std::string &who, uint32_t dtype, uint32_t stream, uint32_t bps) {
    g_last_error = who + ": " + sample_type_name(dtype) + " output, but stream " + std::to_string(stream) + " has " +
                   std::to_string(bps) + " bits per sample";
    return FLACGPU_ERR_UNSUPPORTED;
}
// *bytes = rows * row_elems * elem_bytes, refused when that overflows: `what` ("the padded batch exceeds")
int padded_bytes(const std::string &who, const char *what, uint64_t rows, uint64_t row_elems, uint64_t elem_bytes,
                 uint64_t *bytes) {
    uint64_t b = 0;
    if (__builtin_mul_overflow(rows, row_elems, &b) || __builtin_mul_overflow(b, elem_bytes, &b)) {
        g_last_error = who + ": " + what + " 2^64 bytes";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    *bytes = b;
    return FLACGPU_OK;
}

// K_d6 over the rows of a padded batch (streams or windows x channels_padded), whose table lies in pad_streams: zeroes
// what no frame writes.  A batch without an element has no row to launch for.
void launch_pad_rows(flacgpu_decoder *d, uint32_t rows, const flacgpu_out_format &fmt, void *dst) {
    if (!rows || !fmt.samples_padded) return;
    with_dtype(fmt.dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_pad_rows<elem_bytes<decltype(dt)::value>()>, dim3(rows), dim3(WG), 0, d->st,
                           d->pad_streams.as<const PadStream>(), fmt.channels_padded, fmt.samples_padded,
                           static_cast<uint8_t *>(dst));
    });
}

// flacgpu_decoder_decode_frames behind its argument checks: the frame pass over decode_frames' own table, whose slots
// are the frames, so that pair f says whether frame f parsed and whether its CRC-16 is right.
int decode_frames_impl(flacgpu_decoder *d, int32_t *out, uint32_t flags, flacgpu_frame_record *records) {
    DeviceGuard guard(d->device);
    const uint32_t F = (uint32_t)d->records.size();
    if (!F) return FLACGPU_OK;   // a call without a record to fill does nothing at all
    OutStage o;
    if (int rc = o.open(d->out_stage, out, 4 * d->raw_elements, flags & FLACGPU_DECODE_OUT_DEVICE)) return rc;
    if (!d->raw_tab_uploaded) {   // once per scan: a batch that only goes through decode / decode_as never pays for it
        if (int rc = d->raw_frames.ensure(sizeof(ManyFrame) * (size_t)F)) return rc;
        HIP_TRY(hipMemcpyAsync(d->raw_frames.p, d->raw_tab.data(), sizeof(ManyFrame) * (size_t)F, hipMemcpyHostToDevice, d->st));
        HIP_TRY(hipStreamSynchronize(d->st));
        d->raw_tab_uploaded = true;
    }
    FramePass pass{d};
    if (int rc = pass.open(d->raw_frames.as<const ManyFrame>(), F, d->raw_scratch, F)) return rc;
    pass.launch();
    hipLaunchKernelGGL(k_finish_many, dim3(F), dim3(WG), 0, d->st, pass.frames, d->scratch.as<const int32_t>(),
                       d->codes.as<const uint32_t>(), static_cast<int32_t *>(o.dst), d->counts.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> counts;
    if (int rc = pass.fetch(counts, "flacgpu_decoder_decode_frames")) return rc;
    if (int rc = o.download(d->st)) return rc;
    HIP_TRY(hipStreamSynchronize(d->st));
    memcpy(records, d->records.data(), sizeof(flacgpu_frame_record) * F);
    for (uint32_t f = 0; f < F; f++) records[f].status = pair_status(counts, f);
    return FLACGPU_OK;
}

// ---- frame analysis (flacgpu_decoder_plan_analysis / flacgpu_decoder_analyze) ----
// The frames an analysis covers: every kept frame of a raw scan, else the scan's frame table.
const std::vector<ManyFrame> &analysis_table(const flacgpu_decoder *d) { return d->raw ? d->raw_tab : d->frame_tab; }
struct AnalysisSizes {
    uint64_t frames = 0, subframes = 0, rows = 0;
};
AnalysisSizes analysis_sizes(const flacgpu_decoder *d) {
    AnalysisSizes z;
    for (const ManyFrame &fr : analysis_table(d)) {
        z.frames++;
        z.subframes += fr.channels;
        z.rows += (uint64_t)fr.channels * ((fr.n + 3u) & ~3u);
    }
    return z;
}

// flacgpu_decoder_analyze behind its argument checks.  The frame pass' table is the scan's with `slot` = the frame (so
// that k_frame_crc's pair f is frame f's own), `scratch` = row_offset and `out` = first_subframe: the two prefix sums.
// rows == nullptr: the records-only pass.
int analyze_impl(flacgpu_decoder *d, uint32_t flags, flacgpu_frame_analysis *frames, flacgpu_subframe_plan *subframes,
                 int32_t *rows, const AnalysisSizes &z) {
    DeviceGuard guard(d->device);
    const uint32_t F = (uint32_t)z.frames;
    if (!F) return FLACGPU_OK;
    if (!d->an_tab_uploaded) {
        std::vector<ManyFrame> tab;
        try {
            tab = analysis_table(d);
        } catch (const std::bad_alloc &) {
            g_last_error = "flacgpu_decoder_analyze: out of host memory";
            return FLACGPU_ERR_UNSUPPORTED;
        }
        uint64_t sub_at = 0, row_at = 0;
        for (uint32_t f = 0; f < F; f++) {
            ManyFrame &fr = tab[f];
            fr.slot = f;
            fr.out = sub_at;
            fr.scratch = row_at;
            sub_at += fr.channels;
            row_at += (uint64_t)fr.channels * ((fr.n + 3u) & ~3u);
        }
        if (int rc = d->an_frames.ensure(sizeof(ManyFrame) * (size_t)F)) return rc;
        HIP_TRY(hipMemcpyAsync(d->an_frames.p, tab.data(), sizeof(ManyFrame) * (size_t)F, hipMemcpyHostToDevice, d->st));
        HIP_TRY(hipStreamSynchronize(d->st));   // the table leaves scope
        d->an_tab_uploaded = true;
    }
    // host output: the three arrays are staged back to back in one buffer, each at a multiple of 16 bytes
    const size_t fb = sizeof(flacgpu_frame_analysis) * (size_t)F, sb = sizeof(flacgpu_subframe_plan) * (size_t)z.subframes;
    const size_t rb = rows ? 4 * (size_t)z.rows : 0;
    const size_t s_at = (fb + 15) & ~(size_t)15, r_at = s_at + ((sb + 15) & ~(size_t)15);
    const bool staged = !(flags & FLACGPU_DECODE_OUT_DEVICE);
    flacgpu_frame_analysis *d_frames = frames;
    flacgpu_subframe_plan *d_subs = subframes;
    int32_t *d_rows = rows;
    if (staged) {
        if (int rc = d->out_stage.ensure(r_at + rb)) return rc;
        uint8_t *base = d->out_stage.as<uint8_t>();
        d_frames = reinterpret_cast<flacgpu_frame_analysis *>(base);
        d_subs = reinterpret_cast<flacgpu_subframe_plan *>(base + s_at);
        d_rows = rows ? reinterpret_cast<int32_t *>(base + r_at) : nullptr;
    }
    FramePass pass{d};
    if (int rc = pass.open(d->an_frames.as<const ManyFrame>(), F, 0, F)) return rc;
    HIP_TRY(hipMemsetAsync(d_subs, 0, sb, d->st));   // every entry a subframe does not use is 0
    hipLaunchKernelGGL(k_frame_crc, dim3(F), dim3(64), 0, d->st, d->bytes.as<const uint8_t>(), pass.frames,
                       d->counts.as<uint32_t>());
    const uint32_t lanes = 32;   // as K_d1: every lane reads and writes cache lines of its own
    if (rows)
        hipLaunchKernelGGL(k_analyze_many<true>, dim3((F + lanes - 1) / lanes), dim3(lanes), 0, d->st,
                           d->bytes.as<const uint32_t>(), pass.frames, F, d->counts.as<const uint32_t>(), d_frames, d_subs,
                           d_rows);
    else
        hipLaunchKernelGGL(k_analyze_many<false>, dim3((F + lanes - 1) / lanes), dim3(lanes), 0, d->st,
                           d->bytes.as<const uint32_t>(), pass.frames, F, d->counts.as<const uint32_t>(), d_frames, d_subs,
                           d_rows);
    HIP_TRY(hipGetLastError());
    if (staged) {
        HIP_TRY(hipMemcpyAsync(frames, d_frames, fb, hipMemcpyDeviceToHost, d->st));
        HIP_TRY(hipMemcpyAsync(subframes, d_subs, sb, hipMemcpyDeviceToHost, d->st));
        if (rb) HIP_TRY(hipMemcpyAsync(rows, d_rows, rb, hipMemcpyDeviceToHost, d->st));
    }
    HIP_TRY(hipStreamSynchronize(d->st));
    return FLACGPU_OK;
}

// decode_as, before the frame kernels: for PADDED the first element of every frame and the kernel that zeroes what no
// frame writes (rows' tails, absent channels, streams without samples)
int finish_as_tables(flacgpu_decoder *d, const flacgpu_out_format &fmt, void *dst) {
    if (fmt.layout != FLACGPU_LAYOUT_PADDED) return FLACGPU_OK;
    const uint32_t n = (uint32_t)d->res.size(), Cp = fmt.channels_padded;
    const uint64_t T = fmt.samples_padded;
    const size_t F = d->frame_tab.size();
    if (!n || !Cp || !T) return FLACGPU_OK;
    if (int rc = refuse_rows("flacgpu_decoder_decode_as", (uint64_t)n * Cp)) return rc;
    std::vector<uint64_t> first(F);
    for (size_t f = 0; f < F; f++) {
        const ManyFrame &fr = d->frame_tab[f];
        const uint32_t i = d->slot_stream[fr.slot];
        first[f] = (uint64_t)i * Cp * T + (fr.out - d->res[i].out_offset) / fr.channels;
    }
    std::vector<PadStream> ps(n);
    for (uint32_t i = 0; i < n; i++) {
        const flacgpu_decoded_stream &r = d->res[i];
        ps[i] = r.rc == FLACGPU_OK ? PadStream{r.info.decoded_samples, r.info.channels, 0} : PadStream{0, 0, 0};
    }
    if (F) {
        if (int rc = d->pad_out.ensure(8 * F)) return rc;
        HIP_TRY(hipMemcpyAsync(d->pad_out.p, first.data(), 8 * F, hipMemcpyHostToDevice, d->st));
    }
    if (int rc = d->pad_streams.ensure(sizeof(PadStream) * n)) return rc;
    HIP_TRY(hipMemcpyAsync(d->pad_streams.p, ps.data(), sizeof(PadStream) * n, hipMemcpyHostToDevice, d->st));
    HIP_TRY(hipStreamSynchronize(d->st));   // the tables leave scope
    launch_pad_rows(d, n * Cp, fmt, dst);
    HIP_TRY(hipGetLastError());
    return FLACGPU_OK;
}

// flacgpu_decoder_decode / _decode_as behind their argument checks.  fmt == nullptr: interleaved int32, streams back to
// back; else a validated format other than that one, of out_bytes bytes.  d->res keeps the scan's records (a second
// decode of the same scan starts from them); `streams` gets them completed, after everything that can fail.
int decode_impl(flacgpu_decoder *d, void *out, uint32_t flags, flacgpu_decoded_stream *streams,
                const flacgpu_out_format *fmt = nullptr, uint64_t out_bytes = 0) {
    DeviceGuard guard(d->device);
    const uint32_t n = (uint32_t)d->res.size();
    const bool md5 = !(flags & FLACGPU_DECODE_NO_MD5);
    // A container session's decoder hashes across feeds: the first call with MD5 after a feed appends the feed's samples
    // to the session's chains (`chain`), every other call hashes nothing; k_md5_many (`many`) is the other handles'.
    flacgpu_decoder_session *const ses = d->container;
    const bool chain = ses && md5 && !ses->hashed, many = md5 && !ses;
    OutStage o;
    if (int rc = o.open(d->out_stage, out, fmt ? out_bytes : 4 * d->total, flags & FLACGPU_DECODE_OUT_DEVICE)) return rc;
    int32_t *side = nullptr;   // decode_as with MD5: the interleaved int32 that k_md5_many / k_md5_chain reads
    if (fmt) {
        if ((many || chain) && d->total) {
            if (int rc = d->md5_stage.ensure(4 * d->total)) return rc;
            side = d->md5_stage.as<int32_t>();
        }
        if (int rc = finish_as_tables(d, *fmt, o.dst)) return rc;
    }
    const int32_t *hashed = fmt ? side : static_cast<const int32_t *>(o.dst);
    FramePass pass{d};
    if (int rc = pass.open(d->frames.as<const ManyFrame>(), (uint32_t)d->frame_tab.size(), d->scratch_total, d->n_slots))
        return rc;
    pass.launch();
    if (pass.F && !fmt) {
        hipLaunchKernelGGL(k_finish_many, dim3(pass.F), dim3(WG), 0, d->st, pass.frames, d->scratch.as<const int32_t>(),
                           d->codes.as<const uint32_t>(), static_cast<int32_t *>(o.dst), d->counts.as<uint32_t>());
    } else if (pass.F) {
        const bool padded = fmt->layout == FLACGPU_LAYOUT_PADDED;
        with_dtype(fmt->dtype, [&](auto dt) {
            constexpr uint32_t DT = decltype(dt)::value;
            auto k = side ? k_finish_as<DT, true, true> : k_finish_as<DT, true, false>;
            if constexpr (DT != DT_I32)   // I32 / FLAT took the branch above: no k_finish_as<DT_I32, false, *> is made
                if (!padded) k = side ? k_finish_as<DT, false, true> : k_finish_as<DT, false, false>;
            hipLaunchKernelGGL(k, dim3(pass.F), dim3(WG), 0, d->st, pass.frames, d->scratch.as<const int32_t>(),
                               d->codes.as<const uint32_t>(), static_cast<uint8_t *>(o.dst), d->pad_out.as<const uint64_t>(),
                               fmt->samples_padded, side, d->counts.as<uint32_t>());
        });
    }
    HIP_TRY(hipGetLastError());
    std::vector<Md5Job> jobs;
    std::vector<uint32_t> job_stream, digest;
    if (chain) {   // on the decoder's stream, behind the kernel that wrote the samples; no synchronisation of its own
        std::vector<flacgpu_md5_piece> pieces;
        std::vector<uint32_t> widths;
        try {
            for (uint32_t i = 0; i < n; i++) {
                const flacgpu_decoded_stream &r = d->res[i];
                if (r.rc != FLACGPU_OK || !r.info.decoded_samples) continue;
                pieces.push_back(flacgpu_md5_piece{i, 0, r.out_offset, r.info.decoded_samples * r.info.channels});
                widths.push_back((r.info.bits_per_sample + 7) / 8);
            }
        } catch (const std::bad_alloc &) {
            (void)hipStreamSynchronize(d->st);
            g_last_error = "flacgpu_decoder_decode: out of host memory";
            return FLACGPU_ERR_UNSUPPORTED;
        }
        if (int rc = flacgpu_k::md5_chains_update_widths(ses->chains, hashed, pieces.data(), widths.data(),
                                                         (uint32_t)pieces.size(), d->st)) {
            (void)hipStreamSynchronize(d->st);
            return rc;
        }
    }
    if (many) {
        for (uint32_t i = 0; i < n; i++) {
            const flacgpu_decoded_stream &r = d->res[i];
            if (r.rc != FLACGPU_OK) continue;
            Md5Job j{};
            j.off = r.out_offset;
            j.count = r.info.decoded_samples * r.info.channels;
            j.width = (r.info.bits_per_sample + 7) / 8;
            memcpy(j.expect, r.info.md5, 16);
            jobs.push_back(j);
            job_stream.push_back(i);
        }
    }
    const uint32_t J = (uint32_t)jobs.size();
    if (J) {
        if (int rc = d->jobs.ensure(sizeof(Md5Job) * J)) return rc;
        if (int rc = d->digest.ensure(20 * (size_t)J)) return rc;
        HIP_TRY(hipMemcpyAsync(d->jobs.p, jobs.data(), sizeof(Md5Job) * J, hipMemcpyHostToDevice, d->st));
        hipLaunchKernelGGL(k_md5_many, dim3((J + 63) / 64), dim3(64), 0, d->st, hashed, d->jobs.as<const Md5Job>(), J,
                           d->digest.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        digest.resize(5 * (size_t)J);
        HIP_TRY(hipMemcpyAsync(digest.data(), d->digest.p, 20 * (size_t)J, hipMemcpyDeviceToHost, d->st));
    }
    std::vector<uint32_t> counts;
    if (int rc = pass.fetch(counts, fmt ? "flacgpu_decoder_decode_as" : "flacgpu_decoder_decode")) return rc;
    if (int rc = o.download(d->st)) return rc;
    HIP_TRY(hipStreamSynchronize(d->st));   // the jobs leave scope behind this
    if (n) memcpy(streams, d->res.data(), sizeof(flacgpu_decoded_stream) * n);
    for (uint32_t i = 0; i < n; i++) {
        flacgpu_decoded_stream &r = streams[i];
        const int32_t s = d->slot_of[i];
        if (s >= 0 && r.info.frames) {
            r.info.bad_frames += counts[2 * (size_t)s];
            r.info.bad_crc16 = counts[2 * (size_t)s + 1];
        }
        if (r.rc == FLACGPU_OK && !many) r.info.md5_status = 3;
        if (chain) {   // the session's counts: what this feed's frames add
            ses->cs[i].bad_frames += r.info.bad_frames;
            ses->cs[i].bad_crc16 += r.info.bad_crc16;
        }
    }
    if (chain) ses->hashed = true;
    for (uint32_t j = 0; j < J; j++) {
        flacgpu_stream_info &info = streams[job_stream[j]].info;
        memcpy(info.decoded_md5, &digest[5 * (size_t)j], 16);
        info.md5_status = digest[5 * (size_t)j + 4];
    }
    return FLACGPU_OK;
}

// ---- sample windows ----
// The frames of a stream that samples [start, start + length) touch.  first_of(i) is the first sample of frame i of
// the stream's n_frames, rising; the stream has `total` samples.  A window that is empty or lies past the end touches
// none.  skip: the samples of frame `first` in front of `start`.
template <class FirstOf>
void window_frames(FirstOf first_of, uint32_t n_frames, uint64_t total, uint64_t start, uint64_t length,
                   uint32_t *first, uint32_t *count, uint64_t *skip) {
    *first = *count = 0;
    *skip = 0;
    const uint64_t end = std::min(start + length, total);
    if (start >= end) return;
    const auto holding = [&](uint64_t sample) {   // the last frame that starts at or before `sample`
        uint32_t lo = 0, hi = n_frames;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (first_of(mid) <= sample) lo = mid;
            else hi = mid;
        }
        return lo;
    };
    *first = holding(start);
    *count = holding(end - 1) - *first + 1;
    *skip = start - first_of(*first);
}

void index_frames(flacgpu_decoder *d) {
    const size_t F = d->frame_tab.size();
    d->slot_frame0.assign((size_t)d->n_slots + 1, (uint32_t)F);
    d->frame_first.resize(F);
    for (size_t f = F; f-- > 0;) {
        const ManyFrame &fr = d->frame_tab[f];
        d->slot_frame0[fr.slot] = (uint32_t)f;
        d->frame_first[f] = (fr.out - d->res[d->slot_stream[fr.slot]].out_offset) / fr.channels;
    }
    for (uint32_t s = d->n_slots; s-- > 0;)   // a slot without frames owns an empty run
        d->slot_frame0[s] = std::min(d->slot_frame0[s], d->slot_frame0[s + 1]);
}

// ---- selected frames: the path that sample windows and timelines share ----
// The frames a call chose from the scan's tables, compact, with scratch of their own (by the chosen frames, not by the
// batch), each with the place in a padded row where K_d7 puts what is kept of it.  Its `window` is the pair that counts
// it: the frame's `slot` for the frame pass.
struct Selected {
    std::vector<ManyFrame> sel;
    std::vector<WinFrame> desc;
    uint64_t scratch_total = 0;
    FramePass pass;

    explicit Selected(flacgpu_decoder *d) : pass{d} {}
    bool too_many() const { return sel.size() > 0x7FFFFFFFull; }
    // wf: row, at, keep_first, keep_last and window are the caller's
    void add(ManyFrame fr, WinFrame wf) {
        wf.channels = fr.channels;
        wf.bps = fr.bps;
        fr.slot = wf.window;
        fr.scratch = scratch_total;
        scratch_total += (uint64_t)fr.channels * ((fr.n + 3u) & ~3u);
        sel.push_back(fr);
        desc.push_back(wf);
    }
    // Before any frame, on the decoder's stream: the counts of `pairs` pairs zeroed and K_d6 over the rows of `pad`, whose
    // samples and channels stand where k_pad_rows reads a stream's: it zeroes what no frame writes.
    int open(const std::vector<PadStream> &pad, const flacgpu_out_format &fmt, void *dst, size_t pairs) {
        flacgpu_decoder *d = pass.d;
        const size_t F = sel.size();
        if (int rc = d->pad_streams.ensure(sizeof(PadStream) * pad.size())) return rc;
        if (F) {
            if (int rc = d->win_frames.ensure(sizeof(ManyFrame) * F)) return rc;
            if (int rc = d->win_desc.ensure(sizeof(WinFrame) * F)) return rc;
        }
        if (int rc = pass.open(d->win_frames.as<const ManyFrame>(), (uint32_t)F, scratch_total, pairs)) return rc;
        HIP_TRY(hipMemcpyAsync(d->pad_streams.p, pad.data(), sizeof(PadStream) * pad.size(), hipMemcpyHostToDevice, d->st));
        launch_pad_rows(d, (uint32_t)pad.size() * fmt.channels_padded, fmt, dst);
        return FLACGPU_OK;
    }
    // The frames: their tables onto the device, the frame pass, K_d7.  `pad`, sel and desc are on their way until the
    // caller has waited for the stream.
    int run(const flacgpu_out_format &fmt, void *dst) {
        flacgpu_decoder *d = pass.d;
        const uint32_t F = pass.F;
        if (!F) return FLACGPU_OK;
        HIP_TRY(hipMemcpyAsync(d->win_frames.p, sel.data(), sizeof(ManyFrame) * F, hipMemcpyHostToDevice, d->st));
        HIP_TRY(hipMemcpyAsync(d->win_desc.p, desc.data(), sizeof(WinFrame) * F, hipMemcpyHostToDevice, d->st));
        pass.launch();
        with_dtype(fmt.dtype, [&](auto dt) {
            hipLaunchKernelGGL(k_finish_window<decltype(dt)::value>, dim3(F), dim3(WG), 0, d->st, pass.frames,
                               d->win_desc.as<const WinFrame>(), d->scratch.as<const int32_t>(),
                               d->codes.as<const uint32_t>(), static_cast<uint8_t *>(dst), fmt.samples_padded,
                               d->counts.as<uint32_t>());
        });
        return FLACGPU_OK;
    }
};

// flacgpu_decoder_decode_windows behind its argument checks: out_bytes > 0, every window valid for `fmt`
int decode_windows_impl(flacgpu_decoder *d, void *out, uint64_t out_bytes, const flacgpu_out_format &fmt, uint32_t flags,
                        const flacgpu_window *w, uint32_t n_windows, flacgpu_window_result *results) {
    DeviceGuard guard(d->device);
    const uint32_t Cp = fmt.channels_padded;
    const uint64_t T = fmt.samples_padded;
    if (int rc = refuse_rows("flacgpu_decoder_decode_windows", (uint64_t)n_windows * Cp)) return rc;
    // ---- host: the frames every window touches
    Selected s(d);
    std::vector<PadStream> pad(n_windows);
    try {
        for (uint32_t i = 0; i < n_windows; i++) {
            const flacgpu_decoded_stream &r = d->res[w[i].stream];
            flacgpu_window_result &res = results[i];
            res = flacgpu_window_result{};
            res.rc = r.rc;
            pad[i] = PadStream{0, 0, 0};
            const int32_t slot = d->slot_of[w[i].stream];
            if (r.rc != FLACGPU_OK || slot < 0) continue;
            const uint32_t f0 = d->slot_frame0[slot], nf = d->slot_frame0[slot + 1] - f0;
            uint32_t first = 0, count = 0;
            uint64_t skip = 0;
            window_frames([&](uint32_t k) { return d->frame_first[f0 + k]; }, nf, r.info.decoded_samples, w[i].start,
                          w[i].length, &first, &count, &skip);
            if (!count) continue;
            res.frames = count;
            res.samples = std::min(w[i].length, r.info.decoded_samples - w[i].start);
            pad[i] = PadStream{res.samples, r.info.channels, 0};
            for (uint32_t k = 0; k < count; k++) {
                const ManyFrame &fr = d->frame_tab[f0 + first + k];
                const uint64_t at = d->frame_first[f0 + first + k];   // the frame's first sample in the stream
                WinFrame wf{};
                wf.row = (uint64_t)i * Cp * T;
                wf.keep_first = k ? 0 : (uint32_t)skip;
                wf.keep_last = (uint32_t)std::min<uint64_t>(fr.n, w[i].start + res.samples - at);
                wf.at = at + wf.keep_first - w[i].start;
                wf.window = i;   // k_frame_crc counts per window
                s.add(fr, wf);
            }
        }
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_decode_windows: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (s.too_many()) {
        g_last_error = "flacgpu_decoder_decode_windows: more than 2^31 - 1 selected frames";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    OutStage o;
    if (int rc = o.open(d->out_stage, out, out_bytes, flags & FLACGPU_DECODE_OUT_DEVICE)) return rc;
    if (int rc = s.open(pad, fmt, o.dst, n_windows)) return rc;
    if (int rc = s.run(fmt, o.dst)) return rc;
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> counts;
    if (int rc = s.pass.fetch(counts, "flacgpu_decoder_decode_windows")) return rc;
    if (int rc = o.download(d->st)) return rc;
    HIP_TRY(hipStreamSynchronize(d->st));   // the tables leave scope behind this
    for (uint32_t i = 0; i < n_windows; i++) {
        results[i].bad_frames = counts[2 * (size_t)i];
        results[i].bad_crc16 = counts[2 * (size_t)i + 1];
    }
    return FLACGPU_OK;
}

// ---- frames on a timeline ----
// The rule for every stream of the raw scan: results[i], and (frames != nullptr) every record's place.  `who` names the
// call in the last-error text, which is set for the first refused stream.
void timeline_streams(const flacgpu_decoder *d, flacgpu_timeline_result *results, flacgpu_timeline_frame *frames,
                      const char *who) {
    bool noted = false;
    for (size_t i = 0; i < d->raw_streams.size(); i++) {
        const flacgpu_raw_stream &rs = d->raw_streams[i];
        const char *why = flacenc::timeline_of_records(d->records.data() + rs.first_frame, rs.frames,
                                                       frames ? frames + rs.first_frame : nullptr, results[i]);
        if (why && !noted) {
            g_last_error = std::string(who) + ": stream " + std::to_string(i) + ": " + why;
            noted = true;
        }
    }
}

// plan_timeline's checks of `fmt` against the streams' timelines; the bytes of `out` and of the mask
int timeline_check(const flacgpu_decoder *d, const flacgpu_out_format *fmt, const flacgpu_timeline_result *results,
                   const std::string &who, uint64_t *out_bytes, uint64_t *mask_bytes) {
    const uint32_t n = (uint32_t)d->raw_streams.size();
    if (!sample_type_known(fmt->dtype) || fmt->layout != FLACGPU_LAYOUT_PADDED || fmt->reserved) {
        g_last_error = who + ": unknown dtype, a layout other than PADDED, or reserved not 0";
        return FLACGPU_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (results[i].rc != FLACGPU_OK) continue;
        const flacgpu_frame_record &r0 = d->records[d->raw_streams[i].first_frame];
        if (r0.channels > fmt->channels_padded || results[i].timeline_samples > fmt->samples_padded)
            return refuse_fit(who, "stream " + std::to_string(i), std::to_string(r0.channels) + " channels, " +
                                  std::to_string(results[i].timeline_samples) + " samples on its timeline");
    }
    for (uint32_t i = 0; i < n; i++) {
        if (results[i].rc != FLACGPU_OK) continue;
        const flacgpu_frame_record &r0 = d->records[d->raw_streams[i].first_frame];
        if (too_wide(fmt->dtype, r0.bits_per_sample)) return refuse_bits(who, fmt->dtype, i, r0.bits_per_sample);
    }
    uint64_t bytes = 0, mbytes = 0;   // the caller's stay as they are when either is refused
    const char *what = "the padded batch exceeds";
    if (int rc = padded_bytes(who, what, (uint64_t)n * fmt->channels_padded, fmt->samples_padded,
                              sample_type_bytes(fmt->dtype), &bytes))
        return rc;
    if (int rc = padded_bytes(who, what, n, fmt->samples_padded, 1, &mbytes)) return rc;
    *out_bytes = bytes;
    if (mask_bytes) *mask_bytes = mbytes;
    return FLACGPU_OK;
}

// `count` elements of `es` bytes from element `first`, cut into pieces of at most kFillPiece bytes: every cut lies a
// multiple of 16 bytes behind the run's first byte, so that only the run's own two ends are not whole 16-byte groups
void push_runs(std::vector<FillRun> &runs, uint64_t first, uint64_t count, uint32_t es, uint32_t cond, uint32_t value) {
    const uint64_t per = kFillPiece / es;
    for (uint64_t done = 0; done < count; done += per)
        runs.push_back(FillRun{first + done, (uint32_t)std::min(per, count - done), cond, value, 0});
}

// K_d8 over runs [first, first + count) of tl_runs, whose elements have ES bytes
template <uint32_t ES>
void launch_fill(flacgpu_decoder *d, size_t first, size_t count, void *dst) {
    if (!count) return;
    hipLaunchKernelGGL(k_fill_runs<ES>, dim3((uint32_t)count), dim3(WG), 0, d->st, d->tl_runs.as<const FillRun>() + first,
                       d->counts.as<const uint32_t>(), static_cast<uint8_t *>(dst));
}
void launch_fill_samples(flacgpu_decoder *d, uint32_t dtype, size_t first, size_t count, void *dst) {
    with_dtype(dtype, [&](auto dt) { launch_fill<elem_bytes<decltype(dt)::value>()>(d, first, count, dst); });
}

// flacgpu_decoder_decode_timeline behind its checks (out_bytes > 0): `results` and `tl` (every record's place) are the
// rule's; fills concealed / status.  The placed frames of the streams with rc == 0 go the way of decode_windows'
// selected frames, one "window" per frame, so that the counts come out per frame; k_fill_runs zeroes the gaps beside them
// and, behind k_finish_window and decided by those counts on the device, the frames that did not decode.
int decode_timeline_impl(flacgpu_decoder *d, void *out, uint64_t out_bytes, uint8_t *mask, uint64_t mask_bytes,
                         const flacgpu_out_format &fmt, uint32_t flags, flacgpu_timeline_result *results,
                         std::vector<flacgpu_timeline_frame> &tl) {
    DeviceGuard guard(d->device);
    const uint32_t n = (uint32_t)d->raw_streams.size(), Cp = fmt.channels_padded;
    const uint32_t es = (uint32_t)sample_type_bytes(fmt.dtype);
    const uint64_t T = fmt.samples_padded;
    if (int rc = refuse_rows("flacgpu_decoder_decode_timeline", (uint64_t)n * Cp)) return rc;
    // ---- host: the placed frames; the runs in four groups -- sample gaps, the mask's unconditional runs, the samples'
    // concealment, the mask's concealment
    Selected s(d);
    std::vector<size_t> sel_record;
    std::vector<PadStream> pad(n);
    std::vector<FillRun> gap_runs, mask_runs, hide_runs, mask_hide_runs, runs;
    try {
        s.sel.reserve(tl.size());
        s.desc.reserve(tl.size());
        sel_record.reserve(tl.size());
        hide_runs.reserve(tl.size());
        for (uint32_t i = 0; i < n; i++) {
            pad[i] = PadStream{0, 0, 0};
            if (results[i].rc != FLACGPU_OK) {
                if (mask) push_runs(mask_runs, (uint64_t)i * T, T, 1, FILL_ALWAYS, 0);
                continue;
            }
            const flacgpu_raw_stream &rs = d->raw_streams[i];
            const uint32_t C = d->records[rs.first_frame].channels;
            const uint64_t row = (uint64_t)i * Cp * T;
            pad[i] = PadStream{results[i].timeline_samples, C, 0};
            uint64_t end = 0;   // row position behind the last placed frame
            for (size_t k = rs.first_frame; k < rs.first_frame + rs.frames; k++) {
                if (!(tl[k].flags & FLACGPU_TL_PLACED)) continue;
                const uint64_t at = tl[k].at;
                if (at > end) {
                    for (uint32_t c = 0; c < C; c++) push_runs(gap_runs, row + c * T + end, at - end, es, FILL_ALWAYS, 0);
                    if (mask) push_runs(mask_runs, (uint64_t)i * T + end, at - end, 1, FILL_ALWAYS, 0);
                }
                const uint32_t j = (uint32_t)s.sel.size();
                ManyFrame fr = d->raw_tab[k];
                fr.out = 0;
                WinFrame wf{};
                wf.row = row;
                wf.at = at;
                wf.keep_first = 0;
                wf.keep_last = fr.n;
                wf.window = j;   // k_frame_crc counts per frame
                s.add(fr, wf);
                sel_record.push_back(k);
                for (uint32_t c = 0; c < C; c++) push_runs(hide_runs, row + c * T + at, fr.n, es, j, 0);
                if (mask) {
                    push_runs(mask_runs, (uint64_t)i * T + at, fr.n, 1, FILL_ALWAYS, 1);
                    push_runs(mask_hide_runs, (uint64_t)i * T + at, fr.n, 1, j, 0);
                }
                end = at + fr.n;
            }
            if (mask) push_runs(mask_runs, (uint64_t)i * T + end, T - end, 1, FILL_ALWAYS, 0);
        }
        runs.reserve(gap_runs.size() + mask_runs.size() + hide_runs.size() + mask_hide_runs.size());
        for (const auto *g : {&gap_runs, &mask_runs, &hide_runs, &mask_hide_runs}) runs.insert(runs.end(), g->begin(), g->end());
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_decode_timeline: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (s.too_many() || runs.size() > 0x7FFFFFFFull) {
        g_last_error = "flacgpu_decoder_decode_timeline: more than 2^31 - 1 placed frames or fill runs";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    const bool to_device = flags & FLACGPU_DECODE_OUT_DEVICE;
    OutStage o, m;   // the samples; the mask, if the caller wants one
    if (int rc = o.open(d->out_stage, out, out_bytes, to_device)) return rc;
    if (int rc = m.open(d->tl_mask, mask, mask ? mask_bytes : 0, to_device)) return rc;
    if (!runs.empty())
        if (int rc = d->tl_runs.ensure(sizeof(FillRun) * runs.size())) return rc;
    // rows' tails, absent channels and refused streams; the gaps; the mask's 0s and 1s as if every frame decoded
    if (int rc = s.open(pad, fmt, o.dst, s.sel.size())) return rc;
    if (!runs.empty())
        HIP_TRY(hipMemcpyAsync(d->tl_runs.p, runs.data(), sizeof(FillRun) * runs.size(), hipMemcpyHostToDevice, d->st));
    size_t at = 0;
    launch_fill_samples(d, fmt.dtype, at, gap_runs.size(), o.dst);
    at += gap_runs.size();
    launch_fill<1>(d, at, mask_runs.size(), m.dst);
    at += mask_runs.size();
    if (int rc = s.run(fmt, o.dst)) return rc;
    if (s.pass.F) {   // the concealment: behind the kernels that count, on their stream
        launch_fill_samples(d, fmt.dtype, at, hide_runs.size(), o.dst);
        at += hide_runs.size();
        launch_fill<1>(d, at, mask_hide_runs.size(), m.dst);
    }
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> counts;
    if (int rc = s.pass.fetch(counts, "flacgpu_decoder_decode_timeline")) return rc;
    if (int rc = o.download(d->st)) return rc;
    if (int rc = m.download(d->st)) return rc;
    HIP_TRY(hipStreamSynchronize(d->st));   // the tables leave scope behind this
    for (uint32_t j = 0; j < s.pass.F; j++) {
        const size_t k = sel_record[j];
        const uint32_t status = pair_status(counts, j);
        tl[k].status = status;
        if (!status) continue;
        tl[k].flags |= FLACGPU_TL_CONCEALED;
        flacgpu_timeline_result &r = results[d->records[k].stream];
        r.concealed++;
        r.concealed_samples += d->records[k].block_size;
    }
    return FLACGPU_OK;
}
}  // namespace

// k_md5_many for the encoder's ingest pass (ingest.hip): one job per ingested stream, no digest to compare with
void flacgpu_k::launch_md5_many(const int32_t *samples, const Md5JobRec *jobs, uint32_t n_jobs, uint32_t *digest,
                                hipStream_t st) {
    static_assert(sizeof(Md5JobRec) == sizeof(Md5Job) && offsetof(Md5JobRec, count) == offsetof(Md5Job, count) &&
                      offsetof(Md5JobRec, width) == offsetof(Md5Job, width) &&
                      offsetof(Md5JobRec, expect) == offsetof(Md5Job, expect),
                  "Md5JobRec is Md5Job");
    if (!n_jobs) return;
    hipLaunchKernelGGL(k_md5_many, dim3((n_jobs + 63) / 64), dim3(64), 0, st, samples,
                       reinterpret_cast<const Md5Job *>(jobs), n_jobs, digest);
}

int flacgpu_decoder_create(int device, flacgpu_decoder **out) {
    if (!out) return FLACGPU_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_last_error = "no HIP device";
        return FLACGPU_ERR_NO_DEVICE;
    }
    if (device >= ndev) {
        g_last_error = "no such HIP device";
        return FLACGPU_ERR_NO_DEVICE;
    }
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    flacgpu_decoder *d = new (std::nothrow) flacgpu_decoder();
    if (!d) return FLACGPU_ERR_UNSUPPORTED;
    d->device = device;
    int prev = -1;
    (void)hipGetDevice(&prev);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking);
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        g_last_error = std::string("flacgpu_decoder_create: ") + hipGetErrorString(e);
        delete d;
        return FLACGPU_ERR_HIP;
    }
    *out = d;
    return FLACGPU_OK;
}

void flacgpu_decoder_destroy(flacgpu_decoder *d) {
    if (!d || d->session) return;   // a session's decoder goes with its session (flacgpu_decoder_session_close)
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(d->device);
    if (d->st) (void)hipStreamSynchronize(d->st);
    if (d->st) (void)hipStreamDestroy(d->st);
    d->st = nullptr;
    if (d->ev) (void)hipEventDestroy(d->ev);
    d->ev = nullptr;
    delete d;   // the buffers free themselves, on the decoder's device
    if (prev >= 0) (void)hipSetDevice(prev);
}

// A session's decoder takes its batches from the session's feeds alone: the scan calls leave it as it is.
static bool session_owned(const flacgpu_decoder *d, const char *who) {
    if (!d->session) return false;
    g_last_error = std::string(who) + ": the handle belongs to a decoder session (feed the session instead)";
    return true;
}

// The four scans behind their argument checks: the host door and the device door differ in `in` alone.
static int scan_call(flacgpu_decoder *d, const ScanInput &in, const size_t *len, uint32_t n_streams,
                     flacgpu_decoded_stream *streams, uint64_t *total_samples) {
    if (int rc = scan_impl(d, in, len, n_streams)) return rc;
    index_frames(d);
    d->scanned = true;
    if (n_streams) memcpy(streams, d->res.data(), sizeof(flacgpu_decoded_stream) * n_streams);
    *total_samples = d->total;
    return FLACGPU_OK;
}

// What a raw scan and a session's feed hand back once they are through: the batch is indexed and scanned, and the
// caller gets its streams, their summaries (raw may be null) and the batch's sizes.
static void publish_raw_scan(flacgpu_decoder *d, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                             uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples) {
    const size_t n = d->res.size();
    index_frames(d);
    d->scanned = d->raw = true;
    if (n) memcpy(streams, d->res.data(), sizeof(flacgpu_decoded_stream) * n);
    if (n && raw) memcpy(raw, d->raw_streams.data(), sizeof(flacgpu_raw_stream) * n);
    *total_frames = d->records.size();
    *total_elements = d->raw_elements;
    *total_samples = d->total;
}

static int scan_frames_call(flacgpu_decoder *d, const ScanInput &in, const size_t *len, uint32_t n_streams, uint32_t flags,
                            flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw, uint64_t *total_frames,
                            uint64_t *total_elements, uint64_t *total_samples) {
    if (int rc = scan_raw_impl(d, in, len, n_streams, flags)) return rc;
    publish_raw_scan(d, streams, raw, total_frames, total_elements, total_samples);
    return FLACGPU_OK;
}

// The device door's own checks, before anything is launched: every stream with bytes (a null pointer or a zero length
// is never looked at) must be device memory of the decoder's device -- pinned or managed memory is not --, and where
// the runtime knows the allocation, [d_data[i], d_data[i] + len[i]) must lie inside it.  Then the decoder's stream is
// made to wait for `stream` (NULL: the legacy default stream), so that the first read of the sources is ordered after it.
static int open_device_door(flacgpu_decoder *d, const uint8_t *const *d_data, const size_t *len, uint32_t n_streams,
                            void *stream, const char *who) {
    for (uint32_t i = 0; i < n_streams; i++) {
        if (!d_data[i] || !len[i]) continue;
        hipPointerAttribute_t attr{};
        const hipError_t e = hipPointerGetAttributes(&attr, d_data[i]);
        if (e != hipSuccess) (void)hipGetLastError();   // ordinary host memory is an error to the runtime, not to us
        if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.isManaged || attr.device != d->device) {
            g_last_error = std::string(who) + ": stream " + std::to_string(i) + " is not device memory of device " +
                           std::to_string(d->device);
            return FLACGPU_ERR_INVALID_ARG;
        }
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<uint8_t *>(d_data[i])) != hipSuccess) {
            (void)hipGetLastError();   // an allocation the runtime cannot size: the attributes above are the check
            continue;
        }
        const uintptr_t p = reinterpret_cast<uintptr_t>(d_data[i]), b = reinterpret_cast<uintptr_t>(base);
        if (p < b || len[i] > size || p - b > size - len[i]) {
            g_last_error = std::string(who) + ": stream " + std::to_string(i) + " reaches past the end of its allocation";
            return FLACGPU_ERR_INVALID_ARG;
        }
    }
    if (!d->ev) HIP_TRY(hipEventCreateWithFlags(&d->ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(d->ev, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamWaitEvent(d->st, d->ev, 0));
    return FLACGPU_OK;
}

int flacgpu_decoder_scan(flacgpu_decoder *d, const uint8_t *const *data, const size_t *len, uint32_t n_streams,
                         flacgpu_decoded_stream *streams, uint64_t *total_samples) {
    if (!d || (n_streams && (!data || !len || !streams)) || !total_samples) return FLACGPU_ERR_INVALID_ARG;
    if (session_owned(d, "flacgpu_decoder_scan")) return FLACGPU_ERR_INVALID_ARG;
    d->scanned = d->raw = false;
    DeviceGuard guard(d->device);
    return scan_call(d, ScanInput{data, false}, len, n_streams, streams, total_samples);
}

int flacgpu_decoder_scan_device(flacgpu_decoder *d, const uint8_t *const *d_data, const size_t *len, uint32_t n_streams,
                                void *stream, flacgpu_decoded_stream *streams, uint64_t *total_samples) {
    if (!d || (n_streams && (!d_data || !len || !streams)) || !total_samples) {
        g_last_error = "flacgpu_decoder_scan_device: a NULL handle or a missing array";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (session_owned(d, "flacgpu_decoder_scan_device")) return FLACGPU_ERR_INVALID_ARG;
    d->scanned = d->raw = false;
    DeviceGuard guard(d->device);
    if (int rc = open_device_door(d, d_data, len, n_streams, stream, "flacgpu_decoder_scan_device")) return rc;
    return scan_call(d, ScanInput{d_data, true}, len, n_streams, streams, total_samples);
}

int flacgpu_decoder_scan_frames(flacgpu_decoder *d, const uint8_t *const *data, const size_t *len, uint32_t n_streams,
                                flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw, uint64_t *total_frames,
                                uint64_t *total_elements, uint64_t *total_samples) {
    return flacgpu_decoder_scan_frames_ex(d, data, len, n_streams, 0, streams, raw, total_frames, total_elements,
                                          total_samples);
}

int flacgpu_decoder_scan_frames_ex(flacgpu_decoder *d, const uint8_t *const *data, const size_t *len, uint32_t n_streams,
                                   uint32_t flags, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                                   uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples) {
    if (!d || (n_streams && (!data || !len || !streams)) || !total_frames || !total_elements || !total_samples ||
        (flags & ~FLACGPU_SCAN_SPECULATIVE))
        return FLACGPU_ERR_INVALID_ARG;
    if (session_owned(d, "flacgpu_decoder_scan_frames_ex")) return FLACGPU_ERR_INVALID_ARG;
    d->scanned = d->raw = false;
    DeviceGuard guard(d->device);
    return scan_frames_call(d, ScanInput{data, false}, len, n_streams, flags, streams, raw, total_frames, total_elements,
                            total_samples);
}

int flacgpu_decoder_scan_frames_device(flacgpu_decoder *d, const uint8_t *const *d_data, const size_t *len,
                                       uint32_t n_streams, uint32_t flags, void *stream, flacgpu_decoded_stream *streams,
                                       flacgpu_raw_stream *raw, uint64_t *total_frames, uint64_t *total_elements,
                                       uint64_t *total_samples) {
    if (!d || (n_streams && (!d_data || !len || !streams)) || !total_frames || !total_elements || !total_samples ||
        (flags & ~FLACGPU_SCAN_SPECULATIVE)) {
        g_last_error = "flacgpu_decoder_scan_frames_device: a NULL handle, a missing array or an unknown flag";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (session_owned(d, "flacgpu_decoder_scan_frames_device")) return FLACGPU_ERR_INVALID_ARG;
    d->scanned = d->raw = false;
    DeviceGuard guard(d->device);
    if (int rc = open_device_door(d, d_data, len, n_streams, stream, "flacgpu_decoder_scan_frames_device")) return rc;
    return scan_frames_call(d, ScanInput{d_data, true}, len, n_streams, flags, streams, raw, total_frames, total_elements,
                            total_samples);
}

int flacgpu_decoder_slot_bytes(flacgpu_decoder *d, uint8_t *out, size_t cap, uint64_t *bytes) {
    if (!d || !bytes) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned) {
        g_last_error = "flacgpu_decoder_slot_bytes: no scanned batch";
        return FLACGPU_ERR_INVALID_ARG;
    }
    *bytes = d->slot_bytes;
    if (cap < d->slot_bytes) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (!d->slot_bytes) return FLACGPU_OK;
    if (!out) return FLACGPU_ERR_INVALID_ARG;
    DeviceGuard guard(d->device);
    HIP_TRY(hipMemcpyAsync(out, d->bytes.p, d->slot_bytes, hipMemcpyDeviceToHost, d->st));
    HIP_TRY(hipStreamSynchronize(d->st));
    return FLACGPU_OK;
}

int flacgpu_decoder_session_open(int device, uint32_t n_streams, uint32_t max_frame_bytes, uint32_t flags,
                                 flacgpu_decoder_session **out) {
    if (!out) return FLACGPU_ERR_INVALID_ARG;
    *out = nullptr;
    if (flags || max_frame_bytes < flacenc::kSessionMinW || max_frame_bytes > flacenc::kSessionMaxW) {
        g_last_error = "flacgpu_decoder_session_open: an unknown flag, or max_frame_bytes outside 16 .. 2^22";
        return FLACGPU_ERR_INVALID_ARG;
    }
    flacgpu_decoder *d = nullptr;
    if (int rc = flacgpu_decoder_create(device, &d)) return rc;
    flacgpu_decoder_session *s = new (std::nothrow) flacgpu_decoder_session();
    try {
        if (s) s->streams.resize(n_streams);
    } catch (const std::bad_alloc &) {
        delete s;
        s = nullptr;
    }
    if (!s) {
        flacgpu_decoder_destroy(d);
        g_last_error = "flacgpu_decoder_session_open: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    d->session = true;
    s->d = d;
    s->W = max_frame_bytes;
    *out = s;
    return FLACGPU_OK;
}

int flacgpu_decoder_session_open_container(int device, uint32_t n_streams, uint32_t max_frame_bytes,
                                           flacgpu_decoder_session **out) {
    if (int rc = flacgpu_decoder_session_open(device, n_streams, max_frame_bytes, 0, out)) return rc;
    flacgpu_decoder_session *s = *out;
    *out = nullptr;
    int rc = FLACGPU_OK;
    try {
        s->cs.resize(n_streams);
        for (flacgpu_decoder_session::Container &k : s->cs) meta_feed_init(k.meta);
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_session_open_container: out of host memory";
        rc = FLACGPU_ERR_UNSUPPORTED;
    }
    if (!rc) rc = flacgpu_md5_chains_create(s->d->device, n_streams, &s->chains);
    if (rc) {
        flacgpu_decoder_session_close(s);
        return rc;
    }
    s->container = true;
    s->d->container = s;
    *out = s;
    return FLACGPU_OK;
}

int flacgpu_decoder_session_verdict(flacgpu_decoder_session *s, flacgpu_decoded_stream *out) {
    const uint32_t n = s ? (uint32_t)s->streams.size() : 0;
    if (!s || !s->container || s->dead || !s->finished || s->verdict_given || (n && !out)) {
        g_last_error = "flacgpu_decoder_session_verdict: no container session, not finished yet, or the verdict was given";
        return FLACGPU_ERR_INVALID_ARG;
    }
    std::vector<uint8_t> digest;
    std::vector<flacgpu_decoded_stream> res;
    try {
        digest.resize(16 * (size_t)n);
        res.assign(n, flacgpu_decoded_stream{});
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_session_verdict: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    if (int rc = flacgpu_md5_chains_final(s->chains, digest.data())) return rc;   // pads, downloads; synchronous
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        const flacgpu_decoder_session::Container &k = s->cs[i];
        flacgpu_decoded_stream &r = res[i];
        r.out_offset = total;   // the one-shot batch's layout
        r.info = k.info;
        if (k.phase == flacenc::CS_REFUSED) {
            r.rc = FLACGPU_ERR_INVALID_ARG;
            continue;
        }
        r.info.frames = (uint32_t)k.frames;
        r.info.decoded_samples = k.samples;
        r.info.bad_frames = k.bad_frames;
        r.info.bad_crc16 = k.bad_crc16;
        total += k.samples * k.info.channels;
        if (k.broken || (!s->hashed && k.in_feed)) {   // a feed's frames were never hashed
            r.info.md5_status = 3;
            continue;
        }
        memcpy(r.info.decoded_md5, &digest[16 * (size_t)i], 16);
        static const uint8_t zero[16] = {0};
        r.info.md5_status = !memcmp(k.info.md5, zero, 16) ? 2u : !memcmp(k.info.md5, r.info.decoded_md5, 16) ? 1u : 0u;
    }
    if (n) memcpy(out, res.data(), sizeof(flacgpu_decoded_stream) * n);
    s->verdict_given = true;
    return FLACGPU_OK;
}

void flacgpu_decoder_session_close(flacgpu_decoder_session *s) {
    if (!s) return;
    flacgpu_decoder *d = s->d;
    flacgpu_md5_chains_destroy(s->chains);   // (waits for its updates on the decoder's stream)
    d->container = nullptr;
    {
        DeviceGuard guard(d->device);
        if (d->st) (void)hipStreamSynchronize(d->st);
        s->other.release();   // on the session's device, as the decoder's own buffers
        s->chunks.release();
        s->src_tab.release();
        s->info_tab.release();
        s->meta_tab.release();
        s->meta_src.release();
        s->meta_used.release();
    }
    delete s;
    d->session = false;
    flacgpu_decoder_destroy(d);
}

flacgpu_decoder *flacgpu_decoder_session_decoder(flacgpu_decoder_session *s) { return s ? s->d : nullptr; }

int flacgpu_decoder_session_pending(flacgpu_decoder_session *s, uint64_t *held_bytes, uint64_t *fed_bytes) {
    if (!s || s->dead) return FLACGPU_ERR_INVALID_ARG;
    for (size_t i = 0; held_bytes && i < s->streams.size(); i++) held_bytes[i] = s->streams[i].held;
    if (fed_bytes) *fed_bytes = s->fed;
    return FLACGPU_OK;
}

// The three feeds behind one set of checks.  door: 0 host memory, 1 device memory, 2 finish.
static int session_call(flacgpu_decoder_session *s, int door, const uint8_t *const *data, const size_t *len,
                        const uint8_t *flush, void *stream, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                        uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples) {
    static const char *const kWho[3] = {"flacgpu_decoder_session_feed", "flacgpu_decoder_session_feed_device",
                                        "flacgpu_decoder_session_finish"};
    const char *who = kWho[door];
    const uint32_t n = s ? (uint32_t)s->streams.size() : 0;
    if (!s || (n && ((door != 2 && (!data || !len)) || !streams)) || !total_frames || !total_elements || !total_samples) {
        g_last_error = std::string(who) + ": a NULL handle or a missing array";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (s->dead || s->finished) {
        g_last_error = std::string(who) + (s->dead ? ": an earlier call on this session failed" : ": the session is finished");
        return FLACGPU_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; s->container && flush && i < n; i++)
        if (flush[i]) {   // a container's sender knows no frame boundary: finish alone ends the input
            g_last_error = std::string(who) + ": a container session takes no flush";
            return FLACGPU_ERR_INVALID_ARG;
        }
    flacgpu_decoder *d = s->d;
    DeviceGuard guard(d->device);
    const auto t_in = std::chrono::steady_clock::now();
    std::vector<const uint8_t *> chunk;
    std::vector<uint64_t> bytes, fed_now, used;   // fed_now, used: a container session's (all bytes; those of the metadata)
    std::vector<MetaFeed> meta;
    uint64_t fresh = 0, fed = 0;
    try {
        chunk.assign(n, nullptr);
        bytes.assign(n, 0);
        fed_now.assign(n, 0);
        used.assign(n, 0);
    } catch (const std::bad_alloc &) {
        g_last_error = std::string(who) + ": out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    int rc = door == 1 ? open_device_door(d, data, len, n, stream, who) : FLACGPU_OK;
    // a container's metadata is walked where it lies: device chunks on the decoder's stream, behind the caller's
    if (!rc && s->container) rc = container_meta(s, door, data, len, meta, used);
    if (rc) {
        s->dead = rc == FLACGPU_ERR_HIP;
        return rc;
    }
    for (uint32_t i = 0; door != 2 && i < n; i++)
        if (data[i] && len[i]) {
            fed_now[i] = len[i];
            fed += len[i];
            if (s->container && s->cs[i].phase >= flacenc::CS_LOST) continue;   // dropped
            bytes[i] = len[i] - used[i];   // the metadata's bytes are not the scan's
            fresh += bytes[i];
            if (door == 1 && bytes[i]) chunk[i] = data[i] + used[i];
        }
    if (door == 0) {
        // the chunks alone go up: into the pinned staging at 16-byte boundaries, one copy, and the kernel joins them to
        // the tails that never left the device
        const uint64_t up = fresh + 16 * (uint64_t)n;
        if (fresh) {
            rc = d->staging.ensure(up);
            if (!rc) rc = s->chunks.ensure(up);
            if (rc) {
                s->dead = rc == FLACGPU_ERR_HIP;
                return rc;
            }
            uint8_t *stg = d->staging.as<uint8_t>();
            uint64_t at = 0;
            for (uint32_t i = 0; i < n; i++) {
                if (!bytes[i]) continue;
                memcpy(stg + at, data[i] + used[i], bytes[i]);
                chunk[i] = s->chunks.as<const uint8_t>() + at;
                at = (at + bytes[i] + 15) & ~(uint64_t)15;
            }
            const hipError_t e = hipMemcpyAsync(s->chunks.p, stg, at, hipMemcpyHostToDevice, d->st);
            if (e != hipSuccess) {
                s->dead = true;
                g_last_error = std::string(who) + ": " + hipGetErrorString(e);
                return FLACGPU_ERR_HIP;
            }
        }
    }
    const double stage_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count();
    // s->fed counts what the session took in: all a container session was fed, its metadata and the bytes of dropped
    // streams included (`fed`); of a raw session the bytes that went to the scan (`fresh`), which are all it was fed
    if (s->container) {
        if (int rc = container_step(s, chunk.data(), bytes.data(), fed_now.data(), meta, door == 2)) return rc;
        if (s->meta_fresh) s->meta_on_device = true;   // the feed is committed: the table is the streams' state
        s->timing.stage_ms = stage_ms;
        s->fed += fed;
        s->finished = door == 2;
        // what scan leaves: a batch of regular streams (decode_frames, frame_records and the timeline calls refuse it)
        index_frames(d);
        d->scanned = true;
        if (n) memcpy(streams, d->res.data(), sizeof(flacgpu_decoded_stream) * n);
        if (n && raw) memcpy(raw, d->raw_streams.data(), sizeof(flacgpu_raw_stream) * n);
        *total_frames = d->frame_tab.size();
        *total_elements = *total_samples = d->total;
        return FLACGPU_OK;
    }
    if (int rc = session_step(s, chunk.data(), bytes.data(), flush, door == 2)) return rc;
    s->timing.stage_ms = stage_ms;
    s->fed += fresh;
    s->finished = door == 2;
    publish_raw_scan(d, streams, raw, total_frames, total_elements, total_samples);
    return FLACGPU_OK;
}

int flacgpu_decoder_session_last_feed_timing(flacgpu_decoder_session *s, flacgpu_session_timing *out) {
    if (!s || !out || s->dead) return FLACGPU_ERR_INVALID_ARG;
    *out = s->timing;
    return FLACGPU_OK;
}

int flacgpu_decoder_session_feed(flacgpu_decoder_session *s, const uint8_t *const *data, const size_t *len,
                                 const uint8_t *flush, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                                 uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples) {
    return session_call(s, 0, data, len, flush, nullptr, streams, raw, total_frames, total_elements, total_samples);
}

int flacgpu_decoder_session_feed_device(flacgpu_decoder_session *s, const uint8_t *const *d_data, const size_t *len,
                                        const uint8_t *flush, void *stream, flacgpu_decoded_stream *streams,
                                        flacgpu_raw_stream *raw, uint64_t *total_frames, uint64_t *total_elements,
                                        uint64_t *total_samples) {
    return session_call(s, 1, d_data, len, flush, stream, streams, raw, total_frames, total_elements, total_samples);
}

int flacgpu_decoder_session_finish(flacgpu_decoder_session *s, flacgpu_decoded_stream *streams, flacgpu_raw_stream *raw,
                                   uint64_t *total_frames, uint64_t *total_elements, uint64_t *total_samples) {
    return session_call(s, 2, nullptr, nullptr, nullptr, nullptr, streams, raw, total_frames, total_elements, total_samples);
}

int flacgpu_session_slots_host(const flacgpu_session_slot_src *srcs, uint32_t n_slots, uint8_t *out, size_t cap,
                               uint64_t *bytes) {
    if (!bytes || (n_slots && !srcs)) return FLACGPU_ERR_INVALID_ARG;
    SlotLayout lay;   // the layout a feed gives its slots
    std::vector<SessionSrc> tab;
    try {
        for (uint32_t i = 0; i < n_slots; i++) {
            const uint64_t L = srcs[i].tail_len + srcs[i].chunk_len;
            if (!L) continue;
            lay.add(i, 0, L, 0, 0);
            tab.push_back(SessionSrc{reinterpret_cast<uint64_t>(srcs[i].tail), srcs[i].tail_len,
                                     reinterpret_cast<uint64_t>(srcs[i].chunk), srcs[i].chunk_len});
        }
    } catch (const std::bad_alloc &) {
        return FLACGPU_ERR_UNSUPPORTED;
    }
    const uint64_t total = lay.at ? lay.at + 64 : 0;
    *bytes = total;
    if (cap < total) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (!total) return FLACGPU_OK;
    if (!out) return FLACGPU_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < tab.size(); s++)   // one "lane" after another, as k_session_slots numbers them
        for (uint64_t g = lay.slots[s].base / 16; g < lay.end_of(s) / 16; g++) {
            const uint4 v = session_group(tab[s], g * 16 - lay.slots[s].base);
            memcpy(out + g * 16, &v, 16);
        }
    memset(out + lay.at, 0, 64);   // the look-ahead: the groups from block n_blocks on
    return FLACGPU_OK;
}

int flacgpu_meta_walk_host(const uint8_t *data, size_t len, flacgpu_stream_info *info, uint32_t *min_frame,
                           uint64_t *frames_at) {
    if (!info || !min_frame || !frames_at) return FLACGPU_ERR_INVALID_ARG;
    *frames_at = 0;
    MetaRecord rec;
    meta_walk(data, len, rec);   // the function k_meta_walk runs, compiled for the host
    size_t pos = 0;
    if (const char *why = flacenc::metadata_of_record(rec, info, min_frame, &pos)) {
        if (*why) g_last_error = why;
        return FLACGPU_ERR_INVALID_ARG;
    }
    *frames_at = pos;
    return FLACGPU_OK;
}

int flacgpu_decoder_frame_records(flacgpu_decoder *d, flacgpu_frame_record *records, size_t cap) {
    if (!d) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned || !d->raw) {
        g_last_error = "flacgpu_decoder_frame_records: no scanned batch of raw frame streams";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (d->records.empty()) return FLACGPU_OK;
    if (!records) return FLACGPU_ERR_INVALID_ARG;
    if (cap < d->records.size()) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    memcpy(records, d->records.data(), sizeof(flacgpu_frame_record) * d->records.size());
    return FLACGPU_OK;
}

int flacgpu_decoder_decode_frames(flacgpu_decoder *d, int32_t *out, size_t out_cap_elements, uint32_t flags,
                                  flacgpu_frame_record *records, size_t cap) {
    if (!d || (flags & ~FLACGPU_DECODE_OUT_DEVICE)) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned || !d->raw) {
        g_last_error = "flacgpu_decoder_decode_frames: no scanned batch of raw frame streams";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (!d->records.empty() && !records) return FLACGPU_ERR_INVALID_ARG;
    if (cap < d->records.size() || (d->raw_elements && (!out || out_cap_elements < d->raw_elements))) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    return decode_frames_impl(d, out, flags, records);
}

int flacgpu_decoder_plan_analysis(flacgpu_decoder *d, uint64_t *n_frames, uint64_t *n_subframes, uint64_t *row_elements) {
    if (!d || !n_frames || !n_subframes || !row_elements) return FLACGPU_ERR_INVALID_ARG;
    *n_frames = *n_subframes = *row_elements = 0;
    if (!d->scanned) {
        g_last_error = "flacgpu_decoder_plan_analysis: no scanned batch";
        return FLACGPU_ERR_INVALID_ARG;
    }
    const AnalysisSizes z = analysis_sizes(d);
    *n_frames = z.frames;
    *n_subframes = z.subframes;
    *row_elements = z.rows;
    return FLACGPU_OK;
}

int flacgpu_decoder_analyze(flacgpu_decoder *d, uint32_t flags, flacgpu_frame_analysis *frames, size_t frames_cap,
                            flacgpu_subframe_plan *subframes, size_t subframes_cap, int32_t *rows, size_t rows_cap) {
    if (!d || (flags & ~FLACGPU_DECODE_OUT_DEVICE)) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned) {
        g_last_error = "flacgpu_decoder_analyze: no scanned batch";
        return FLACGPU_ERR_INVALID_ARG;
    }
    const AnalysisSizes z = analysis_sizes(d);
    if (z.frames && (!frames || !subframes)) return FLACGPU_ERR_INVALID_ARG;
    if (frames_cap < z.frames || subframes_cap < z.subframes || (rows && rows_cap < z.rows)) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    return analyze_impl(d, flags, frames, subframes, rows, z);
}

int flacgpu_decoder_plan_timeline(flacgpu_decoder *d, const flacgpu_out_format *fmt, flacgpu_timeline_result *results,
                                  uint64_t *out_bytes, uint64_t *mask_bytes) {
    if (!d || !fmt || !out_bytes) return FLACGPU_ERR_INVALID_ARG;
    *out_bytes = 0;
    if (mask_bytes) *mask_bytes = 0;
    if (!d->scanned || !d->raw) {
        g_last_error = "flacgpu_decoder_plan_timeline: no scanned batch of raw frame streams";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (!d->raw_streams.empty() && !results) return FLACGPU_ERR_INVALID_ARG;
    timeline_streams(d, results, nullptr, "flacgpu_decoder_plan_timeline");
    return timeline_check(d, fmt, results, "flacgpu_decoder_plan_timeline", out_bytes, mask_bytes);
}

int flacgpu_decoder_decode_timeline(flacgpu_decoder *d, void *out, size_t out_cap_bytes, uint8_t *mask,
                                    size_t mask_cap_bytes, const flacgpu_out_format *fmt, uint32_t flags,
                                    flacgpu_timeline_result *results, flacgpu_timeline_frame *frames, size_t frames_cap) {
    if (!d || !fmt || (flags & ~FLACGPU_DECODE_OUT_DEVICE)) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned || !d->raw) {
        g_last_error = "flacgpu_decoder_decode_timeline: no scanned batch of raw frame streams";
        return FLACGPU_ERR_INVALID_ARG;
    }
    const size_t n = d->raw_streams.size(), R = d->records.size();
    if (n && !results) return FLACGPU_ERR_INVALID_ARG;
    std::vector<flacgpu_timeline_result> res;
    std::vector<flacgpu_timeline_frame> tl;
    try {   // a refused call writes nothing: the rule runs on copies
        res.resize(n);
        tl.resize(R);
    } catch (const std::bad_alloc &) {
        g_last_error = "flacgpu_decoder_decode_timeline: out of host memory";
        return FLACGPU_ERR_UNSUPPORTED;
    }
    timeline_streams(d, res.data(), tl.data(), "flacgpu_decoder_decode_timeline");
    const std::string note = g_last_error;   // the first refused stream, if any: what an accepted call leaves
    uint64_t out_bytes = 0, mask_bytes = 0;
    if (int rc = timeline_check(d, fmt, res.data(), "flacgpu_decoder_decode_timeline", &out_bytes, &mask_bytes)) return rc;
    if ((out_bytes && (!out || out_cap_bytes < out_bytes)) || (mask && mask_cap_bytes < mask_bytes) ||
        (frames && frames_cap < R)) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (reinterpret_cast<uintptr_t>(out) % sample_type_align(fmt->dtype)) {
        g_last_error = "flacgpu_decoder_decode_timeline: out is not aligned to its element size";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (out_bytes || (mask && mask_bytes))
        if (int rc = decode_timeline_impl(d, out, out_bytes, mask, mask_bytes, *fmt, flags, res.data(), tl)) return rc;
    if (n) memcpy(results, res.data(), sizeof(flacgpu_timeline_result) * n);
    if (frames && R) memcpy(frames, tl.data(), sizeof(flacgpu_timeline_frame) * R);
    g_last_error = note;
    return FLACGPU_OK;
}

int flacgpu_decoder_decode(flacgpu_decoder *d, int32_t *out, size_t out_cap_samples, uint32_t flags,
                           flacgpu_decoded_stream *streams) {
    if (!d || (flags & ~(FLACGPU_DECODE_OUT_DEVICE | FLACGPU_DECODE_NO_MD5))) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned) {
        g_last_error = "flacgpu_decoder_decode: no scanned batch";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (!d->res.empty() && !streams) return FLACGPU_ERR_INVALID_ARG;
    if (d->total && (!out || out_cap_samples < d->total)) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    return decode_impl(d, out, flags, streams);
}

int flacgpu_decoder_plan_output(const flacgpu_out_format *fmt, const flacgpu_decoded_stream *streams,
                                uint32_t n_streams, uint64_t *out_bytes) {
    if (!fmt || !out_bytes || (n_streams && !streams)) return FLACGPU_ERR_INVALID_ARG;
    *out_bytes = 0;
    const bool padded = fmt->layout == FLACGPU_LAYOUT_PADDED;
    if (!sample_type_known(fmt->dtype) || fmt->layout > FLACGPU_LAYOUT_PADDED || fmt->reserved ||
        (!padded && (fmt->channels_padded || fmt->samples_padded))) {
        g_last_error = "flacgpu_decoder_plan_output: unknown dtype or layout, reserved not 0, or padded fields under FLAT";
        return FLACGPU_ERR_INVALID_ARG;
    }
    uint64_t total = 0;
    bool any = false;
    for (uint32_t i = 0; i < n_streams; i++) {
        const flacgpu_decoded_stream &r = streams[i];
        if (r.rc != FLACGPU_OK) continue;
        if (too_wide(fmt->dtype, r.info.bits_per_sample))
            return refuse_bits("flacgpu_decoder_plan_output", fmt->dtype, i, r.info.bits_per_sample);
        total += r.info.decoded_samples * r.info.channels;
        any = any || (r.info.decoded_samples && r.info.channels);
    }
    const uint64_t es = sample_type_bytes(fmt->dtype);
    if (!padded) {
        *out_bytes = total * es;
        return FLACGPU_OK;
    }
    for (uint32_t i = 0; i < n_streams && any; i++) {
        const flacgpu_decoded_stream &r = streams[i];
        if (r.rc != FLACGPU_OK) continue;
        if (r.info.channels > fmt->channels_padded || r.info.decoded_samples > fmt->samples_padded)
            return refuse_fit("flacgpu_decoder_plan_output", "stream " + std::to_string(i),
                              std::to_string(r.info.channels) + " channels, " + std::to_string(r.info.decoded_samples) +
                                  " samples");
    }
    return padded_bytes("flacgpu_decoder_plan_output", "the padded batch exceeds", (uint64_t)n_streams * fmt->channels_padded,
                        fmt->samples_padded, es, out_bytes);
}

int flacgpu_decoder_decode_as(flacgpu_decoder *d, void *out, size_t out_cap_bytes, const flacgpu_out_format *fmt,
                              uint32_t flags, flacgpu_decoded_stream *streams) {
    if (!d || !fmt || (flags & ~(FLACGPU_DECODE_OUT_DEVICE | FLACGPU_DECODE_NO_MD5))) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned) {
        g_last_error = "flacgpu_decoder_decode_as: no scanned batch";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (!d->res.empty() && !streams) return FLACGPU_ERR_INVALID_ARG;
    uint64_t out_bytes = 0;
    if (int rc = flacgpu_decoder_plan_output(fmt, d->res.data(), (uint32_t)d->res.size(), &out_bytes)) return rc;
    if (fmt->dtype == FLACGPU_SAMPLE_I32 && fmt->layout == FLACGPU_LAYOUT_FLAT)
        return flacgpu_decoder_decode(d, static_cast<int32_t *>(out), out_cap_bytes / 4, flags, streams);
    if (out_bytes && (!out || out_cap_bytes < out_bytes)) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (reinterpret_cast<uintptr_t>(out) % sample_type_align(fmt->dtype)) {
        g_last_error = "flacgpu_decoder_decode_as: out is not aligned to its element size";
        return FLACGPU_ERR_INVALID_ARG;
    }
    return decode_impl(d, out, flags, streams, fmt, out_bytes);
}

int flacgpu_window_frames(const uint32_t *frame_n, uint32_t n_frames, uint64_t start, uint64_t length, uint32_t *first,
                          uint32_t *count, uint64_t *skip) {
    uint64_t end = 0;
    if ((n_frames && !frame_n) || !first || !count || !skip || __builtin_add_overflow(start, length, &end))
        return FLACGPU_ERR_INVALID_ARG;
    std::vector<uint64_t> first_of(n_frames);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_frames; i++) {
        first_of[i] = total;
        total += frame_n[i];
    }
    window_frames([&](uint32_t i) { return first_of[i]; }, n_frames, total, start, length, first, count, skip);
    return FLACGPU_OK;
}

int flacgpu_decoder_plan_windows(const flacgpu_out_format *fmt, const flacgpu_decoded_stream *streams,
                                 uint32_t n_streams, const flacgpu_window *w, uint32_t n_windows, uint64_t *out_bytes) {
    if (!fmt || !out_bytes || (n_streams && !streams) || (n_windows && !w)) return FLACGPU_ERR_INVALID_ARG;
    *out_bytes = 0;
    if (!sample_type_known(fmt->dtype) || fmt->layout != FLACGPU_LAYOUT_PADDED || fmt->reserved) {
        g_last_error = "flacgpu_decoder_plan_windows: unknown dtype, a layout other than PADDED, or reserved not 0";
        return FLACGPU_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; i < n_windows; i++) {
        uint64_t end = 0;
        if (w[i].stream >= n_streams || w[i].reserved || __builtin_add_overflow(w[i].start, w[i].length, &end)) {
            g_last_error = "flacgpu_decoder_plan_windows: window " + std::to_string(i) +
                           " names no stream of the batch, has reserved not 0, or start + length overflows";
            return FLACGPU_ERR_INVALID_ARG;
        }
        const flacgpu_decoded_stream &r = streams[w[i].stream];
        if (w[i].length > fmt->samples_padded || (r.rc == FLACGPU_OK && r.info.channels > fmt->channels_padded))
            return refuse_fit("flacgpu_decoder_plan_windows", "window " + std::to_string(i),
                              std::to_string(w[i].length) + " samples of stream " + std::to_string(w[i].stream));
    }
    for (uint32_t i = 0; i < n_windows; i++) {
        const flacgpu_decoded_stream &r = streams[w[i].stream];
        if (r.rc == FLACGPU_OK && too_wide(fmt->dtype, r.info.bits_per_sample))
            return refuse_bits("flacgpu_decoder_plan_windows", fmt->dtype, w[i].stream, r.info.bits_per_sample);
    }
    return padded_bytes("flacgpu_decoder_plan_windows", "the windows exceed", (uint64_t)n_windows * fmt->channels_padded,
                        fmt->samples_padded, sample_type_bytes(fmt->dtype), out_bytes);
}

int flacgpu_decoder_decode_windows(flacgpu_decoder *d, void *out, size_t out_cap_bytes, const flacgpu_out_format *fmt,
                                   uint32_t flags, const flacgpu_window *w, uint32_t n_windows,
                                   flacgpu_window_result *results) {
    if (!d || !fmt || (flags & ~(FLACGPU_DECODE_OUT_DEVICE | FLACGPU_DECODE_NO_MD5))) return FLACGPU_ERR_INVALID_ARG;
    if (!d->scanned) {
        g_last_error = "flacgpu_decoder_decode_windows: no scanned batch";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (n_windows && (!w || !results)) return FLACGPU_ERR_INVALID_ARG;
    uint64_t out_bytes = 0;
    if (int rc = flacgpu_decoder_plan_windows(fmt, d->res.data(), (uint32_t)d->res.size(), w, n_windows, &out_bytes))
        return rc;
    if (out_bytes && (!out || out_cap_bytes < out_bytes)) {
        g_last_error = "output buffer too small";
        return FLACGPU_ERR_BUFFER_TOO_SMALL;
    }
    if (reinterpret_cast<uintptr_t>(out) % sample_type_align(fmt->dtype)) {
        g_last_error = "flacgpu_decoder_decode_windows: out is not aligned to its element size";
        return FLACGPU_ERR_INVALID_ARG;
    }
    if (!out_bytes) {   // no element to write: every window is empty or on a stream with rc != 0
        for (uint32_t i = 0; i < n_windows; i++) {
            results[i] = flacgpu_window_result{};
            results[i].rc = d->res[w[i].stream].rc;
        }
        return FLACGPU_OK;
    }
    return decode_windows_impl(d, out, out_bytes, *fmt, flags, w, n_windows, results);
}
