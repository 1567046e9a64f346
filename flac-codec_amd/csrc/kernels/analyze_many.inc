// analyze_many.inc -- the batch decoder's frame analysis (decode_many.hip; flacgpu_decoder_analyze).
// Included inside decode_many.hip's anonymous namespace, after decode_many.inc (ManyFrame) and spec_end.inc, with
// kernels/frame_analysis.h (the walk, shared with the host) included at file scope.
//   K_a1 k_analyze_many  lane per frame, k_decode_many's shape: the frame's header by parse_frame_header, its subframes
//                        by analyze_subframes.  Every field goes to global memory as it is read, into subframe records
//                        that one memset has cleared: no record is held in registers and no per-lane array exists, so
//                        the kernel uses no scratch memory.  There is no synthesis and hence no history ring (no MAXO);
//                        the row stores are plain.  ROWS == false stores no sample and steps over VERBATIM bodies,
//                        warm-ups and escaped partitions in one move each.
// The frame table is FramePass's, with two fields read differently: `scratch` is the frame's row_offset and `out` its
// first_subframe (both prefix sums of the host's), and `slot` is the frame's own index, so that counts[2 f + 1] -- which
// k_frame_crc, launched in front of this kernel on the same stream, has finished -- is the frame's own CRC-16 verdict.

// analyze_subframes' bit source: decode.inc's BitReader on the batch buffer, clamped at the slot's end - 4 like SpecBits
struct AnalysisBits {
    BitReader r;
    const uint32_t *words;
    uint64_t start, cap;
    __device__ __forceinline__ uint32_t pos() const { return r.pos(); }
    __device__ __forceinline__ void seek(uint32_t bit) {
        r.init(words, start + (bit >> 3), cap, bit & ~7u);
        r.skip(bit & 7u);
    }
    __device__ __forceinline__ uint32_t get(uint32_t n) { return r.get(n); }
    __device__ __forceinline__ uint32_t zeros(uint32_t limit) { return r.unary1(limit); }
    __device__ __forceinline__ uint32_t rice(uint32_t k, uint32_t limit) { return r.rice(k, 1u << k, limit); }
};

template <bool ROWS>
__global__ void __launch_bounds__(64) k_analyze_many(const uint32_t *__restrict__ words,
                                                     const ManyFrame *__restrict__ frames, uint32_t n_frames,
                                                     const uint32_t *__restrict__ counts,
                                                     flacgpu_frame_analysis *__restrict__ out_frames,
                                                     flacgpu_subframe_plan *__restrict__ out_subs,
                                                     int32_t *__restrict__ rows) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    const ManyFrame fr = frames[f];
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
    const uint32_t end_bit = (uint32_t)(fr.end - fr.start) * 8;
    const uint32_t ldb = (fr.n + 3u) & ~3u;
    AnalysisBits b;
    b.words = words;
    b.start = fr.start;
    b.cap = fr.cap;
    b.r.init(words, fr.start, fr.cap, 0);
    FrameHead fh;
    bool bad = !parse_frame_header(b.r, bytes, fr.start, fh);
    const uint32_t header_bits = b.r.pos();
    const uint32_t acode = fh.acode;
    const uint32_t bps = bps_of_code(fh.bps_code, fr.bps);
    const uint32_t nch = acode < 8 ? acode + 1 : 2;
    // the records and rows of this frame were laid out for the scan's block size and channels: anything else is
    // refused here, before the first store of the walk
    if (fh.n != fr.n || bps != fr.bps || nch != fr.channels || header_bits > end_bit) bad = true;
    uint32_t body = 0;
    if (!bad && !analyze_subframes<ROWS>(b, fr.n, acode, bps, end_bit, out_subs + fr.out, ROWS ? rows + fr.scratch : rows,
                                         ldb, &body))
        bad = true;
    flacgpu_frame_analysis a;
    a.row_offset = fr.scratch;
    a.first_subframe = fr.out;
    a.block_size = fr.n;
    a.header_bytes = header_bits >> 3;
    a.status = (bad ? 1u : 0u) | (counts[2 * (size_t)f + 1] ? 2u : 0u);
    a.assignment_code = acode;
    a.plan.assignment = (uint8_t)(acode >= 8 ? acode : 0u);
    a.plan.channels = (uint8_t)fr.channels;
    a.plan.block_size = (uint16_t)(fr.n & 0xFFFFu);
    a.plan.body_bits = body;
    out_frames[f] = a;
}
