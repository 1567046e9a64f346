// autocorr.inc -- K3: exact autocorrelation (shared f64 tiles, deep history, generic, MFMA experiment).
// Part of flacenc_gpu.hip (one translation unit; included inside its anonymous namespace).

// ---------------------------------------------------------------------------------
// K3: window + autocorrelation in the reference's exact summation order.
// ac[lag] = sum_{i=0}^{n-1-lag} w[i]*w[i+lag] is a LEFT FOLD with every product rounded
// first (encode.rs:3495).  Equivalently, for j = lag..n-1: acc[lag] += w[j]*w[j-lag] in
// increasing j -- the same products in the same order.  One lane owns one candidate and a
// group of LG lags; it walks its candidate's samples sequentially, keeps the last H
// windowed samples in a statically indexed register ring and updates its LG chains
// (independent => full f64 pipeline with one wave per SIMD).  blockIdx.y selects the lag
// group so the ring indexing stays static.  The window value is wave-uniform (scalar load).
// H lags are computed (H = max order + 1 rounded up to a multiple of 4); extra lags are
// simply not read by K4.
// ---------------------------------------------------------------------------------

// A workgroup that is BEHIND gets the SIMD: a wave's issue priority falls with the quarter of the block it has reached.  (The
// SIMD issues oldest wave first: left alone, the first-launched of a CU's two workgroups runs ahead and the other one ends
// alone, one wave per SIMD.)
__device__ __forceinline__ void ac4_progress_prio(uint32_t t, uint32_t ntiles) {
    if ((t & 7u) == 0) {   // wave-uniform
        const uint32_t qd = 4u * t / ntiles;
        if (qd == 0) __builtin_amdgcn_s_setprio(3);
        else if (qd == 1) __builtin_amdgcn_s_setprio(2);
        else if (qd == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    }
}

// FMA: one v_fma_f64 per term instead of a multiply and an add -- ONLY where both factors are integers below 2^26 (samples
// under a window value of exactly 1.0: the flat middle of a Tukey window): their product is then exact, so
// round(round(a b) + acc) = round(a b + acc) and the fused instruction rounds exactly like the reference's two (Params::fma_t0)
template <int A, int LG, bool FIRST, bool FMA = false>
__device__ __forceinline__ void ac3_block(const double (&w)[16], const double (&prev)[16],
                                          double (&acc)[LG]) {
    if constexpr (FMA) {
        static_assert(!FIRST, "the first block of a frame lies under the window's taper");
#pragma unroll
        for (int s = 0; s < 16; s++) {
#pragma unroll
            for (int k = 0; k < LG; k++) {
                const int lag = A + k;
                const double o = (s - lag >= 0) ? w[(s - lag >= 0) ? s - lag : 0]
                                                : prev[(s - lag >= 0) ? 0 : 16 + s - lag];
                acc[k] = __builtin_fma(w[s], o, acc[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < 16; s++) {
        // all products of a sample first, then the adds: a dependent f64 pair issued back to
        // back stalls the wave (7.3 instead of 5 cycles per instruction with one wave per SIMD)
        double prod[LG];
#pragma unroll
        for (int k = 0; k < LG; k++) {
            const int lag = A + k;
            const double o = (s - lag >= 0) ? w[(s - lag >= 0) ? s - lag : 0]
                                            : prev[(s - lag >= 0) ? 0 : 16 + s - lag];
            prod[k] = w[s] * o;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < LG; k++) {
            const int lag = A + k;
            if (FIRST && s < lag) continue;  // i >= lag only (first block of the frame)
            acc[k] = acc[k] + prod[k];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- lags up to 32 (LPC orders 17..32): the history of a 16-sample block is the TWO blocks before
// it, so four f64 block buffers rotate (period: two tiles).  FIRST: 0 steady state, 1 / 2 the first /
// second block of the frame (terms whose partner lies before the frame start are not formed).
template <int A, int LG, int FIRST, bool FMA = false>
__device__ __forceinline__ void ac3_block_deep(const double (&w)[16], const double (&p1)[16],
                                               const double (&p2)[16], double (&acc)[LG]) {
    if constexpr (FMA) {   // (as in ac3_block: exact products only)
        static_assert(FIRST == 0, "the first blocks of a frame lie under the window's taper");
#pragma unroll
        for (int s = 0; s < 16; s++) {
#pragma unroll
            for (int k = 0; k < LG; k++) {
                const int idx = s - (A + k);
                const double o = idx >= 0 ? w[idx >= 0 ? idx : 0]
                               : idx >= -16 ? p1[(idx < 0 && idx >= -16) ? 16 + idx : 0]
                                            : p2[(idx < -16) ? 32 + idx : 0];
                acc[k] = __builtin_fma(w[s], o, acc[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < 16; s++) {
        double prod[LG];
#pragma unroll
        for (int k = 0; k < LG; k++) {
            const int idx = s - (A + k);
            const double o = idx >= 0 ? w[idx >= 0 ? idx : 0]
                           : idx >= -16 ? p1[(idx < 0 && idx >= -16) ? 16 + idx : 0]
                                        : p2[(idx < -16) ? 32 + idx : 0];
            prod[k] = w[s] * o;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < LG; k++) {
            const int lag = A + k;
            if (FIRST == 1 && s < lag) continue;
            if (FIRST == 2 && 16 + s < lag) continue;
            acc[k] = acc[k] + prod[k];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---------------------------------------------------------------------------------
// K3 for frames whose length is a multiple of 32, lags <= 16 (k_autocorr4): stereo L / R / mid / side candidates of
// <= 24-bit samples, or independent channels.  Lane = candidate (64 per workgroup), NS waves split the lags; every
// lane accumulates its lags strictly in sample order (the reference's left fold per lag, encode.rs:3403-3413), 16
// samples at a time, with the previous 16-sample block as history, both in registers and statically indexed
// (ac3_block).  The int -> windowed-f64 conversion (mid/side, wasted-bits shift, cvt, window multiply:
// encode.rs:1799) is done ONCE per candidate sample by the workgroup and handed to the NS lag-group waves through a
// double-buffered f64 tile in LDS.  (A kernel whose every lag-group wave converted a private copy of the raw rows
// itself, without workgroup barriers, was slower -- 0.231 against 0.177 ms, 683 against 274 MB of HBM traffic per
// launch, profiles/r02_a_traffic.json -- and has been removed.)
//   producers: the waves convert the next tile straight from their global loads, in units dealt out so
//     that lags + conversion balance (Ac4Share below; a lane holds 2 consecutive samples of one L or R
//     row; the partner row's samples come from lane ^ 8 with one DPP row_ror:8 move each; L-lanes emit L
//     and mid, R-lanes R and side);
//   consumers: lane = candidate row, 8 ds_read_b128 per 16-sample block (row stride 34 doubles:
//     conflict-free for the 16-lane groups of ds_read_b128), then ac3_block;
//   one workgroup barrier per 32-sample tile.
// Per 64 candidates x 32 samples: 832 mul/add + ~150 conversion instructions (832 + 4 x 128 with private copies).
// ---------------------------------------------------------------------------------
constexpr int AC4_TS = 32;             // samples per tile
constexpr int AC4_LDW = AC4_TS + 2;    // f64 row stride: 68 dwords = 4 mod 64

__device__ __forceinline__ int32_t dpp_row_ror8(int32_t v) {  // the value of lane ^ 8
    int32_t r = __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);
    asm volatile("" : "+v"(r));  // keep it a plain v_mov_b32_dpp (see lane_prev in wave_cand.inc)
    return r;
}

// The conversion of a tile is cut into UNITS of 128 raw samples (STEREO: 4 frames x {L, R} x 16 samples,
// otherwise 4 rows x 32 samples; a lane holds 2 consecutive samples of one row, and in the stereo layout its
// partner row's pair sits on lane ^ 8 of the same 16-lane DPP row).  The units are dealt to the lag-group
// waves at compile time so that lags + conversion balance: a wave with one lag more than the others converts
// less (13 lags over 4 waves: 3 + 3 + 3 + 4 lags, 3 + 3 + 2 + 0 units -- 252 / 252 / 232 / 256 instructions
// per tile instead of 232 / 232 / 232 / 296 with equal shares; the slowest wave paces every barrier).
template <bool STEREO>
struct Ac4Units {
    static constexpr int PER_TILE = STEREO ? 8 : 16;
    static constexpr int COST = STEREO ? 20 : 10;   // instructions per unit, roughly
};
// units of wave w (and the first one) when the waves carry lg0..lg3 lags: greedy, cheapest wave first
struct Ac4Share {
    int units[8], first[8];
};
template <bool STEREO>
constexpr Ac4Share ac4_share_n(int ns, const int (&lg)[8]) {
    Ac4Share r{};
    int cost[8] = {};
    for (int w = 0; w < 8; w++) {
        cost[w] = 64 * lg[w];
        r.units[w] = 0;
    }
    for (int u = 0; u < Ac4Units<STEREO>::PER_TILE; u++) {
        int best = 0;
        for (int w = 1; w < ns; w++)
            if (cost[w] < cost[best]) best = w;
        r.units[best]++;
        cost[best] += Ac4Units<STEREO>::COST;
    }
    int f = 0;
    for (int w = 0; w < 8; w++) {
        r.first[w] = f;
        f += r.units[w];
    }
    return r;
}
template <bool STEREO>
constexpr Ac4Share ac4_share(int ns, int lg0, int lg1, int lg2, int lg3) {
    const int lg[8] = {lg0, lg1, lg2, lg3, 0, 0, 0, 0};
    return ac4_share_n<STEREO>(ns, lg);
}

// A staged load is a GLOBAL load whatever the compiler knows about its pointer (a frame pointer read from Params::inter_tab
// is a generic one): while a flat load is in flight gfx9 cannot count vmcnt, and every wait would be for all the staging sets.
// (One set: the loads as they were, nothing to count.)
// The staging sets of a producer: AC4_FETCH_DEPTH (kernels/shape.h) for the stereo producers; ONE for independent channels,
// whose units carry more per-unit state (row pointers, the planar copy's) -- a second set takes those instantiations from
// four waves per SIMD to three (or from three to two), and held to their occupancy they spill (DESIGN.md section 4).
template <bool STEREO>
constexpr int ac4_depth() { return STEREO ? AC4_FETCH_DEPTH : 1; }
#define AC4_DEPTH_OF(P) (std::remove_cv_t<std::remove_reference_t<decltype(P)>>::DEPTH)
typedef int32_t ac4_i2 __attribute__((ext_vector_type(2)));
typedef double ac4_d2 __attribute__((ext_vector_type(2)));
template <int DEPTH, class T>
__device__ __forceinline__ T ac4_ld(const void *q) {
    if constexpr (DEPTH > 1) return *(const __attribute__((address_space(1))) T *)q;
    else return *reinterpret_cast<const T *>(q);
}
template <int DEPTH>
__device__ __forceinline__ int2 ac4_ld_int2(const void *q) {
    const ac4_i2 v = ac4_ld<DEPTH, ac4_i2>(q);
    return make_int2(v.x, v.y);
}
template <int DEPTH>
__device__ __forceinline__ double2 ac4_ld_double2(const void *q) {
    const ac4_d2 v = ac4_ld<DEPTH, ac4_d2>(q);
    return make_double2(v.x, v.y);
}
// The ORs of a conversion are formed where it stands and not wherever their first reader is (the kernel's tail): left to
// sink behind the f64 blocks they keep the staged registers alive across the request that refills them, and the loop then
// copies whole sets at its end -- behind a wait for every load in flight.
template <int DEPTH>
__device__ __forceinline__ void ac4_pin(uint32_t &v) {
    if constexpr (DEPTH > 1) asm volatile("" : "+v"(v));
}
template <int U, bool STEREO>
struct Ac4Producer {
    static constexpr int NU = U > 0 ? U : 1;
    static constexpr int DEPTH = ac4_depth<STEREO>();
    const int32_t *gsrc[NU];   // this lane's 2 samples of tile 0, per unit
    const double *wsrc[NU];    // their window values (tile 0)
    uint32_t dst_a[NU], dst_b[NU];  // f64 indices of the two converted rows inside a buffer (+ column)
    uint32_t sh_a[NU], sh_b[NU];    // right shifts (wasted bits; mid: + 1)
    int32_t sgn;                // second output = other + sgn * own (L-lanes: mid, R-lanes: side)
    uint32_t ntiles;
    int2 stage[DEPTH][NU];     // the rotating staging sets (ac4_fetch_slot, kernels/shape.h)
    double2 wst[DEPTH][NU];
};

// U units per tile for this wave, the first of them U0
template <int U, int U0, bool STEREO>
__device__ __forceinline__ void ac4_setup(const Params &p, uint32_t frame0, uint32_t nframes, uint32_t n,
                                          const double *__restrict__ win, uint32_t group,
                                          Ac4Producer<U, STEREO> &P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t total = nframes * p.ncand;
    const uint32_t cand0 = group * 64;
    P.ntiles = n / AC4_TS;
    auto wasted_of = [&](uint32_t cc) -> uint32_t {  // candidate cc of this launch (clamped)
        const CandInfo ci = p.cinfo[(size_t)frame0 * p.ncand + (cc < total ? cc : total - 1)];
        return (ci.active && !ci.is_const) ? ci.wasted : 0u;
    };
    if constexpr (STEREO) {
        // unit u: frames 4 (u >> 1) .. + 3 of the group, samples [16 (u & 1), + 16) of the tile;
        // lane = frame-in-unit (2 bits) | R (1 bit) | sample pair (3 bits)
        const uint32_t f_lo = cand0 / 4, f_last = nframes - 1;
        const uint32_t is_r = (lane >> 3) & 1u;
        P.sgn = is_r ? -1 : 1;
#pragma unroll
        for (int it = 0; it < U; it++) {
            const uint32_t u = U0 + it;
            const uint32_t scol = 16u * (u & 1u) + 2u * (lane & 7u);
            const uint32_t fl = 4u * (u >> 1) + (lane >> 4);           // frame of the group, 0..15
            const uint32_t fr = f_lo + fl < nframes ? f_lo + fl : f_last;
            P.gsrc[it] = p.planar + ((size_t)(frame0 + fr) * 2 + is_r) * p.ldb + scol;
            P.wsrc[it] = win + scol;
            P.dst_a[it] = (4 * fl + is_r) * AC4_LDW + scol;         // L or R
            P.dst_b[it] = (4 * fl + 2 + is_r) * AC4_LDW + scol;     // mid or side
            P.sh_a[it] = wasted_of(cand0 + 4 * fl + is_r);
            P.sh_b[it] = wasted_of(cand0 + 4 * fl + 2 + is_r) + (is_r ? 0u : 1u);
        }
    } else {
        // unit u: candidate rows 4 u .. 4 u + 3, all 32 samples of the tile (16 lanes x 2 per row)
        P.sgn = 0;
#pragma unroll
        for (int it = 0; it < U; it++) {
            const uint32_t u = U0 + it;
            const uint32_t scol = 2u * (lane & 15u);
            const uint32_t r = 4u * u + (lane >> 4);      // candidate row 0..63
            const uint32_t g = cand0 + r < total ? cand0 + r : total - 1;
            P.gsrc[it] = p.planar + ((size_t)frame0 * p.channels + g) * p.ldb + scol;
            P.wsrc[it] = win + scol;
            P.dst_a[it] = r * AC4_LDW + scol;
            P.dst_b[it] = P.dst_a[it];
            P.sh_a[it] = wasted_of(cand0 + r);
            P.sh_b[it] = 0;
        }
    }
}
// the loads of tile t (clamped to the frame) into staging set SET = ac4_fetch_slot(t).set
template <int SET, int U, bool STEREO>
__device__ __forceinline__ void ac4_fetch(Ac4Producer<U, STEREO> &P, uint32_t t) {
    t = ac4_fetch_slot(t, P.ntiles, AC4_DEPTH_OF(P)).tile;
#pragma unroll
    for (int it = 0; it < U; it++) {
        P.stage[SET][it] = ac4_ld_int2<AC4_DEPTH_OF(P)>(P.gsrc[it] + t * AC4_TS);
        P.wst[SET][it] = ac4_ld_double2<AC4_DEPTH_OF(P)>(P.wsrc[it] + t * AC4_TS);
    }
}
// windowed[i] = (f64)x[i] * w[i] (encode.rs:1799) of the staged samples into buffer `dst`
template <int SET, int U, bool STEREO>
__device__ __forceinline__ void ac4_convert(const Ac4Producer<U, STEREO> &P, double *dst) {
#pragma unroll
    for (int it = 0; it < U; it++) {
        const double w[2] = {P.wst[SET][it].x, P.wst[SET][it].y};
        const int32_t own[2] = {P.stage[SET][it].x, P.stage[SET][it].y};
        double a[2], b[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            a[e] = (double)(own[e] >> P.sh_a[it]) * w[e];
            if constexpr (STEREO) {
                const int32_t other = dpp_row_ror8(own[e]);
                // mid = (l + r) >> 1 (joined with the wasted-bits shift), side = l - r; <= 24-bit inputs
                const int32_t v = __mul24(own[e], P.sgn) + other;
                b[e] = (double)(v >> P.sh_b[it]) * w[e];
            }
        }
        *reinterpret_cast<double2 *>(dst + P.dst_a[it]) = make_double2(a[0], a[1]);
        if constexpr (STEREO) *reinterpret_cast<double2 *>(dst + P.dst_b[it]) = make_double2(b[0], b[1]);
    }
}
// ---- DIRECT input (stereo, interleaved i32 PCM exactly as FlacSampleWriter::write receives it, encode.rs:558):
// the producers read (l, r) pairs from Params::inter instead of planar rows, so no K0 split pass runs at
// all.  The wasted-bits shift needs the OR of a whole candidate, which nobody has computed yet -- but a right
// shift by w trailing zero bits is an exact division by 2^w, (f64)x 2^-w is exact, and scaling by a power
// of two commutes with every rounding of the products and of the left fold (no underflow at these
// magnitudes): the autocorrelation of the shifted samples is the autocorrelation of the unshifted ones
// times 2^(-2w), bit for bit.  So the producers also OR what they convert (L, R, (l+r)>>1, l-r), the
// workgroup combines the ORs at the end, every lane scales its sums by 2^(-2 ctz(OR)) and the ORs are
// left in the orbits array for k_candinfo, which now runs AFTER this kernel.
// unit u: frames 4 (u >> 1) .. + 3 of the group, samples [16 (u & 1), + 16) of the tile; lane = frame-in-unit
// (2 bits) | sample (4 bits): one (l, r) pair and one window value per lane and unit, four f64 out.
template <int U>
struct Ac4Direct {
    static constexpr int NU = U > 0 ? U : 1;
    static constexpr int DEPTH = ac4_depth<true>();
    const int32_t *gsrc[NU];   // this lane's (l, r) of tile 0
    const double *wsrc[NU];
    uint32_t dst[NU];          // f64 index of the L entry; R, mid, side follow at AC4_LDW strides
    uint32_t orow[NU];         // candidate row of L within the group
    uint32_t ors[NU][4];
    uint32_t ntiles;
    int2 stage[DEPTH][NU];
    double wst[DEPTH][NU];
};
template <int U, int U0>
__device__ __forceinline__ void ac4_setup_direct(const Params &p, uint32_t frame0, uint32_t nframes, uint32_t n,
                                                 const double *__restrict__ win, uint32_t group, Ac4Direct<U> &P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t f_lo = group * 16, f_last = nframes - 1;
    P.ntiles = n / AC4_TS;
#pragma unroll
    for (int it = 0; it < U; it++) {
        const uint32_t u = U0 + it;
        const uint32_t col = 16u * (u & 1u) + (lane & 15u);
        const uint32_t fl = 4u * (u >> 1) + (lane >> 4);           // frame of the group, 0..15
        const uint32_t fr = f_lo + fl < nframes ? f_lo + fl : f_last;
        P.gsrc[it] = inter_frame(p, frame0 + fr, 2 * n) + (size_t)col * 2;
        P.wsrc[it] = win + col;
        P.dst[it] = (4 * fl) * AC4_LDW + col;
        P.orow[it] = 4 * fl;
#pragma unroll
        for (int c = 0; c < 4; c++) P.ors[it][c] = 0;
    }
}
template <int SET, int U>
__device__ __forceinline__ void ac4_fetch(Ac4Direct<U> &P, uint32_t t) {
    t = ac4_fetch_slot(t, P.ntiles, AC4_DEPTH_OF(P)).tile;
#pragma unroll
    for (int it = 0; it < U; it++) {
        P.stage[SET][it] = ac4_ld_int2<AC4_DEPTH_OF(P)>(P.gsrc[it] + t * (AC4_TS * 2));
        P.wst[SET][it] = ac4_ld<AC4_DEPTH_OF(P), double>(P.wsrc[it] + t * AC4_TS);
    }
}
// (a second copy of this loop without the window multiplications for the tiles under window values of exactly 1.0 was
// measured SLOWER -- k_autocorr4 0.151 -> 0.156 ms: the copy costs more than four multiplications; the `flat` argument is
// what is left of it)
template <int SET, int U>
__device__ __forceinline__ void ac4_convert(Ac4Direct<U> &P, double *dst, bool = false) {
#pragma unroll
    for (int it = 0; it < U; it++) {
        const int32_t l = P.stage[SET][it].x, r = P.stage[SET][it].y;
        const int32_t m = (l + r) >> 1, sd = l - r;   // <= 24-bit inputs: no overflow (encode.rs:2721, 2734)
        const double w = P.wst[SET][it];
        P.ors[it][0] |= (uint32_t)l;
        P.ors[it][1] |= (uint32_t)r;
        P.ors[it][2] |= (uint32_t)m;
        P.ors[it][3] |= (uint32_t)sd;
#pragma unroll
        for (int c = 0; c < 4; c++) ac4_pin<AC4_DEPTH_OF(P)>(P.ors[it][c]);
        double *d = dst + P.dst[it];
        d[0] = (double)l * w;
        d[AC4_LDW] = (double)r * w;
        d[2 * AC4_LDW] = (double)m * w;
        d[3 * AC4_LDW] = (double)sd * w;
    }
}
// the ORs of this lane's units into the workgroup's array (one word per candidate row of the group); the
// last tile was converted twice (the prefetch clamps), which an OR does not mind
template <int U>
__device__ __forceinline__ void ac4_finish(const Ac4Direct<U> &P, uint32_t *ors) {
#pragma unroll
    for (int it = 0; it < U; it++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t v = P.ors[it][c];
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);   // the 16 lanes of a frame
            if ((threadIdx.x & 15) == 0) atomicOr(&ors[P.orow[it] + c], v);
        }
    }
}
// ---- SPLIT input (independent channels, interleaved i32 PCM [sample][channel]): the producers ARE the K0 pass.
// They read their two samples of a channel from the interleaved batch (Params::split_src, stride = channels),
// write them to the planar row the later kernels read (Params::split_dst: an 8-byte store, 128 contiguous
// bytes per 16-lane group), OR them for the wasted bits and convert them -- so an independent-channel batch with
// LPC makes one pass less over its input (k_deinterleave_n: 8 B per sample read + written at the HBM roofline).
// The ORs and the 2^(-2 wasted) scaling work exactly as for the stereo direct input above.
// unit u: candidate rows 4 u .. 4 u + 3 of the group, all 32 samples of the tile (16 lanes x 2 per row).
template <int U>
struct Ac4Split {
    static constexpr int NU = U > 0 ? U : 1;
    static constexpr int DEPTH = ac4_depth<false>();
    const int32_t *gsrc[NU];   // this lane's first sample of tile 0 (the second one `stride` dwords further)
    int32_t *pdst[NU];         // the same pair in the planar row
    const double *wsrc[NU];
    uint32_t dst[NU], orow[NU], ors[NU];
    uint32_t ntiles, stride;
    bool store;                // false: one channel -- the input IS the planar row (Params::split_dst == nullptr)
    int2 stage[DEPTH][NU];
    double2 wst[DEPTH][NU];
};
template <int U, int U0>
__device__ __forceinline__ void ac4_setup_split(const Params &p, uint32_t frame0, uint32_t nframes, uint32_t n,
                                                const double *__restrict__ win, uint32_t group, Ac4Split<U> &P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t total = nframes * p.ncand, cand0 = group * 64, C = p.channels;
    P.ntiles = n / AC4_TS;
    P.stride = C;
    P.store = p.split_dst != nullptr;
#pragma unroll
    for (int it = 0; it < U; it++) {
        const uint32_t u = U0 + it;
        const uint32_t scol = 2u * (lane & 15u);
        const uint32_t r = 4u * u + (lane >> 4);      // candidate row 0..63
        const uint32_t g = cand0 + r < total ? cand0 + r : total - 1;
        const uint32_t fr = g / C, ch = g - fr * C;
        P.gsrc[it] = split_frame(p, frame0 + fr, n * C) + (size_t)scol * C + ch;
        P.pdst[it] = p.split_dst + ((size_t)frame0 * C + g) * p.ldb + scol;
        P.wsrc[it] = win + scol;
        P.dst[it] = r * AC4_LDW + scol;
        P.orow[it] = r;
        P.ors[it] = 0;
    }
}
template <int SET, int U>
__device__ __forceinline__ void ac4_fetch(Ac4Split<U> &P, uint32_t t) {
    t = ac4_fetch_slot(t, P.ntiles, AC4_DEPTH_OF(P)).tile;
#pragma unroll
    for (int it = 0; it < U; it++) {
        const int32_t *s = P.gsrc[it] + (size_t)t * AC4_TS * P.stride;
        P.stage[SET][it] = make_int2(ac4_ld<AC4_DEPTH_OF(P), int32_t>(s), ac4_ld<AC4_DEPTH_OF(P), int32_t>(s + P.stride));
        P.wst[SET][it] = ac4_ld_double2<AC4_DEPTH_OF(P)>(P.wsrc[it] + t * AC4_TS);
    }
}
template <int SET, int U>
__device__ __forceinline__ void ac4_convert(Ac4Split<U> &P, double *dst, uint32_t t) {
    t = t < P.ntiles ? t : P.ntiles - 1;   // (the prefetch clamps: the last tile is stored twice, same bytes)
#pragma unroll
    for (int it = 0; it < U; it++) {
        const int2 v = P.stage[SET][it];
        P.ors[it] |= (uint32_t)v.x | (uint32_t)v.y;
        ac4_pin<AC4_DEPTH_OF(P)>(P.ors[it]);
        if (P.store) *reinterpret_cast<int2 *>(P.pdst[it] + t * AC4_TS) = v;
        *reinterpret_cast<double2 *>(dst + P.dst[it]) = make_double2((double)v.x * P.wst[SET][it].x, (double)v.y * P.wst[SET][it].y);
    }
}
template <int U>
__device__ __forceinline__ void ac4_finish(const Ac4Split<U> &P, uint32_t *ors) {
#pragma unroll
    for (int it = 0; it < U; it++) {
        uint32_t v = P.ors[it];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);   // the 16 lanes of a row
        if ((threadIdx.x & 15) == 0) atomicOr(&ors[P.orow[it]], v);
    }
}
// ---- SPLIT producers for 4 or 8 channels: the lanes read CONTIGUOUS memory.  A frame's tile (32 samples x C
// channels) is 32 C consecutive dwords; unit u = 128 of them: frame u / (C / 4) of the group, part u % (C / 4);
// lane l takes the two dwords 2 l, 2 l + 1 of the unit = channels ch, ch + 1 of one sample (8-byte loads, four
// cache lines per instruction instead of thirty-two with the strided pairs above) and feeds TWO rows.
template <int U, int C>
struct Ac4SplitC {
    static constexpr int NU = U > 0 ? U : 1;
    static constexpr int DEPTH = ac4_depth<false>();
    const int32_t *gsrc[NU];   // this lane's (ch, ch + 1) pair of tile 0
    int32_t *pdst[NU];         // planar row of ch at this lane's sample (row of ch + 1: + ldb)
    const double *wsrc[NU];
    uint32_t dst[NU], orow[NU], ors[NU][2];
    uint32_t ntiles, ldb;
    int2 stage[DEPTH][NU];
    double wst[DEPTH][NU];
};
template <int U, int U0, int C>
__device__ __forceinline__ void ac4_setup_split(const Params &p, uint32_t frame0, uint32_t nframes, uint32_t n,
                                                const double *__restrict__ win, uint32_t group, Ac4SplitC<U, C> &P) {
    static_assert(C == 4 || C == 8, "contiguous split: 4 or 8 channels");
    const uint32_t lane = threadIdx.x & 63;
    constexpr uint32_t FPG = 64 / C, PARTS = C / 4;          // frames per group, units per frame and tile
    const uint32_t f_lo = group * FPG, f_last = nframes - 1;
    P.ntiles = n / AC4_TS;
    P.ldb = p.ldb;
#pragma unroll
    for (int it = 0; it < U; it++) {
        const uint32_t u = U0 + it;
        const uint32_t fi = u / PARTS, part = u % PARTS;
        const uint32_t d = part * 128u + 2u * lane;          // dword of the frame's tile
        const uint32_t s = d / C, ch = d % C;
        const uint32_t fr = f_lo + fi < nframes ? f_lo + fi : f_last;
        P.gsrc[it] = split_frame(p, frame0 + fr, n * C) + d;
        P.pdst[it] = p.split_dst ? p.split_dst + ((size_t)(frame0 + fr) * C + ch) * p.ldb + s : nullptr;
        P.wsrc[it] = win + s;
        P.dst[it] = (fi * C + ch) * AC4_LDW + s;
        P.orow[it] = fi * C + ch;
        P.ors[it][0] = P.ors[it][1] = 0;
    }
}
template <int SET, int U, int C>
__device__ __forceinline__ void ac4_fetch(Ac4SplitC<U, C> &P, uint32_t t) {
    t = ac4_fetch_slot(t, P.ntiles, AC4_DEPTH_OF(P)).tile;
#pragma unroll
    for (int it = 0; it < U; it++) {
        P.stage[SET][it] = ac4_ld_int2<AC4_DEPTH_OF(P)>(P.gsrc[it] + (size_t)t * (AC4_TS * C));
        P.wst[SET][it] = ac4_ld<AC4_DEPTH_OF(P), double>(P.wsrc[it] + t * AC4_TS);
    }
}
template <int SET, int U, int C>
__device__ __forceinline__ void ac4_convert(Ac4SplitC<U, C> &P, double *dst, uint32_t t) {
    t = t < P.ntiles ? t : P.ntiles - 1;   // (the prefetch clamps: the last tile is stored twice, same bytes)
#pragma unroll
    for (int it = 0; it < U; it++) {
        const int2 v = P.stage[SET][it];
        P.ors[it][0] |= (uint32_t)v.x;
        P.ors[it][1] |= (uint32_t)v.y;
        ac4_pin<AC4_DEPTH_OF(P)>(P.ors[it][0]);
        ac4_pin<AC4_DEPTH_OF(P)>(P.ors[it][1]);
        if (P.pdst[it]) {   // (wave-uniform: XPOSE batches keep no planar rows)
            int32_t *o = P.pdst[it] + t * AC4_TS;
            o[0] = v.x;
            o[P.ldb] = v.y;
        }
        double *d = dst + P.dst[it];
        d[0] = (double)v.x * P.wst[SET][it];
        d[AC4_LDW] = (double)v.y * P.wst[SET][it];
    }
}
template <int U, int C>
__device__ __forceinline__ void ac4_finish(const Ac4SplitC<U, C> &P, uint32_t *ors) {
#pragma unroll
    for (int it = 0; it < U; it++) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            uint32_t v = P.ors[it][c];
#pragma unroll
            for (int off = 32; off >= C / 2; off >>= 1) v |= __shfl_xor(v, off, 64);   // the lanes of the same channel pair
            if ((threadIdx.x & 63) < C / 2) atomicOr(&ors[P.orow[it] + c], v);
        }
    }
}
// Measurement builds (-DAC4_TIMELINE=1, tools/ac4_timeline.py): every lag-group wave of k_autocorr4 leaves, per tile, the
// low words of six 100 MHz time stamps in a side buffer of the library's own (ac4_tl, read back through
// flacgpu_ac4_timeline): 0 top of the tile, 1 its staged loads have arrived (the wait in front of the conversion; the
// tile's first sixteen LDS reads are issued before it and are awaited with it), 2 tile t + 1 converted and the next
// loads requested, 3 / 4 the two f64 blocks done, 5 past the barrier.  The stamps stay in scalar registers while the tile
// runs; the record of tile t is stored by lane 0 in tile t + 1, behind that tile's load wait, so that no store of the
// timeline's own is outstanding where a wave waits for its input.
#ifndef AC4_TIMELINE
#define AC4_TIMELINE 0
#endif
#if AC4_TIMELINE
constexpr uint32_t AC4_TL_WAVES = 512 * 4, AC4_TL_TILES = 128, AC4_TL_WORDS = 8;
__device__ uint32_t ac4_tl[AC4_TL_WAVES * AC4_TL_TILES * AC4_TL_WORDS];
struct Ac4Timeline {
    uint32_t rec[6], t_prev;   // (stamps 0 and 1 of a tile are taken while the previous tile's record is still unwritten)
    uint32_t cur[2];
    uint32_t *row;   // this wave's records, nullptr: not recorded
    bool pending;
};
__device__ __forceinline__ void ac4_tl_init(Ac4Timeline &T, uint32_t group, uint32_t nwaves, uint32_t ntiles) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = group * nwaves + wave;
    T.row = (nwaves <= 4 && w < AC4_TL_WAVES && ntiles <= AC4_TL_TILES) ? ac4_tl + (size_t)w * AC4_TL_TILES * AC4_TL_WORDS : nullptr;
    T.pending = false;
    T.t_prev = 0;
}
__device__ __forceinline__ void ac4_tl_flush(Ac4Timeline &T) {
    if (T.row && T.pending && (threadIdx.x & 63) == 0) {
        uint32_t *o = T.row + T.t_prev * AC4_TL_WORDS;
        *reinterpret_cast<uint4 *>(o) = make_uint4(T.rec[0], T.rec[1], T.rec[2], T.rec[3]);
        *reinterpret_cast<uint4 *>(o + 4) = make_uint4(T.rec[4], T.rec[5], T.t_prev, 1u);
    }
    T.pending = false;
}
#define AC4_STAMP(k)                                                                    \
    do {                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                              \
        (k < 2 ? tl.cur[k & 1] : tl.rec[k]) = (uint32_t)__builtin_amdgcn_s_memrealtime(); \
        __builtin_amdgcn_sched_barrier(0);                                              \
    } while (0)
// the wait for staging set SET, made here and not at the conversion's first use of it
#define AC4_TL_ARRIVED(P, SET, U)                                                       \
    do {                                                                                \
        _Pragma("unroll") for (int it_ = 0; it_ < (U); it_++)                           \
            asm volatile("" ::"v"((P).stage[SET][it_].x), "v"((P).stage[SET][it_].y)); \
    } while (0)
#else
#define AC4_STAMP(k) do { } while (0)
#endif

__device__ __forceinline__ void ac4_read(const double *row, uint32_t col, double (&w)[16]) {
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const double2 v = *reinterpret_cast<const double2 *>(row + col + 2 * q);
        w[2 * q] = v.x;
        w[2 * q + 1] = v.y;
    }
}

// A, LG: first lag and lag count of this wave; U, U0: its conversion units per tile and the first of them
// DIRECT: interleaved input, ORs and scaling as described above (ors = the workgroup's 64 words)
// FUSE_LPC (DIRECT only): the wave also leaves its lags in the (then idle) tile `wt[0]`, row = candidate, for the
// Levinson tail of k_autocorr4
template <int A, int LG, int U, int U0, bool STEREO, bool DIRECT = false, int SPLITC = 0, bool FUSE_LPC = false>
__device__ __forceinline__ void ac4_wave(const Params &p, double (*wt)[64 * AC4_LDW], uint32_t frame0,
                                         uint32_t nframes, uint32_t n, const double *__restrict__ win,
                                         uint32_t group, uint32_t *ors = nullptr) {
    const uint32_t lane = threadIdx.x & 63;
    // DIRECT && !STEREO: the SPLIT producers (independent channels, K0 folded in); SPLITC = 4 / 8: contiguous reads
    constexpr bool SPLIT = DIRECT && !STEREO;
    std::conditional_t<SPLIT && SPLITC != 0, Ac4SplitC<U, SPLITC ? SPLITC : 4>,
                       std::conditional_t<SPLIT, Ac4Split<U>, std::conditional_t<DIRECT, Ac4Direct<U>, Ac4Producer<U, STEREO>>>> P;
    if constexpr (SPLIT && SPLITC != 0) {
        ac4_setup_split<U, U0, SPLITC>(p, frame0, nframes, n, win, group, P);
        if (threadIdx.x < 64) ors[threadIdx.x] = 0;   // before the first barrier below
    } else if constexpr (SPLIT) {
        ac4_setup_split<U, U0>(p, frame0, nframes, n, win, group, P);
        if (threadIdx.x < 64) ors[threadIdx.x] = 0;   // before the first barrier below
    } else if constexpr (DIRECT) {
        ac4_setup_direct<U, U0>(p, frame0, nframes, n, win, group, P);
        if (threadIdx.x < 64) ors[threadIdx.x] = 0;   // before the first barrier below
    } else {
        ac4_setup<U, U0, STEREO>(p, frame0, nframes, n, win, group, P);
    }
    const uint32_t total = nframes * p.ncand;
    const uint32_t cc = group * 64 + lane;
    const bool live = cc < total;
    double acc[LG];
#pragma unroll
    for (int k = 0; k < LG; k++) acc[k] = -0.0;  // f64 `sum()` identity
    auto convert = [&](auto set, double *dstbuf, uint32_t t) {
        constexpr int SET = decltype(set)::value;
        if constexpr (SPLIT) ac4_convert<SET>(P, dstbuf, t);
        else if constexpr (DIRECT) ac4_convert<SET>(P, dstbuf, t >= p.fma_t0 && t < p.fma_t1);
        else ac4_convert<SET>(P, dstbuf);
    };
    const uint32_t myrow = lane * AC4_LDW;
    double w0[16], w1[16];
#pragma unroll
    for (int s = 0; s < 16; s++) w1[s] = 0.0;
#if AC4_TIMELINE
    Ac4Timeline tl;
    ac4_tl_init(tl, group, blockDim.x >> 6, P.ntiles);
#endif
    // the input pipeline (ac4_fetch_slot, kernels/shape.h): tile 0 converted, tiles 1 .. DEPTH requested
    constexpr uint32_t D = decltype(P)::DEPTH;
    static_assert(D == 1 || D == 2, "the tile loop is unrolled for one or two staging sets");
    ac4_fetch<0>(P, 0);
    convert(std::integral_constant<int, 0>{}, wt[0], 0);
    ac4_fetch<1 % D>(P, 1);
    if constexpr (D == 2) ac4_fetch<0>(P, 2);
    __syncthreads();
    // PHASE = t % DEPTH: the set of tile t + 1 is a compile-time constant, the staging registers statically indexed
    auto tile = [&](auto first, auto phase, uint32_t t) {
        constexpr bool FIRST = decltype(first)::value;
        constexpr int SET = (int)ac4_fetch_slot(decltype(phase)::value + 1u, ~0u, D).set;
        ac4_progress_prio(t, P.ntiles);
        AC4_STAMP(0);
        const double *cur = wt[t & 1] + myrow;
        ac4_read(cur, 0, w0);
        __builtin_amdgcn_sched_barrier(0);
#if AC4_TIMELINE
        AC4_TL_ARRIVED(P, SET, U);
        AC4_STAMP(1);
        ac4_tl_flush(tl);   // the record of tile t - 1
        tl.rec[0] = tl.cur[0];
        tl.rec[1] = tl.cur[1];
#endif
        // tile t + 1 (a repeat of the last tile at the end: unused); only ITS loads are awaited (a counted vmcnt): the
        // requests of tile t + 2 .. t + DEPTH stay in flight across the f64 blocks
        convert(std::integral_constant<int, SET>{}, wt[(t + 1) & 1], t + 1);
        ac4_fetch<SET>(P, ac4_fetch_next(t, D));
        AC4_STAMP(2);
        __builtin_amdgcn_sched_barrier(0);
        // tiles [fma_t0, fma_t1): every term's factors lie under window values of exactly 1.0 (wave-uniform)
        const bool exact = !FIRST && t >= p.fma_t0 && t < p.fma_t1;
        if (exact) {
            if constexpr (!FIRST) ac3_block<A, LG, false, true>(w0, w1, acc);
        } else {
            ac3_block<A, LG, FIRST>(w0, w1, acc);
        }
        AC4_STAMP(3);
        ac4_read(cur, 16, w1);
        __builtin_amdgcn_sched_barrier(0);
        if (exact) ac3_block<A, LG, false, true>(w1, w0, acc);
        else ac3_block<A, LG, false>(w1, w0, acc);
        AC4_STAMP(4);
        __syncthreads();
        AC4_STAMP(5);
#if AC4_TIMELINE
        tl.t_prev = t;
        tl.pending = true;
#endif
    };
    tile(std::true_type{}, std::integral_constant<uint32_t, 0>{}, 0);
    if constexpr (D == 1) {
#pragma unroll 1
        for (uint32_t t = 1; t < P.ntiles; t++) tile(std::false_type{}, std::integral_constant<uint32_t, 0>{}, t);
    } else {
        // pairs of tiles and a tail of its own, not a loop left in its middle: the edge such an exit leaves in the flow
        // graph (from behind the odd tile to the loop's top) makes the compiler wait for both sets at the top
        uint32_t t = 1;
#pragma unroll 1
        for (; t + 1 < P.ntiles; t += 2) {
            tile(std::false_type{}, std::integral_constant<uint32_t, 1>{}, t);
            tile(std::false_type{}, std::integral_constant<uint32_t, 0>{}, t + 1);
        }
        if (t < P.ntiles) tile(std::false_type{}, std::integral_constant<uint32_t, 1>{}, t);
    }
#if AC4_TIMELINE
    ac4_tl_flush(tl);
#endif
    if constexpr (DIRECT) {   // the tile loop ended with a barrier
        ac4_finish(P, ors);
        __syncthreads();
        const uint32_t orv = ors[lane];
        if (A == 0 && live) p.stats[4 + (size_t)frame0 * p.ncand + cc] = orv;   // the orbits array (k_candinfo)
        const uint32_t w2 = orv ? 2u * (uint32_t)__builtin_ctz(orv) : 0u;
        const double scale = __longlong_as_double((long long)(1023u - w2) << 52);   // 2^(-2 wasted), exact
#pragma unroll
        for (int k = 0; k < LG; k++) acc[k] *= scale;
    }
    if (live) {
        double *out = p.ac + ((size_t)frame0 * p.ncand + cc) * AC_LD + A;
#pragma unroll
        for (int k = 0; k < LG; k++) out[k] = acc[k];
    }
    if constexpr (FUSE_LPC) {
        static_assert(DIRECT, "the tile loop and the OR exchange end with barriers: wt[0] is idle here");
        double *row = wt[0] + lane * AC4_LDW + A;   // (AC4_LDW >= 17 lags; every wave is past its last tile read)
#pragma unroll
        for (int k = 0; k < LG; k++) row[k] = acc[k];
    }
}

// NL lags split over NS waves; lag ranges are [NL * w / NS, NL * (w + 1) / NS)
// FUSE_LPC (DIRECT instantiations; VERDICT r03 item 5): K4 -- Levinson-Durbin, order choice, quantisation
// (encode.rs:3536-3580, 3656-3702, 3334-3401), which is also the candidate info of the direct path -- runs in this kernel's
// tail: the lag-group waves leave their sums in LDS, wave 0 (lane = candidate) takes all NL of them and does what
// k_lpc_u<NL - 1> did in a launch of its own behind this kernel (0.015-0.018 ms and a 9 MB round trip per batch).
template <int NL, int NS, bool STEREO, bool DIRECT = false, int SPLITC = 0, bool FUSE_LPC = false>
__global__ void __launch_bounds__(64 * NS)
k_autocorr4(Params p, uint32_t frame0, uint32_t nframes, uint32_t n, const double *__restrict__ win) {
    // DIRECT: STEREO -> interleaved stereo read in place; !STEREO -> interleaved independent channels split here
    __shared__ __attribute__((aligned(16))) double wt[2][64 * AC4_LDW];
    __shared__ uint32_t ors[64];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int B0 = 0, B1 = NL * 1 / NS, B2 = NL * 2 / NS, B3 = NL * 3 / NS, B4 = NL * 4 / NS;
    if constexpr (NS == 8) {
        // EIGHT lag-group waves per 64 candidates (A/B of VERDICT r02 item 8: four waves per SIMD instead of two at
        // 8192 frames; every wave still reads the whole tile, so the LDS read traffic doubles)
        constexpr int C0 = 0, C1 = NL * 1 / 8, C2 = NL * 2 / 8, C3 = NL * 3 / 8, C4 = NL * 4 / 8, C5 = NL * 5 / 8,
                      C6 = NL * 6 / 8, C7 = NL * 7 / 8, C8 = NL;
        constexpr int LGS[8] = {C1 - C0, C2 - C1, C3 - C2, C4 - C3, C5 - C4, C6 - C5, C7 - C6, C8 - C7};
        constexpr Ac4Share S = ac4_share_n<STEREO>(8, LGS);
#define AC4_W(i, a, b) case i: ac4_wave<a, b - a, S.units[i], S.first[i], STEREO, DIRECT, 0, FUSE_LPC>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
        switch (wave) {
            AC4_W(0, C0, C1) AC4_W(1, C1, C2) AC4_W(2, C2, C3) AC4_W(3, C3, C4) AC4_W(4, C4, C5) AC4_W(5, C5, C6) AC4_W(6, C6, C7)
            default: ac4_wave<C7, C8 - C7, S.units[7], S.first[7], STEREO, DIRECT, 0, FUSE_LPC>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
        }
#undef AC4_W
    } else if constexpr (NS == 2) {
        constexpr Ac4Share S = ac4_share<STEREO>(2, B1 - B0, B2 - B1, 0, 0);
        if (wave == 0) ac4_wave<B0, B1 - B0, S.units[0], S.first[0], STEREO, DIRECT>(p, wt, frame0, nframes, n, win, blockIdx.x, ors);
        else ac4_wave<B1, B2 - B1, S.units[1], S.first[1], STEREO, DIRECT>(p, wt, frame0, nframes, n, win, blockIdx.x, ors);
    } else {
        constexpr Ac4Share S = ac4_share<STEREO>(4, B1 - B0, B2 - B1, B3 - B2, B4 - B3);
        switch (wave) {
        case 0: ac4_wave<B0, B1 - B0, S.units[0], S.first[0], STEREO, DIRECT, SPLITC, FUSE_LPC>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
        case 1: ac4_wave<B1, B2 - B1, S.units[1], S.first[1], STEREO, DIRECT, SPLITC, FUSE_LPC>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
        case 2: ac4_wave<B2, B3 - B2, S.units[2], S.first[2], STEREO, DIRECT, SPLITC, FUSE_LPC>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
        default: ac4_wave<B3, B4 - B3, S.units[3], S.first[3], STEREO, DIRECT, SPLITC, FUSE_LPC>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
        }
    }
    if constexpr (FUSE_LPC) {
        static_assert(NS != 2 && NL - 1 <= 16, "DIRECT instantiations: four or eight lag-group waves, order <= 16");
        __syncthreads();                     // every wave's lags are in wt[0], the ORs in `ors`
        if (wave != 0) return;
        const uint32_t lane = threadIdx.x;
        const uint32_t cc = blockIdx.x * 64 + lane;
        if (cc >= nframes * p.ncand) return;
        const uint32_t idx = frame0 * p.ncand + cc;
        const bool act = p.exhaustive ? true : active_in_assignment(p.finfo[idx / p.ncand].assignment, idx % p.ncand);
        const CandInfo ci = cand_info_from_or(p, idx % p.ncand, ors[lane], act);
        p.cinfo[idx] = ci;
        const double *row = wt[0] + lane * AC4_LDW;
        lpc_candidate<NL - 1>(p, idx, n, ci, [row](int i) { return row[i]; });
    }
}

// ---- lags up to 32 (LPC orders 17..32): as k_autocorr4, with the two blocks of history of ac3_block_deep (four f64
// block buffers rotating with a period of two tiles).  K4 is a launch of its own behind this kernel (k_lpc_u<32>): in the
// kernel's tail, as in k_autocorr4, it was measured slower -- 228 instead of 153 VGPRs leave no room for another
// kernel's wave beside two of these (profiles/r04_autocorr_lpc_fuse.json)
template <int A, int LG, int U, int U0, bool STEREO, bool DIRECT = false>
__device__ __forceinline__ void ac4_wave_deep(const Params &p, double (*wt)[64 * AC4_LDW], uint32_t frame0,
                                              uint32_t nframes, uint32_t n, const double *__restrict__ win,
                                              uint32_t group, uint32_t *ors = nullptr) {
    const uint32_t lane = threadIdx.x & 63;
    std::conditional_t<DIRECT, Ac4Direct<U>, Ac4Producer<U, STEREO>> P;
    if constexpr (DIRECT) {
        ac4_setup_direct<U, U0>(p, frame0, nframes, n, win, group, P);
        if (threadIdx.x < 64) ors[threadIdx.x] = 0;   // before the first barrier below
    } else {
        ac4_setup<U, U0, STEREO>(p, frame0, nframes, n, win, group, P);
    }
    const uint32_t total = nframes * p.ncand;
    const uint32_t cc = group * 64 + lane;
    const bool live = cc < total;
    double acc[LG];
#pragma unroll
    for (int k = 0; k < LG; k++) acc[k] = -0.0;  // f64 `sum()` identity
    double wa[16], wb[16], wc[16], wd[16];
#pragma unroll
    for (int s = 0; s < 16; s++) wc[s] = wd[s] = 0.0;
    // the input pipeline of ac4_wave (ac4_fetch_slot, kernels/shape.h); the loop below is unrolled by two tiles already
    constexpr uint32_t D = decltype(P)::DEPTH;
    static_assert(D == 1 || D == 2, "the tile loop is unrolled for one or two staging sets");
    ac4_fetch<0>(P, 0);
    ac4_convert<0>(P, wt[0]);
    ac4_fetch<1 % D>(P, 1);
    if constexpr (D == 2) ac4_fetch<0>(P, 2);
    __syncthreads();
    const uint32_t myrow = lane * AC4_LDW;
    // one tile: X0, X1 receive its two blocks; Y0, Y1 hold the previous tile's; PHASE = t % DEPTH
    auto tile = [&](auto first, auto phase, uint32_t t, double (&X0)[16], double (&X1)[16], double (&Y0)[16], double (&Y1)[16]) {
        constexpr bool FIRST = decltype(first)::value;
        constexpr int SET = (int)ac4_fetch_slot(decltype(phase)::value + 1u, ~0u, D).set;
        ac4_progress_prio(t, P.ntiles);
        const double *cur = wt[t & 1] + myrow;
        ac4_read(cur, 0, X0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (DIRECT) ac4_convert<SET>(P, wt[(t + 1) & 1], t + 1 >= p.fma_t0 && t + 1 < p.fma_t1);
        else ac4_convert<SET>(P, wt[(t + 1) & 1]);
        ac4_fetch<SET>(P, ac4_fetch_next(t, D));
        __builtin_amdgcn_sched_barrier(0);
        const bool exact = !FIRST && t >= p.fma_t0 && t < p.fma_t1;   // (see ac4_wave)
        if (exact) {
            if constexpr (!FIRST) ac3_block_deep<A, LG, 0, true>(X0, Y1, Y0, acc);
        } else {
            ac3_block_deep<A, LG, FIRST ? 1 : 0>(X0, Y1, Y0, acc);
        }
        ac4_read(cur, 16, X1);
        __builtin_amdgcn_sched_barrier(0);
        if (exact) {
            if constexpr (!FIRST) ac3_block_deep<A, LG, 0, true>(X1, X0, Y1, acc);
        } else {
            ac3_block_deep<A, LG, FIRST ? 2 : 0>(X1, X0, Y1, acc);
        }
        __syncthreads();
    };
    using Ph0 = std::integral_constant<uint32_t, 0>;
    using Ph1 = std::integral_constant<uint32_t, 1 % D>;
    tile(std::true_type{}, Ph0{}, 0, wa, wb, wc, wd);
    uint32_t t = 1;
#pragma unroll 1
    for (; t + 1 < P.ntiles; t += 2) {  // n is a multiple of 64: an even number of tiles
        tile(std::false_type{}, Ph1{}, t, wc, wd, wa, wb);
        tile(std::false_type{}, Ph0{}, t + 1, wa, wb, wc, wd);
    }
    if (t < P.ntiles) tile(std::false_type{}, Ph1{}, t, wc, wd, wa, wb);
    if constexpr (DIRECT) {   // the tile loop ended with a barrier
        ac4_finish(P, ors);
        __syncthreads();
        const uint32_t orv = ors[lane];
        if (A == 0 && live) p.stats[4 + (size_t)frame0 * p.ncand + cc] = orv;   // the orbits array (k_candinfo)
        const uint32_t w2 = orv ? 2u * (uint32_t)__builtin_ctz(orv) : 0u;
        const double scale = __longlong_as_double((long long)(1023u - w2) << 52);   // 2^(-2 wasted), exact
#pragma unroll
        for (int k = 0; k < LG; k++) acc[k] *= scale;
    }
    if (live) {
        double *out = p.ac + ((size_t)frame0 * p.ncand + cc) * AC_LD + A;
#pragma unroll
        for (int k = 0; k < LG; k++) out[k] = acc[k];
    }
}

template <bool STEREO, bool DIRECT = false>
__global__ void __launch_bounds__(256, 2)
k_autocorr4_deep(Params p, uint32_t frame0, uint32_t nframes, uint32_t n, const double *__restrict__ win) {
    static_assert(!DIRECT || STEREO, "direct input: interleaved stereo");
    __shared__ __attribute__((aligned(16))) double wt[2][64 * AC4_LDW];
    __shared__ uint32_t ors[64];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr Ac4Share S = ac4_share<STEREO>(4, 8, 8, 8, 9);   // 33 lags: 8 + 8 + 8 + 9
    switch (wave) {
    case 0: ac4_wave_deep<0, 8, S.units[0], S.first[0], STEREO, DIRECT>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
    case 1: ac4_wave_deep<8, 8, S.units[1], S.first[1], STEREO, DIRECT>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
    case 2: ac4_wave_deep<16, 8, S.units[2], S.first[2], STEREO, DIRECT>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
    default: ac4_wave_deep<24, 9, S.units[3], S.first[3], STEREO, DIRECT>(p, wt, frame0, nframes, n, win, blockIdx.x, ors); break;
    }
}

// ---------------------------------------------------------------------------------
// K3 (tiled): generic kernel (any candidate set, block length and order); the samples reach the lanes
// through LDS.  A 256-thread workgroup serves 64 candidates; its 4 waves are the 4 lag groups.
// Per tile of TS samples:
//   1. the planar rows those candidates need (<= 72) are staged with coalesced 16-byte loads
//      (global -> registers for tile i+1 is issued while tile i is consumed);
//   2. all 256 lanes together turn them into the candidates' WINDOWED f64 samples
//      (mid/side derivation, wasted-bit shift, (f64)x * w[i], encode.rs:1799) exactly once;
//   3. every wave walks the 64 f64 columns for its lag group: one LDS read + LG mul/add pairs
//      per sample, ring of the last H values in registers, statically indexed.
// ---------------------------------------------------------------------------------
constexpr int AC_MAXROWS = 72;

template <int H, int A, int LG, bool FIRST, bool GUARDED>
__device__ __forceinline__ void ac_block_w(double (&hist)[H], double (&acc)[LG], const double *tw,
                                           uint32_t col0, uint32_t base, uint32_t n) {
    double w[H];
#pragma unroll
    for (int s = 0; s < H; s++) w[s] = tw[col0 + s];
#pragma unroll
    for (int s = 0; s < H; s++) {
        hist[s] = w[s];
        if (!GUARDED || base + s < n) {
#pragma unroll
            for (int k = 0; k < LG; k++) {
                const int lag = A + k;
                if (!FIRST || s >= lag) {
                    const double prod = w[s] * hist[(s - lag + 2 * H) % H];
                    acc[k] = acc[k] + prod;
                }
            }
        }
    }
}

template <int H, int A, int LG, int KB, int LDT, int LDW, int NW>
__device__ __forceinline__ void ac_wave(const Params &p, int32_t (*tile)[AC_MAXROWS * LDT],
                                        double *wt, uint32_t frame0, uint32_t nframes, uint32_t n,
                                        const double *__restrict__ win) {
    constexpr int TS = H * KB;          // samples per tile
    constexpr int Q = TS / 4;           // int4 per row per tile
    constexpr int NT = 64 * NW;         // threads per workgroup
    constexpr int NLOAD = (AC_MAXROWS * Q + NT - 1) / NT;
    constexpr int CW = (TS + NW - 1) / NW;  // columns converted per wave
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t total = nframes * p.ncand;
    const uint32_t cand0 = blockIdx.x * 64;
    const uint32_t last_c = cand0 + 63 < total ? cand0 + 63 : total - 1;
    const bool live = cand0 + lane < total;
    const uint32_t cc = live ? cand0 + lane : last_c;
    const uint32_t f_lo = cand0 / p.ncand, f_hi = last_c / p.ncand;
    const uint32_t frame = frame0 + cc / p.ncand;
    const uint32_t cand = cc % p.ncand;
    const uint32_t nrows = (f_hi - f_lo + 1) * p.channels;
    const int32_t *gbase = p.planar + (size_t)(frame0 + f_lo) * p.channels * p.ldb;
    // this lane's two source rows inside the staged set
    uint32_t ca = cand, cb = cand;
    int mode = 0;
    if (p.stereo4) {
        if (cand >= 2) { ca = 0; cb = 1; mode = cand == 2 ? 1 : 2; }
    }
    const uint32_t ra = (cc / p.ncand - f_lo) * p.channels + ca;
    const uint32_t rb = (cc / p.ncand - f_lo) * p.channels + cb;
    const CandInfo ci = p.cinfo[(size_t)frame * p.ncand + cand];
    const uint32_t wasted = (ci.active && !ci.is_const) ? ci.wasted : 0;

    double hist[H], acc[LG];
#pragma unroll
    for (int k = 0; k < LG; k++) acc[k] = -0.0;  // f64 `sum()` identity
#pragma unroll
    for (int s = 0; s < H; s++) hist[s] = 0.0;

    const uint32_t ntiles = (n + TS - 1) / TS;
    int4 stage[NLOAD];
    auto fetch = [&](uint32_t t) {
#pragma unroll
        for (int k = 0; k < NLOAD; k++) {
            const uint32_t idx = tid + k * NT;
            const uint32_t r = idx / Q, c4 = idx - r * Q;
            const uint32_t col = t * TS + 4 * c4;
            stage[k] = (r < nrows && col < p.ldb)
                           ? *reinterpret_cast<const int4 *>(gbase + (size_t)r * p.ldb + col)
                           : make_int4(0, 0, 0, 0);
        }
    };
    auto commit = [&](uint32_t buf) {
#pragma unroll
        for (int k = 0; k < NLOAD; k++) {
            const uint32_t idx = tid + k * NT;
            const uint32_t r = idx / Q, c4 = idx - r * Q;
            if (r < AC_MAXROWS) *reinterpret_cast<int4 *>(&tile[buf][r * LDT + 4 * c4]) = stage[k];
        }
    };
    fetch(0);
    commit(0);
    __syncthreads();
    double *tw = wt + lane * LDW;  // this lane's candidate row of windowed samples
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint32_t buf = t & 1;
        const uint32_t tbase = t * TS;
        if (t + 1 < ntiles) fetch(t + 1);
        {   // step 2: wave `wave` converts columns [wave*CW, wave*CW + CW) of all 64 candidates
            const int32_t *ta = &tile[buf][ra * LDT];
            const int32_t *tb = &tile[buf][rb * LDT];
#pragma unroll
            for (int c = 0; c < CW; c++) {
                const uint32_t col = wave * CW + c;
                if (col < (uint32_t)TS) {
                    const int32_t v = combine(mode, ta[col], tb[col]) >> wasted;
                    tw[col] = (double)v * win[tbase + col];
                }
            }
        }
        __syncthreads();
        if (tbase + TS <= n && t > 0) {
#pragma unroll 1
            for (int b = 0; b < KB; b++)
                ac_block_w<H, A, LG, false, false>(hist, acc, tw, b * H, tbase + b * H, n);
        } else {
#pragma unroll 1
            for (int b = 0; b < KB; b++) {
                const uint32_t base = tbase + b * H;
                if (base >= n) break;
                if (base == 0) ac_block_w<H, A, LG, true, true>(hist, acc, tw, b * H, base, n);
                else ac_block_w<H, A, LG, false, true>(hist, acc, tw, b * H, base, n);
            }
        }
        if (t + 1 < ntiles) commit(buf ^ 1);
        __syncthreads();
    }
    if (live) {
        double *out = p.ac + ((size_t)frame * p.ncand + cand) * AC_LD + A;
#pragma unroll
        for (int k = 0; k < LG; k++) out[k] = acc[k];
    }
}

constexpr int AC_TILE = 64;   // samples per LDS tile (32 + a 128-VGPR cap overlapped better with other kernels
                              // but ran 0.55 instead of 0.35 ms on its own: net loss)
template <int H, int NW>
__global__ void __launch_bounds__(64 * NW)
k_autocorr2(Params p, uint32_t frame0, uint32_t nframes, uint32_t n, const double *__restrict__ win) {
    constexpr int LG = H / NW;       // lags per wave (lag group)
    constexpr int KB = (AC_TILE / H) > 0 ? (AC_TILE / H) : 1;
    constexpr int LDT = H * KB + 4;  // int row stride: 16-byte aligned rows
    constexpr int LDW = H * KB + 1;  // f64 row stride: odd => lanes (= rows) hit distinct banks
    __shared__ __attribute__((aligned(16))) int32_t tile[2][AC_MAXROWS * LDT];
    __shared__ double wt[64 * LDW];
    // wave = lag group; each wave runs its own statically indexed code
    switch (threadIdx.x >> 6) {
    case 0: ac_wave<H, 0 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
    case 1: ac_wave<H, 1 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
    case 2: ac_wave<H, 2 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
    case 3: ac_wave<H, 3 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
    default:
        if constexpr (NW == 8) {
            switch (threadIdx.x >> 6) {
            case 4: ac_wave<H, 4 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
            case 5: ac_wave<H, 5 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
            case 6: ac_wave<H, 6 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
            default: ac_wave<H, 7 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt, frame0, nframes, n, win); break;
            }
        }
        break;
    }
}

// ---------------------------------------------------------------------------------
// K3 for a RAGGED batch (Params::frame_n): k_autocorr2's scheme -- 64 candidates per workgroup, lane = candidate, wave = lag
// group, the samples through LDS tiles -- with every candidate's length n and window taken from the per-frame tables.
//   * One workgroup keeps 64 candidates of MIXED lengths; nothing is ordered by length on the host.  The tile loop runs to
//     the group's longest frame (nmax, the same in all four waves: each holds the same 64 candidates).
//   * A lane past its own n adds NOTHING: its terms are skipped by the per-sample guard of ac_block_w (base + s < n), never
//     formed and added as zeros -- so each lag's sum is the reference's left fold over i < n, one multiply and one add per
//     term, in exactly the instruction sequence k_autocorr2 runs for a batch whose frames all have this n (there the guard
//     is the short last tile's).  The -0.0 start and the order of the adds are ac_wave's.
//   * The window value is per lane (window_pool + frame_win[frame] + i), read only for i < n; beyond, the converted sample
//     is 0.0 and is never used.  The staged rows are read up to the tile's end like k_autocorr2's (planar rows, < ldb).
//   * A tile that every lane of the wave has in full takes the unguarded blocks (wave-uniform test).
// ---------------------------------------------------------------------------------
template <int H, int A, int LG, int KB, int LDT, int LDW, int NW>
__device__ __forceinline__ void ac_wave_ragged(const Params &p, int32_t (*tile)[AC_MAXROWS * LDT], double *wt) {
    constexpr int TS = H * KB;          // samples per tile
    constexpr int Q = TS / 4;           // int4 per row per tile
    constexpr int NT = 64 * NW;         // threads per workgroup
    constexpr int NLOAD = (AC_MAXROWS * Q + NT - 1) / NT;
    constexpr int CW = (TS + NW - 1) / NW;  // columns converted per wave
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t total = p.n_frames * p.ncand;
    const uint32_t cand0 = blockIdx.x * 64;
    const uint32_t last_c = cand0 + 63 < total ? cand0 + 63 : total - 1;
    const bool live = cand0 + lane < total;
    const uint32_t cc = live ? cand0 + lane : last_c;
    const uint32_t f_lo = cand0 / p.ncand, f_hi = last_c / p.ncand;
    const uint32_t frame = cc / p.ncand;
    const uint32_t cand = cc % p.ncand;
    const uint32_t nrows = (f_hi - f_lo + 1) * p.channels;
    const int32_t *gbase = p.planar + (size_t)f_lo * p.channels * p.ldb;
    const uint32_t n = p.frame_n[frame];                       // this lane's frame length
    const double *__restrict__ win = p.window_pool + p.frame_win[frame];
    uint32_t nmax = n;                                         // the longest frame of the group
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)nmax, off, 64);
        nmax = o > nmax ? o : nmax;
    }
    nmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)nmax);
    // this lane's two source rows inside the staged set
    uint32_t ca = cand, cb = cand;
    int mode = 0;
    if (p.stereo4) {
        if (cand >= 2) { ca = 0; cb = 1; mode = cand == 2 ? 1 : 2; }
    }
    const uint32_t ra = (frame - f_lo) * p.channels + ca;
    const uint32_t rb = (frame - f_lo) * p.channels + cb;
    const CandInfo ci = p.cinfo[(size_t)frame * p.ncand + cand];
    const uint32_t wasted = (ci.active && !ci.is_const) ? ci.wasted : 0;

    double hist[H], acc[LG];
#pragma unroll
    for (int k = 0; k < LG; k++) acc[k] = -0.0;  // f64 `sum()` identity
#pragma unroll
    for (int s = 0; s < H; s++) hist[s] = 0.0;

    const uint32_t ntiles = (nmax + TS - 1) / TS;
    int4 stage[NLOAD];
    auto fetch = [&](uint32_t t) {
#pragma unroll
        for (int k = 0; k < NLOAD; k++) {
            const uint32_t idx = tid + k * NT;
            const uint32_t r = idx / Q, c4 = idx - r * Q;
            const uint32_t col = t * TS + 4 * c4;
            stage[k] = (r < nrows && col < p.ldb)
                           ? *reinterpret_cast<const int4 *>(gbase + (size_t)r * p.ldb + col)
                           : make_int4(0, 0, 0, 0);
        }
    };
    auto commit = [&](uint32_t buf) {
#pragma unroll
        for (int k = 0; k < NLOAD; k++) {
            const uint32_t idx = tid + k * NT;
            const uint32_t r = idx / Q, c4 = idx - r * Q;
            if (r < AC_MAXROWS) *reinterpret_cast<int4 *>(&tile[buf][r * LDT + 4 * c4]) = stage[k];
        }
    };
    fetch(0);
    commit(0);
    __syncthreads();
    double *tw = wt + lane * LDW;  // this lane's candidate row of windowed samples
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint32_t buf = t & 1;
        const uint32_t tbase = t * TS;
        if (t + 1 < ntiles) fetch(t + 1);
        {   // wave `wave` converts columns [wave*CW, wave*CW + CW) of all 64 candidates
            const int32_t *ta = &tile[buf][ra * LDT];
            const int32_t *tb = &tile[buf][rb * LDT];
#pragma unroll
            for (int c = 0; c < CW; c++) {
                const uint32_t col = wave * CW + c;
                if (col < (uint32_t)TS) {
                    const uint32_t i = tbase + col;
                    double v = 0.0;
                    if (i < n) v = (double)(combine(mode, ta[col], tb[col]) >> wasted) * win[i];
                    tw[col] = v;
                }
            }
        }
        __syncthreads();
        if (t > 0 && __all(tbase + TS <= n)) {   // (wave-uniform)
#pragma unroll 1
            for (int b = 0; b < KB; b++)
                ac_block_w<H, A, LG, false, false>(hist, acc, tw, b * H, tbase + b * H, n);
        } else {
#pragma unroll 1
            for (int b = 0; b < KB; b++) {
                const uint32_t base = tbase + b * H;
                if (base >= nmax) break;
                if (base == 0) ac_block_w<H, A, LG, true, true>(hist, acc, tw, b * H, base, n);
                else ac_block_w<H, A, LG, false, true>(hist, acc, tw, b * H, base, n);
            }
        }
        if (t + 1 < ntiles) commit(buf ^ 1);
        __syncthreads();
    }
    if (live) {
        double *out = p.ac + ((size_t)frame * p.ncand + cand) * AC_LD + A;
#pragma unroll
        for (int k = 0; k < LG; k++) out[k] = acc[k];
    }
}

template <int H, int NW>
__global__ void __launch_bounds__(64 * NW)
k_autocorr_ragged(Params p) {
    static_assert(NW == 4, "four lag-group waves");
    constexpr int LG = H / NW;       // lags per wave (lag group)
    constexpr int KB = (AC_TILE / H) > 0 ? (AC_TILE / H) : 1;
    constexpr int LDT = H * KB + 4;  // int row stride: 16-byte aligned rows
    constexpr int LDW = H * KB + 1;  // f64 row stride: odd => lanes (= rows) hit distinct banks
    __shared__ __attribute__((aligned(16))) int32_t tile[2][AC_MAXROWS * LDT];
    __shared__ double wt[64 * LDW];
    switch (threadIdx.x >> 6) {
    case 0: ac_wave_ragged<H, 0 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt); break;
    case 1: ac_wave_ragged<H, 1 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt); break;
    case 2: ac_wave_ragged<H, 2 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt); break;
    default: ac_wave_ragged<H, 3 * LG, LG, KB, LDT, LDW, NW>(p, tile, wt); break;
    }
}

// ---------------------------------------------------------------------------------
// EXPERIMENT (not on the product path): autocorrelation on the f64 matrix cores.
// Block-Gram form: with X[a][m] = w[16 a + m] (a = 0..n/16-1, m = 0..15),
//   G1 = X^T X            (pairs inside one 16-sample block)
//   G2[m][m'] = sum_a X[a][m] X[a+1][m']   (pairs straddling two consecutive blocks)
//   ac[lag] = sum_{m'-m=lag} G1[m][m'] + sum_{m'+16-m=lag} G2[m][m'],   0 <= lag <= 16.
// One wave per candidate; per 64 samples two v_mfma_f64_16x16x4_f64 (lane l feeds
// A[l&15][l>>4] = B[l>>4][l&15] = w[64 s + l] for G1, B = w[64 s + 16 + l] for G2).
// The summation order differs from the reference's left fold, so the result is NOT
// bit-exact; flacgpu_experiment_mfma_autocorr() measures both its speed and how many
// candidates' quantised LPC parameters change.  On MI355X the f64 MFMA peak equals the f64
// VALU peak, so this buys no time either (DESIGN.md section 4, K3).
// ---------------------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(WG) k_autocorr_mfma(Params p, uint32_t n,
                                                      const double *__restrict__ win,
                                                      double *__restrict__ ac_out) {
    __shared__ double acc[4][20];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t total = p.n_frames * p.ncand;
    const uint32_t cidx = blockIdx.x * 4 + wave;
    const bool live = cidx < total;
    const uint32_t cc = live ? cidx : 0;
    const uint32_t frame = cc / p.ncand, cand = cc % p.ncand;
    const CandSrc src = cand_src(p, frame, cand);
    const CandInfo ci = p.cinfo[cc];
    const uint32_t wasted = (ci.active && !ci.is_const) ? ci.wasted : 0;
    if (lane < 20) acc[wave][lane] = 0.0;
    auto load = [&](uint32_t s) -> double {
        const uint32_t i = 64 * s + lane;
        if (i >= n) return 0.0;
        return (double)(combine(src.mode, src.a[i], src.b[i]) >> wasted) * win[i];
    };
    double4_t g1 = {0, 0, 0, 0}, g2 = {0, 0, 0, 0};
    const uint32_t nsteps = (n + 63) / 64;
    double cur = load(0);
    for (uint32_t s = 0; s < nsteps; s++) {
        const double nxt = (s + 1 < nsteps) ? load(s + 1) : 0.0;
        const double from_cur = __shfl(cur, (int)((lane + 16) & 63), 64);
        const double from_nxt = __shfl(nxt, (int)((lane + 16) & 63), 64);
        const double wb = lane < 48 ? from_cur : from_nxt;
        g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(cur, cur, g1, 0, 0, 0);
        g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(cur, wb, g2, 0, 0, 0);
        cur = nxt;
    }
    __syncthreads();
    // lane l holds D[row = (l >> 4) + 4 r][col = l & 15] (f64 C/D layout)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = (int)(lane >> 4) + 4 * r, j = (int)(lane & 15);
        if (j - i >= 0) atomicAdd(&acc[wave][j - i], g1[r]);
        if (j + 16 - i <= 16) atomicAdd(&acc[wave][j + 16 - i], g2[r]);
    }
    __syncthreads();
    if (live && lane <= 16) ac_out[(size_t)cc * AC_LD + lane] = acc[wave][lane];
}
