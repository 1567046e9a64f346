// lpc.inc -- K4: Levinson-Durbin, order choice, quantisation.
// Part of flacenc_gpu.hip (one translation unit; included inside its anonymous namespace).

// ---------------------------------------------------------------------------------
// K4: Levinson-Durbin + order estimate + quantisation, one lane per candidate
// ---------------------------------------------------------------------------------
__device__ __forceinline__ long long total_key(double x) {  // f64::total_cmp key
    long long b = __double_as_longlong(x);
    b ^= (long long)((unsigned long long)(b >> 63) >> 1);
    return b;
}

// The device's log() may differ from the host libm's in the last place; that can only change the order
// choice when the two best estimates agree to ~1e-12.  Candidates inside tie_band are listed for the
// host, which re-decides them with its own libm (flacgpu: resolve_order_ties).
__device__ __forceinline__ void note_order_tie(const Params &p, uint32_t idx, bool have_second, double second,
                                               double best_bits) {
    if (have_second && fabs(second - best_bits) <= p.tie_band * fabs(best_bits)) {
        const uint32_t slot = atomicAdd(&p.stats[1], 1u);
        if (slot < p.tie_cap) p.tie_list[slot] = idx;
    }
}

// the order estimate's bits of the chosen order as 1/8 bit per sample, 1..255 (LpcParams::est8: a hint, see Params::defer_fixed)
__device__ __forceinline__ uint8_t lpc_est8(double best_bits, uint32_t n) {
    const double e = best_bits * 8.0 / (double)n;
    return (uint8_t)(e >= 255.0 ? 255 : e >= 1.0 ? (int)e + 1 : 1);   // rounded UP: the hint must not flatter LPC
}

// Levinson-Durbin recursion up to `upto` orders (lp_coefficients, encode.rs:3536-3580), every loop
// unrolled and guarded so that the arrays stay in registers
template <int LMAX>
__device__ __forceinline__ void levinson_u(const double (&acr)[LMAX + 1], uint32_t upto, double (&c)[LMAX],
                                           double (&errs)[LMAX]) {
    double cn[LMAX];
    double k = acr[1] / acr[0];
    c[0] = k;
    double err = acr[0] * (1.0 - k * k);
    errs[0] = err;
#pragma unroll
    for (int i = 1; i < LMAX; i++) {
        if ((uint32_t)i < upto) {
            double s = -0.0;
#pragma unroll
            for (int j = 0; j < i; j++) {
                double prod = acr[i - j] * c[j];
                s = s + prod;
            }
            double q = acr[i + 1] - s;
            double kk = q / err;
#pragma unroll
            for (int j = 0; j < i; j++) {
                double t = kk * c[i - 1 - j];
                cn[j] = c[j] - t;
            }
            cn[i] = kk;
#pragma unroll
            for (int j = 0; j <= i; j++) c[j] = cn[j];
            err = err * (1.0 - kk * kk);
            errs[i] = err;
        }
    }
}

// K4 with max_lpc_order <= LMAX known at compile time (with run-time loop bounds the coefficient arrays would sit in
// scratch memory and every access would be a memory round trip: 8 / 12 / 16 / 32 are instantiated).
// lpc_candidate: one lane = one candidate; `ac(i)` returns autocorrelation lag i (from HBM in k_lpc_u, from the LDS hand-off of
// the lag-group waves in the fused tail of k_autocorr4).
template <int LMAX, class AcAt>
__device__ __forceinline__ void lpc_candidate(const Params &p, uint32_t idx, uint32_t n, CandInfo ci, AcAt &&ac) {
    static_assert(LMAX <= FLACGPU_MAX_LPC_ORDER, "order");
    LpcParams *out = p.lpc + idx;
    if (!ci.active || ci.is_const) {
        out->status = 1;
        return;
    }
    const uint32_t L = p.max_lpc_order;
    if (n <= L) {  // InsufficientLpcSamples, encode.rs:3300
        out->status = 1;
        atomicAdd(&p.stats[0], 1u);
        return;
    }
    // precision table, encode.rs:3305-3315
    const uint32_t precision = n <= 192 ? 7 : n <= 384 ? 8 : n <= 576 ? 9 : n <= 1152 ? 10
                               : n <= 2304 ? 11 : n <= 4608 ? 12 : 13;
    double acr[LMAX + 1], c[LMAX], errs[LMAX];
#pragma unroll
    for (int i = 0; i <= LMAX; i++) acr[i] = (uint32_t)i <= L ? ac(i) : 0.0;
    // pass 1: errors of every order
    levinson_u<LMAX>(acr, L, c, errs);
    // compute_best_order, encode.rs:3656-3702 (bits-per-residual NOT clamped, :3675)
    const double LN_2 = 0.693147180559945309417232121458176568;
    const double error_scale = 0.5 / (double)n;
    const double denom = 2.0 * LN_2;
    int best = -1;
    double best_bits = 0.0, second = 0.0;
    bool have_second = false;
    bool going = true;
#pragma unroll
    for (int i = 0; i < LMAX; i++) {
        going = going && (uint32_t)i < L && errs[i] > 0.0;  // take_while(error > 0.0)
        if (!going) continue;
        uint32_t order = i + 1;
        double header_bits = (double)(order * ((uint32_t)ci.bps + precision));
        double bpr = log(errs[i] * error_scale) / denom;
        double bits = __builtin_fma(bpr, (double)(n - order), header_bits);
        bits = bits * (1.0 + ((i & 1) ? p.tie_perturb : -p.tie_perturb));   // test knob, exact when 0
        if (best < 0) {
            best = (int)i;
            best_bits = bits;
        } else if (total_key(bits) < total_key(best_bits)) {
            second = best_bits;
            have_second = true;
            best = (int)i;
            best_bits = bits;
        } else if (!have_second || total_key(bits) < total_key(second)) {
            second = bits;
            have_second = true;
        }
    }
    if (best < 0) {  // NoBestLpcOrder
        out->status = 2;
        atomicAdd(&p.stats[0], 1u);
        return;
    }
    note_order_tie(p, idx, have_second, second, best_bits);
    const uint32_t order = (uint32_t)best + 1;
    // pass 2: coefficients of the chosen order (same recursion, same roundings)
    levinson_u<LMAX>(acr, order, c, errs);
    // quantize, encode.rs:3334-3401
    const int32_t max_coeff = (1 << (precision - 1)) - 1, min_coeff = -(1 << (precision - 1));
    double l = fabs(c[0]);
#pragma unroll
    for (int i = 1; i < LMAX; i++) {
        if ((uint32_t)i < order) {
            double a = fabs(c[i]);
            if (total_key(a) >= total_key(l)) l = a;
        }
    }
    if (!(l > 0.0)) {  // ZeroLpCoefficients (also NaN)
        out->status = 3;
        atomicAdd(&p.stats[0], 1u);
        return;
    }
    // floor(log2(l)) as the host libm computes it: exponent, bumped when l sits in the
    // (few-ulp) band below 2^(e+1) where log2() rounds up to e+1 (table built on the host)
    int32_t fl;
    if (isinf(l)) {
        fl = INT32_MAX;
    } else {
        int e = ilogb(l);
        fl = e;
        if (e >= -64 && e < 64 && l >= p.log2_thr[e + 64]) {
            fl = e + 1;
            atomicAdd(&p.stats[2], 1u);
        }
    }
    int32_t sh = (int32_t)((uint32_t)(int32_t)(precision - 1) - (uint32_t)fl - 1u);
    if (sh > 15) sh = 15;
    if (sh < -16) {  // LpNegativeShiftError
        out->status = 4;
        atomicAdd(&p.stats[0], 1u);
        return;
    }
    double error = 0.0;
    const double scale = (double)(1 << (sh >= 0 ? sh : -sh));
#pragma unroll
    for (int i = 0; i < LMAX; i++) {
        if ((uint32_t)i >= order) continue;
        double sum = sh >= 0 ? __builtin_fma(c[i], scale, error) : (c[i] / scale) + error;
        double rr = round(sum);
        int32_t q = (rr != rr) ? 0 : rr >= 2147483647.0 ? INT32_MAX : rr <= -2147483648.0 ? INT32_MIN
                                                                                         : (int32_t)rr;
        q = q < min_coeff ? min_coeff : q > max_coeff ? max_coeff : q;
        error = sum - (double)q;
        out->qlp[i] = q;
    }
    out->status = 0;
    out->order = (uint8_t)order;
    out->precision = (uint8_t)precision;
    out->shift = (uint8_t)(sh >= 0 ? sh : 0);
    out->est8 = lpc_est8(best_bits, n);
}

template <int LMAX>
__global__ void __launch_bounds__(64) k_lpc_u(Params p) {
    const uint32_t idx = p.f0 * p.ncand + blockIdx.x * 64 + threadIdx.x;
    if (idx >= (p.f0 + p.fcount) * p.ncand) return;
    const uint32_t frame = idx / p.ncand;
    const uint32_t n = frame_len(p, frame);
    // DIRECT input: the ORs came out of the autocorrelation kernel just before; this kernel is k_candinfo too
    CandInfo ci;
    if (p.inter || p.split_src) {
        const bool act = p.exhaustive ? true : active_in_assignment(p.finfo[idx / p.ncand].assignment, idx % p.ncand);
        ci = cand_info_from_or(p, idx % p.ncand, p.stats[4 + idx], act);
        p.cinfo[idx] = ci;
    } else {
        ci = p.cinfo[idx];
    }
    const double *ac = p.ac + (size_t)idx * AC_LD;
    lpc_candidate<LMAX>(p, idx, n, ci, [ac](int i) { return ac[i]; });
}
