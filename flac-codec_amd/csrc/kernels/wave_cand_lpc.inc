// wave_cand_lpc.inc -- LPC half of a candidate wave's analysis: in-place FIR with the quantised coefficients of
// K4, Rice search of the stored residual (encode.rs:3174-3203 + the same residual coding).  Textually included
// (wave_cand_body.inc / wave_cand_split.inc).  In scope: p, lane, x[SPL] (shifted; destroyed), lpw, qv, wasted,
// bps_eff, N, SPL, MAXO, HAND (Params::hand_meta: the fold keeps the signs) and a WaveRice `lw` to fill.  Leaves lpc_ok, lpc_bits, lorder, lprec, lshift, lw.
    // ---- LPC (encode.rs:3174-3203 + the same residual coding)
    bool lpc_ok = false;
    uint32_t lpc_bits = 0;
    const uint32_t lstatus = sread(lpw, 0), lmeta = sread(lpw, 1);
    const uint32_t lprec = (lmeta >> 8) & 0xFF, lshift = (lmeta >> 16) & 0xFF;
    uint32_t lorder = 0;
    if (lstatus == 0) {
        lorder = lmeta & 0xFF;
        int32_t hp[MAXO];
#pragma unroll
        for (int k = 0; k < MAXO; k++) hp[k] = lane_prev(x[SPL - MAXO + k]);
        // ResidualOverflow: not tested up front (the wave-uniform bound sum|c| * 2^(bps-1) >> shift that used to clear
        // most candidates fails for the large coefficients of high-order resonant predictors, and the exact test costs
        // a second pass over MAXO taps): wave_rice_stored's fold below tells whether it was possible at all, and only
        // a re-run asked for by the host (p.check_fir, types.h) pays for the exact test
        const bool check = p.check_fir != 0;   // wave-uniform
        bool ovf = false;
        if (check) ovf = fir64_overflows<SPL, MAXO>(x, hp, lpw, lorder, lshift);
        if (__any(ovf)) {
            if (lane == 0) atomicAdd(&p.stats[0], 1u);
        } else {
            // taps rounded up to a multiple of 2 (coefficients beyond the order are zero); one region, whatever the order
            fir64_dyn<SPL, MAXO, 2, FIR_TURN(SPL)>(x, hp, lpw, lorder, lshift);
            CAND_STAMP(5);   // FIR done
            CAND_PRIO_CHECK();
            lw = wave_rice_stored<SPL, MAXO, HAND>(x, lorder, p, !check);
            lpc_ok = lw.ok;
            if (!lpc_ok && lane == 0) atomicAdd(&p.stats[0], 1u);
            lpc_bits = 8u + wasted + lorder * bps_eff + 4u + 5u + lorder * lprec + lw.bits;
        }
    }
