// openwurli-hip: ONE step of the legacy DK preamp on independent cases, through each of its four device forms (debug hook
// ow_debug_dk_step, include/openwurli_hip_test.h).  The step exists as dk_step, dk_step_pair (ow_chain_dev.h), dk_step_wide
// (ow_chain_wide.h) and dk_step_row (ow_chain_row.h); the chain kernels only ever take them through musical play, where Newton converges
// in two or three updates.  This kernel hands any state to the production functions themselves -- state prepared as the chain kernels do
// at block start (dk_load: the fourteen rows, then dk_refresh_gm), stored with dk_store -- so that the rare exits (no update, six updates,
// the junction clamp, a singular 2x2) can be compared one step at a time (tests/test_gpu_dk_step.py).  No copy of the step lives here.
//
// cs_in / cs_out are state rows in the chain kernels' own layout, [14][n] (field-major), case c in column c.  A wavefront whose last
// lanes, quad or row have no case runs them on the last case (the wave-uniform Newton loop and the cross-lane moves want every lane
// active, as in the chain kernels' ragged last wavefront) and stores nothing for them.
#pragma once
#include "ow_chain_row.h"

namespace owdev {

enum { DKF_LANE = 0, DKF_PAIR = 1, DKF_WIDE = 2, DKF_ROW = 3 };

template <int FORM>
__global__ __launch_bounds__(64) void k_debug_dk_step(const OwConsts* __restrict__ K, const double* __restrict__ cs_in, const double* __restrict__ input,
                                                      const double* __restrict__ g_ldr, const double* __restrict__ g_ldr_prev, int n,
                                                      double* __restrict__ cs_out, double* __restrict__ out) {
    const int lane = threadIdx.x;
    const long long t = (long long)blockIdx.x * 64 + lane;
    if constexpr (FORM == DKF_LANE) {
        // k_preamp: one solver state per lane
        const bool valid = t < n;
        const int c = valid ? (int)t : n - 1;
        DkSt st;
        dk_load(st, cs_in, n, c, 0);
        const double o = dk_step(st, input[c], g_ldr[c], g_ldr_prev[c], K);
        if (valid) { dk_store(st, cs_out, n, c, 0); out[c] = o; }
    } else if constexpr (FORM == DKF_PAIR) {
        // k_preamp_pair: lane = engine, case 2k its main and case 2k + 1 its shadow state; g_ldr / g_ldr_prev are the engine's (case 2k's)
        const long long ca = 2 * t, cb = 2 * t + 1;
        const bool va = ca < n, vb = cb < n;
        const int a = va ? (int)ca : n - 1, b = vb ? (int)cb : n - 1;
        DkSt sm, ss;
        dk_load(sm, cs_in, n, a, 0);
        dk_load(ss, cs_in, n, b, 0);
        DkPairRes R;
        dk_pair_res_load(R, K);
        double om, os;
        dk_step_pair(sm, ss, input[a], input[b], g_ldr[a], g_ldr_prev[a], K, R, om, os);
        if (va) { dk_store(sm, cs_out, n, a, 0); out[a] = om; }
        if (vb) { dk_store(ss, cs_out, n, b, 0); out[b] = os; }
    } else if constexpr (FORM == DKF_WIDE) {
        // k_preamp_wide: four lanes per solver state; the lane of the quad that stores rotates with the case (the state is replicated)
        const int q = lane & 3;
        const long long cw = t >> 2;
        const bool valid = cw < n;
        const int c = valid ? (int)cw : n - 1;
        DkWideRows R;
        dk_wide_rows_load(R, K, q);
        DkSt st;
        dk_load(st, cs_in, n, c, 0);
        const double o = dk_step_wide(st, R, q, input[c], g_ldr[c], g_ldr_prev[c], K);
        if (valid && q == (c & 3)) { dk_store(st, cs_out, n, c, 0); out[c] = o; }
    } else {
        // k_chain_row: sixteen lanes per solver state; the lane of the row that stores rotates with the case
        const long long cr = t >> 4;
        const bool valid = cr < n;
        const int c = valid ? (int)cr : n - 1;
        DkRowK R;
        dk_row_consts(R, K, lane);
        DkSt st;
        dk_load(st, cs_in, n, c, 0);
        const double o = dk_step_row(st, R, lane, input[c], g_ldr[c], g_ldr_prev[c]);
        if (valid && (lane & 15) == (c & 15)) { dk_store(st, cs_out, n, c, 0); out[c] = o; }
    }
}

}  // namespace owdev
