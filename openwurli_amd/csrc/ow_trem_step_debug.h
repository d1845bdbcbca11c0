// openwurli-hip: ONE step of the Twin-T tremolo oscillator on independent cases, through each of its three device forms (debug hook
// ow_debug_trem_step, include/openwurli_hip_test.h).  The step exists as trem_osc_step (ow_chain_dev.h: lane = engine, state parked in
// LDS), trem_osc_step_wide (ow_trem_wide.h: four lanes per system) and trem_osc_step_row (ow_trem_row.h: sixteen lanes per system, with
// its own generic-sweep and backward-Euler wrappers); the tremolo kernels only ever take them through the settled oscillation, where
// Newton converges in a few unlimited sweeps.  This kernel hands any state to the production functions themselves -- loaded and stored
// by the kernels' own trem_load / trem_wide_load / trem_row_load and their stores, matrices staged as k_tremolo / k_tremolo_wide stage
// them -- so that the junction limiter, the 3.5 V cap, other pivots, a singular Jacobian, fifty sweeps, the backward-Euler retry and the
// NaN reset can be compared one step at a time (tests/test_gpu_trem_step.py).  No copy of the step lives here.
//
// cs_in / cs_out are the eighteen tremolo state rows in the chain kernels' own layout: [18][n] (field-major, case c in column c) for the
// lane and quad forms, [n][18] (the I = 1 layout of the trajectory kernels, one block of rows per case) for the row form.  The cell (env,
// r_ldr) is carried but not stepped.  Lanes without a case leave as k_tremolo's do (lane form); quads without a case run the last case
// and store nothing, as k_tremolo_wide's do.
#pragma once
#include "ow_trem_row.h"

namespace owdev {

enum { TSF_LANE = 0, TSF_WIDE = 1, TSF_ROW = 2 };

template <int FORM>
__global__ __launch_bounds__(64) void k_debug_trem_step(const OwConsts* __restrict__ K, const double* __restrict__ cs_in, int n, double* __restrict__ cs_out,
                                                        double* __restrict__ out, unsigned long long* __restrict__ info) {
    const int lane = threadIdx.x;
    if constexpr (FORM == TSF_LANE) {
        // k_tremolo: one system per lane, matrices and state in LDS
        __shared__ TremMats M;
        __shared__ TremPark P;
        trem_mats_load(&M, K, lane, 64);
        __syncthreads();
        const long long t = (long long)blockIdx.x * 64 + lane;
        if (t >= n) return;
        const int c = (int)t;
        TremState st;
        trem_load(st, &P, cs_in, n, c);
        int z = 0;
        asm volatile("" : "+v"(z));
        const double o = trem_osc_step(st, &P, K, &M + z);
        trem_store(st, &P, cs_out, n, c);          // (cs_out arrives zeroed: its CS_T_BE row ends as this step's increment)
        out[c] = o;
        info[c] = (unsigned long long)st.be_fallbacks;
    } else if constexpr (FORM == TSF_WIDE) {
        // k_tremolo_wide: four lanes per system
        __shared__ TremMats M;
        trem_mats_load(&M, K, lane, 64);
        __syncthreads();
        const long long cw = (long long)blockIdx.x * 16 + (lane >> 2);
        const bool valid = cw < n;
        const int c = valid ? (int)cw : n - 1;
        TremWide st;
        trem_wide_load(st, cs_in, n, c);
        const double o = trem_osc_step_wide(st, K, &M);
        if (valid && (lane & 3) == 0) {
            trem_wide_store(st, cs_out, n, c);
            out[c] = o;
            info[c] = (unsigned long long)st.be_fallbacks;
        }
    } else {
        // k_trem_settle_row / k_trem_traj_extend_row: one system per wavefront
        const int c = (int)blockIdx.x;             // (the grid is n blocks)
        TremRowK rk;
        trem_row_consts(rk, K, lane);
        TremRow st;
        trem_row_load(st, cs_in + (size_t)18 * c, lane);
        const double o = trem_osc_step_row(st, rk, K, lane);
        double* dst = cs_out + (size_t)18 * c;
        trem_row_store_circuit(st, dst + CS_T_V, dst + CS_T_I, dst + CS_T_IP, lane);
        if (lane == 0) {
            dst[CS_T_ENV] = st.env; dst[CS_T_RLDR] = cs_in[(size_t)18 * c + CS_T_RLDR];
            out[c] = o;
            info[c] = (unsigned long long)st.be_fallbacks;
        }
    }
}

}  // namespace owdev
