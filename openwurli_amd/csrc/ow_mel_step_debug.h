// openwurli-hip: ONE step of the melange 12-node preamp solver on independent cases, through each device form of it (debug hook
// ow_debug_mel_step, include/openwurli_hip_test.h).  set_runtime_R; process_sample exists as mel_process (ow_melange_dev.h: rank-one
// update of the nominal inverse), mel_process_lit (ow_melange_lit.h: the engine's S in LDS, fast leading block or generic rebuild),
// mel_process_col (ow_melange_col.h: column-streamed, fast or generic) and mel_eng_sample (ow_melange_eng.h: both solver states of an
// engine in one lane); the preamp kernels only ever take them through musical signals, where Newton converges in a few sweeps.  This
// kernel hands any state to the production functions themselves, staged as the kernels stage them, so that the input clamp,
// set_runtime_R's exits, the limiter and the 0.1 A cap, 265 sweeps, the ringing test, the backward-Euler fallback, its cooldown, the
// voltage-damp net and the NaN reset can be compared one step at a time (tests/test_gpu_mel_step.py).  No copy of the step lives here.
//
// states / states_out: [n][21] = v[12], ip[3], ipp[3], input_prev, pot, be_cooldown (as a double); x, r: [n]; out: [n] = the step's
// return value; info: [n][2] = the step's increments of be_fallbacks and nan_resets.  The pair forms take case 2k as an engine's main
// state and case 2k+1 as its shadow (lit / col: lanes l and l + 32 of a 32-engine wavefront; eng: one lane) and build the matrices
// for the main's pot, as production does; the eng form gives the shadow the main's resistance and input 0, as k_preamp_mel_eng does.
// Lanes without a case run the last case and store nothing.
#pragma once
#include "ow_melange_eng.h"

namespace owdev {

enum { MSF_RANK1 = 0, MSF_LIT_FAST = 1, MSF_LIT_GENERIC = 2, MSF_COL_FAST = 3, MSF_COL_GENERIC = 4, MSF_ENG_FAST = 5, MSF_ENG_GENERIC = 6 };

__device__ inline void mel_dbg_load(MelSt& s, const double* __restrict__ row) {
    for (int i = 0; i < 12; ++i) s.v[i] = row[i];
    for (int i = 0; i < 3; ++i) { s.ip[i] = row[12 + i]; s.ipp[i] = row[15 + i]; }
    s.input_prev = row[18]; s.pot = row[19];
    s.be_cooldown = (uint32_t)row[20];
    s.nan_resets = 0; s.be_fallbacks = 0;
}
__device__ inline void mel_dbg_store(const MelSt& s, double o, int c, double* __restrict__ states_out, double* __restrict__ out, unsigned* __restrict__ info) {
    double* row = states_out + (size_t)21 * c;
    for (int i = 0; i < 12; ++i) row[i] = s.v[i];
    for (int i = 0; i < 3; ++i) { row[12 + i] = s.ip[i]; row[15 + i] = s.ipp[i]; }
    row[18] = s.input_prev; row[19] = s.pot; row[20] = (double)s.be_cooldown;
    out[c] = o;
    info[2 * c] = s.be_fallbacks; info[2 * c + 1] = s.nan_resets;
}

// lu_scratch: the generic rebuilds' workspace, sized and indexed as host_pool.inc sizes d_mel_lu for the kernel of the form (lit: one
// [12][12][32] slab per workgroup; col / eng: [144][lu_ld] lane-minor, lu_ld = 2 * (pairs + 32), spare columns for lanes without a pair).
template <int FORM>
__global__ __launch_bounds__(64) void k_debug_mel_step(const OwConsts* __restrict__ K, const double* __restrict__ states, const double* __restrict__ x,
                                                       const double* __restrict__ r, int n, double* __restrict__ states_out, double* __restrict__ out,
                                                       unsigned* __restrict__ info, double* __restrict__ lu_scratch, size_t lu_ld) {
    const int lane = threadIdx.x;
    const double alpha = 2.0 * (K->os_sr * 1.0);                    // gen_preamp.rs:1991-1992
    const int pairs = (n + 1) / 2;
    if constexpr (FORM == MSF_RANK1) {
        // k_preamp_mel / k_mel_settle: one state per lane, MelMats in LDS
        __shared__ MelMats M;
        mel_mats_load(&M, K, lane, 64);
        __syncthreads();
        const long long t = (long long)blockIdx.x * 64 + lane;
        const bool valid = t < n;
        const int c = valid ? (int)t : n - 1;
        MelSt st;
        mel_dbg_load(st, states + (size_t)21 * c);
        mel_set_r(st, r[c]);
        int z = 0;
        asm volatile("" : "+v"(z));
        const double o = mel_process(st, x[c], &M + z);
        if (valid) mel_dbg_store(st, o, c, states_out, out, info);
    } else if constexpr (FORM == MSF_LIT_FAST || FORM == MSF_LIT_GENERIC) {
        // k_preamp_mel_lit: lane = (engine, main | shadow), S of the wavefront's 32 engines in LDS, one rebuild per engine by its two lanes.
        // The rebuilds contain workgroup barriers: every lane runs to the end.
        __shared__ double S_all[12 * 12 * 32];
        const int el = lane & 31, role = lane >> 5;
        const long long cw = 2 * ((long long)blockIdx.x * 32 + el) + role;
        const bool valid = cw < n;
        const int c = valid ? (int)cw : n - 1;
        double* lu = lu_scratch + (size_t)blockIdx.x * (12 * 12 * 32) + el;
        double* S = S_all + el;
        MelSt st;
        mel_dbg_load(st, states + (size_t)21 * c);
        mel_set_r(st, r[c]);
        const double pot_main = __shfl(st.pot, el);
        double kk[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        bool fast = FORM == MSF_LIT_FAST && K->ml_ok != 0;
        if (fast) {
            __syncthreads();
            fast = mel_lit_rebuild_fast(K, pot_main, role, alpha, S);
            __syncthreads();
            if (fast) mel_lit_kernel(S, kk);
        }
        if (!fast) mel_lit_rebuild(pot_main, role, alpha, lu, S, kk);
        const double g66 = PRE_G[6][6] + (ow_div(1.0, pot_main) - PRE_POT_0_G_NOM);
        const double an66 = alpha * PRE_C[6][6] - g66;
        const double o = mel_process_lit(st, x[c], K->m_aneg0, an66, S, kk, nullptr, 0);
        if (valid) mel_dbg_store(st, o, c, states_out, out, info);
    } else if constexpr (FORM == MSF_COL_FAST || FORM == MSF_COL_GENERIC) {
        // k_preamp_mel_col: lane = (engine, main | shadow), each lane rebuilds for itself; 36 running S N_i sums per lane in LDS
        __shared__ double sni_all[36 * 64];
        const int el = lane & 31, role = lane >> 5;
        const long long e = (long long)blockIdx.x * 32 + el;
        const bool pvalid = e < pairs;
        const long long cw = 2 * e + role;
        const bool valid = cw < n;
        const int c = valid ? (int)cw : n - 1;
        double* lu = lu_scratch + (size_t)2 * (pvalid ? (size_t)e : (size_t)pairs + el) + role;
        MelSt st;
        mel_dbg_load(st, states + (size_t)21 * c);
        mel_set_r(st, r[c]);
        const double pot_main = __shfl(st.pot, el);
        const double o = mel_process_col(st, x[c], pot_main, alpha, K, sni_all + lane, FORM == MSF_COL_GENERIC, lu, lu_ld, nullptr, 0);
        if (valid) mel_dbg_store(st, o, c, states_out, out, info);
    } else {
        // k_preamp_mel_eng: lane = engine, both solver states in the lane, one rebuild for the two
        __shared__ double sni_all[36 * 64];
        const long long e = (long long)blockIdx.x * 64 + lane;
        const bool pvalid = e < pairs;
        const int ec = pvalid ? (int)e : pairs - 1;
        const int c0 = 2 * ec;
        const bool has1 = 2 * ec + 1 < n;
        const int c1 = has1 ? 2 * ec + 1 : n - 1;
        double* lu = lu_scratch + (size_t)2 * (pvalid ? (size_t)e : (size_t)pairs + (lane & 31));
        MelSt st[2];
        mel_dbg_load(st[0], states + (size_t)21 * c0);
        mel_dbg_load(st[1], states + (size_t)21 * c1);
        mel_set_r(st[0], r[c0]);
        mel_set_r(st[1], r[c0]);
        const double pot = st[0].pot;
        double o[2];
        mel_eng_sample(st, x[c0], pot, alpha, K, sni_all + lane, FORM == MSF_ENG_GENERIC, lu, lu_ld, nullptr, 0, o);
        if (pvalid) {
            mel_dbg_store(st[0], o[0], c0, states_out, out, info);
            if (has1) mel_dbg_store(st[1], o[1], c1, states_out, out, info);
        }
    }
}

}  // namespace owdev
