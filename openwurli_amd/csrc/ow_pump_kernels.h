// openwurli-hip: the pump measurements (`preamp-bench pump-sweep` / `pump-trace` / `pump-spike` / `pump-step` / `pump-sinusoid`,
// tools/preamp-bench/src/main.rs:2329-3063) -- ONE gen_preamp::CircuitState per point, driven directly: CircuitState::default() (DC_OP,
// DC_NL_I, the tables of the rate), set_runtime_R_r_ldr, `settle` samples, optionally one more zero-input sample, then `capture` samples
// under a resistance schedule, reduced in the lane.  No adapter, no settled state, no shadow partner, no thermal noise.
//
// Mapping: lane = point, 32 points per wavefront, one launch per sample rate (the rate's matrices are pool constants, as in every melange
// kernel).  The step is mel_process_lit's body (ow_melange_lit.h, entered through mel_process_lit_diag for the two counters MelSt lacks) on
// the point's own S in LDS -- the literal rebuild, the form tests/test_gpu_mel_step.py pins -- and the rebuild is that file's too:
// mel_lit_rebuild_fast / mel_lit_rebuild build one S by a PAIR of lanes, so lane l + 32 of the wavefront is point l's helper for the
// rebuild and idles through the step.  Nothing is lost by that: the commands bring 1 to 832 points, a handful of wavefronts on 256 CUs,
// and every one of them is a serial recurrence of 10^5..10^6 samples.  The kernel is bound by the latency of that recurrence (one
// wavefront per SIMD, dependent f64 operations), not by any throughput.
//
// The reference's lazy rebuild (matrices_dirty, gen_preamp.rs:1973-1984, 3408-3411) is kept: a state runs on the tables it was created
// with (OwConsts::m_s0 / m_k0: the codegen tables within 0.5 Hz of 48 kHz, set_sample_rate's rebuild at the nominal pot elsewhere; S N_i
// is formed from S where it is used, which gives the tables' own S_NI bit for bit -- the host entry point checks that) until a
// set_runtime_R_r_ldr moved the resistance, and is rebuilt at the next processed sample.  A static point therefore rebuilds once, a
// moving one per sample.  The rebuild contains workgroup barriers, so the whole wavefront takes part whenever one of its points is dirty;
// a point that is not gets the matrices of the resistance it was last built for again (they are a pure function of rate and resistance),
// and one that never was built gets its tables back.  The NaN reset puts the pot back to nominal WITHOUT marking the matrices dirty
// (:3616-3636): the resistance the matrices were built for is kept apart from the state's.
//
// Statistics accumulate serially, in the reference's order of operations (pump-sweep :2397-2411, pump-spike's measure :2601-2614, the
// sample-to-sample step of the slew and of pump-sinusoid :2777-2790, 3002-3011); the finishing divisions and roots are the host's.
// Host code sorts a launch's points by resistance: at 1 k..5 kOhm every sample exhausts the trapezoidal solve (265 sweeps) and takes the fallback --
// a hundred times the work of a tame sample -- and those lanes should share wavefronts.  The trace goes out sample-major ([capture][points]: the lanes of a wavefront store neighbouring doubles) and
// k_pump_trace_rows turns it into the caller's rows.
#pragma once
#include "ow_melange_lit.h"

namespace owdev {

enum { PUMP_STATIC = 0, PUMP_STEP = 1, PUMP_TABLE = 2 };   // TABLE: the host tabulated the linear ramp / the log-cosine (its own libm, as the reference's)
struct OwPumpDev {
    double r_settle, r_to, amp, w;       // w = 2 pi f / sr: the input is amp * sin(w * k), k counted from the first settle sample
    long long settle, capture;
    long long sched_off;                 // PUMP_TABLE: where this point's [capture] resistances start in r_sched
    int kind, extra;
};
enum { PM_SUM = 0, PM_SUM_SQ, PM_MIN, PM_MAX, PM_PSUM, PM_PSUM_SQ, PM_RAW_SUM, PM_RAW_SUM_SQ, PM_EXTRA, PM_MAX_STEP, PM_NR, PM_BE, PM_DAMP, PM_NAN, PM_COUNT };

// met: [n][PM_COUNT]; trace: nullptr or [max capture][trace_ld >= n]; lu_scratch: one [12][12][32] slab per workgroup (generic rebuild only)
__global__ __launch_bounds__(64) void k_pump_points(const OwConsts* __restrict__ K, const OwPumpDev* __restrict__ pts, int n, const double* __restrict__ r_sched,
                                                    double* __restrict__ met, double* __restrict__ trace, long long trace_ld, int generic_only,
                                                    double* __restrict__ lu_scratch) {
    __shared__ double S_all[12 * 12 * 32];
    const int lane = threadIdx.x;
    const int el = lane & 31, role = lane >> 5;
    const long long pi = (long long)blockIdx.x * 32 + el;
    const bool mine = pi < n && role == 0;
    const OwPumpDev p = pts[pi < n ? pi : n - 1];
    double* S = S_all + el;
    double* lu = lu_scratch + (size_t)blockIdx.x * (12 * 12 * 32) + el;
    const double alpha = 2.0 * (K->os_sr * 1.0);                    // gen_preamp.rs:1991-1992
    const double pot_nominal = 9.99999999999999854e4;

    MelSt st;                                                       // CircuitState::default() (:1748-1821)
    for (int i = 0; i < 12; ++i) st.v[i] = PRE_DC_OP[i];
    for (int i = 0; i < 3; ++i) { st.ip[i] = PRE_DC_NL_I[i]; st.ipp[i] = PRE_DC_NL_I[i]; }
    st.input_prev = 0.0; st.pot = pot_nominal; st.be_cooldown = 0u; st.nan_resets = 0u; st.be_fallbacks = 0u;
    MelDiag dg = {0u, 0u};
    // the tables the state was created with; built: a rebuild of this point's own has replaced them, for the resistance s_pot
    double kk[3][3], an66 = K->m_aneg0[6][6], s_pot = pot_nominal;
    bool built = false;
    if (role == 0)
        for (int i = 0; i < 12; ++i) for (int j = 0; j < 12; ++j) MS(i, j) = K->m_s0[i][j];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) kk[i][j] = K->m_k0[i][j];
    bool dirty = false;
    if (mine) { const double before = st.pot; mel_set_r(st, p.r_settle); dirty = st.pot != before; }

    const long long total = mine ? p.settle + (long long)p.extra + p.capture : 0;
    long long tmax = total;
    for (int off = 32; off > 0; off >>= 1) { const long long o = __shfl_xor(tmax, off); tmax = o > tmax ? o : tmax; }

    double sum = 0.0, sum_sq = 0.0, vmin = INFINITY, vmax = -INFINITY;
    double psum = 0.0, psum_sq = 0.0, raw_sum = 0.0, raw_sum_sq = 0.0, y0 = 0.0;
    double extra = 0.0, prev = 0.0, max_step = 0.0;
    bool have_prev = false;
    for (long long t = 0; t < tmax; ++t) {
        const bool act = t < total;
        const long long j = t - p.settle - (long long)p.extra;      // index into the capture once it is >= 0
        const bool cap = act && j >= 0;
        const bool is_extra = act && p.extra != 0 && t == p.settle;
        double x = 0.0;
        if (cap && p.kind != PUMP_STATIC) {
            const double before = st.pot;
            if (p.kind == PUMP_TABLE) mel_set_r(st, r_sched[p.sched_off + j]);
            else if (j == 0) mel_set_r(st, p.r_to);
            if (st.pot != before) dirty = true;
        }
        if (act && !is_extra && p.amp != 0.0) x = p.amp * sin(p.w * (double)(cap ? p.settle + j : t));
        // lazy rebuild (:3408-3411) by the lane pair; see the head of the file for who takes part with what
        const bool need = act && dirty;
        if (__any(need)) {
            const double pot_b = __shfl(need ? st.pot : s_pot, el);
            bool fast = K->ml_ok != 0 && generic_only == 0;
            if (fast) {
                __syncthreads();                                          // the previous sample's reads of S are done
                fast = mel_lit_rebuild_fast(K, pot_b, role, alpha, S);
                __syncthreads();                                          // both lanes' columns are in place
                if (fast) mel_lit_kernel(S, kk);
            }
            if (!fast) mel_lit_rebuild(pot_b, role, alpha, lu, S, kk);
            if (need) { built = true; dirty = false; }
            if (built) {
                s_pot = pot_b;
                const double g66 = PRE_G[6][6] + (ow_div(1.0, pot_b) - PRE_POT_0_G_NOM);
                an66 = alpha * PRE_C[6][6] - g66;
            } else {
                if (role == 0)
                    for (int i = 0; i < 12; ++i) for (int j2 = 0; j2 < 12; ++j2) MS(i, j2) = K->m_s0[i][j2];
                for (int i = 0; i < 3; ++i) for (int j2 = 0; j2 < 3; ++j2) kk[i][j2] = K->m_k0[i][j2];
            }
        }
        if (act) {
            const double y = mel_process_lit_diag(st, x, K->m_aneg0, an66, S, kk, nullptr, 0, dg);
            if (is_extra) extra = y;
            if (cap) {
                sum += y;
                sum_sq += y * y;
                if (y < vmin) vmin = y;
                if (y > vmax) vmax = y;
                if ((j & 1) == 0) {
                    y0 = y;
                } else {
                    const double pm = 0.5 * (y0 + y);
                    psum += pm;
                    psum_sq += pm * pm;
                    raw_sum += y0 + y;
                    raw_sum_sq += y0 * y0 + y * y;
                }
                if (have_prev) { const double step = fabs(y - prev); if (step > max_step) max_step = step; }
                if (trace) trace[(size_t)j * (size_t)trace_ld + (size_t)pi] = y;
            }
            if (cap || is_extra) { prev = y; have_prev = true; }
        }
    }
    if (mine) {
        double* m = met + (size_t)pi * PM_COUNT;
        m[PM_SUM] = sum; m[PM_SUM_SQ] = sum_sq; m[PM_MIN] = vmin; m[PM_MAX] = vmax;
        m[PM_PSUM] = psum; m[PM_PSUM_SQ] = psum_sq; m[PM_RAW_SUM] = raw_sum; m[PM_RAW_SUM_SQ] = raw_sum_sq;
        m[PM_EXTRA] = extra; m[PM_MAX_STEP] = max_step;
        m[PM_NR] = (double)dg.nr_exhausted; m[PM_BE] = (double)st.be_fallbacks; m[PM_DAMP] = (double)dg.voltage_damps; m[PM_NAN] = (double)st.nan_resets;
    }
}

// trace [cap][ld] (sample-major) -> rows [n][stride], samples k < cap of every point; 32 x 32 tiles through LDS so that both sides move
// whole lines.  Block (32, 8), grid (ceil(cap / 32), ceil(n / 32)): the long dimension is x.
__global__ __launch_bounds__(256) void k_pump_trace_rows(const double* __restrict__ trace, long long ld, int n, long long cap, double* __restrict__ rows,
                                                         long long stride) {
    __shared__ double tile[32][33];
    const long long p0 = (long long)blockIdx.y * 32, k0 = (long long)blockIdx.x * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const long long k = k0 + r, q = p0 + threadIdx.x;
        tile[r][threadIdx.x] = (k < cap && q < n) ? trace[(size_t)k * (size_t)ld + (size_t)q] : 0.0;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const long long q = p0 + r, k = k0 + threadIdx.x;
        if (q < n && k < cap) rows[(size_t)q * (size_t)stride + (size_t)k] = tile[threadIdx.x][r];
    }
}

}  // namespace owdev
