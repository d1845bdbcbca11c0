// openwurli-hip: melange 12-node DK preamp (cargo feature `melange-preamp` of the reference), device code.
//
//   lane = (engine, main|shadow) as in k_preamp.
//
// The reference re-inverts the 12x12 system matrix (LU, partial pivoting) on every sample whose R_ldr moved
// (gen_preamp.rs:1990-2062, 3408-3411) -- i.e. on every 96 kHz sample while the tremolo runs, in both states.  R_ldr
// enters the MNA matrix in exactly one entry, A[6][6] += 1/R - 1/R_nom, so the inverse is a rank-one update of the
// inverse at the nominal 100 kOhm (Sherman-Morrison):
//     S(R) = S0 - c u w^T,   c = dg / (1 + dg S0[6][6]),  u = S0[:,6],  w = S0[6,:],  dg = 1/R - 1/R_nom
// and S(R) rhs, K(R) = N_v S(R) N_i, S(R) N_i i_nl follow from pool-uniform constants (S0, u, w, w N_i, N_v u) without
// ever forming a per-engine matrix.  This is the same construction the reference's own legacy solver uses for R_ldr
// (dk_preamp_legacy.rs:196-214).  It is mathematically identical to the reference's per-sample LU and differs from it
// by f64 rounding of a different (shorter) operation sequence; the measured deviation from the literal-LU oracle is in
// DESIGN.md section 2.  S0 itself is the reference's LU inverse at (chain rate, 100 kOhm), built on the host.
// The BE-fallback matrices are never rebuilt by the reference (gen_preamp.rs:2058-2061): codegen tables.
//
// Mirrors gen_preamp.rs:1973-1984 (set_runtime_R), :3041-3095 (build_rhs), :3122-3357 (solve_nonlinear),
// :3399-3663 (process_sample), dk_preamp/melange_adapter.rs:12-94; thermal noise :1434-1561, 3433-3461, 3522-3535.
#pragma once
#include "ow_kernels.h"

namespace owdev {

struct MelSt {
    double v[12], ip[3], ipp[3], input_prev, pot;
    uint32_t be_cooldown;
    uint32_t nan_resets, be_fallbacks;
};

// pool-uniform trapezoidal constants at the chain rate and the nominal pot, staged in LDS
struct MelMats {
    double s0[12][12], aneg0[12][12], k0[3][3], sni0[12][3];
    double u[12], w[12], wn[3], nvu[3], s66, g_nom;
};
OW_DEV void mel_mats_load(MelMats* __restrict__ m, const OwConsts* __restrict__ K, int tid, int nthreads) {
    double* dst = (double*)m;
    const double* src = &K->m_s0[0][0];
    for (int i = tid; i < (int)(sizeof(MelMats) / sizeof(double)); i += nthreads) dst[i] = src[i];
}

// solve_nonlinear (gen_preamp.rs:3122-3357) with the 3x3 kernel in registers; returns last_nr_iterations (265 = failed)
#ifdef OW_DBG_COUNTERS
__device__ unsigned long long g_ow_dbg[8];
#endif
__device__ inline uint32_t mel_solve_nl(const double p[3], const double kk[3][3], const double ip[3], const double ipp[3], double i_nl[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) i_nl[i] = 2.0 * ip[i] - ipp[i];
#ifndef OW_MEL_MAXIT
#define OW_MEL_MAXIT 265
#endif
    for (int iter = 0; iter < OW_MEL_MAXIT; ++iter) {
#ifdef OW_DBG_COUNTERS
        {   // [0] sweep bodies summed over lanes, [1] sweep bodies as the wavefront executes them
            const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
            atomicAdd(&g_ow_dbg[0], 1ull);
            if ((int)(threadIdx.x & 63) == __builtin_ctzll(act)) atomicAdd(&g_ow_dbg[1], 1ull);
        }
#endif
        double vd[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) vd[q] = p[q] + kk[q][0] * i_nl[0] + kk[q][1] * i_nl[1] + kk[q][2] * i_nl[2];
        const double nvt0 = PRE_DEVICE_0_N_VT;
        const double vcl = clampd(vd[0], -40.0 * nvt0, 40.0 * nvt0);
        double idev[3], jdev[3];
        idev[0] = PRE_DEVICE_0_IS * (fast_exp(OW_DIV_C(vcl, PRE_DEVICE_0_N_VT)) - 1.0);
        jdev[0] = (PRE_DEVICE_0_IS / nvt0) * fast_exp(OW_DIV_C(vcl, PRE_DEVICE_0_N_VT));
        const double e1 = fast_exp(OW_DIV_C(vd[1] * 1.0, PRE_DEVICE_1_NF * PRE_DEVICE_1_VT));
        idev[1] = PRE_DEVICE_1_IS * (e1 - 1.0) * 1.0;
        jdev[1] = PRE_DEVICE_1_IS / (PRE_DEVICE_1_NF * PRE_DEVICE_1_VT) * e1;
        const double e2 = fast_exp(OW_DIV_C(vd[2] * 1.0, PRE_DEVICE_2_NF * PRE_DEVICE_2_VT));
        idev[2] = PRE_DEVICE_2_IS * (e2 - 1.0) * 1.0;
        jdev[2] = PRE_DEVICE_2_IS / (PRE_DEVICE_2_NF * PRE_DEVICE_2_VT) * e2;
        const double f[3] = {i_nl[0] - idev[0], i_nl[1] - idev[1], i_nl[2] - idev[2]};
        double a[3][3], b[3] = {f[0], f[1], f[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) a[i][j] = (i == j ? 1.0 : 0.0) - jdev[i] * kk[i][j];
        bool singular = false;
        double yp[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int col = 0; col < 3; ++col) {
            int max_row = col;
            double max_val = fabs(a[col][col]);
#pragma unroll
            for (int row = col + 1; row < 3; ++row) {
                const double v = fabs(a[row][col]);
                if (v > max_val) { max_val = v; max_row = row; }
            }
            if (!singular && max_val < 1e-15) singular = true;
            if (!singular) {
                // row exchange only when some lane of the wavefront picked an off-diagonal pivot (wave-uniform branch): the selects are
                // no-ops for every other lane
                if (__builtin_amdgcn_ballot_w64(max_row != col) != 0ull) {
#pragma unroll
                for (int row = col + 1; row < 3; ++row) {
                    const bool sw = (max_row == row);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const double x = a[col][j], y = a[row][j];
                        a[col][j] = sw ? y : x;
                        a[row][j] = sw ? x : y;
                    }
                    const double x = b[col], y = b[row];
                    b[col] = sw ? y : x;
                    b[row] = sw ? x : y;
                }
                }
                const double pivot = a[col][col];
                yp[col] = ow_rcp_refined(pivot);       // every quotient over this pivot (elimination factors, back substitution) shares it
#pragma unroll
                for (int row = col + 1; row < 3; ++row) {
                    const double factor = ow_div_y(a[row][col], pivot, yp[col]);
#pragma unroll
                    for (int j = col + 1; j < 3; ++j) a[row][j] -= factor * a[col][j];
                    b[row] -= factor * b[col];
                }
            }
        }
        if (!singular) {
#pragma unroll
            for (int i = 2; i >= 0; --i) {
                double sum = b[i];
#pragma unroll
                for (int j = i + 1; j < 3; ++j) sum -= a[i][j] * b[j];
                b[i] = ow_div_y(sum, a[i][i], yp[i]);      // (the reference's second |a[i][i]| < 1e-15 test cannot fire: a[i][i] is column i's pivot)
            }
        }
        if (!singular) {
            double dv[3], al[3] = {1.0, 1.0, 1.0};
#pragma unroll
            for (int q = 0; q < 3; ++q) dv[q] = -(kk[q][0] * b[0] + kk[q][1] * b[1] + kk[q][2] * b[2]);
            const double vts[3] = {PRE_DEVICE_0_N_VT, PRE_DEVICE_1_VT, PRE_DEVICE_2_VT};
            const double vcr[3] = {PRE_DEVICE_0_VCRIT, PRE_DEVICE_1_VCRIT, PRE_DEVICE_2_VCRIT};
            bool any_limited = false;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (fabs(dv[q]) > 1e-4) {
                    const double v_lim = pnjlim(vd[q] + dv[q], vd[q], vts[q], vcr[q]);
                    const double ratio = fmax(ow_div(v_lim - vd[q], dv[q]), 0.01);
                    if (ratio < al[q]) { al[q] = ratio; if (ratio < 1.0) any_limited = true; }
                }
            }
            double as = fmin(al[0], fmin(al[1], al[2]));
            if (as < 1.0) any_limited = true;
            const double max_di = fmax(fmax(fabs(b[0]), fabs(b[1])), fabs(b[2]));
            if (max_di * as > 0.1) as = fmin(fmax(ow_div(0.1, max_di), 0.01), as);
#pragma unroll
            for (int q = 0; q < 3; ++q) i_nl[q] -= as * b[q];
            bool conv = true;
            if (!any_limited) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double step = dv[q] * as;
                    const double thr = 1e-3 * fmax(fabs(vd[q]), fabs(vd[q] + step)) + 1e-6;
                    if (fabs(step) > thr) conv = false;
                }
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double i_thr = 1e-3 * fmax(fmax(fabs(i_nl[q]), fabs(idev[q])), 1e-9) + 1e-12;
                if (fabs(f[q]) > i_thr) conv = false;
            }
            if (conv) return (uint32_t)iter;
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double cl = fmax(fabs(i_nl[q]) * 0.1, 0.01);
                i_nl[q] -= clampd(f[q] * 0.5, -cl, cl);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (!isfinite(i_nl[q])) i_nl[q] = ip[q];
    return 265u;
}


// ---- thermal noise of the main state (gen_preamp.rs:1465-1561).  `nz` points at this engine's column of a [NZ_COUNT][stride]
// array of f64 bit patterns: the global noise buffer (stride I) or the block's LDS copy (stride 32).  Out of line: the path is
// off by default and must not cost the noise-free loop registers.
__device__ inline uint64_t nz_splitmix64(uint64_t& st) {                     // :1493-1499
    st += 0x9E3779B97F4A7C15ull;
    uint64_t z = st;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// set_seed / the RNG half of reset (:1865-1874, 2094-2100): streams from the engine's master seed, caches and lag cleared
__device__ __noinline__ void nz_reseed(double* nz, int stride) {
    uint64_t sm = dbits(nz[(size_t)NZ_SEED * stride]);
    (void)nz_splitmix64(sm);
    for (int k = 0; k < 11; ++k) {
        uint64_t s4[4];
        for (int q = 0; q < 4; ++q) s4[q] = nz_splitmix64(sm);
        if (!(s4[0] | s4[1] | s4[2] | s4[3])) s4[0] = 1;
        for (int q = 0; q < 4; ++q) nz[(size_t)(NZ_RNG + 4 * k + q) * stride] = bitsd(s4[q]);
        nz[(size_t)(NZ_CACHE + k) * stride] = 0.0;
        nz[(size_t)(NZ_WPREV + k) * stride] = 0.0;
        nz[(size_t)(NZ_LAST + k) * stride] = 0.0;
    }
    nz[(size_t)NZ_VALID * stride] = bitsd(0ull);
}
__device__ __noinline__ void nz_clear_lag(double* nz, int stride) {               // NaN reset of process_sample (:3625-3627)
    for (int k = 0; k < 11; ++k) { nz[(size_t)(NZ_WPREV + k) * stride] = 0.0; nz[(size_t)(NZ_LAST + k) * stride] = 0.0; }
}
__device__ inline double nz_next_f64(double* nz, int stride, int k) {        // xoshiro256++ (:1467-1489)
    uint64_t s0 = dbits(nz[(size_t)(NZ_RNG + 4 * k) * stride]), s1 = dbits(nz[(size_t)(NZ_RNG + 4 * k + 1) * stride]);
    uint64_t s2 = dbits(nz[(size_t)(NZ_RNG + 4 * k + 2) * stride]), s3 = dbits(nz[(size_t)(NZ_RNG + 4 * k + 3) * stride]);
    const uint64_t sum = s0 + s3;
    const uint64_t result = ((sum << 23) | (sum >> 41)) + s0;
    const uint64_t t = s1 << 17;
    s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3;
    s2 ^= t;
    s3 = (s3 << 45) | (s3 >> 19);
    nz[(size_t)(NZ_RNG + 4 * k) * stride] = bitsd(s0); nz[(size_t)(NZ_RNG + 4 * k + 1) * stride] = bitsd(s1);
    nz[(size_t)(NZ_RNG + 4 * k + 2) * stride] = bitsd(s2); nz[(size_t)(NZ_RNG + 4 * k + 3) * stride] = bitsd(s3);
    return (double)(result >> 11) * (1.0 / 9007199254740992.0);
}
// One sample of the two-draw thermal stamp (:3433-3452): i_n[k] = w_new + w_prev into NZ_LAST, w_prev <- w_new.
__device__ __noinline__ void nz_draw(double* nz, int stride, double scale_half, double sqrt_inv_r10) {
    uint64_t valid = dbits(nz[(size_t)NZ_VALID * stride]);
    for (int k = 0; k < 11; ++k) {
        double g;
        if ((valid >> k) & 1ull) {                                            // Marsaglia polar: cached second value (:1547-1561)
            valid &= ~(1ull << k);
            g = nz[(size_t)(NZ_CACHE + k) * stride];
        } else {
            // The reference loops until a pair falls inside the unit disc (p = pi/4 per try).  Bounded here so that a corrupt
            // (all-zero) generator state can never hang a wavefront: 128 rejections in a row have probability 1e-86.
            g = 0.0;
            for (int tries = 0; tries < 128; ++tries) {
                const double u = 2.0 * nz_next_f64(nz, stride, k) - 1.0;
                const double v = 2.0 * nz_next_f64(nz, stride, k) - 1.0;
                const double ss = u * u + v * v;
                if (ss > 0.0 && ss < 1.0) {
                    const double factor = sqrt(-2.0 * log(ss) / ss);
                    nz[(size_t)(NZ_CACHE + k) * stride] = v * factor;
                    valid |= 1ull << k;
                    g = u * factor;
                    break;
                }
            }
        }
        const double sir = k == 10 ? sqrt_inv_r10 : PRE_NOISE_THERMAL_SQRT_INV_R_DEFAULT[k];
        const double w_new = scale_half * sir * g;
        const double i_n = w_new + nz[(size_t)(NZ_WPREV + k) * stride];
        nz[(size_t)(NZ_WPREV + k) * stride] = w_new;
        nz[(size_t)(NZ_LAST + k) * stride] = i_n;
    }
    nz[(size_t)NZ_VALID * stride] = bitsd(valid);
}
// rhs[ni-1] += i_n; rhs[nj-1] -= i_n for the 11 sources in order (:3443-3451); indices are compile-time after unrolling
__device__ inline void nz_stamp(double rhs[12], const double* nz, int stride) {
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const double i_n = nz[(size_t)(NZ_LAST + k) * stride];
        const int ni = (int)PRE_NOISE_THERMAL_NODE_I[k], nj = (int)PRE_NOISE_THERMAL_NODE_J[k];
        if (ni > 0) rhs[ni - 1] += i_n;
        if (nj > 0) rhs[nj - 1] -= i_n;
    }
}

// Backward-Euler fallback (gen_preamp.rs:3483-3572) with the never-rebuilt 48 kHz / 100 kOhm codegen tables.
// nz != nullptr: replay of this sample's thermal stamp (:3522-3535).
// Inlined behind __builtin_expect (cold): out of line it pinned the caller's register budget (a callee cannot be capped) and the kernel
// to one wavefront per SIMD.  Rolled loops: this path runs once in thousands of samples.
__device__ inline uint32_t mel_be_fallback(const MelSt& st, double input, double vn[12], double i_nl[3], const double* nz, int nz_stride) {
    double rhs[12], vp[12], p[3];
#pragma unroll 1
    for (int i = 0; i < 12; ++i) {
        double sum = PRE_RHS_CONST_BE[i];
        for (int j = 0; j < 12; ++j) sum += PRE_A_NEG_BE_DEFAULT[i][j] * st.v[j];
        for (int j = 0; j < 3; ++j) sum += PRE_N_I[j][i] * st.ip[j];
        rhs[i] = sum;
    }
    rhs[0] += input / PRE_INPUT_RESISTANCE;
    if (nz)
        for (int k = 0; k < 11; ++k) {
            const double i_n = nz[(size_t)(NZ_LAST + k) * nz_stride];
            const int ni = (int)PRE_NOISE_THERMAL_NODE_I[k], nj = (int)PRE_NOISE_THERMAL_NODE_J[k];
            if (ni > 0) rhs[ni - 1] += i_n;
            if (nj > 0) rhs[nj - 1] -= i_n;
        }
#pragma unroll 1
    for (int i = 0; i < 12; ++i) {
        double sum = 0.0;
        for (int j = 0; j < 12; ++j) sum += PRE_S_BE_DEFAULT[i][j] * rhs[j];
        vp[i] = sum;
    }
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
        double sum = 0.0;
        for (int j = 0; j < 12; ++j) sum += PRE_N_V[i][j] * vp[j];
        p[i] = sum;
    }
    double kb[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) kb[i][j] = PRE_K_BE_DEFAULT[i][j];
    const uint32_t it = mel_solve_nl(p, kb, st.ip, st.ipp, i_nl);
#pragma unroll 1
    for (int i = 0; i < 12; ++i) {
        double x = vp[i];
        for (int j = 0; j < 3; ++j) x += PRE_S_NI_BE_DEFAULT[i][j] * i_nl[j];
        vn[i] = x;
    }
    return it;
}

// gen_preamp::process_sample (gen_preamp.rs:3399-3663).  Returns the OUT node voltage.
// nz: this sample's thermal stamp (already drawn into NZ_LAST by nz_draw) or nullptr when the state draws no noise.
__device__ inline double mel_process(MelSt& st, double input_in, const MelMats* __restrict__ M, const double* nz = nullptr, int nz_stride = 0) {
    const double input = isfinite(input_in) ? clampd(input_in, -100.0, 100.0) : 0.0;
    // rank-one factor of the current R_ldr (replaces the lazy rebuild_matrices of the reference)
    const double dg = ow_div(1.0, st.pot) - M->g_nom;
    const double c = ow_div(dg, 1.0 + dg * M->s66);
#pragma unroll
    for (int i = 0; i < 12; ++i) st.v[i] = st.v[i] + 1e-25 - 1e-25;
#pragma unroll
    for (int i = 0; i < 3; ++i) st.ip[i] = st.ip[i] + 1e-25 - 1e-25;
    const bool force_be = st.be_cooldown > 0u;
    if (st.be_cooldown > 0u) st.be_cooldown -= 1u;
    const double* v = st.v;
#define AN(i, j) M->aneg0[i][j]
    const double an66 = AN(6, 6) - dg;                               // A_neg = alpha C - G_eff: only [6][6] depends on R
    double rhs[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 15.0};     // RHS_CONST (gen_preamp.rs:760-773)
    rhs[0] += AN(0, 0) * v[0] + AN(0, 1) * v[1];
    rhs[1] += AN(1, 0) * v[0] + AN(1, 1) * v[1] + AN(1, 2) * v[2];
    rhs[2] += AN(2, 1) * v[1] + AN(2, 2) * v[2] + AN(2, 3) * v[3] + AN(2, 4) * v[4] + AN(2, 5) * v[5];
    rhs[3] += AN(3, 2) * v[2] + AN(3, 3) * v[3] + AN(3, 4) * v[4] + AN(3, 7) * v[7] + AN(3, 11) * v[11];
    rhs[4] += AN(4, 2) * v[2] + AN(4, 3) * v[3] + AN(4, 4) * v[4] + AN(4, 7) * v[7] + AN(4, 8) * v[8];
    rhs[5] += AN(5, 2) * v[2] + AN(5, 5) * v[5] + AN(5, 6) * v[6];
    rhs[6] += AN(6, 5) * v[5] + an66 * v[6] + AN(6, 10) * v[10];
    rhs[7] += AN(7, 3) * v[3] + AN(7, 4) * v[4] + AN(7, 7) * v[7] + AN(7, 10) * v[10];
    rhs[8] += AN(8, 4) * v[4] + AN(8, 8) * v[8] + AN(8, 9) * v[9];
    rhs[9] += AN(9, 8) * v[8] + AN(9, 9) * v[9];
    rhs[10] += AN(10, 6) * v[6] + AN(10, 7) * v[7] + AN(10, 10) * v[10];
#undef AN
    rhs[2] += PRE_N_I[0][2] * st.ip[0];
    rhs[2] += PRE_N_I[1][2] * st.ip[1];
    rhs[4] += PRE_N_I[1][4] * st.ip[1];
    rhs[4] += PRE_N_I[2][4] * st.ip[2];
    rhs[5] += PRE_N_I[1][5] * st.ip[1];
    rhs[7] += PRE_N_I[2][7] * st.ip[2];
    rhs[8] += PRE_N_I[2][8] * st.ip[2];
    rhs[0] += (input + st.input_prev) / PRE_INPUT_RESISTANCE;
    if (nz) nz_stamp(rhs, nz, nz_stride);
    // v_pred = S(R) rhs = S0 rhs - c u (w . rhs)
    double wr = 0.0;
#pragma unroll
    for (int j = 0; j < 12; ++j) wr += M->w[j] * rhs[j];
    // (at the nominal pot c is exactly 0 and S(R) is S0: the correction vanishes there whatever wr is -- 0 * inf would make every node NaN
    // where the reference has overflowed voltages that its ringing test still sees)
    const double cwr = c == 0.0 ? 0.0 : c * wr;
    double v_pred[12];
    {   // column sweep: every row still accumulates its terms in j order (same sums), but only the twelve running sums are live
        // while a column of the matrix streams through, instead of whole rows of it waiting in registers
        double acc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
#pragma unroll
            for (int i = 0; i < 12; ++i) acc[i] += M->s0[i][j] * rhs[j];
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) v_pred[i] = acc[i] - cwr * M->u[i];
    }
    const double p[3] = {-v_pred[2], v_pred[2] - v_pred[5], v_pred[4] - v_pred[8]};
    double kk[3][3];                                                  // K(R) = K0 - c (N_v u)(w N_i)^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) kk[i][j] = M->k0[i][j] - c * M->nvu[i] * M->wn[j];
    double i_nl[3];
    uint32_t last_it = mel_solve_nl(p, kk, st.ip, st.ipp, i_nl);
    const double cwi = c == 0.0 ? 0.0 : c * (M->wn[0] * i_nl[0] + M->wn[1] * i_nl[1] + M->wn[2] * i_nl[2]);
    double vn[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {                                     // v = v_pred + S(R) N_i i_nl
        double x = v_pred[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) x += M->sni0[i][j] * i_nl[j];
        vn[i] = x - cwi * M->u[i];
    }
    const bool nr_failed = last_it >= 265u;
    bool ringing = false;
#pragma unroll
    for (int i = 0; i < 11; ++i) ringing = ringing || (fabs(vn[i]) > 55.0);
    if (__builtin_expect(nr_failed || ringing || force_be, 0)) {
        if (ringing || nr_failed) st.be_cooldown = 64u;
        st.be_fallbacks += 1u;
        // The out-of-line retry takes its operands by address: hand it copies, so that the solver state and the candidate solution
        // of the common path are never address-taken (they would live in scratch / spilled registers for every sample otherwise).
        MelSt tmp = st;
        double vn2[12], inl2[3];
        last_it = mel_be_fallback(tmp, input, vn2, inl2, nz, nz_stride);
#pragma unroll
        for (int i = 0; i < 12; ++i) vn[i] = vn2[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) i_nl[i] = inl2[i];
    }
    {   // voltage-damp net (gen_preamp.rs:3576-3613); threshold = fma(max|DC_OP|, 0.05, 2.0), the path's one explicit mul_add
        double max_delta = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) { const double d = fabs(vn[i] - st.v[i]); if (d > max_delta) max_delta = d; }
        double max_dc = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) { const double a = fabs(PRE_DC_OP[i]); if (a > max_dc) max_dc = a; }
        const double thr = fma(max_dc, 0.05, 2.0);
        if (max_delta > thr) {
            const double damp = fmax(ow_div(thr, max_delta), 0.01);
#pragma unroll
            for (int i = 0; i < 12; ++i) vn[i] = st.v[i] + damp * (vn[i] - st.v[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) i_nl[i] = st.ip[i] + damp * (i_nl[i] - st.ip[i]);
        }
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) finite = finite && isfinite(vn[i]);
    if (!finite) {                                          // gen_preamp.rs:3616-3636
#pragma unroll
        for (int i = 0; i < 12; ++i) st.v[i] = PRE_DC_OP[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) { st.ip[i] = PRE_DC_NL_I[i]; st.ipp[i] = PRE_DC_NL_I[i]; }
        st.input_prev = 0.0;
        st.pot = 9.99999999999999854e4;
        st.be_cooldown = 0u;
        st.nan_resets += 1u;
        return clampd(PRE_DC_OP[10] * 1.0, -10.0, 10.0);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) st.v[i] = vn[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { st.ipp[i] = st.ip[i]; st.ip[i] = i_nl[i]; }
    st.input_prev = input;
    const double raw = isfinite(vn[10]) ? vn[10] : 0.0;
    return raw * 1.0;
}

OW_DEV void mel_set_r(MelSt& st, double r_in) {  // set_runtime_R_r_ldr, gen_preamp.rs:1973-1984
    if (!isfinite(r_in)) return;
    const double r = clampd(r_in, 1000.0, 1000000.0);
    if (fabs(r - st.pot) < 1e-12) return;
    st.pot = r;
}

// chain-state slots of the melange states: 21 doubles + 1 packed word each
enum { CSM_V = 0, CSM_IP = 12, CSM_IPP = 15, CSM_INPREV = 18, CSM_POT = 19, CSM_WORD = 20, CSM_COUNT = 21 };
OW_DEV void mel_load(MelSt& s, const double* __restrict__ cs, int I, int e, int base) {
#pragma unroll
    for (int i = 0; i < 12; ++i) s.v[i] = CSF(base + CSM_V + i);
#pragma unroll
    for (int i = 0; i < 3; ++i) { s.ip[i] = CSF(base + CSM_IP + i); s.ipp[i] = CSF(base + CSM_IPP + i); }
    s.input_prev = CSF(base + CSM_INPREV); s.pot = CSF(base + CSM_POT);
    s.be_cooldown = (uint32_t)dbits(CSF(base + CSM_WORD));
    s.nan_resets = 0; s.be_fallbacks = 0;
}
OW_DEV void mel_store(const MelSt& s, double* __restrict__ cs, int I, int e, int base) {
#pragma unroll
    for (int i = 0; i < 12; ++i) CSF(base + CSM_V + i) = s.v[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { CSF(base + CSM_IP + i) = s.ip[i]; CSF(base + CSM_IPP + i) = s.ipp[i]; }
    CSF(base + CSM_INPREV) = s.input_prev; CSF(base + CSM_POT) = s.pot;
    CSF(base + CSM_WORD) = bitsd((uint64_t)s.be_cooldown);
}

// init_state (melange_adapter.rs:22-29): the settled codegen-rate state; set_sample_rate only swaps matrices (pool constants here)
__device__ inline void mel_init_state(MelSt& st, const double* __restrict__ settled) {
    for (int i = 0; i < 12; ++i) st.v[i] = settled[i];
    for (int i = 0; i < 3; ++i) { st.ip[i] = settled[12 + i]; st.ipp[i] = settled[15 + i]; }
    st.input_prev = 0.0;
    st.pot = 9.99999999999999854e4;
    st.be_cooldown = 0u;
}

// CircuitState::default() + 176 400 zero-input samples at the codegen rate (melange_adapter.rs:14-20): one lane.
// K48 holds the 48 kHz codegen tables as its melange constants.
__global__ __launch_bounds__(64) void k_mel_settle(const OwConsts* __restrict__ K48, double* __restrict__ settled) {
    __shared__ MelMats M;
    mel_mats_load(&M, K48, threadIdx.x, 64);
    __syncthreads();
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    MelSt st;
    for (int i = 0; i < 12; ++i) st.v[i] = PRE_DC_OP[i];
    for (int i = 0; i < 3; ++i) { st.ip[i] = PRE_DC_NL_I[i]; st.ipp[i] = PRE_DC_NL_I[i]; }
    st.input_prev = 0.0; st.pot = 9.99999999999999854e4; st.be_cooldown = 0u; st.nan_resets = 0; st.be_fallbacks = 0;
    for (int n = 0; n < 176400; ++n) {
        int z = 0;
        asm volatile("" : "+v"(z));
        mel_process(st, 0.0, &M + z);
    }
    for (int i = 0; i < 12; ++i) settled[i] = st.v[i];
    for (int i = 0; i < 3; ++i) { settled[12 + i] = st.ip[i]; settled[15 + i] = st.ipp[i]; }
}

// DkPreamp::new / reset for engines [e0, e0+ne): both states from the settled state
__global__ __launch_bounds__(64) void k_mel_init(double* __restrict__ cs, const double* __restrict__ settled, double* __restrict__ noise, int I,
                                                 int e0, int ne) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= 2 * ne) return;
    const int e = e0 + (t % ne), role = t / ne;
    MelSt st;
    mel_init_state(st, settled);
    mel_store(st, cs, I, e, role ? CS_M_SHADOW : CS_M_MAIN);
    if (role == 0 && noise) nz_reseed(noise + e, I);   // a fresh state restarts its noise streams from the engine's master seed
}
// gen_preamp::set_seed for engines [e0, e0+ne): NZ_SEED was written by the host
__global__ __launch_bounds__(64) void k_mel_noise_seed(double* __restrict__ noise, int I, int e0, int ne) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < ne) nz_reseed(noise + e0 + t, I);
}

// Preamp stream with the melange solver: same staging / lane-pair structure as k_preamp.
__global__ __launch_bounds__(64) void k_preamp_mel(const OwConsts* __restrict__ K, double* __restrict__ cs,
                                                   const double* __restrict__ settled, const OwEngineArgs* __restrict__ args,
                                                   const OwEngineOut* __restrict__ eout, const double* __restrict__ sum, const OwTremSrc tsrc,
                                                   double* __restrict__ pre, double* __restrict__ noise, int I, int L,
                                                   int Lcap, int e0, int ne) {
    __shared__ double tile[32 * (OW_PCHUNK + 1)];
    __shared__ MelMats M;
    __shared__ double NZL[NZ_COUNT * 32];   // thermal-noise columns of the block's 32 main states (used only when some engine has noise on)
    mel_mats_load(&M, K, threadIdx.x, 64);
    __syncthreads();
    const int lane = threadIdx.x;
    const int el = lane & 31, role = lane >> 5;
    const int eb = e0 + blockIdx.x * 32;
    const int e = eb + el;
    const bool valid = e < e0 + ne;
    const int ec = valid ? e : (e0 + ne - 1);
    const int osr = K->oversample ? 2 : 1;
    const TremCol rc = trem_col(tsrc, I, ec);

    MelSt st;
    double ua[3], ub[3];
    Smoother sd;
    {
        const int e = ec;
        smoother_load(sd, cs, I, e, CS_SM_DEPTH);
        if (args[e].set_flags & 1u) sd.retarget(args[e].depth_target, K->ramp_samples);
        mel_load(st, cs, I, e, role ? CS_M_SHADOW : CS_M_MAIN);
        for (int i = 0; i < 3; ++i) { ua[i] = CSF(CS_OS_UA + i); ub[i] = CSF(CS_OS_UB + i); }
        const uint64_t fl = dbits(CSF(CS_FLAGS));
        if (fl & 1ull) {  // deferred preamp.reset() + oversampler.reset() from the output NaN guard (engine.rs:450-457)
            mel_init_state(st, settled);
            for (int i = 0; i < 3; ++i) { ua[i] = 0.0; ub[i] = 0.0; }
        }
    }
    uint32_t adapter_resets = 0;
    // thermal noise: only the main state draws (melange_adapter.rs:50-57); block-rate switch and gain (engine.rs:394-400)
    const bool nz_mine = noise != nullptr && valid && role == 0;
    const bool nz_on = nz_mine && args[ec].noise_on != 0u;
    const double scale_half = K->m_noise_scale * 1.0 * args[ec].thermal_gain * 0.5;   // scale * noise_gain * thermal_gain * 0.5 (:3435)
    const bool nz_loaded = nz_on;          // the column lives in LDS for the block
    double* nzcol = NZL + el;
    bool nz_need_reseed = false, nz_need_clear = false;
    if (nz_loaded)
        for (int r = 0; r < NZ_COUNT; ++r) nzcol[r * 32] = noise[(size_t)r * I + e];
    if (nz_mine && (dbits(CSF(CS_FLAGS)) & 1ull)) {   // the deferred preamp.reset() above re-created the main state
        if (nz_loaded) nz_reseed(nzcol, 32); else nz_need_reseed = true;
    }
    for (int base = 0; base < L; base += OW_PCHUNK) {
        const int cn = min(OW_PCHUNK, L - base);
        for (int r = 0; r < 32; ++r) {
            const int er = eb + r;
            double x = 0.0;
            if (er < e0 + ne && lane < cn && !eout[er].sum_nonfinite) {
                if (args[er].main_mask) x = sum[((size_t)0 * I + er) * Lcap + base + lane];
                if (args[er].steal_mask) x += sum[((size_t)1 * I + er) * Lcap + base + lane];
            }
            tile[r * (OW_PCHUNK + 1) + lane] = x;
        }
        __syncthreads();
        for (int n = 0; n < cn; ++n) {
            const double x = tile[el * (OW_PCHUNK + 1) + n];
            const double depth = clampd(sd.next(), 0.0, 1.0);   // engine.rs:533-534
            double in[2];
            if (osr == 2) {
                const double a = allpass3(OW_OS_A0, OW_OS_A1, OW_OS_A2, ua, x);
                const double b = allpass3(OW_OS_B0, OW_OS_B1, OW_OS_B2, ub, x);
                in[0] = role ? 0.0 : a;
                in[1] = role ? 0.0 : b;
            } else {
                in[0] = role ? 0.0 : x;
                in[1] = 0.0;
            }
            for (int j = 0; j < osr; ++j) {
                const size_t s_idx = (size_t)((base + n) * osr + j);
                mel_set_r(st, trem_shunt(depth, trem_col_at(rc, (uint32_t)s_idx)));            // tremolo.rs:152-167; melange_adapter.rs:82-85
                int z = 0;
                asm volatile("" : "+v"(z));                                        // keep the LDS constant reads inside the loop
                const double* nzp = nullptr;
                if (nz_on && scale_half != 0.0) {
                    // sqrt(1/R) of the LDR source follows set_runtime_R (:1983); the untouched nominal pot keeps the baked literal
                    const double sir10 = st.pot == 9.99999999999999854e4 ? PRE_NOISE_THERMAL_SQRT_INV_R_DEFAULT[10] : sqrt(1.0 / st.pot);
                    nz_draw(nzcol, 32, scale_half, sir10);
                    nzp = nzcol;
                }
                const uint32_t nan_before = st.nan_resets;
                const double o = mel_process(st, in[j], &M + z, nzp, 32);
                if (nz_mine && st.nan_resets != nan_before) {                      // process_sample's NaN reset clears the lag (:3625-3627)
                    if (nz_loaded) nz_clear_lag(nzcol, 32); else nz_need_clear = true;
                }
                const double other = __shfl_xor(o, 32);
                double result = role ? (other - o) : (o - other);                  // main - pump (:74-76)
                if (!isfinite(result)) {                                           // :77-80, reset(): both states from init_state
                    mel_init_state(st, settled);
                    if (nz_mine) { if (nz_loaded) nz_reseed(nzcol, 32); else nz_need_reseed = true; }
                    result = 0.0;
                    adapter_resets += 1u;
                }
                if (valid && role == 0) pre[s_idx * I + e] = result;
            }
        }
        __syncthreads();
    }
    if (nz_loaded) {
        for (int r = 0; r < NZ_COUNT; ++r) noise[(size_t)r * I + e] = nzcol[r * 32];
    } else if (nz_mine) {
        if (nz_need_reseed) nz_reseed(noise + e, I);
        else if (nz_need_clear) nz_clear_lag(noise + e, I);
    }
    if (valid) {
        mel_store(st, cs, I, e, role ? CS_M_SHADOW : CS_M_MAIN);
        if (role == 0) {
            for (int i = 0; i < 3; ++i) { CSF(CS_OS_UA + i) = ua[i]; CSF(CS_OS_UB + i) = ub[i]; }
            smoother_store(sd, cs, I, e, CS_SM_DEPTH);
            const uint64_t fl = dbits(CSF(CS_FLAGS));
            if (fl & 1ull) CSF(CS_FLAGS) = bitsd(fl & ~1ull);
            const uint32_t nr = adapter_resets + st.nan_resets;
            if (nr) {
                const uint64_t d = dbits(CSF(CS_DIAG));
                CSF(CS_DIAG) = bitsd((d & 0xFFFFFFFFull) | ((uint64_t)((uint32_t)(d >> 32) + nr) << 32));
            }
        }
    }
}

}  // namespace owdev
