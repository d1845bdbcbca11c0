// openwurli-hip: preamp-measurement kernels (`preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep`,
// tools/preamp-bench/src/main.rs:150-369).  One point = a sine of (freq, amplitude) -> fresh Oversampler -> 2x-oversampled preamp
// (main - shadow, NaN guard) -> downsample_2x, 22 050 samples at BASE_SR.  The sine is generated in the kernel and the analysis is fused
// into it: the peak of |out| over the gain window and the five single-bin DFT sums of cmd_harmonics over the harmonics window.  Nothing
// is written per sample unless a trace is asked for.
//
//   k_pbench_row    legacy preamp, a row of sixteen lanes per solver state (k_job_chain_row's role split): wavefronts 0-3 run the
//                   up-sampler and dk_step_row for main and shadow of two points each, wavefront 4 downsamples a chunk behind, keeps the
//                   peak, sums the DFTs (one lane per point and harmonic) and generates the next chunk's sine into `tin`.  Small grids.
//   k_pbench<MEL>   lane pair (point, main|shadow), k_job_chain<MEL>'s step: the melange path, and for legacy the path of large grids.
// Per point the two kernels run the same operations on the same operands in the same order: bit-identical (OW_PBENCH_ROW=0/1).
#pragma once
#include "ow_chain_row.h"

namespace owdev {

struct OwPbenchDev {         // one point (host: ow_preamp_measure)
    double freq, amp;        // the sine: amp * sin(2 pi freq i / BASE_SR)
    double r_ldr;            // set_ldr_resistance's argument
    double r_reset;          // the resistance the legacy reset()'s DC solve runs at (ignored by the melange preamp)
};

// per point: the gain-window peak, then (re, im) of dft_magnitude at k x freq, k = 1..5
enum { PB_MET_PEAK = 0, PB_MET_RE1 = 1, PB_MET_COUNT = 11 };
#define OW_PB_N 22050            // OW_PBENCH_SAMPLES
#define OW_PB_GAIN_LO 13230      // OW_PBENCH_GAIN_LO: measure_gain_at's settle (BASE_SR * 0.3) as usize
#define OW_PB_HARM_LO 16537      // OW_PBENCH_HARM_LO: cmd_harmonics' output.len() * 3 / 4
#define OW_PB_TWO_PI 6.283185307179586      // 2.0 * PI, exact
#define OW_PB_SR 44100.0                    // BASE_SR

// 2.0 * PI * (k * freq): the first two factors of dft_magnitude's phase (main.rs:899; dft_magnitude(signal, 2.0 * freq, ..) etc., freq itself
// for k = 1)
OW_DEV double pb_tpf(int k, double freq) { return OW_PB_TWO_PI * (k == 1 ? freq : (double)k * freq); }
// the input sample of main.rs:170-171 / 270-271: amplitude * (2.0 * PI * freq * t).sin(), t = i as f64 / BASE_SR
OW_DEV double pb_sine(double amp, double freq, long long i) { return amp * sin(OW_PB_TWO_PI * freq * ((double)i / OW_PB_SR)); }
// one term of dft_magnitude's loop: phase = 2.0 * PI * freq * i as f64 / sr, i counted from the window start
OW_DEV void pb_dft_acc(double tpf, long long m, double s, double& re, double& im) {
    double sn, cs;
    sincos(tpf * (double)m / OW_PB_SR, &sn, &cs);
    re += s * cs;
    im -= s * sn;
}

// preamp.reset() at r_reset, then set_ldr_resistance(r_ldr) (dk_preamp_legacy.rs:620-640)
OW_DEV void pb_legacy_start(const OwConsts* __restrict__ K, const OwPbenchDev& pd, DkSt& st, double& r_ldr, double& g_ldr, double& g_prev) {
    r_ldr = pd.r_reset;
    dk_dc_reset(K, r_ldr, st);
    g_ldr = 1.0 / r_ldr;
    g_prev = g_ldr;
    const double r_new = fmax(pd.r_ldr, 1000.0);
    if (fabs(r_new - r_ldr) > 0.01) { r_ldr = r_new; g_ldr = 1.0 / r_new; }
}

__global__ __launch_bounds__(320) void k_pbench_row(const OwConsts* __restrict__ K, const OwPbenchDev* __restrict__ pts, double* __restrict__ met,
                                                    double* __restrict__ trace, int n_pts, long long stride) {
    __shared__ double tin[2][8 * (OW_FCHUNK + 1)];            // the sine, [slot][point of the block][sample]
    __shared__ double ring[2][OW_FCHUNK * 2][8];               // preamp out at the chain rate: [slot][sample x phase][point of the block]
    __shared__ double tout[8 * (OW_FCHUNK + 1)];               // downsampled out of the chunk
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pb = blockIdx.x * 8;
    const long long n = OW_PB_N;
    const long long n_chunks = (n + OW_FCHUNK - 1) / OW_FCHUNK;

    if (wv < 4) {
        const int row = lane >> 4, role = row >> 1;
        const int jl = 2 * wv + (row & 1);
        const int p = pb + jl;
        const OwPbenchDev pd = pts[p < n_pts ? p : n_pts - 1];
        DkRowK R;
        dk_row_consts(R, K, lane);
        DkSt st;
        double r_ldr, g_ldr, g_prev;
        double us[3] = {0, 0, 0};
        pb_legacy_start(K, pd, st, r_ldr, g_ldr, g_prev);
        const double sgn = role ? -1.0 : 1.0;
        auto preamp_step = [&](double x) -> double {
            const double o = dk_step_row(st, R, lane, x, g_ldr, g_prev);
            g_prev = g_ldr;
            const double other = xor32(o);
            double res = (o - other) * sgn;
            if (!isfinite(res)) {                                // the adapter's NaN guard: reset() at the current r_ldr
                dk_dc_reset(K, r_ldr, st); g_ldr = 1.0 / r_ldr; g_prev = g_ldr;
                res = 0.0;
            }
            return res;
        };
        __syncthreads();                                         // chunk 0's sine
        for (long long c = 0; c <= n_chunks; ++c) {
            if (c < n_chunks) {
                const long long base = c * OW_FCHUNK;
                const int cn = (int)((n - base) < OW_FCHUNK ? (n - base) : OW_FCHUNK);
                const double* tx = tin[c & 1];
                double (*slot)[8] = ring[c & 1];
                for (int sidx = 0; sidx < cn; ++sidx) {
                    const double x = tx[jl * (OW_FCHUNK + 1) + sidx];
                    const double y = allpass3(R.oc0, R.oc1, R.oc2, us, x);      // upsample_2x: branch A on even lanes, B on odd ones
                    const double in[2] = {role ? 0.0 : rowb<0>(y), role ? 0.0 : rowb<1>(y)};
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const double pk = preamp_step(in[k]);
                        if (role == 0 && (lane & 15) == 0) slot[sidx * 2 + k][jl] = pk;
                    }
                }
            }
            __syncthreads();
        }
        return;
    }

    // ---- wavefront 4.  Sine generator: lane -> (point lane >> 4 and lane >> 4 + 4, sample lane & 15) of the next chunk.
    const int g_s = lane & 15, g_r0 = lane >> 4, g_r1 = g_r0 + 4;
    const OwPbenchDev g0 = pts[pb + g_r0 < n_pts ? pb + g_r0 : n_pts - 1], g1 = pts[pb + g_r1 < n_pts ? pb + g_r1 : n_pts - 1];
    auto gen = [&](long long c) {
        const long long i = c * OW_FCHUNK + g_s;
        double* tx = tin[c & 1];
        tx[g_r0 * (OW_FCHUNK + 1) + g_s] = i < n ? pb_sine(g0.amp, g0.freq, i) : 0.0;
        tx[g_r1 * (OW_FCHUNK + 1) + g_s] = i < n ? pb_sine(g1.amp, g1.freq, i) : 0.0;
    };
    // downsampler: lanes 0..7 own a point each, the others shadow them; DFT: lane = 5 x point + (k - 1) for lanes 0..39
    const int jl = lane & 7;
    const bool own = lane < 8 && pb + jl < n_pts;
    const int d_r = lane / 5, d_k = lane - 5 * d_r + 1;
    const bool dft = lane < 40 && pb + d_r < n_pts;
    const double tpf = pb_tpf(d_k, pts[pb + d_r < n_pts ? pb + d_r : n_pts - 1].freq);
    double da[3] = {0, 0, 0}, db[3] = {0, 0, 0}, dd = 0.0;
    double pk = 0.0, re = 0.0, im = 0.0;
    gen(0);
    __syncthreads();
    for (long long c = 0; c <= n_chunks; ++c) {
        if (c + 1 < n_chunks) gen(c + 1);                        // tin[(c + 1) & 1]: read by the preamp wavefronts after this barrier
        if (c >= 1) {
            const long long base = (c - 1) * OW_FCHUNK;
            const int cn = (int)((n - base) < OW_FCHUNK ? (n - base) : OW_FCHUNK);
            const double (*slot)[8] = ring[(c - 1) & 1];
            for (int sidx = 0; sidx < cn; ++sidx) {               // downsample_2x
                const double fa = allpass3(OW_OS_A0, OW_OS_A1, OW_OS_A2, da, slot[sidx * 2][jl]);
                const double fb = allpass3(OW_OS_B0, OW_OS_B1, OW_OS_B2, db, slot[sidx * 2 + 1][jl]);
                const double pre = (fa + dd) * 0.5;
                dd = fb;
                if (base + sidx >= OW_PB_GAIN_LO) pk = fmax(pk, fabs(pre));          // peak = peak.max(down[0].abs())
                if (lane < 8) tout[jl * (OW_FCHUNK + 1) + sidx] = pre;
            }
            OW_WAVE_SYNC();
            if (dft && base + cn > OW_PB_HARM_LO) {              // in the reference's sample order
                for (int sidx = 0; sidx < cn; ++sidx) {
                    const long long i = base + sidx;
                    if (i >= OW_PB_HARM_LO) pb_dft_acc(tpf, i - OW_PB_HARM_LO, tout[d_r * (OW_FCHUNK + 1) + sidx], re, im);
                }
            }
            if (trace)
                for (int k = lane; k < 8 * OW_FCHUNK; k += 64) {
                    const int r = k / OW_FCHUNK, sm = k - r * OW_FCHUNK;
                    if (pb + r < n_pts && sm < cn) trace[(size_t)(pb + r) * stride + base + sm] = tout[r * (OW_FCHUNK + 1) + sm];
                }
            OW_WAVE_SYNC();
        }
        __syncthreads();
    }
    if (own) met[(size_t)(pb + jl) * PB_MET_COUNT + PB_MET_PEAK] = pk;
    if (dft) {
        double* m = met + (size_t)(pb + d_r) * PB_MET_COUNT + PB_MET_RE1 + 2 * (d_k - 1);
        m[0] = re;
        m[1] = im;
    }
}

// k_job_chain<MEL>'s preamp (lane pair: main in lanes 0-31, shadow in 32-63, 32 points per wavefront) on the in-kernel sine, with the same
// fused analysis: the main lane keeps the peak and sums H1..H3, the shadow lane H4 and H5, from the chunk's tile.
template <bool MEL>
__global__ __launch_bounds__(64) void k_pbench(const OwConsts* __restrict__ K, const OwPbenchDev* __restrict__ pts, double* __restrict__ met,
                                               double* __restrict__ trace, const double* __restrict__ settled, int n_pts, long long stride) {
    __shared__ double tout[32 * (OW_PCHUNK + 1)];
    __shared__ double LU_all[MEL ? 12 * 12 * 32 : 1];
    __shared__ double S_all[MEL ? 12 * 12 * 32 : 1];
    const int lane = threadIdx.x;
    const int jl = lane & 31, role = lane >> 5;
    const int pb = blockIdx.x * 32;
    const int p = pb + jl;
    const bool valid = p < n_pts;
    const OwPbenchDev pd = pts[valid ? p : n_pts - 1];
    const long long n = OW_PB_N;

    DkSt st;
    MelSt ms;
    double r_ldr = 1000000.0, g_ldr = 1e-6, g_prev = 1e-6;
    double* lu = LU_all + (MEL ? jl : 0);
    double* S = S_all + (MEL ? jl : 0);
    const double alpha = 2.0 * (K->os_sr * 1.0);
    double s_pot = __longlong_as_double(0x7ff8000000000000LL);
    double kk[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    double an66 = 0.0;
    if (MEL) {
        mel_init_state(ms, settled);                  // reset() clones the settled state (melange_adapter.rs:88-93)
        ms.nan_resets = 0; ms.be_fallbacks = 0;
        mel_set_r(ms, pd.r_ldr);
    } else {
        pb_legacy_start(K, pd, st, r_ldr, g_ldr, g_prev);
    }
    auto preamp_step = [&](double x) -> double {
        double o;
        if (MEL) {
            const double pot_main = __shfl(ms.pot, jl);
            if (__any(!(pot_main == s_pot))) {
                double kt[3][3];
                mel_lit_rebuild(pot_main, role, alpha, lu, S, kt);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) kk[a][b] = kt[a][b];
                s_pot = pot_main;
                const double g66 = PRE_G[6][6] + (ow_div(1.0, pot_main) - PRE_POT_0_G_NOM);
                an66 = alpha * PRE_C[6][6] - g66;
            }
            o = mel_process_lit(ms, x, K->m_aneg0, an66, S, kk, nullptr, 0);
        } else {
            o = dk_step(st, x, g_ldr, g_prev, K);
            g_prev = g_ldr;
        }
        const double other = xor32_t(o);
        double res = role ? (other - o) : (o - other);
        if (!isfinite(res)) {
            if (MEL) { mel_init_state(ms, settled); }
            else { dk_dc_reset(K, r_ldr, st); g_ldr = 1.0 / r_ldr; g_prev = g_ldr; }
            res = 0.0;
        }
        return res;
    };
    double ua[3] = {0, 0, 0}, ub[3] = {0, 0, 0}, da[3] = {0, 0, 0}, db[3] = {0, 0, 0}, dd = 0.0;
    double pk = 0.0, re[3] = {0, 0, 0}, im[3] = {0, 0, 0};
    const int k0 = role ? 4 : 1, nk = role ? 2 : 3;
    double tpf[3];
    for (int q = 0; q < 3; ++q) tpf[q] = pb_tpf(k0 + q, pd.freq);

    for (long long base = 0; base < n; base += OW_PCHUNK) {
        const int cn = (int)((n - base) < OW_PCHUNK ? (n - base) : OW_PCHUNK);
        for (int s = 0; s < cn; ++s) {
            const double x = pb_sine(pd.amp, pd.freq, base + s);
            const double a = allpass3(OW_OS_A0, OW_OS_A1, OW_OS_A2, ua, x);
            const double b = allpass3(OW_OS_B0, OW_OS_B1, OW_OS_B2, ub, x);
            double pp[2];
            const double in[2] = {role ? 0.0 : a, role ? 0.0 : b};
            for (int k = 0; k < 2; ++k) pp[k] = preamp_step(in[k]);
            const double fa = allpass3(OW_OS_A0, OW_OS_A1, OW_OS_A2, da, pp[0]);
            const double fb = allpass3(OW_OS_B0, OW_OS_B1, OW_OS_B2, db, pp[1]);
            const double pre = (fa + dd) * 0.5;
            dd = fb;
            if (role == 0) {
                if (base + s >= OW_PB_GAIN_LO) pk = fmax(pk, fabs(pre));
                tout[jl * (OW_PCHUNK + 1) + s] = pre;
            }
        }
        __syncthreads();
        if (base + cn > OW_PB_HARM_LO) {
            for (int s = 0; s < cn; ++s) {
                const long long i = base + s;
                if (i < OW_PB_HARM_LO) continue;
                const double y = tout[jl * (OW_PCHUNK + 1) + s];
                for (int q = 0; q < nk; ++q) pb_dft_acc(tpf[q], i - OW_PB_HARM_LO, y, re[q], im[q]);
            }
        }
        if (trace)
            for (int r = 0; r < 32; ++r)
                if (pb + r < n_pts && lane < cn) trace[(size_t)(pb + r) * stride + base + lane] = tout[r * (OW_PCHUNK + 1) + lane];
        __syncthreads();
    }
    if (!valid) return;
    double* m = met + (size_t)p * PB_MET_COUNT;
    if (role == 0) m[PB_MET_PEAK] = pk;
    for (int q = 0; q < nk; ++q) {
        m[PB_MET_RE1 + 2 * (k0 + q - 1)] = re[q];
        m[PB_MET_RE1 + 2 * (k0 + q - 1) + 1] = im[q];
    }
}

}  // namespace owdev
