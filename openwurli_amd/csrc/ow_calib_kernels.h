// openwurli-hip: calibration-sweep kernels (`preamp-bench calibrate` / `sensitivity`, tools/preamp-bench/src/main.rs:1069-1395).
//
//   k_calib_voice    lane = point: ModalReed::new(.., onset 0, ..) -> Pickup::new_with_scale(ds_actual) -> x output_scale, 0.5 s at
//                    44.1 kHz.  Writes the T2 (pickup) and T3 (x out_scale) rows, T1 (reed) only when taps were asked for; the T1 window
//                    peak (y_peak) is reduced in registers.  The reed and pickup are the voice path's own (note_on_lane, VoiceRegs::step).
//   (T4 is the batch chain: k_job_chain<MEL> in JOB_OUT_PA_INPUT mode at volume 1.0, ow_job_kernels.h)
//   k_calib_out      lane = point: T4 x volume^2 -> behavioural power_amp -> Speaker -> x POST_SPEAKER_GAIN at 44.1 kHz, or the two
//                    halves around a melange power amp launch (k_mpa_debug)
//   k_calib_metrics  workgroup = (point, stage): window peak, sum of squares and the H1 / H2 single-bin DFTs of one T row
#pragma once
#include "ow_job_kernels.h"

namespace owdev {

struct OwCalibDev {          // one grid point, as the kernels need it (host: ow_calibrate)
    int note, velocity;      // 33..96, 0..127
    double ds_actual;        // pickup_displacement_scale_with_config (tables.rs:283-288)
    double out_scale;        // output_scale_with_config (tables.rs:578-620)
    double f0;               // params.fundamental_hz, the frequency h2_h1_ratio_db analyses (main.rs:1143, 1182)
};

#define OW_CALIB_WIN_LO 4410     // (0.100 * BASE_SR) as usize, main.rs:1138
#define OW_CALIB_WIN_HI 17640    // (0.400 * BASE_SR) as usize, main.rs:1139
enum { CALIB_MET_PEAK = 0, CALIB_MET_SUMSQ = 1, CALIB_MET_RE1 = 2, CALIB_MET_IM1 = 3, CALIB_MET_RE2 = 4, CALIB_MET_IM2 = 5, CALIB_MET_COUNT = 6 };

// run_calibrate's T1..T3 (main.rs:1149-1187).  t1 may be nullptr.  t1_peak[p] = peak_abs(reed[4410..17640)).
__global__ __launch_bounds__(64) void k_calib_voice(const OwConsts* __restrict__ K, const double* __restrict__ nt, double* __restrict__ vrec,
                                                    const OwCalibDev* __restrict__ pts, double* __restrict__ t1, double* __restrict__ t2,
                                                    double* __restrict__ t3, double* __restrict__ t1_peak, int n_pts, long long n, long long stride) {
    __shared__ double tile[64 * (OW_VCHUNK + 1)];
    __shared__ double rtile[64 * (OW_VCHUNK + 1)];
    __shared__ double lcoef[OW_LCOEF_ROWS * 64];
    __shared__ double oscale[64];
    const int lane = threadIdx.x;
    const int pb = blockIdx.x * 64;
    const int p = pb + lane;
    const bool active = p < n_pts;
    double* rec = vrec + (size_t)blockIdx.x * OW_VREC_DOUBLES + lane;
    VoiceRegs v;
    oscale[lane] = 0.0;
    if (active) {
        const OwCalibDev pd = pts[p];
        const double vel = (double)pd.velocity / 127.0;                                    // main.rs:1147
        MlpOut corr;                                                                       // no MLP (the --mlp flag is ignored, main.rs:1134)
        for (int i = 0; i < 5; ++i) { corr.cents[i] = 0.0; corr.decay[i] = 1.0; }
        corr.ds = 1.0;
        // amplitudes = mode_amplitudes * dwell * amp_offsets * vel_scale on the detuned f0, seed note * 2654435761 (main.rs:1150-1170):
        // note_on_lane's reed with identity corrections (x 2^(0/1200) and / 1.0 are exact)
        note_on_lane(rec, nt, K, pd.note, vel, (uint32_t)pd.note * 2654435761u, corr);
        // ModalReed::new(.., onset_time_s = 0.0, ..) (reed.rs:159-173): round(0 * sr) = 0 ramp samples, increment 0
        rec[VF_ONSET_N * 64] = bitsd(0ull);
        rec[VF_ONSET_INC * 64] = 0.0;
        rec[VF_NCNT * 64] = bitsd(dbits(rec[VF_NCNT * 64]) & 0xFFFFFFFF00000000ull);     // no attack noise: remaining = 0
        rec[VF_DS * 64] = pd.ds_actual;                                                    // Pickup::new_with_scale(BASE_SR, ds_actual)
        rec[VF_GAIN * 64] = 1.0;                                                           // T2 is the pickup output itself (x 1.0 is exact)
        oscale[lane] = pd.out_scale;
        v.load(rec);
        lcoef_load(lcoef + lane, rec);
    }
    __syncthreads();
    double pk = 0.0;
    for (long long base = 0; base < n; base += OW_VCHUNK) {
        const int cn = (int)((n - base) < OW_VCHUNK ? (n - base) : OW_VCHUNK);
        for (int s = 0; s < cn; ++s) {
            double r = 0.0, y = 0.0;
            // no onset ramp, no attack noise, no damper: the steady step is the whole of the reed (onset 1.0 multiplies exactly)
            if (active) y = v.step<true>(lcoef + lane, nullptr, nullptr, &r);
            const long long i = base + s;
            if (i >= OW_CALIB_WIN_LO && i < OW_CALIB_WIN_HI) pk = fmax(pk, fabs(r));       // peak_abs: fold(0.0, f64::max) of |x|
            tile[lane * (OW_VCHUNK + 1) + s] = y;
            rtile[lane * (OW_VCHUNK + 1) + s] = r;
        }
        __syncthreads();
        // transposed, coalesced stores: 2 point rows per pass (32 samples each)
        for (int r = (lane >> 5); r < 64; r += 2) {
            const int s = lane & 31;
            if (pb + r < n_pts && s < cn) {
                const size_t o = (size_t)(pb + r) * stride + base + s;
                const double y = tile[r * (OW_VCHUNK + 1) + s];
                t2[o] = y;
                t3[o] = y * oscale[r];                                                     // main.rs:1186
                if (t1) t1[o] = rtile[r * (OW_VCHUNK + 1) + s];
            }
        }
        __syncthreads();
    }
    if (active) t1_peak[p] = pk;
}

// T5 (main.rs:1210-1222) at the base rate.  mode CALIB_OUT_FULL: dst = speaker(power_amp(src x vol x vol)) x PSG;
// CALIB_OUT_ATT: dst = src x vol x vol (the melange power amp's input); CALIB_OUT_SPEAKER: dst = speaker(src) x PSG (its output).
enum { CALIB_OUT_FULL = 0, CALIB_OUT_ATT = 1, CALIB_OUT_SPEAKER = 2 };
__global__ __launch_bounds__(64) void k_calib_out(const OwConsts* __restrict__ K, const double* __restrict__ src, double* __restrict__ dst,
                                                  double volume, double speaker, int n_pts, long long n, long long stride, int mode) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pts) return;
    const double* x = src + (size_t)p * stride;
    double* y = dst + (size_t)p * stride;
    if (mode == CALIB_OUT_ATT) {
        for (long long i = 0; i < n; ++i) y[i] = x[i] * volume * volume;              // audio taper
        return;
    }
    SpeakerSt sp = speaker_fresh(K->sr, speaker);                                      // at BASE_SR
    for (long long i = 0; i < n; ++i) {
        const double amp = mode == CALIB_OUT_FULL ? power_amp(x[i] * volume * volume) : x[i];
        y[i] = speaker_process(sp, amp, K->spk_thermal_alpha) * 7.498942093324558;        // tables::POST_SPEAKER_GAIN
    }
}

// One workgroup per (point, stage): over the window [4410, 17640) of row rows[stage] + point * stride -- the peak of |x|, the sum of
// squares and, where dft_mask has the stage's bit, the two single-bin DFTs of dft_magnitude (main.rs:893-903) at f0 and 2 f0 with the
// reference's phase 2 pi f i / sr per sample (no recurrence).  out: [n_pts][4][CALIB_MET_COUNT] (T2..T5), this launch's rows at stage0 +
// blockIdx.y; the finish (dB, floors) is host work.  (Like k_audit_dft: four wavefronts, lane-strided sums, a fixed reduction tree.)
struct CalibMetRows { const double* rows[4]; };
__global__ __launch_bounds__(256) void k_calib_metrics(CalibMetRows a, const OwCalibDev* __restrict__ pts, long long stride, double sr,
                                                       uint32_t dft_mask, int stage0, double* __restrict__ out) {
    __shared__ double red[CALIB_MET_COUNT][4];
    const int p = blockIdx.x, stage = blockIdx.y;
    const double* x = a.rows[stage] + (size_t)p * stride + OW_CALIB_WIN_LO;
    const uint32_t n = OW_CALIB_WIN_HI - OW_CALIB_WIN_LO;
    const bool dft = (dft_mask >> stage) & 1u;
    const double f = pts[p].f0;
    const double tpf1 = 2.0 * 3.14159265358979323846 * f;                              // 2.0 * PI * freq (then * i / sr)
    const double tpf2 = 2.0 * 3.14159265358979323846 * (2.0 * f);
    double v[CALIB_MET_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const double s = x[i];
        v[CALIB_MET_PEAK] = fmax(v[CALIB_MET_PEAK], fabs(s));
        v[CALIB_MET_SUMSQ] += s * s;
        if (dft) {
            double sn, cs;
            sincos(tpf1 * (double)i / sr, &sn, &cs);
            v[CALIB_MET_RE1] += s * cs;
            v[CALIB_MET_IM1] -= s * sn;
            sincos(tpf2 * (double)i / sr, &sn, &cs);
            v[CALIB_MET_RE2] += s * cs;
            v[CALIB_MET_IM2] -= s * sn;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        v[CALIB_MET_PEAK] = fmax(v[CALIB_MET_PEAK], __shfl_down(v[CALIB_MET_PEAK], off));
        for (int k = 1; k < CALIB_MET_COUNT; ++k) v[k] += __shfl_down(v[k], off);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < CALIB_MET_COUNT; ++k) red[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
    if (threadIdx.x < CALIB_MET_COUNT) {
        const int k = threadIdx.x;
        const double r = k == CALIB_MET_PEAK ? fmax(fmax(red[k][0], red[k][1]), fmax(red[k][2], red[k][3]))
                                             : (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        out[((size_t)p * 4 + stage0 + stage) * CALIB_MET_COUNT + k] = r;
    }
}

}  // namespace owdev
