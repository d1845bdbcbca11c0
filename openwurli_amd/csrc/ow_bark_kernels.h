// openwurli-hip: bark-audit kernels (`preamp-bench bark-audit`, tools/preamp-bench/src/main.rs:551-664): H2 / H1 of a note at the reed,
// behind the pickup and behind the preamp.
//
//   k_bark_voice      lane = job: ModalReed::new(.., onset 0, ..) -> Pickup::new_with_scale(the table's displacement scale), k_calib_voice's
//                     stage without a calibration config.  Writes the pickup row, the reed row only when taps were asked for; peak_abs of
//                     both over the measuring window is reduced in registers.  Bound by the voice step's serial arithmetic, as k_job_voice.
//   k_bark_chain_row  legacy preamp, a row of sixteen lanes per solver state (k_job_chain_row's role split): wavefronts 0-3 run the
//                     up-sampler and dk_step_row for main and shadow of two jobs each, wavefront 4 follows one chunk behind with the
//                     half-band down-sampler alone and writes the preamp row -- process_oversampled (main.rs:961-974), no volume, power amp
//                     or speaker.  Bound by the serial latency of one chain step.
//   (the melange preamp, and legacy grids too large for the row form: k_job_chain<MEL> in JOB_OUT_PA_INPUT mode at volume 1.0,
//    ow_job_kernels.h; the four magnitudes: k_dft_probes, ow_note_audit_kernels.h)
#pragma once
#include "ow_chain_row.h"
#include "ow_job_kernels.h"

namespace owdev {

enum { BARK_ST_REED_PEAK = 0, BARK_ST_PU_PEAK = 1, BARK_ST_DS = 2, BARK_ST_COUNT = 3 };

// cmd_bark_audit's stages 1 and 2 (main.rs:584-622) for n samples.  reed may be nullptr.  stats [n_jobs][BARK_ST_COUNT]: peak_abs(reed[m0..]),
// peak_abs(pu[m0..]) and the displacement scale the pickup ran with (tables::pickup_displacement_scale(note), the note table's entry).
__global__ __launch_bounds__(64) void k_bark_voice(const OwConsts* __restrict__ K, const double* __restrict__ nt, double* __restrict__ vrec,
                                                   const OwJobDev* __restrict__ jobs, double* __restrict__ reed, double* __restrict__ pu,
                                                   double* __restrict__ stats, int n_jobs, long long n, long long m0, long long stride) {
    __shared__ double tile[64 * (OW_VCHUNK + 1)];
    __shared__ double rtile[64 * (OW_VCHUNK + 1)];
    __shared__ double lcoef[OW_LCOEF_ROWS * 64];
    const int lane = threadIdx.x;
    const int jb = blockIdx.x * 64;
    const int j = jb + lane;
    const bool active = j < n_jobs;
    double* rec = vrec + (size_t)blockIdx.x * OW_VREC_DOUBLES + lane;
    VoiceRegs v;
    double ds = 0.0;
    if (active) {
        const OwJobDev jd = jobs[j];
        const double vel = (double)jd.velocity / 127.0;                                    // main.rs:582
        MlpOut corr;                                                                       // no MLP
        for (int i = 0; i < 5; ++i) { corr.cents[i] = 0.0; corr.decay[i] = 1.0; }
        corr.ds = 1.0;
        // amplitudes = mode_amplitudes * dwell * amp_offsets * vel_scale on the detuned f0, seed note * 2654435761 (main.rs:585-605):
        // note_on_lane's reed with identity corrections (x 2^(0/1200) and / 1.0 are exact), as k_calib_voice
        note_on_lane(rec, nt, K, jd.note, vel, (uint32_t)jd.note * 2654435761u, corr);
        // ModalReed::new(.., onset_time_s = 0.0, ..) (reed.rs:159-173): round(0 * sr) = 0 ramp samples, increment 0
        rec[VF_ONSET_N * 64] = bitsd(0ull);
        rec[VF_ONSET_INC * 64] = 0.0;
        rec[VF_NCNT * 64] = bitsd(dbits(rec[VF_NCNT * 64]) & 0xFFFFFFFF00000000ull);     // no attack noise: remaining = 0
        rec[VF_GAIN * 64] = 1.0;                                                           // the pickup output itself (x 1.0 is exact)
        ds = rec[VF_DS * 64];                                                              // Pickup::new_with_scale(BASE_SR, the table's scale x 1.0)
        v.load(rec);
        lcoef_load(lcoef + lane, rec);
    }
    __syncthreads();
    double rpk = 0.0, ppk = 0.0;
    for (long long base = 0; base < n; base += OW_VCHUNK) {
        const int cn = (int)((n - base) < OW_VCHUNK ? (n - base) : OW_VCHUNK);
        for (int s = 0; s < cn; ++s) {
            double r = 0.0, y = 0.0;
            if (active) y = v.step<true>(lcoef + lane, nullptr, nullptr, &r);
            if (base + s >= m0) {                                                          // peak_abs: fold(0.0, f64::max) of |x| -- order-free
                rpk = fmax(rpk, fabs(r));
                ppk = fmax(ppk, fabs(y));
            }
            tile[lane * (OW_VCHUNK + 1) + s] = y;
            rtile[lane * (OW_VCHUNK + 1) + s] = r;
        }
        __syncthreads();
        // transposed, coalesced stores: 2 job rows per pass (32 samples each)
        for (int r = (lane >> 5); r < 64; r += 2) {
            const int s = lane & 31;
            if (jb + r < n_jobs && s < cn) {
                const size_t o = (size_t)(jb + r) * stride + base + s;
                pu[o] = tile[r * (OW_VCHUNK + 1) + s];
                if (reed) reed[o] = rtile[r * (OW_VCHUNK + 1) + s];
            }
        }
        __syncthreads();
    }
    if (active) {
        double* o = stats + (size_t)j * BARK_ST_COUNT;
        o[BARK_ST_REED_PEAK] = rpk; o[BARK_ST_PU_PEAK] = ppk; o[BARK_ST_DS] = ds;
    }
}

// k_job_chain<false> in JOB_OUT_PA_INPUT mode with the row step: eight jobs per workgroup, wavefronts 0-3 = up-sampler + the two preamp
// steps of a sample for two jobs each (rows 0-1 main, rows 2-3 shadow), wavefront 4 = the down-sampler, one lane per job, a chunk behind.
// Same statements per job in the same order as that kernel (x volume x volume included: 1.0 for bark-audit): bit-identical
// (tests/test_gpu_bark_audit.py, OW_BARK_ROW=0/1).  The hand-over is k_job_chain_row's: a two-slot LDS ring, one workgroup barrier per chunk.
__global__ __launch_bounds__(320) void k_bark_chain_row(const OwConsts* __restrict__ K, const OwJobDev* __restrict__ jobs, const double* __restrict__ in,
                                                        double* __restrict__ out, int n_jobs, long long n, long long stride) {
    __shared__ double tin[8 * (OW_FCHUNK + 1)];
    __shared__ double ring[2][OW_FCHUNK * 2][8];               // preamp out at the chain rate: [slot][sample x phase][job of the block]
    __shared__ double tout[8 * (OW_FCHUNK + 1)];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int jb = blockIdx.x * 8;
    const int osr = K->oversample ? 2 : 1;
    const long long n_chunks = (n + OW_FCHUNK - 1) / OW_FCHUNK;

    if (wv < 4) {
        const int row = lane >> 4, role = row >> 1;
        const int jl = 2 * wv + (row & 1);
        const int j = jb + jl;
        const bool valid = j < n_jobs;
        const OwJobDev jd = jobs[valid ? j : n_jobs - 1];
        DkRowK R;
        dk_row_consts(R, K, lane);
        DkSt st;
        double r_ldr = 1000000.0, g_ldr = 1.0 / 1000000.0, g_prev = g_ldr;
        double us[3] = {0, 0, 0};
        dk_dc_reset(K, r_ldr, st);                               // DkPreamp::new(preamp_sr); set_ldr_resistance(r_ldr)  (main.rs:628-629)
        {
            const double r_new = fmax(jd.r_ldr, 1000.0);
            if (fabs(r_new - r_ldr) > 0.01) { r_ldr = r_new; g_ldr = 1.0 / r_new; }
        }
        const double sgn = role ? -1.0 : 1.0;
        auto preamp_step = [&](double x) -> double {
            const double o = dk_step_row(st, R, lane, x, g_ldr, g_prev);
            g_prev = g_ldr;
            const double other = xor32(o);
            double res = (o - other) * sgn;
            if (!isfinite(res)) {
                dk_dc_reset(K, r_ldr, st); g_ldr = 1.0 / r_ldr; g_prev = g_ldr;
                res = 0.0;
            }
            return res;
        };
        const int f_jl = 2 * wv + ((lane >> 4) & 1), f_n = lane & 15;
        for (long long c = 0; c <= n_chunks; ++c) {
            if (c < n_chunks) {
                const long long base = c * OW_FCHUNK;
                const int cn = (int)((n - base) < OW_FCHUNK ? (n - base) : OW_FCHUNK);
                if (lane < 32) {
                    double x = 0.0;
                    if (jb + f_jl < n_jobs && f_n < cn) x = in[(size_t)(jb + f_jl) * stride + base + f_n];
                    tin[f_jl * (OW_FCHUNK + 1) + f_n] = x;
                }
                OW_WAVE_SYNC();
                double (*slot)[8] = ring[c & 1];
                for (int sidx = 0; sidx < cn; ++sidx) {
                    const double x = tin[jl * (OW_FCHUNK + 1) + sidx];
                    if (osr == 2) {                                  // main.rs:961-974: per-sample up(1) -> 2x process (-> down(1) on the output wavefront)
                        const double y = allpass3(R.oc0, R.oc1, R.oc2, us, x);      // branch A on even lanes, B on odd ones
                        const double xin[2] = {role ? 0.0 : rowb<0>(y), role ? 0.0 : rowb<1>(y)};
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            const double pk = preamp_step(xin[k]);
                            if (role == 0 && (lane & 15) == 0) slot[sidx * 2 + k][jl] = pk;
                        }
                    } else {
                        const double pk = preamp_step(role ? 0.0 : x);
                        if (role == 0 && (lane & 15) == 0) slot[sidx * 2][jl] = pk;
                    }
                }
            }
            __syncthreads();
        }
        return;
    }

    // ---- the down-sampling wavefront: lanes 0..7 own a job each, the others shadow them
    const int jl = lane & 7;
    const int j = jb + jl;
    const bool valid = j < n_jobs;
    const OwJobDev jd = jobs[valid ? j : n_jobs - 1];
    double da[3] = {0, 0, 0}, db[3] = {0, 0, 0}, dd = 0.0;
    const double vol2_a = jd.volume;
    for (long long c = 0; c <= n_chunks; ++c) {
        if (c >= 1) {
            const long long base = (c - 1) * OW_FCHUNK;
            const int cn = (int)((n - base) < OW_FCHUNK ? (n - base) : OW_FCHUNK);
            const double (*slot)[8] = ring[(c - 1) & 1];
            for (int sidx = 0; sidx < cn; ++sidx) {
                double pre;
                if (osr == 2) {
                    const double fa = allpass3(OW_OS_A0, OW_OS_A1, OW_OS_A2, da, slot[sidx * 2][jl]);
                    const double fb = allpass3(OW_OS_B0, OW_OS_B1, OW_OS_B2, db, slot[sidx * 2 + 1][jl]);
                    pre = (fa + dd) * 0.5;
                    dd = fb;
                } else {
                    pre = slot[sidx * 2][jl];
                }
                const double att = pre * vol2_a * vol2_a;           // JOB_OUT_PA_INPUT's value
                if (lane < 8) tout[jl * (OW_FCHUNK + 1) + sidx] = att;
            }
            OW_WAVE_SYNC();
            for (int k = lane; k < 8 * OW_FCHUNK; k += 64) {
                const int r = k / OW_FCHUNK, sm = k - r * OW_FCHUNK;
                if (jb + r < n_jobs && sm < cn) out[(size_t)(jb + r) * stride + base + sm] = tout[r * (OW_FCHUNK + 1) + sm];
            }
            OW_WAVE_SYNC();
        }
        __syncthreads();
    }
}

}  // namespace owdev
