// openwurli-hip: `preamp-bench render-poly` kernels (tools/preamp-bench/src/main.rs:1397-1592) for many chords at once.
//
// A chord of n notes is n + 1 independent serial chains: the voices' sum through ONE chain (`final`) and every voice through a chain of
// its OWN (their outputs added in voice order: `separate_sum`); residual = final - separate_sum is the chord's intermodulation.  Each
// chain is a fresh legacy preamp after set_ldr_resistance(r) THEN reset() -- the DC solve runs at the chord's --ldr, the opposite order
// of `render` (k_job_chain) -- with per-sample 2x oversampling -> x volume^2 -> optional power amp at BASE rate -> Speaker(character) ->
// x POST_SPEAKER_GAIN, f64.
//
//   k_poly_voice   lane = voice, k_job_voice's loop with the command's seed note * 2654435761 + i and the MLP on.
//   k_poly_chain   lane pair (chain, main|shadow) as k_job_chain: 32 chain slots per wavefront.  The host packs the chords so that none
//                  straddles a wavefront: a chord's shared chain sits in slot s0, its voices' chains in s0 + 1 .. s0 + n.  The shared
//                  chain's input is summed from the voice rows while they are staged through LDS; after each staged chunk the chord's
//                  shared-chain lane walks the chunk in sample order, forms separate_sum and residual and carries the whole-render peaks
//                  and the window's peak / sum of squares -- the reference's own (sequential) summation order.
#pragma once
#include "ow_job_kernels.h"

namespace owdev {

struct OwPolyVoiceDev { uint8_t note, velocity, pad[2]; uint32_t seed; };   // one voice row
struct OwPolyChordDev {      // one chord (host: ow_poly_chord)
    double volume, speaker, r_ldr;
    int32_t n_notes, no_poweramp;
    int32_t voice_row0;      // first of its n_notes rows in the chunk's voice block
    int32_t pad;
};
// one chain slot of a wavefront: the chord (index in the chunk, -1: empty slot) and which of its chains (0: shared, k: voice k - 1)
struct OwPolySlotDev { int32_t chord, k; };

// per chord: whole-render peaks of final / residual, then window peak and window sum of squares of final, separate_sum, residual
enum { POLY_MET_PEAK = 0, POLY_MET_RES_PEAK = 1, POLY_MET_WPK = 2, POLY_MET_WSS = 5, POLY_MET_COUNT = 8 };
#define OW_POLY_WIN_LO 8820       // (0.2 * BASE_SR) as usize (main.rs:1516)
#define OW_POLY_WIN_HI 88200      // (2.0 * BASE_SR) (main.rs:1517), min(.., n) by the caller

// Voice::note_on(note, vel / 127, 44100, note * 2654435761 + i, mlp = true) + Voice::render for n samples (main.rs:1435-1449), lane = voice.
__global__ __launch_bounds__(64) void k_poly_voice(const OwConsts* __restrict__ K, const double* __restrict__ nt, double* __restrict__ vrec,
                                                   const OwPolyVoiceDev* __restrict__ voices, double* __restrict__ reed, int n_voices, long long n,
                                                   long long stride) {
    __shared__ double tile[64 * (OW_VCHUNK + 1)];
    __shared__ double lcoef[OW_LCOEF_ROWS * 64];
    const int lane = threadIdx.x;
    const int vb = blockIdx.x * 64;
    const bool active = vb + lane < n_voices;
    double* rec = vrec + (size_t)blockIdx.x * OW_VREC_DOUBLES + lane;
    VoiceRegs v;
    if (active) {
        const OwPolyVoiceDev vd = voices[vb + lane];
        const int note = vd.note;                                          // 33..96: the host refuses the others
        const double vel = (double)vd.velocity / 127.0;                    // main.rs:1436
        double raw[11];
        mlp_raw_scalar(clampd(((double)note - 21.0) / (108.0 - 21.0), 0.0, 1.0), clampd(vel, 0.0, 1.0), raw);
        const MlpOut corr = mlp_finish(note, raw, true);
        note_on_lane(rec, nt, K, note, vel, vd.seed, corr);                // main.rs:1437-1440
        v.load(rec);
        lcoef_load(lcoef + lane, rec);
    }
    for (long long base = 0; base < n; base += OW_VCHUNK) {
        const int cn = (int)((n - base) < OW_VCHUNK ? (n - base) : OW_VCHUNK);
        for (int s = 0; s < cn; ++s) tile[lane * (OW_VCHUNK + 1) + s] = active ? v.step<false>(lcoef + lane) : 0.0;
        __syncthreads();
        for (int r = (lane >> 5); r < 64; r += 2) {                        // transposed, coalesced store: 2 voice rows per pass
            const int s = lane & 31;
            if (vb + r < n_voices && s < cn) reed[(size_t)(vb + r) * stride + base + s] = tile[r * (OW_VCHUNK + 1) + s];
        }
        __syncthreads();
    }
}

// The chains of the chords of one wavefront.  slots: [blocks][32].  fin / sep / res: NULL or [chords][stride] rows of the chunk.
// met: [chords][POLY_MET_COUNT].  win_hi = min(OW_POLY_WIN_HI, n).
__global__ __launch_bounds__(64) void k_poly_chain(const OwConsts* __restrict__ K, const OwPolyChordDev* __restrict__ chords,
                                                   const OwPolySlotDev* __restrict__ slots, const double* __restrict__ reed, double* __restrict__ fin,
                                                   double* __restrict__ sep, double* __restrict__ res, double* __restrict__ met, long long n,
                                                   long long stride, long long win_hi) {
    __shared__ double tin[32 * (OW_PCHUNK + 1)];
    __shared__ double tout[32 * (OW_PCHUNK + 1)];
    __shared__ int s_row[32];        // voice row the slot reads (-1: none), per slot
    __shared__ int s_cnt[32];        // shared-chain slots: the chord's n_notes; others 0
    __shared__ int s_chord[32];      // shared-chain slots: the chord; others -1
    const int lane = threadIdx.x;
    const int jl = lane & 31, role = lane >> 5;
    const OwPolySlotDev sl = slots[(size_t)blockIdx.x * 32 + jl];
    const bool valid = sl.chord >= 0;
    const OwPolyChordDev cd = chords[valid ? sl.chord : slots[(size_t)blockIdx.x * 32].chord];    // slot 0 of a block is never empty
    if (role == 0) {
        s_row[jl] = (valid && sl.k > 0) ? cd.voice_row0 + sl.k - 1 : -1;
        s_cnt[jl] = (valid && sl.k == 0) ? cd.n_notes : 0;
        s_chord[jl] = (valid && sl.k == 0) ? sl.chord : -1;
    }
    const double sr = K->sr;

    // DkPreamp::new(OVERSAMPLED_SR); set_ldr_resistance(r_ldr); reset()  (main.rs:1462-1464, dk_preamp_legacy.rs:620-640): the clamp to
    // 1 kohm and the 0.01 ohm hysteresis against new()'s 1 Mohm, then the DC solve at THAT resistance
    DkSt st;
    double r_ldr = 1000000.0;
    {
        const double r_new = fmax(cd.r_ldr, 1000.0);
        if (fabs(r_new - r_ldr) > 0.01) r_ldr = r_new;
    }
    dk_dc_reset(K, r_ldr, st);
    double g_ldr = 1.0 / r_ldr, g_prev = g_ldr;
    // one preamp sample for this lane's state (main: audio, shadow: 0.0): main - pump, the NaN reset on the chain's own two states
    auto preamp_step = [&](double x) -> double {
        const double o = dk_step(st, x, g_ldr, g_prev, K);
        g_prev = g_ldr;
        const double other = xor32_t(o);
        double r = role ? (other - o) : (o - other);
        if (!isfinite(r)) {
            dk_dc_reset(K, r_ldr, st); g_ldr = 1.0 / r_ldr; g_prev = g_ldr;
            r = 0.0;
        }
        return r;
    };
    double ua[3] = {0, 0, 0}, ub[3] = {0, 0, 0}, da[3] = {0, 0, 0}, db[3] = {0, 0, 0}, dd = 0.0;
    SpeakerSt sp = speaker_fresh(sr, cd.speaker);      // at BASE_SR (main.rs:1471-1472)
    const double vol = cd.volume;
    const bool walker = valid && sl.k == 0 && role == 0;      // the chord's one lane that recombines its chains
    const int nn = cd.n_notes;
    double pk = 0.0, rpk = 0.0, wpk[3] = {0, 0, 0}, wss[3] = {0, 0, 0};
    __syncthreads();

    for (long long base = 0; base < n; base += OW_PCHUNK) {
        const int cn = (int)((n - base) < OW_PCHUNK ? (n - base) : OW_PCHUNK);
        // stage the voice rows (lane = sample of the chunk) ...
        for (int r = 0; r < 32; ++r) {
            const int row = s_row[r];
            double x = 0.0;
            if (row >= 0 && lane < cn) x = reed[(size_t)row * stride + base + lane];
            tin[r * (OW_PCHUNK + 1) + lane] = x;
        }
        // ... and every shared chain's input from them, in voice order (sum_buf[j] += voice_buf[j], main.rs:1452-1454); a lane reads
        // back the column it wrote
        for (int r = 0; r < 32; ++r) {
            const int c = s_cnt[r];
            if (c == 0) continue;
            double s = 0.0;
            for (int k = 1; k <= c; ++k) s += tin[(r + k) * (OW_PCHUNK + 1) + lane];
            tin[r * (OW_PCHUNK + 1) + lane] = s;
        }
        __syncthreads();
        for (int s = 0; s < cn; ++s) {
            const double x = tin[jl * (OW_PCHUNK + 1) + s];
            // process_oversampled (main.rs:961-974): per sample up(1) -> 2x process_sample -> down(1)
            const double a = allpass3(OW_OS_A0, OW_OS_A1, OW_OS_A2, ua, x);
            const double b = allpass3(OW_OS_B0, OW_OS_B1, OW_OS_B2, ub, x);
            double p[2];
            const double in[2] = {role ? 0.0 : a, role ? 0.0 : b};
            for (int k = 0; k < 2; ++k) p[k] = preamp_step(in[k]);
            const double fa = allpass3(OW_OS_A0, OW_OS_A1, OW_OS_A2, da, p[0]);
            const double fb = allpass3(OW_OS_B0, OW_OS_B1, OW_OS_B2, db, p[1]);
            const double pre = (fa + dd) * 0.5;
            dd = fb;
            // main.rs:1475-1483: volume^2 (audio taper) -> optional power amp at base rate -> speaker -> POST_SPEAKER_GAIN
            const double att = pre * vol * vol;
            const double amp = cd.no_poweramp ? att : power_amp(att);
            const double y = speaker_process(sp, amp, K->spk_thermal_alpha) * 7.498942093324558;
            if (role == 0) tout[jl * (OW_PCHUNK + 1) + s] = y;
        }
        __syncthreads();
        // the chord's lane, in sample order: separate_sum[i] += ..., residual[i] = final[i] - separate_sum[i] (main.rs:1486-1513), the
        // whole-render peaks (:1530, :1543) and the window figures (peak_abs / the sum of rms_db, :912-927, over [8820, win_hi)).
        // separate_sum and residual go to the (consumed) input tile's first two rows of the chord for the coalesced store.
        if (walker) {
            for (int s = 0; s < cn; ++s) {
                const double f = tout[jl * (OW_PCHUNK + 1) + s];
                double ss = 0.0;
                for (int k = 1; k <= nn; ++k) ss += tout[(jl + k) * (OW_PCHUNK + 1) + s];
                const double rs = f - ss;
                tin[jl * (OW_PCHUNK + 1) + s] = ss;
                tin[(jl + 1) * (OW_PCHUNK + 1) + s] = rs;
                pk = fmax(pk, fabs(f));
                rpk = fmax(rpk, fabs(rs));
                const long long i = base + s;
                if (i >= OW_POLY_WIN_LO && i < win_hi) {
                    wpk[0] = fmax(wpk[0], fabs(f)); wpk[1] = fmax(wpk[1], fabs(ss)); wpk[2] = fmax(wpk[2], fabs(rs));
                    wss[0] += f * f; wss[1] += ss * ss; wss[2] += rs * rs;
                }
            }
        }
        __syncthreads();
        if (fin || sep || res)
            for (int r = 0; r < 32; ++r) {
                const int c = s_chord[r];
                if (c < 0 || lane >= cn) continue;
                const size_t o = (size_t)c * stride + base + lane;
                if (fin) fin[o] = tout[r * (OW_PCHUNK + 1) + lane];
                if (sep) sep[o] = tin[r * (OW_PCHUNK + 1) + lane];
                if (res) res[o] = tin[(r + 1) * (OW_PCHUNK + 1) + lane];
            }
        __syncthreads();
    }
    if (walker) {
        double* m = met + (size_t)sl.chord * POLY_MET_COUNT;
        m[POLY_MET_PEAK] = pk; m[POLY_MET_RES_PEAK] = rpk;
        for (int q = 0; q < 3; ++q) { m[POLY_MET_WPK + q] = wpk[q]; m[POLY_MET_WSS + q] = wss[q]; }
    }
}

}  // namespace owdev
