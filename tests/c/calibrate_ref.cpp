// Test-side CPU restatement of `preamp-bench calibrate` (tools/preamp-bench/src/main.rs:1128-1262) over the oracle's headers, which it
// includes unchanged: run_calibrate and its helpers (peak_abs, peak_db, rms_db, dft_magnitude, h2_h1_ratio_db, to_dbfs,
// process_oversampled) and the two `_with_config` table functions (tables.rs:283-288, 578-620), in the reference's statement order.
// tests/test_calibrate_host.py builds it with the oracle Makefile's flags and loads it with ctypes; it is the checker of ow_calibrate.
#include "ow_tables.hpp"
#include "ow_voice.hpp"
#include "ow_chain.hpp"
#include "ow_melange.hpp"
#include "ow_power_amp.hpp"

#include <cmath>
#include <vector>

using namespace owo;

namespace {
const double BASE_SR = 44100.0;                  // main.rs:27
const double OVERSAMPLED_SR = BASE_SR * 2.0;     // main.rs:28

struct CalibrationConfig {                       // tables.rs:254-277
    double ds_at_c4, ds_exponent, ds_clamp_lo, ds_clamp_hi, target_db, voicing_slope;
    bool zero_trim;
};

double pickup_displacement_scale_with_config(int midi, const CalibrationConfig& cfg) {   // tables.rs:283-288
    const double c = reed_compliance(midi);
    const double c_ref = reed_compliance(60);
    const double ds = cfg.ds_at_c4 * std::pow(c / c_ref, cfg.ds_exponent);
    return rclamp(ds, cfg.ds_clamp_lo, cfg.ds_clamp_hi);
}

double output_scale_with_config(int midi, double velocity_norm, const CalibrationConfig& cfg) {   // tables.rs:578-620
    const double HPF_FC = 2312.0;
    const double ds = pickup_displacement_scale_with_config(midi, cfg);
    const double f0 = midi_to_freq(midi);
    const double scurve_v = velocity_scurve(velocity_norm);
    const double vel_scale = std::pow(scurve_v, velocity_exponent(midi));
    const double vel_scale_c4 = std::pow(scurve_v, velocity_exponent(60));
    const double effective_ds = std::fmax(ds * vel_scale, 1e-6);
    const double effective_ds_ref = std::fmax(cfg.ds_at_c4 * vel_scale_c4, 1e-6);
    const double rms = pickup_rms_proxy(effective_ds, f0, HPF_FC);
    const double rms_ref = pickup_rms_proxy(effective_ds_ref, midi_to_freq(60), HPF_FC);
    const double flat_db = -20.0 * std::log10(rms / rms_ref);
    const double voicing_db = cfg.voicing_slope * std::fmax((double)midi - 60.0, 0.0);
    const double trim = cfg.zero_trim ? 0.0 : register_trim_db(midi);
    const double vel_blend = std::pow(velocity_norm, 1.3);
    const double effective_trim = trim * vel_blend;
    return std::pow(10.0, (cfg.target_db + flat_db + voicing_db + effective_trim) / 20.0);
}

double dft_magnitude(const double* signal, size_t len, double freq, double sr) {          // main.rs:893-903
    const double n = (double)len;
    double re = 0.0, im = 0.0;
    for (size_t i = 0; i < len; ++i) {
        const double phase = 2.0 * PI_ * freq * (double)i / sr;
        re += signal[i] * std::cos(phase);
        im -= signal[i] * std::sin(phase);
    }
    return 2.0 * std::sqrt((re / n) * (re / n) + (im / n) * (im / n));
}
double peak_abs(const double* s, size_t n) {                                               // main.rs:910-912
    double m = 0.0;
    for (size_t i = 0; i < n; ++i) m = std::fmax(m, std::fabs(s[i]));
    return m;
}
double to_dbfs(double val) { return val > 1e-15 ? 20.0 * std::log10(val) : -120.0; }      // main.rs:2241-2247
double peak_db(const double* s, size_t n) { return to_dbfs(peak_abs(s, n)); }              // main.rs:914-916
double rms_db(const double* s, size_t n) {                                                 // main.rs:918-927
    double sum = 0.0;
    for (size_t i = 0; i < n; ++i) sum += s[i] * s[i];
    const double mean_sq = sum / (double)n;
    return mean_sq > 0.0 ? 10.0 * std::log10(mean_sq) : -120.0;
}
double h2_h1_ratio_db(const double* s, size_t n, double fundamental_hz, double sr) {       // main.rs:929-937
    const double h1 = dft_magnitude(s, n, fundamental_hz, sr);
    const double h2 = dft_magnitude(s, n, 2.0 * fundamental_hz, sr);
    return h1 > 1e-15 ? 20.0 * std::log10(h2 / h1) : -120.0;
}

// the PreampModel `create_preamp` returns (main.rs:133-148): legacy 8-node or melange 12-node at OVERSAMPLED_SR
struct AnyPreamp {
    int kind;
    DkPreamp legacy;
    MelangePreamp mel;
    explicit AnyPreamp(int k) : kind(k) { if (kind) mel.init(OVERSAMPLED_SR); else legacy.init(OVERSAMPLED_SR); }
    void set_ldr_resistance(double r) { if (kind) mel.set_ldr_resistance(r); else legacy.set_ldr_resistance(r); }
    double process_sample(double x) { return kind ? mel.process_sample(x) : legacy.process_sample(x); }
};

std::vector<double> process_oversampled(const std::vector<double>& input, AnyPreamp& preamp) {   // main.rs:961-974
    const size_t n = input.size();
    Oversampler os;
    std::vector<double> out(n, 0.0);
    for (size_t i = 0; i < n; ++i) {
        double up[2] = {0.0, 0.0};
        os.upsample_2x(&input[i], 1, up);
        const double processed[2] = {preamp.process_sample(up[0]), preamp.process_sample(up[1])};
        double down[1] = {0.0};
        os.downsample_2x(processed, down, 1);
        out[i] = down[0];
    }
    return out;
}
}  // namespace

extern "C" {
double ocal_pickup_displacement_scale(int midi, const double* cfg6, int zero_trim) {
    const CalibrationConfig c{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5], zero_trim != 0};
    return pickup_displacement_scale_with_config(midi, c);
}
double ocal_output_scale(int midi, double velocity_norm, const double* cfg6, int zero_trim) {
    const CalibrationConfig c{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5], zero_trim != 0};
    return output_scale_with_config(midi, velocity_norm, c);
}

// One (note, velocity) of run_calibrate's loop.  cfg6: ds_at_c4, ds_exponent, ds_clamp lo, hi, target_db, voicing_slope.
// row18: the CalibrateRow fields after midi / velocity, in order.  taps: NULL or [5][22050] (T1..T5).
void ocal_run_point(int note, int vel_byte, const double* cfg6, int zero_trim, double volume, double speaker_char, int preamp_kind,
                    int power_amp_kind, double* row18, double* taps) {
    const CalibrationConfig cfg{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5], zero_trim != 0};
    const double duration = 0.5;
    const size_t measure_start = (size_t)(0.100 * BASE_SR);
    const size_t measure_end = (size_t)(0.400 * BASE_SR);
    const size_t wn = measure_end - measure_start;

    const NoteParams params = note_params(note);
    const double freq = params.fundamental_hz;
    const double ds_actual = pickup_displacement_scale_with_config(note, cfg);
    const double velocity = (double)vel_byte / 127.0;

    // T1: raw reed
    const double detuned = params.fundamental_hz * freq_detune((uint8_t)note);
    double dwell[NUM_MODES], amp_offsets[NUM_MODES], amplitudes[NUM_MODES];
    dwell_attenuation(velocity, detuned, params.mode_ratios, dwell);
    mode_amplitude_offsets((uint8_t)note, amp_offsets);
    const double vel_exp = velocity_exponent(note);
    const double vel_scale = std::pow(velocity_scurve(velocity), vel_exp);
    for (int i = 0; i < NUM_MODES; ++i) amplitudes[i] = params.mode_amplitudes[i] * dwell[i] * amp_offsets[i] * vel_scale;
    ModalReed reed;
    reed.init(detuned, params.mode_ratios, amplitudes, params.mode_decay_rates, 0.0, velocity, BASE_SR, (uint32_t)note * 2654435761u);
    const size_t n_samples = (size_t)(duration * BASE_SR);
    std::vector<double> reed_buf(n_samples, 0.0);
    reed.render(reed_buf.data(), n_samples);
    const double reed_peak = peak_abs(&reed_buf[measure_start], wn);
    const double y_peak = reed_peak * ds_actual;

    // T2: after the pickup
    Pickup pickup;
    pickup.init(BASE_SR);
    pickup.displacement_scale = ds_actual;
    std::vector<double> t2_buf = reed_buf;
    pickup.process(t2_buf.data(), n_samples);
    const double* t2w = &t2_buf[measure_start];
    const double t2_pk = peak_db(t2w, wn), t2_rm = rms_db(t2w, wn), t2_h2 = h2_h1_ratio_db(t2w, wn, freq, BASE_SR);

    // T3: after output_scale
    const double out_scale = output_scale_with_config(note, velocity, cfg);
    std::vector<double> t3_buf(n_samples);
    for (size_t i = 0; i < n_samples; ++i) t3_buf[i] = t2_buf[i] * out_scale;
    const double* t3w = &t3_buf[measure_start];
    const double t3_pk = peak_db(t3w, wn), t3_rm = rms_db(t3w, wn);

    // T4: after the preamp (oversampled): new() + set_ldr_resistance(1e6), no reset()
    AnyPreamp preamp(preamp_kind);
    preamp.set_ldr_resistance(1000000.0);
    const std::vector<double> t4_buf = process_oversampled(t3_buf, preamp);
    const double* t4w = &t4_buf[measure_start];
    const double t4_pk = peak_db(t4w, wn), t4_rm = rms_db(t4w, wn), t4_h2 = h2_h1_ratio_db(t4w, wn, freq, BASE_SR);

    // T5: volume + power amp + speaker at the base rate
    PowerAmp power_amp;
    MelangePowerAmp mpa;
    if (power_amp_kind) mpa.init(44100.0);
    Speaker speaker;
    speaker.init(BASE_SR);
    speaker.set_character(speaker_char);
    std::vector<double> t5_buf(n_samples, 0.0);
    for (size_t i = 0; i < n_samples; ++i) {
        const double attenuated = t4_buf[i] * volume * volume;
        const double amplified = power_amp_kind ? mpa.process(attenuated) : power_amp.process(attenuated);
        t5_buf[i] = speaker.process(amplified) * POST_SPEAKER_GAIN;
    }
    const double* t5w = &t5_buf[measure_start];
    const double t5_pk = peak_db(t5w, wn), t5_rm = rms_db(t5w, wn), t5_h2 = h2_h1_ratio_db(t5w, wn, freq, BASE_SR);

    // derived
    const double proxy = 20.0 * std::log10(out_scale);
    const double trim = cfg.zero_trim ? 0.0 : register_trim_db(note);
    const double proxy_error = t3_rm - cfg.target_db;
    const double tanh_compression = t4_pk - t5_pk;

    const double r[18] = {cfg.ds_at_c4, ds_actual, y_peak, t2_pk, t2_rm, t2_h2, t3_pk, t3_rm, t4_pk, t4_rm, t4_h2,
                          t5_pk, t5_rm, t5_h2, proxy, trim, proxy_error, tanh_compression};
    for (int i = 0; i < 18; ++i) row18[i] = r[i];
    if (taps) {
        const std::vector<double>* bufs[5] = {&reed_buf, &t2_buf, &t3_buf, &t4_buf, &t5_buf};
        for (int k = 0; k < 5; ++k)
            for (size_t i = 0; i < n_samples; ++i) taps[(size_t)k * n_samples + i] = (*bufs[k])[i];
    }
}
}  // extern "C"
