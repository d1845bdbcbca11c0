// Test-side CPU restatement of `preamp-bench bark-audit` (tools/preamp-bench/src/main.rs:551-664) over the oracle's headers, which it
// includes unchanged: cmd_bark_audit's loop body and its helpers (peak_abs, dft_magnitude, process_oversampled), in the reference's
// statement order, one sample after the other.  tests/bark_audit_ref.py builds it with the oracle Makefile's flags (a second time with
// -DOW_ORACLE_VOICE_PERTURB: the voice's library calls off by one ulp, oracle/ow_voice.hpp) and loads it with ctypes; it is the checker
// of ow_bark_audit.  duration and measure_start are the command's constants 0.5 and 0.25, parameters here as they are in the C-ABI.
#include "ow_tables.hpp"
#include "ow_voice.hpp"
#include "ow_chain.hpp"
#include "ow_melange.hpp"

#include <cmath>
#include <cstdint>
#include <vector>

using namespace owo;

namespace {
const double BASE_SR = 44100.0;                  // main.rs:27
const double OVERSAMPLED_SR = BASE_SR * 2.0;     // main.rs:28

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
size_t as_samples(double seconds) { return (size_t)as_u64(seconds * BASE_SR); }
}  // namespace

extern "C" {
size_t obr_samples(double seconds) { return as_samples(seconds); }

double obr_dft_magnitude(const double* signal, size_t len, double freq, double sr) { return dft_magnitude(signal, len, freq, sr); }

// One (note, velocity) of cmd_bark_audit's loops.  row11: fundamental_hz, displacement_scale, reed_peak, y_peak, pu_peak, pu_h1, pu_h2,
// pu_h2_h1, pre_h1, pre_h2, pre_h2_h1.  taps: NULL or [3][n] (reed, pickup, preamp).  Returns n, or 0 with nothing written when the
// measuring window would be empty (the command's slice would panic).
size_t obr_run(int note, int vel_byte, double duration, double measure_start, int preamp_kind, double* row11, double* taps) {
    const NoteParams params = note_params(note);
    const double freq = params.fundamental_hz;
    const double h2_freq = freq * 2.0;
    const double velocity = (double)vel_byte / 127.0;

    // Stage 1: raw reed
    const double detuned = params.fundamental_hz * freq_detune((uint8_t)note);
    double dwell[NUM_MODES], amp_offsets[NUM_MODES], amplitudes[NUM_MODES];
    dwell_attenuation(velocity, detuned, params.mode_ratios, dwell);
    mode_amplitude_offsets((uint8_t)note, amp_offsets);
    const double vel_exp = velocity_exponent(note);
    const double vel_scale = std::pow(velocity_scurve(velocity), vel_exp);
    for (int i = 0; i < NUM_MODES; ++i) amplitudes[i] = params.mode_amplitudes[i] * dwell[i] * amp_offsets[i] * vel_scale;
    ModalReed reed;
    reed.init(detuned, params.mode_ratios, amplitudes, params.mode_decay_rates, 0.0, velocity, BASE_SR, (uint32_t)note * 2654435761u);
    const size_t n_samples = as_samples(duration);
    const size_t measure_offset = as_samples(measure_start);
    if (measure_offset >= n_samples) return 0;
    const size_t wn = n_samples - measure_offset;
    std::vector<double> reed_buf(n_samples, 0.0);
    reed.render(reed_buf.data(), n_samples);
    const double reed_peak = peak_abs(&reed_buf[measure_offset], wn);
    const double displacement_scale = pickup_displacement_scale(note);
    const double y_peak = reed_peak * displacement_scale;

    // Stage 2: after the pickup
    Pickup pickup;
    pickup.init(BASE_SR);
    pickup.displacement_scale = displacement_scale;
    std::vector<double> pu_buf = reed_buf;
    pickup.process(pu_buf.data(), n_samples);
    const double* pu_steady = &pu_buf[measure_offset];
    const double pu_peak = peak_abs(pu_steady, wn);
    const double pu_h1 = dft_magnitude(pu_steady, wn, freq, BASE_SR);
    const double pu_h2 = dft_magnitude(pu_steady, wn, h2_freq, BASE_SR);
    const double pu_h2_h1 = pu_h1 > 1e-15 ? pu_h2 / pu_h1 : 0.0;

    // Stage 3: after the preamp (oversampled): new() + set_ldr_resistance(1e6), no reset()
    AnyPreamp preamp(preamp_kind);
    preamp.set_ldr_resistance(1000000.0);
    const std::vector<double> preamp_buf = process_oversampled(pu_buf, preamp);
    const double* pre_steady = &preamp_buf[measure_offset];
    const double pre_h1 = dft_magnitude(pre_steady, wn, freq, BASE_SR);
    const double pre_h2 = dft_magnitude(pre_steady, wn, h2_freq, BASE_SR);
    const double pre_h2_h1 = pre_h1 > 1e-15 ? pre_h2 / pre_h1 : 0.0;

    const double r[11] = {freq, displacement_scale, reed_peak, y_peak, pu_peak, pu_h1, pu_h2, pu_h2_h1, pre_h1, pre_h2, pre_h2_h1};
    for (int i = 0; i < 11; ++i) row11[i] = r[i];
    if (taps) {
        const std::vector<double>* bufs[3] = {&reed_buf, &pu_buf, &preamp_buf};
        for (int k = 0; k < 3; ++k)
            for (size_t i = 0; i < n_samples; ++i) taps[(size_t)k * n_samples + i] = (*bufs[k])[i];
    }
    return n_samples;
}
}  // extern "C"
