// Test-side CPU restatement of `preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep` (tools/preamp-bench/src/main.rs:150-369)
// over the oracle's headers, which it includes unchanged: measure_gain_at (:157-190) with the ONE preamp object that cmd_sweep /
// cmd_tremolo_sweep reuse (reset() per point, no per-point reset resistance), cmd_harmonics' fresh preamp without reset() (:256-323) and
// dft_magnitude (:893-903), in the reference's statement order.  tests/preamp_bench_ref.py builds it with the oracle Makefile's flags and
// loads it with ctypes; it is the checker of ow_preamp_measure.
#include "ow_chain.hpp"
#include "ow_melange.hpp"

#include <cmath>
#include <vector>

using namespace owo;

namespace {
const double BASE_SR = 44100.0;                  // main.rs:27
const double OVERSAMPLED_SR = BASE_SR * 2.0;     // main.rs:28
const size_t N_TOTAL = (size_t)(BASE_SR * 0.5);  // cmd_harmonics (:266); = n_settle + n_measure of measure_gain_at (:165-166)
const size_t N_SETTLE = (size_t)(BASE_SR * 0.3);

// the PreampModel `create_preamp` returns (main.rs:132-148): legacy 8-node or melange 12-node at OVERSAMPLED_SR, noise off
struct AnyPreamp {
    int kind;
    DkPreamp legacy;
    MelangePreamp mel;
    explicit AnyPreamp(int k) : kind(k) { if (kind) mel.init(OVERSAMPLED_SR); else legacy.init(OVERSAMPLED_SR); }
    void reset() { if (kind) mel.reset(); else legacy.reset(); }
    void set_ldr_resistance(double r) { if (kind) mel.set_ldr_resistance(r); else legacy.set_ldr_resistance(r); }
    double process_sample(double x) { return kind ? mel.process_sample(x) : legacy.process_sample(x); }
};

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

// The loop body measure_gain_at and cmd_harmonics share (:168-186, :268-279): N_TOTAL samples through a fresh Oversampler and `preamp`
// as it stands.  met9: gain (peak over [N_SETTLE, N_TOTAL) / amplitude), 20 log10(gain), H1..H5 over the last quarter, THD %, H2/H3 dB.
void run(AnyPreamp& preamp, double freq, double amplitude, double* met9, double* trace) {
    Oversampler os;
    std::vector<double> output(N_TOTAL, 0.0);
    double peak = 0.0;
    for (size_t i = 0; i < N_TOTAL; ++i) {
        const double t = (double)i / BASE_SR;
        const double input = amplitude * std::sin(2.0 * PI_ * freq * t);
        double up[2] = {0.0, 0.0};
        os.upsample_2x(&input, 1, up);
        const double processed[2] = {preamp.process_sample(up[0]), preamp.process_sample(up[1])};
        double down[1] = {0.0};
        os.downsample_2x(processed, down, 1);
        if (i >= N_SETTLE) peak = std::fmax(peak, std::fabs(down[0]));
        output[i] = down[0];
    }
    const double gain = peak / amplitude;
    const size_t start = output.size() * 3 / 4;
    const double* signal = &output[start];
    const size_t len = output.size() - start;
    const double h1 = dft_magnitude(signal, len, freq, BASE_SR);
    const double h2 = dft_magnitude(signal, len, 2.0 * freq, BASE_SR);
    const double h3 = dft_magnitude(signal, len, 3.0 * freq, BASE_SR);
    const double h4 = dft_magnitude(signal, len, 4.0 * freq, BASE_SR);
    const double h5 = dft_magnitude(signal, len, 5.0 * freq, BASE_SR);
    const double thd = (std::sqrt(h2 * h2 + h3 * h3 + h4 * h4 + h5 * h5) / h1) * 100.0;
    const double h2_h3 = h3 > 1e-15 ? 20.0 * std::log10(h2 / h3) : INFINITY;
    const double m[9] = {gain, 20.0 * std::log10(gain), h1, h2, h3, h4, h5, thd, h2_h3};
    for (int k = 0; k < 9; ++k) met9[k] = m[k];
    if (trace)
        for (size_t i = 0; i < N_TOTAL; ++i) trace[i] = output[i];
}
}  // namespace

extern "C" {
// cmd_sweep / cmd_tremolo_sweep / cmd_gain: ONE preamp object (create_preamp), then measure_gain_at(preamp, freq[i], amp[i], r_ldr[i]) for
// i = 0..n-1 in order -- reset(), set_ldr_resistance(r_ldr[i]) and the run.  met9: [n][9], trace: NULL or [n][N_TOTAL].
void opb_measure_seq(int kind, int n, const double* freq, const double* amp, const double* r_ldr, double* met9, double* trace) {
    AnyPreamp preamp(kind);
    for (int i = 0; i < n; ++i) {
        preamp.reset();
        preamp.set_ldr_resistance(r_ldr[i]);
        run(preamp, freq[i], amp[i], met9 + (size_t)i * 9, trace ? trace + (size_t)i * N_TOTAL : nullptr);
    }
}
// cmd_harmonics: a fresh preamp, set_ldr_resistance(r_ldr), no reset().
void opb_harmonics(int kind, double freq, double amp, double r_ldr, double* met9, double* trace) {
    AnyPreamp preamp(kind);
    preamp.set_ldr_resistance(r_ldr);
    run(preamp, freq, amp, met9, trace);
}
// One independent point of the device's model: a fresh preamp whose r_ldr is moved to r_reset, reset() (the legacy DC solve at r_reset),
// then set_ldr_resistance(r_ldr).  With r_reset = the previous point's resistance this is point i of opb_measure_seq.
void opb_point(int kind, double freq, double amp, double r_ldr, double r_reset, double* met9, double* trace) {
    AnyPreamp preamp(kind);
    preamp.set_ldr_resistance(r_reset);
    preamp.reset();
    preamp.set_ldr_resistance(r_ldr);
    run(preamp, freq, amp, met9, trace);
}
}  // extern "C"
