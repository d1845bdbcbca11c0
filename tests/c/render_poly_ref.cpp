// Test-side CPU restatement of `preamp-bench render-poly` (tools/preamp-bench/src/main.rs:1397-1592) over the oracle's headers, which it
// includes unchanged: the chord's voices (seed note * 2654435761 + i, MLP on) and their sum, the shared chain, one chain per voice added
// in voice order, the residual, and the window figures of the report -- in the reference's statement order.  A chain is a fresh legacy
// DkPreamp at 88 200 Hz with set_ldr_resistance(r) BEFORE reset() (:1462-1464, :1488-1490), process_oversampled (:961-974), volume^2,
// PowerAmp::new() unless --no-poweramp, Speaker(character), POST_SPEAKER_GAIN.  tests/render_poly_ref.py builds it with the oracle
// Makefile's flags (a second time with -DOW_ORACLE_EXP_PERTURB for the sensitivity variant) and loads it with ctypes; it is the checker
// of ow_render_poly.
#include "ow_engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

using namespace owo;

namespace {
const double BASE_SR = 44100.0;                  // main.rs:27
const double OVERSAMPLED_SR = BASE_SR * 2.0;     // main.rs:28

double peak_abs(const double* s, size_t n) {     // main.rs:912-914
    double p = 0.0;
    for (size_t i = 0; i < n; ++i) p = std::fmax(p, std::fabs(s[i]));
    return p;
}
double to_dbfs(double val) { return val > 1e-15 ? 20.0 * std::log10(val) : -120.0; }     // main.rs:2241-2247
double mean_sq(const double* s, size_t n) {      // rms_db's first line, main.rs:921
    double sum = 0.0;
    for (size_t i = 0; i < n; ++i) sum += s[i] * s[i];
    return sum / (double)n;
}
double rms_db_of(double ms) { return ms > 0.0 ? 10.0 * std::log10(ms) : -120.0; }        // main.rs:922-926

// process_oversampled (main.rs:961-974)
std::vector<double> process_oversampled(const std::vector<double>& input, DkPreamp& preamp) {
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

// one chain of the command (main.rs:1462-1483 and :1488-1506): the chain's output samples
std::vector<double> chain(const std::vector<double>& input, double volume, double speaker_char, double r_ldr, bool no_poweramp) {
    DkPreamp preamp;
    preamp.init(OVERSAMPLED_SR);                 // create_preamp, `--model dk` of the default build
    preamp.set_ldr_resistance(r_ldr);
    preamp.reset();
    const std::vector<double> pre = process_oversampled(input, preamp);
    PowerAmp power_amp;
    Speaker speaker;
    speaker.init(BASE_SR);
    speaker.set_character(speaker_char);
    std::vector<double> out(input.size(), 0.0);
    for (size_t i = 0; i < input.size(); ++i) {
        const double attenuated = pre[i] * volume * volume;
        const double amplified = no_poweramp ? attenuated : power_amp.process(attenuated);
        out[i] = speaker.process(amplified) * POST_SPEAKER_GAIN;
    }
    return out;
}
}  // namespace

extern "C" {
// (duration * BASE_SR) as usize
size_t orp_samples(double duration) { return (size_t)as_u64(duration * BASE_SR); }

// cmd_render_poly for one chord.  row15: the fields of ow_poly_row in order (peak, residual_peak, win_peak[3], win_mean_sq[3], peak_db[3],
// rms_db[3], intermod_ratio_db).  final_out / sep_out / res_out: NULL or [n]; voices_out: NULL or [n_notes][n], the voices' OWN chains'
// outputs (the terms of separate_sum).  Returns n, 0 when the reference's window slice would panic (n <= 8820).
size_t orp_render(int n_notes, const uint8_t* notes, const uint8_t* velocities, double duration, double volume, double speaker_char, double r_ldr,
                  int no_poweramp, double* row15, double* final_out, double* sep_out, double* res_out, double* voices_out) {
    const size_t n_samples = orp_samples(duration);
    const size_t measure_start = (size_t)as_u64(0.2 * BASE_SR);
    const size_t measure_end = (size_t)as_u64(std::fmin(2.0 * BASE_SR, (double)n_samples));
    if (measure_start >= measure_end) return 0;
    std::vector<double> sum_buf(n_samples, 0.0);
    std::vector<std::vector<double>> individual_bufs;
    for (int i = 0; i < n_notes; ++i) {
        const double velocity = (double)velocities[i] / 127.0;
        const uint32_t noise_seed = (uint32_t)notes[i] * 2654435761u + (uint32_t)i;
        Voice voice;
        voice.note_on(notes[i], velocity, BASE_SR, noise_seed, true);
        std::vector<double> voice_buf(n_samples, 0.0);
        for (size_t off = 0; off < n_samples; off += 1024) voice.render(voice_buf.data() + off, std::min((size_t)1024, n_samples - off));
        for (size_t j = 0; j < n_samples; ++j) sum_buf[j] += voice_buf[j];
        individual_bufs.push_back(std::move(voice_buf));
    }
    const std::vector<double> final_output = chain(sum_buf, volume, speaker_char, r_ldr, no_poweramp != 0);
    std::vector<double> separate_sum(n_samples, 0.0);
    for (int k = 0; k < n_notes; ++k) {
        const std::vector<double> sep = chain(individual_bufs[k], volume, speaker_char, r_ldr, no_poweramp != 0);
        for (size_t i = 0; i < n_samples; ++i) separate_sum[i] += sep[i];
        if (voices_out) std::copy(sep.begin(), sep.end(), voices_out + (size_t)k * n_samples);
    }
    std::vector<double> residual(n_samples, 0.0);
    for (size_t i = 0; i < n_samples; ++i) residual[i] = final_output[i] - separate_sum[i];

    const size_t wn = measure_end - measure_start;
    const double* w[3] = {&final_output[measure_start], &separate_sum[measure_start], &residual[measure_start]};
    row15[0] = peak_abs(final_output.data(), n_samples);
    row15[1] = peak_abs(residual.data(), n_samples);
    for (int k = 0; k < 3; ++k) {
        row15[2 + k] = peak_abs(w[k], wn);
        row15[5 + k] = mean_sq(w[k], wn);
        row15[8 + k] = to_dbfs(row15[2 + k]);
        row15[11 + k] = rms_db_of(row15[5 + k]);
    }
    row15[14] = row15[11] - row15[13];
    if (final_out) std::copy(final_output.begin(), final_output.end(), final_out);
    if (sep_out) std::copy(separate_sum.begin(), separate_sum.end(), sep_out);
    if (res_out) std::copy(residual.begin(), residual.end(), res_out);
    return n_samples;
}
}  // extern "C"
