// Test-side CPU restatement of the note audits `preamp-bench intermod-audit` (tools/preamp-bench/src/main.rs:675-903, the static table
// tables.rs:675-801) and `overshoot` (:2137-2247) over the oracle's headers, which it includes unchanged.  Everything is serial and in the
// reference's order: one note, one probe, one sample after the other.  tests/note_audit_ref.py builds it with the oracle Makefile's flags
// (a second time with -DOW_ORACLE_VOICE_PERTURB for the sensitivity variant of the voice row) and loads it with ctypes; it is the checker
// of ow_intermod_risk, ow_intermod_probes, ow_dft_magnitudes, ow_intermod_audit and ow_overshoot.
#include "ow_voice.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

using namespace owo;

namespace {
const double BASE_SR = 44100.0;                  // main.rs:27
const double PI = 3.14159265358979323846;        // std::f64::consts::PI

struct Product { int mode; uint32_t nearest_integer; double mode_ratio, fractional_offset, beat_hz, effective_amplitude, perceptual_weight, risk_score; };
struct Report { double fundamental_hz, mu, max_risk, total_risk; Product products[6]; };

double perceptual_beat_weight(double beat_hz) {                                   // tables.rs:703-725
    if (beat_hz < 0.5) return 0.0;
    if (beat_hz < 2.0) return 0.5 * (beat_hz - 0.5) / 1.5;
    if (beat_hz <= 5.0) return 0.5 + 0.5 * (beat_hz - 2.0) / 3.0;
    if (beat_hz <= 10.0) return 1.0;
    if (beat_hz <= 40.0) return 0.1 + 0.9 * (40.0 - beat_hz) / 30.0;
    return 0.1;
}
void dwell_attenuation_ff(double fundamental_hz, const double ratios[NUM_MODES], double atten[NUM_MODES]) {   // tables.rs:731-747
    const double t_dwell = rclamp(0.75 / fundamental_hz, 0.0003, 0.020);
    const double sigma_sq = 8.0 * 8.0;
    for (int i = 0; i < NUM_MODES; ++i) {
        const double ft = fundamental_hz * ratios[i] * t_dwell;
        atten[i] = std::exp(-ft * ft / (2.0 * sigma_sq));
    }
    const double a0 = atten[0];
    if (a0 > 1e-30)
        for (int i = 0; i < NUM_MODES; ++i) atten[i] /= a0;
}
Report intermod_risk(int midi) {                                                  // tables.rs:755-801
    Report r;
    std::memset(&r, 0, sizeof(r));
    r.fundamental_hz = midi_to_freq(midi);
    r.mu = tip_mass_ratio(midi);
    double ratios[NUM_MODES], dwell[NUM_MODES], coupling[NUM_MODES];
    mode_ratios(r.mu, ratios);
    dwell_attenuation_ff(r.fundamental_hz, ratios, dwell);
    spatial_coupling_coefficients(r.mu, reed_length_mm(midi), coupling);
    for (int i = 1; i < NUM_MODES; ++i) {
        Product& p = r.products[i - 1];
        p.mode = i + 1;
        p.mode_ratio = ratios[i];
        p.nearest_integer = as_u32(std::round(ratios[i]));
        p.fractional_offset = std::fabs(ratios[i] - (double)p.nearest_integer);
        p.beat_hz = p.fractional_offset * r.fundamental_hz;
        p.effective_amplitude = BASE_MODE_AMPLITUDES[i] * coupling[i] * dwell[i];
        p.perceptual_weight = perceptual_beat_weight(p.beat_hz);
        p.risk_score = p.effective_amplitude * p.perceptual_weight;
        r.max_risk = std::fmax(r.max_risk, p.risk_score);
        r.total_risk += p.risk_score;
    }
    return r;
}

double dft_magnitude(const double* signal, size_t len, double freq, double sr) {  // main.rs:893-903
    const double n = (double)len;
    double re = 0.0, im = 0.0;
    for (size_t i = 0; i < len; ++i) {
        const double phase = 2.0 * PI * freq * (double)i / sr;
        re += signal[i] * std::cos(phase);
        im -= signal[i] * std::sin(phase);
    }
    const double a = re / n, b = im / n;
    return 2.0 * std::sqrt(a * a + b * b);
}

// spectral_grass (main.rs:682-720); energies_out: NULL or the two sums; counts_out: NULL or the probes that entered them
void spectral_grass(const double* signal, size_t len, double fundamental_hz, double sr, size_t max_harmonic, double out[3], double* energies_out,
                    uint32_t* counts_out) {
    double harmonic_energy = 0.0, midpoint_energy = 0.0;
    uint32_t nh = 0, nm = 0;
    for (size_t n = 1; n <= max_harmonic; ++n) {
        const double freq = (double)n * fundamental_hz;
        if (freq >= sr / 2.0) break;
        const double mag = dft_magnitude(signal, len, freq, sr);
        harmonic_energy += mag * mag;
        ++nh;
    }
    for (size_t n = 1; n < max_harmonic; ++n) {
        const double freq = ((double)n + 0.5) * fundamental_hz;
        if (freq >= sr / 2.0) break;
        const double mag = dft_magnitude(signal, len, freq, sr);
        midpoint_energy += mag * mag;
        ++nm;
    }
    out[0] = harmonic_energy > 0.0 ? 10.0 * std::log10(harmonic_energy) : -120.0;
    out[1] = midpoint_energy > 0.0 ? 10.0 * std::log10(midpoint_energy) : -120.0;
    out[2] = out[0] - out[1];
    if (energies_out) { energies_out[0] = harmonic_energy; energies_out[1] = midpoint_energy; }
    if (counts_out) { counts_out[0] = nh; counts_out[1] = nm; }
}

double rms_window(const double* signal, size_t len, size_t start, size_t end) {   // main.rs:2231-2239
    const size_t s = std::min(start, len), e = std::min(end, len);
    if (e <= s) return 0.0;
    double sum_sq = 0.0;
    for (size_t i = s; i < e; ++i) sum_sq += signal[i] * signal[i];
    return std::sqrt(sum_sq / (double)(e - s));
}
double peak_to(const double* signal, size_t len, size_t end) {                    // output[..t.min(len)].iter().map(|x| x.abs()).fold(0.0, f64::max)
    double pk = 0.0;
    for (size_t i = 0; i < std::min(end, len); ++i) pk = std::fmax(pk, std::fabs(signal[i]));
    return pk;
}
double to_dbfs(double val) { return val > 1e-15 ? 20.0 * std::log10(val) : -120.0; }   // main.rs:2241-2247
}  // namespace

extern "C" {
size_t onr_samples(double duration) { return (size_t)as_u64(duration * BASE_SR); }

// out: fundamental_hz, mu, max_risk, total_risk, then per product mode, nearest_integer, mode_ratio, fractional_offset, beat_hz,
// effective_amplitude, perceptual_weight, risk_score (4 + 6 x 8 doubles)
void onr_intermod_risk(int midi, double* out) {
    const Report r = intermod_risk(midi);
    out[0] = r.fundamental_hz; out[1] = r.mu; out[2] = r.max_risk; out[3] = r.total_risk;
    for (int k = 0; k < 6; ++k) {
        const Product& p = r.products[k];
        double* o = out + 4 + 8 * k;
        o[0] = (double)p.mode; o[1] = (double)p.nearest_integer; o[2] = p.mode_ratio; o[3] = p.fractional_offset; o[4] = p.beat_hz;
        o[5] = p.effective_amplitude; o[6] = p.perceptual_weight; o[7] = p.risk_score;
    }
}
double onr_perceptual_beat_weight(double beat_hz) { return perceptual_beat_weight(beat_hz); }

double onr_dft_magnitude(const double* signal, size_t len, double freq, double sr) { return dft_magnitude(signal, len, freq, sr); }

// Voice::render_note(note, velocity_u8 / 127.0, duration, BASE_SR).  Returns n; writes min(n, cap) samples.
size_t onr_render(int note, int velocity_u8, double duration, double* out, size_t cap) {
    const std::vector<double> v = render_note(note, (double)velocity_u8 / 127.0, duration, BASE_SR);
    std::copy(v.begin(), v.begin() + std::min(cap, v.size()), out);
    return v.size();
}

// The probe frequencies of the render analysis in the order it visits them (harmonics, midpoints, then the listed products' pairs).
// freqs: [75].  Returns the count.
int onr_probes(int midi, double* freqs, uint32_t* n_harm, uint32_t* n_mid) {
    const Report r = intermod_risk(midi);
    const double f0 = midi_to_freq(midi);
    const size_t max_harmonic = std::min((size_t)as_u64(std::floor(BASE_SR / 2.0 / f0)), (size_t)32);
    int c = 0;
    *n_harm = *n_mid = 0;
    for (size_t n = 1; n <= max_harmonic; ++n) {
        const double freq = (double)n * f0;
        if (freq >= BASE_SR / 2.0) break;
        freqs[c++] = freq; ++*n_harm;
    }
    for (size_t n = 1; n < max_harmonic; ++n) {
        const double freq = ((double)n + 0.5) * f0;
        if (freq >= BASE_SR / 2.0) break;
        freqs[c++] = freq; ++*n_mid;
    }
    for (int k = 0; k < 6; ++k) {
        if (r.products[k].risk_score < 0.001) continue;
        freqs[c++] = r.products[k].mode_ratio * f0;
        freqs[c++] = (double)r.products[k].nearest_integer * f0;
    }
    return c;
}

// The render analysis of one note on a given signal (main.rs:822-888).  Returns 1 for "(signal too short)", else 0.
// out: h_db, m_db, ratio_db, verdict (0 DIRTY .. 3 CLEAN), harmonic_energy, midpoint_energy, n_harmonics, n_midpoints, start, end (10);
// detail: per product listed (0 / 1), intermod_freq, nearest_freq, intermod_mag, nearest_mag, ratio_db, risk_score (6 x 7).
int onr_intermod_audit(const double* signal, size_t len, int midi, double* out, double* detail) {
    const double fundamental_hz = midi_to_freq(midi);
    const size_t start = (size_t)as_u64(0.5 * BASE_SR);
    const size_t end = (size_t)as_u64(std::fmin(2.0 * BASE_SR, (double)len));
    out[8] = (double)start; out[9] = (double)end;
    if (end <= start) return 1;
    const double* sustain = signal + start;
    const size_t n = end - start;
    const size_t max_harmonic = (size_t)as_u64(std::floor(BASE_SR / 2.0 / fundamental_hz));
    uint32_t counts[2];
    spectral_grass(sustain, n, fundamental_hz, BASE_SR, std::min(max_harmonic, (size_t)32), out, out + 4, counts);
    out[3] = out[2] > 40.0 ? 3.0 : out[2] > 30.0 ? 2.0 : out[2] > 20.0 ? 1.0 : 0.0;
    out[6] = (double)counts[0]; out[7] = (double)counts[1];
    const Report r = intermod_risk(midi);
    for (int k = 0; k < 6; ++k) {
        const Product& p = r.products[k];
        double* d = detail + 7 * k;
        d[0] = p.risk_score < 0.001 ? 0.0 : 1.0;
        d[1] = p.mode_ratio * fundamental_hz;
        d[2] = (double)p.nearest_integer * fundamental_hz;
        d[3] = d[4] = d[5] = 0.0;
        d[6] = p.risk_score;
        if (p.risk_score < 0.001) continue;
        d[3] = dft_magnitude(sustain, n, d[1], BASE_SR);
        d[4] = dft_magnitude(sustain, n, d[2], BASE_SR);
        d[5] = d[4] > 1e-15 ? 20.0 * std::log10(d[3] / d[4]) : 0.0;
    }
    return 0;
}

// cmd_overshoot's figures of one signal (main.rs:2173-2214).  out: peak_0_10, peak_0_50, rms_100_200, rms_1000_1500, overshoot_db,
// bark_decay_db, pk_dbfs, rms1_dbfs, rms2_dbfs; edges_out: NULL or the six unclamped window edges.
void onr_overshoot(const double* signal, size_t len, double* out, size_t* edges_out) {
    const size_t t_10ms = (size_t)as_u64(0.010 * BASE_SR), t_50ms = (size_t)as_u64(0.050 * BASE_SR), t_100ms = (size_t)as_u64(0.100 * BASE_SR);
    const size_t t_200ms = (size_t)as_u64(0.200 * BASE_SR), t_1000ms = (size_t)as_u64(1.000 * BASE_SR), t_1500ms = (size_t)as_u64(1.500 * BASE_SR);
    out[0] = peak_to(signal, len, t_10ms);
    out[1] = peak_to(signal, len, t_50ms);
    out[2] = rms_window(signal, len, t_100ms, t_200ms);
    out[3] = rms_window(signal, len, t_1000ms, t_1500ms);
    out[4] = out[2] > 1e-15 ? 20.0 * std::log10(out[0] / out[2]) : std::nan("");
    out[5] = out[3] > 1e-15 ? 20.0 * std::log10(out[1] / out[3]) : std::nan("");
    out[6] = to_dbfs(out[0]); out[7] = to_dbfs(out[2]); out[8] = to_dbfs(out[3]);
    if (edges_out) { edges_out[0] = t_10ms; edges_out[1] = t_50ms; edges_out[2] = t_100ms; edges_out[3] = t_200ms; edges_out[4] = t_1000ms; edges_out[5] = t_1500ms; }
}
}  // extern "C"
