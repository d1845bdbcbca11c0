// Test-side CPU restatement of `preamp-bench centroid-track` (tools/preamp-bench/src/main.rs:1925-2135) over the oracle's headers, which
// it includes unchanged.  Render: Voice::render_note_with_scale (seed note * 2654435761, MLP off, attack noise on), a fresh legacy
// DkPreamp at 88 200 Hz with set_ldr_resistance(r) BEFORE reset() (:1989-1991), process_oversampled (:961-974), volume^2, PowerAmp::new()
// unless --no-poweramp, Speaker(character), POST_SPEAKER_GAIN.  Analysis: periodic-Hann frames of window_samples every hop_samples while
// pos + window <= len && pos + window / 2 <= end (integer half), spectral_centroid (:1931-1958) per frame -- a brute-force DFT over the
// bins k_min..=k_max with phase = 2.0 * PI * k * i / n formed left to right and the bins added in ascending k.
// tests/centroid_track_ref.py builds it with the oracle Makefile's flags (a second time with -DOW_ORACLE_EXP_PERTURB for the sensitivity
// variant) and loads it with ctypes; it is the checker of ow_centroid_track and ow_centroid_analyze.
#include "ow_engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

using namespace owo;

namespace {
const double BASE_SR = 44100.0;                  // main.rs:27
const double OVERSAMPLED_SR = BASE_SR * 2.0;     // main.rs:28
const double PI = 3.14159265358979323846;        // std::f64::consts::PI

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

// spectral_centroid (main.rs:1931-1958); spectrum: NULL or [k_max - k_min + 1][2] receiving (re, im) per bin
double spectral_centroid(const double* signal, size_t n, double sr, double min_freq, double max_freq, double* spectrum) {
    const double freq_resolution = sr / (double)n;
    const size_t k_min = (size_t)as_u64(std::ceil(min_freq / freq_resolution));
    const size_t k_max = std::min((size_t)as_u64(std::floor(max_freq / freq_resolution)), n / 2);
    double weighted_sum = 0.0, power_sum = 0.0;
    for (size_t k = k_min; k <= k_max; ++k) {
        const double freq = (double)k * freq_resolution;
        double re = 0.0, im = 0.0;
        for (size_t i = 0; i < n; ++i) {
            const double s = signal[i];
            const double phase = 2.0 * PI * (double)k * (double)i / (double)n;
            re += s * std::cos(phase);
            im -= s * std::sin(phase);
        }
        if (spectrum) { spectrum[2 * (k - k_min)] = re; spectrum[2 * (k - k_min) + 1] = im; }
        const double mag_sq = re * re + im * im;
        weighted_sum += freq * mag_sq;
        power_sum += mag_sq;
    }
    return power_sum > 0.0 ? weighted_sum / power_sum : 0.0;
}
}  // namespace

extern "C" {
// (duration * BASE_SR) as usize
size_t oct_samples(double duration) { return (size_t)as_u64(duration * BASE_SR); }
// ((ms / 1000.0) * BASE_SR) as usize (main.rs:2012-2014)
size_t oct_ms_to_samples(double ms) { return (size_t)as_u64((ms / 1000.0) * BASE_SR); }
// k_min, k_max of a frame of n samples; returns k_max - k_min + 1 (<= 0: no bin)
long long oct_bins(size_t n, size_t* k_min_out, size_t* k_max_out) {
    const double freq_resolution = BASE_SR / (double)n;
    const size_t k_min = (size_t)as_u64(std::ceil(50.0 / freq_resolution));
    const size_t k_max = std::min((size_t)as_u64(std::floor((BASE_SR / 4.0) / freq_resolution)), n / 2);
    if (k_min_out) *k_min_out = k_min;
    if (k_max_out) *k_max_out = k_max;
    return (long long)k_max - (long long)k_min + 1;
}

// final_output of the command (main.rs:1979-2009).  Returns n; writes min(n, cap) samples.
size_t oct_render(int note, int velocity_u8, double duration, double volume, double speaker_char, double r_ldr, int no_preamp, int no_poweramp,
                  int has_scale, double scale, double* out, size_t cap) {
    const uint32_t seed = (uint32_t)note * 2654435761u;            // Voice::render_note_with_scale, voice.rs:201-221
    Voice voice;
    voice.note_on(note, (double)velocity_u8 / 127.0, BASE_SR, seed, false);
    if (has_scale) voice.pickup.displacement_scale = scale;
    const size_t n = oct_samples(duration);
    std::vector<double> reed(n, 0.0);
    for (size_t off = 0; off < n; off += 1024) voice.render(reed.data() + off, std::min((size_t)1024, n - off));
    std::vector<double> pre;
    if (no_preamp) {
        pre = reed;
    } else {
        DkPreamp preamp;
        preamp.init(OVERSAMPLED_SR);                               // create_preamp, `--model dk` of the default build
        preamp.set_ldr_resistance(r_ldr);
        preamp.reset();
        pre = process_oversampled(reed, preamp);
    }
    PowerAmp power_amp;
    Speaker speaker;
    speaker.init(BASE_SR);
    speaker.set_character(speaker_char);
    for (size_t i = 0; i < n; ++i) {
        const double attenuated = pre[i] * volume * volume;
        const double amplified = no_poweramp ? attenuated : power_amp.process(attenuated);
        const double y = speaker.process(amplified) * POST_SPEAKER_GAIN;
        if (i < cap) out[i] = y;
    }
    return n;
}

// The frame loop (main.rs:2011-2072) on a given signal.  frames_out: NULL or [cap] centroids; spectra_out: NULL or [cap][bins][2];
// windowed frames use the periodic Hann table.  Returns the number of frames the loop visits (writes min(count, cap)); hop_samples == 0
// returns (size_t)-1 (the reference would not return).
size_t oct_analyze(const double* signal, size_t len, size_t window_samples, size_t hop_samples, size_t end_sample, double* frames_out, double* spectra_out,
                   size_t cap) {
    if (hop_samples == 0) return (size_t)-1;
    std::vector<double> hann(window_samples);
    for (size_t i = 0; i < window_samples; ++i) hann[i] = 0.5 * (1.0 - std::cos(2.0 * PI * (double)i / (double)window_samples));
    size_t k_min = 0, k_max = 0;
    const long long bins = oct_bins(window_samples ? window_samples : 1, &k_min, &k_max);
    std::vector<double> windowed(window_samples);
    size_t count = 0, pos = 0;
    while (pos + window_samples <= len && pos + window_samples / 2 <= end_sample) {
        for (size_t i = 0; i < window_samples; ++i) windowed[i] = signal[pos + i] * hann[i];
        if (count < cap) {
            double* sp = (spectra_out && bins > 0) ? spectra_out + count * (size_t)bins * 2 : nullptr;
            const double c = spectral_centroid(windowed.data(), window_samples, BASE_SR, 50.0, BASE_SR / 4.0, sp);
            if (frames_out) frames_out[count] = c;
        }
        ++count;
        pos += hop_samples;
    }
    return count;
}
}  // extern "C"
