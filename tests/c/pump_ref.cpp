// TEST INFRASTRUCTURE (CPU, f64): restatement of the numeric cores of `preamp-bench pump-sweep` / `pump-trace` / `pump-spike` / `pump-step` /
// `pump-sinusoid` (tools/preamp-bench/src/main.rs:2329-3063) over the oracle's MelState (oracle/ow_melange.hpp), one run of one
// CircuitState::default() per point -- what ow_pump_measure computes on the device.  Loaded by tests/pump_ref.py.
//
// Sensitivity variant (nudge = +1 / -1): after every rebuild_matrices -- set_sample_rate's and the lazy one -- every non-zero entry of s, k
// and s_ni moves to a neighbouring double, up and down alternately (polarity -1 the other way round).  That is what another arrangement of
// the same LU arithmetic does to the matrices; MelState's R-only knob mel_r_ulp() changes no bit here (1 / R is absorbed in g_eff[6][6]).
#include "ow_melange.hpp"
#include "../../include/openwurli_hip.h"
#include <cstddef>
#include <cstring>

namespace {
using owo::MelState;

void nudge(MelState& st, int polarity) {
    if (!polarity) return;
    int c = 0;
    auto move = [&](double& x) {
        if (x == 0.0) return;
        const bool up = ((c++ & 1) == 0) == (polarity > 0);
        x = std::nextafter(x, up ? INFINITY : -INFINITY);
    };
    for (int i = 0; i < owo::PN; ++i) for (int j = 0; j < owo::PN; ++j) move(st.s[i][j]);
    for (int i = 0; i < owo::PM; ++i) for (int j = 0; j < owo::PM; ++j) move(st.k[i][j]);
    for (int i = 0; i < owo::PN; ++i) for (int j = 0; j < owo::PM; ++j) move(st.s_ni[i][j]);
}
// gen_preamp::process_sample with the lazy rebuild (gen_preamp.rs:3408-3411) done here, so that the nudge can follow it
double step(MelState& st, double x, int polarity) {
    if (st.matrices_dirty) { st.rebuild_matrices(); st.matrices_dirty = false; nudge(st, polarity); }
    return st.process_sample(x);
}
}  // namespace

extern "C" {

// One point (include/openwurli_hip.h ow_pump_point): row as ow_pump_measure fills it, trace NULL or [capture].  Returns 0, -1 on a point
// ow_pump_measure refuses for its shape (capture == 0, a ramp shorter than 2, an unknown schedule).
int opr_run(const ow_pump_point* p, int polarity, ow_pump_row* row, double* trace) {
    if (p->capture == 0 || p->schedule > OW_PUMP_LOGCOS || (p->schedule == OW_PUMP_RAMP && p->capture < 2)) return -1;
    MelState st;
    st.init_default();                                                    // CircuitState::default()
    if (std::fabs(p->sample_rate - PRE_SAMPLE_RATE) > 0.5) {              // main.rs:2388-2390, 2843-2845, 2971-2973 (and :2680: within 0.5 Hz
        st.set_sample_rate(p->sample_rate);                               // set_sample_rate copies the tables default() already holds)
        nudge(st, polarity);
    }
    st.set_runtime_r_ldr(p->r_settle);
    const double two_pi_dt = 2.0 * 3.14159265358979323846 * p->in_freq / p->sample_rate;      // :2722
    auto input = [&](uint64_t k) { return p->in_amp != 0.0 ? p->in_amp * std::sin(two_pi_dt * (double)k) : 0.0; };   // :2733
    for (uint64_t i = 0; i < p->settle; ++i) (void)step(st, input(i), polarity);
    std::memset(row, 0, sizeof *row);
    bool have_prev = false;
    double prev = 0.0;
    if (p->extra_sample) { row->extra = step(st, 0.0, polarity); prev = row->extra; have_prev = true; }   // :2778, 2857, 2994
    const double dt = 1.0 / p->sample_rate, omega = 2.0 * 3.14159265358979323846 * p->sched_freq;         // :2966-2967
    double sum = 0.0, sum_sq = 0.0, vmin = INFINITY, vmax = -INFINITY;                                    // :2397-2400
    double psum = 0.0, psum_sq = 0.0, raw_sum = 0.0, raw_sum_sq = 0.0, y0 = 0.0, max_step = 0.0;          // :2602-2605
    for (uint64_t k = 0; k < p->capture; ++k) {
        if (p->schedule == OW_PUMP_STEP) {
            if (k == 0) st.set_runtime_r_ldr(p->r_to);                                                    // :2861
        } else if (p->schedule == OW_PUMP_RAMP) {
            const double t = (double)k / (double)(p->capture - 1);                                        // :2780-2782
            st.set_runtime_r_ldr(p->r_settle + (p->r_to - p->r_settle) * t);
        } else if (p->schedule == OW_PUMP_LOGCOS) {
            const double t = (double)k * dt;                                                              // :2996-2998
            st.set_runtime_r_ldr(std::exp(p->ln_mid + p->ln_amp * std::cos(omega * t)));
        }
        const double y = step(st, input(p->settle + k), polarity);
        sum += y; sum_sq += y * y;                                                                        // :2403-2410
        if (y < vmin) vmin = y;
        if (y > vmax) vmax = y;
        if ((k & 1) == 0) y0 = y;
        else {                                                                                            // :2609-2613
            const double pm = 0.5 * (y0 + y);
            psum += pm; psum_sq += pm * pm;
            raw_sum += y0 + y; raw_sum_sq += y0 * y0 + y * y;
        }
        if (have_prev) { const double s = std::fabs(y - prev); if (s > max_step) max_step = s; }          // :2785-2789, 3003-3011
        prev = y; have_prev = true;
        if (trace) trace[k] = y;
    }
    const double nf = (double)p->capture;
    row->sum = sum; row->sum_sq = sum_sq; row->min = vmin; row->max = vmax;
    row->mean = sum / nf;                                                                                 // :2412-2414
    row->std = std::sqrt(std::fmax(sum_sq / nf - row->mean * row->mean, 0.0));
    const uint64_t pairs = p->capture / 2;                                                                // :2615-2618
    row->pair_mean = psum / (double)pairs;
    row->pair_std = std::sqrt(std::fmax(psum_sq / (double)pairs - row->pair_mean * row->pair_mean, 0.0));
    const double raw_mean = raw_sum / (double)(2 * pairs);
    row->raw_std = std::sqrt(std::fmax(raw_sum_sq / (double)(2 * pairs) - raw_mean * raw_mean, 0.0));
    row->max_step = max_step;
    row->nr_exhausted = st.diag_nr_max_iter_count; row->be_fallbacks = st.diag_be_fallback_count;
    row->voltage_damps = st.diag_voltage_damp_count; row->nan_resets = st.diag_nan_reset_count;
    return 0;
}

// cmd_pump_trace's figures of a trace (main.rs:2482-2516): out = mean, std (two-pass), min, max, then the five one-pole high-pass RMS values
void opr_trace_stats(const double* buf, size_t samples, double* out) {
    double s = 0.0;
    for (size_t i = 0; i < samples; ++i) s += buf[i];
    const double mean = s / (double)samples;
    double sum_sq = 0.0, vmin = INFINITY, vmax = -INFINITY;
    for (size_t i = 0; i < samples; ++i) {
        const double d = buf[i] - mean;
        sum_sq += d * d;
        if (buf[i] < vmin) vmin = buf[i];
        if (buf[i] > vmax) vmax = buf[i];
    }
    out[0] = mean; out[1] = std::sqrt(sum_sq / (double)samples); out[2] = vmin; out[3] = vmax;
    const double dt = 1.0 / 48000.0;
    const double bands[5] = {0.1, 1.0, 10.0, 100.0, 1000.0};
    for (int b = 0; b < 5; ++b) {
        const double rc = 1.0 / (2.0 * 3.14159265358979323846 * bands[b]);
        const double a = rc / (rc + dt);
        double py = 0.0, px = buf[0], acc = 0.0;
        for (size_t i = 0; i < samples; ++i) {
            const double y = a * (py + buf[i] - px);
            py = y; px = buf[i];
            acc += y * y;
        }
        out[4 + b] = std::sqrt(acc / (double)samples);
    }
}

// cmd_pump_step's tail statistics (main.rs:2874-2888): out = tail_mean, tail_std, initial, total_swing
void opr_step_tail(const double* buf, size_t samples, double* out) {
    const size_t tail_start = (samples * 9 / 10) & ~(size_t)1;
    const double* tail = buf + tail_start;
    const size_t pairs = (samples - tail_start) / 2;
    double s = 0.0, ss = 0.0;
    for (size_t k = 0; k < pairs; ++k) {
        const double pm = 0.5 * (tail[2 * k] + tail[2 * k + 1]);
        s += pm; ss += pm * pm;
    }
    out[0] = s / (double)pairs;
    out[1] = std::sqrt(std::fmax(ss / (double)pairs - out[0] * out[0], 0.0));
    out[2] = 0.5 * (buf[0] + buf[1]);
    out[3] = out[0] - out[2];
}

// cmd_pump_sinusoid's bifurcation count (main.rs:3018-3032)
size_t opr_sinusoid_bifurcs(const double* y, size_t samples) {
    size_t n = 0;
    double prev_pm = 0.5 * (y[0] + y[1]);
    for (size_t i = 2; i < samples; i += 2) {
        const double pm = 0.5 * (y[i] + (i + 1 < samples ? y[i + 1] : y[i]));
        if (std::fabs(pm - prev_pm) > 0.1) ++n;
        prev_pm = pm;
    }
    return n;
}

}  // extern "C"
