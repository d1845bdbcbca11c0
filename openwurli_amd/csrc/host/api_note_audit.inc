// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the note audits `preamp-bench intermod-audit`
// (tools/preamp-bench/src/main.rs:675-903; the static table is tables.rs:675-801) and `overshoot` (:2137-2247), many (note, velocity) jobs
// per call.  Both audit Voice::render_note's row alone: k_job_voice renders it, k_dft_probes / k_window_stats reduce it, the host finishes.
namespace {
namespace note_audit {
const double SR = 44100.0;                         // BASE_SR, main.rs:27
const size_t BUDGET_BYTES = size_t(8) << 30;       // per chunk (a job takes one voice row), as the other offline entry points'

// ---- tables::intermod_risk on the host, over the functions k_note_table is built from (ow_voice_dev.h) -----------------------------
double perceptual_beat_weight(double beat_hz) {     // tables.rs:703-725, its branch order
    if (beat_hz < 0.5) return 0.0;
    if (beat_hz < 2.0) return 0.5 * (beat_hz - 0.5) / 1.5;
    if (beat_hz <= 5.0) return 0.5 + 0.5 * (beat_hz - 2.0) / 3.0;
    if (beat_hz <= 10.0) return 1.0;
    if (beat_hz <= 40.0) return 0.1 + 0.9 * (40.0 - beat_hz) / 30.0;
    return 0.1;
}
void dwell_attenuation_ff(double fundamental_hz, const double ratios[7], double atten[7]) {     // tables.rs:731-747
    const double t_dwell = owdev::clampd(0.75 / fundamental_hz, 0.0003, 0.020);
    const double sigma_sq = 8.0 * 8.0;
    for (int i = 0; i < 7; ++i) {
        const double ft = fundamental_hz * ratios[i] * t_dwell;
        atten[i] = std::exp(-ft * ft / (2.0 * sigma_sq));
    }
    const double a0 = atten[0];
    if (a0 > 1e-30)
        for (int i = 0; i < 7; ++i) atten[i] /= a0;
}
inline uint32_t rust_as_u32(double x) { return !(x > 0.0) ? 0u : (x >= 4294967295.0 ? 4294967295u : (uint32_t)x); }
void intermod_risk(uint8_t midi, ow_intermod_report& r) {                                       // tables.rs:755-801
    std::memset(&r, 0, sizeof(r));
    const double m = (double)midi;
    r.midi = midi;
    r.fundamental_hz = owdev::midi_to_freq(m);
    r.mu = owdev::tip_mass_ratio(m);
    double betas[7], ratios[7], dwell[7], kraw[7];
    owdev::eigenvalues(r.mu, betas);
    owdev::mode_ratios(betas, ratios);
    dwell_attenuation_ff(r.fundamental_hz, ratios, dwell);
    owdev::spatial_coupling_raw(betas, owdev::reed_length_mm(m), kraw);
    const double base_amp[7] = OW_BASE_MODE_AMPLITUDES;
    for (int i = 1; i < 7; ++i) {
        ow_intermod_product& p = r.products[i - 1];
        const double ratio = ratios[i];
        p.mode = (uint32_t)(i + 1);
        p.mode_ratio = ratio;
        p.nearest_integer = rust_as_u32(std::round(ratio));
        p.fractional_offset = std::fabs(ratio - (double)p.nearest_integer);
        p.beat_hz = p.fractional_offset * r.fundamental_hz;
        p.effective_amplitude = base_amp[i] * owdev::spatial_coupling_norm(kraw[i], kraw[0]) * dwell[i];
        p.perceptual_weight = perceptual_beat_weight(p.beat_hz);
        p.risk_score = p.effective_amplitude * p.perceptual_weight;
        r.max_risk = std::fmax(r.max_risk, p.risk_score);                                       // f64::max
        r.total_risk += p.risk_score;
    }
}

// ---- the probe list of the render analysis (:841-843, spectral_grass :691-707, the detail :869-876) --------------------------------
struct Probes {
    double freq[OW_INTERMOD_MAX_PROBES];
    uint32_t n_harm = 0, n_mid = 0, count = 0;
    int detail[6];                                  // index of a product's (mode frequency, nearest harmonic) pair, -1: not listed
};
void make_probes(const ow_intermod_report& rep, Probes& p) {
    const double f0 = rep.fundamental_hz;
    const size_t max_harmonic = std::min<size_t>(rust_as_usize(std::floor(SR / 2.0 / f0)), 32);
    for (size_t n = 1; n <= max_harmonic; ++n) {
        const double freq = (double)n * f0;
        if (freq >= SR / 2.0) break;
        p.freq[p.count++] = freq; ++p.n_harm;
    }
    for (size_t n = 1; n < max_harmonic; ++n) {
        const double freq = ((double)n + 0.5) * f0;
        if (freq >= SR / 2.0) break;
        p.freq[p.count++] = freq; ++p.n_mid;
    }
    for (int k = 0; k < 6; ++k) {
        p.detail[k] = -1;
        if (rep.products[k].risk_score < 0.001) continue;
        p.detail[k] = (int)p.count;
        p.freq[p.count++] = rep.products[k].mode_ratio * f0;
        p.freq[p.count++] = (double)rep.products[k].nearest_integer * f0;
    }
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------
// d_sig [rows][stride], d_freqs [rows][n_probes] -> d_sums [rows][n_probes][2], on st (no synchronisation); rows beyond 65 535: more launches
void launch_dft(const double* d_sig, size_t rows, size_t stride, size_t start, size_t end, double sr, const double* d_freqs, size_t n_probes, double* d_sums,
                hipStream_t st) {
    if (rows == 0 || n_probes == 0) return;
    for (size_t r0 = 0; r0 < rows; r0 += 65535) {
        owdev::k_dft_probes<<<dim3((unsigned)n_probes, (unsigned)std::min<size_t>(65535, rows - r0)), dim3(OW_NA_THREADS), 0, st>>>(
            d_sig, stride, start, end - start, sr, d_freqs, (uint32_t)n_probes, (uint32_t)r0, d_sums);
        HIP_OK(hipGetLastError());
    }
}
void launch_windows(const double* d_sig, size_t rows, size_t stride, owdev::OwNaWindows w, double* d_out, hipStream_t st) {
    if (rows == 0 || w.count == 0) return;
    for (size_t r0 = 0; r0 < rows; r0 += 65535) {
        w.row0 = (uint32_t)r0;
        owdev::k_window_stats<<<dim3(w.count, (unsigned)std::min<size_t>(65535, rows - r0)), dim3(OW_NA_THREADS), 0, st>>>(d_sig, stride, w, d_out);
        HIP_OK(hipGetLastError());
    }
}

// ---- what the two commands share: checks, then Voice::render_note rows in chunks ----------------------------------------------------
// returns the samples per job; `fields`: the size fields' names for the ABI refusal
template <class Cfg>
size_t checked_samples(const Cfg* cfg, const char* fields, const double* audio_out, size_t audio_stride) {
    if (!cfg) throw std::runtime_error("null argument");
    if (cfg->struct_size != sizeof(Cfg) || cfg->job_size != sizeof(ow_note_job)) throw std::runtime_error(abi_mismatch(fields));
    const double x = cfg->duration_s * SR;                 // Voice::render_note: (duration * sample_rate) as usize
    if (!(x < 2147483648.0)) throw std::runtime_error("duration_s must give fewer than 2^31 samples");
    const size_t n = rust_as_usize(x);
    if (audio_out && audio_stride < n) throw std::runtime_error("audio_stride smaller than the " + std::to_string(n) + " samples of a job");
    return n;
}
void check_jobs(const ow_note_job* jobs, size_t n_jobs, const void* rows_out) {
    if (!jobs || !rows_out) throw std::runtime_error("null argument");
    if (n_jobs > (size_t)INT32_MAX / 64) throw std::runtime_error("too many jobs");
    for (size_t i = 0; i < n_jobs; ++i) check_note_velocity("job " + std::to_string(i) + ": ", jobs[i].note, jobs[i].velocity);
}
// waits for the stream on every way out of the chunk loop, a thrown HIP error included: the caller's host and device buffers, declared
// before the call, are released only after nothing queued can touch them any more
struct StreamDrain {
    hipStream_t s;
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};
// Renders the jobs' voice rows chunk by chunk into HBM and hands every chunk to analyse(c0, cn, d_rows, stride, stream), which queues its
// launches and copies on that stream; the stream is synchronised after each chunk, then finish(c0, cn) runs on the host.
template <class Analyse, class Finish>
void for_each_chunk(int device, const ow_note_job* jobs, size_t n_jobs, size_t n, size_t extra_bytes_per_job, double* audio_out, size_t audio_stride,
                    Analyse analyse, Finish finish) {
    OfflineCall call(device, SR, OW_PREAMP_LEGACY8, /*note_table=*/true);      // the constants k_job_voice reads: the rate alone matters here
    hipStream_t st = call.st();
    const StreamDrain drain{st};
    const size_t stride = (size_t)row_stride((long long)n);
    const size_t row_bytes = sizeof(double) * stride;
    // per job: its row, its share of a block's voice records (one block of 64 jobs), its job record, the analysis' own buffers
    const size_t job_bytes = row_bytes + sizeof(double) * (OW_VREC_DOUBLES / 64) + sizeof(owdev::OwJobDev) + extra_bytes_per_job;
    const size_t chunk = budget_chunk(BUDGET_BYTES - sizeof(double) * OW_VREC_DOUBLES, job_bytes, call.sw.note_audit_chunk, n_jobs);
    DevMem m_vrec, m_jobs, m_reed;                                             // released on every exit path
    m_vrec.alloc(sizeof(double) * ((chunk + 63) / 64) * OW_VREC_DOUBLES);
    m_jobs.alloc(sizeof(owdev::OwJobDev) * chunk);
    m_reed.alloc(row_bytes * chunk);
    std::vector<owdev::OwJobDev> hj;
    for (size_t c0 = 0; c0 < n_jobs; c0 += chunk) {
        const size_t cn = std::min(chunk, n_jobs - c0);
        hj.assign(cn, owdev::OwJobDev{});
        for (size_t i = 0; i < cn; ++i) {
            owdev::OwJobDev& d = hj[i];
            std::memset(&d, 0, sizeof(d));
            d.note = jobs[c0 + i].note; d.velocity = jobs[c0 + i].velocity;    // Voice::render_note: MLP off, attack noise on, the table's displacement scale
            d.volume = 1.0; d.speaker = 0.0; d.r_ldr = 1000000.0;              // not read by k_job_voice
        }
        HIP_OK(hipMemcpyAsync(m_jobs.p, hj.data(), sizeof(owdev::OwJobDev) * cn, hipMemcpyHostToDevice, st));
        owdev::k_job_voice<<<dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, st>>>(call.dK(), call.nt(), m_vrec.as<double>(), m_jobs.as<owdev::OwJobDev>(),
                                                                                  m_reed.as<double>(), (int)cn, (long long)n, (long long)stride);
        HIP_OK(hipGetLastError());
        analyse(c0, cn, m_reed.as<double>(), stride, st);
        if (audio_out) rows_to_host(audio_out + c0 * audio_stride, audio_stride, m_reed.p, stride, n, cn, st);
        HIP_OK(hipStreamSynchronize(st));                                      // the buffers are reused by the next chunk
        finish(c0, cn);
    }
}

// ---- intermod-audit's finish (spectral_grass :688-719, the verdict :845-853, the detail :873-881) ----------------------------------
void finish_intermod(const Probes& p, const double* sums, double n_window, ow_intermod_row& r) {
    auto mag = [&](uint32_t k) { return measure::dft_magnitude(sums[2 * k], sums[2 * k + 1], n_window); };
    double he = 0.0, me = 0.0;
    for (uint32_t k = 0; k < p.n_harm; ++k) { const double a = mag(k); he += a * a; }
    for (uint32_t k = 0; k < p.n_mid; ++k) { const double a = mag(p.n_harm + k); me += a * a; }
    r.harmonic_energy = he; r.midpoint_energy = me;
    r.h_db = he > 0.0 ? 10.0 * std::log10(he) : -120.0;
    r.m_db = me > 0.0 ? 10.0 * std::log10(me) : -120.0;
    r.ratio_db = r.h_db - r.m_db;
    r.verdict = r.ratio_db > 40.0 ? OW_INTERMOD_CLEAN : r.ratio_db > 30.0 ? OW_INTERMOD_OK : r.ratio_db > 20.0 ? OW_INTERMOD_MARGINAL : OW_INTERMOD_DIRTY;
    for (int k = 0; k < 6; ++k) {
        if (p.detail[k] < 0) continue;
        ow_intermod_detail& d = r.products[k];
        d.intermod_mag = mag((uint32_t)p.detail[k]);
        d.nearest_mag = mag((uint32_t)p.detail[k] + 1);
        d.ratio_db = d.nearest_mag > 1e-15 ? 20.0 * std::log10(d.intermod_mag / d.nearest_mag) : 0.0;
    }
}
// the static part of a row, and its probes
void start_intermod_row(const ow_note_job& j, size_t start, size_t end, ow_intermod_row& r, Probes& p) {
    std::memset(&r, 0, sizeof(r));
    ow_intermod_report rep;
    intermod_risk(j.note, rep);
    make_probes(rep, p);
    r.midi = j.note; r.velocity = j.velocity;
    r.too_short = end <= start ? 1 : 0;
    r.n_harmonics = p.n_harm; r.n_midpoints = p.n_mid;
    r.window_start = (uint32_t)start; r.window_end = (uint32_t)end;
    r.fundamental_hz = rep.fundamental_hz;
    for (int k = 0; k < 6; ++k) {
        ow_intermod_detail& d = r.products[k];
        d.mode = rep.products[k].mode; d.nearest_integer = rep.products[k].nearest_integer;
        d.intermod_freq = rep.products[k].mode_ratio * rep.fundamental_hz;
        d.nearest_freq = (double)rep.products[k].nearest_integer * rep.fundamental_hz;
        d.risk_score = rep.products[k].risk_score;
        d.listed = p.detail[k] >= 0 ? 1 : 0;
    }
}

// ---- overshoot's windows and finish (:2173-2214, rms_window :2231-2239) -------------------------------------------------------------
owdev::OwNaWindows overshoot_windows(size_t n) {
    auto at = [&](double t) { return (uint32_t)std::min(rust_as_usize(t * SR), n); };
    owdev::OwNaWindows w;
    std::memset(&w, 0, sizeof(w));
    w.count = 4;
    w.start[0] = 0; w.end[0] = at(0.010); w.kind[0] = owdev::NA_WIN_PEAK;
    w.start[1] = 0; w.end[1] = at(0.050); w.kind[1] = owdev::NA_WIN_PEAK;
    w.start[2] = at(0.100); w.end[2] = at(0.200); w.kind[2] = owdev::NA_WIN_SUM_SQ;
    w.start[3] = at(1.000); w.end[3] = at(1.500); w.kind[3] = owdev::NA_WIN_SUM_SQ;
    return w;
}
void finish_overshoot(const ow_note_job& j, const owdev::OwNaWindows& w, const double* s, ow_overshoot_row& r) {
    auto rms = [&](int k) { return w.end[k] <= w.start[k] ? 0.0 : std::sqrt(s[k] / (double)(w.end[k] - w.start[k])); };
    std::memset(&r, 0, sizeof(r));
    r.note = j.note; r.velocity = j.velocity;
    r.peak_0_10 = s[0]; r.peak_0_50 = s[1];
    r.rms_100_200 = rms(2); r.rms_1000_1500 = rms(3);
    r.overshoot_db = r.rms_100_200 > 1e-15 ? 20.0 * std::log10(r.peak_0_10 / r.rms_100_200) : std::nan("");
    r.bark_decay_db = r.rms_1000_1500 > 1e-15 ? 20.0 * std::log10(r.peak_0_50 / r.rms_1000_1500) : std::nan("");
    r.pk_dbfs = measure::to_dbfs(r.peak_0_10);
    r.rms1_dbfs = measure::to_dbfs(r.rms_100_200);
    r.rms2_dbfs = measure::to_dbfs(r.rms_1000_1500);
}
}  // namespace note_audit
}  // namespace

extern "C" {
int ow_intermod_risk(uint8_t midi, ow_intermod_report* out) {
    try {
        if (!out) throw std::runtime_error("null argument");
        note_audit::intermod_risk(midi, *out);
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_intermod_risk: ") + ex.what()); return -1; }
}

int ow_intermod_probes(uint8_t midi, double* freqs_out, uint32_t* n_harmonics_out, uint32_t* n_midpoints_out) {
    try {
        if (!freqs_out || !n_harmonics_out || !n_midpoints_out) throw std::runtime_error("null argument");
        check_note_velocity("", midi, 0);
        ow_intermod_report rep;
        note_audit::intermod_risk(midi, rep);
        note_audit::Probes p;
        note_audit::make_probes(rep, p);
        std::copy(p.freq, p.freq + p.count, freqs_out);
        *n_harmonics_out = p.n_harm; *n_midpoints_out = p.n_mid;
        return (int)p.count;
    } catch (const std::exception& ex) { set_err(std::string("ow_intermod_probes: ") + ex.what()); return -1; }
}

int ow_dft_magnitudes(const double* signals, size_t n_rows, size_t stride, size_t start, size_t end, double sample_rate, const double* freqs,
                      size_t n_probes, int device, int signals_is_device, double* mags_out) {
    try {
        if (end > stride) throw std::runtime_error("window end " + std::to_string(end) + " beyond the stride of " + std::to_string(stride) + " samples");
        if (end <= start) throw std::runtime_error("empty window: end " + std::to_string(end) + " <= start " + std::to_string(start));
        check_positive_finite("", "sample_rate", sample_rate);
        if (n_rows == 0 || n_probes == 0) return 0;
        if (!signals || !freqs || !mags_out) throw std::runtime_error("null argument");
        if (n_probes > 0x7fffffffull || n_rows > 0xffffffffull / 2) throw std::runtime_error("too many probes or rows");
        if (stride > note_audit::BUDGET_BYTES / sizeof(double) / n_rows || n_probes > note_audit::BUDGET_BYTES / (3 * sizeof(double)) / n_rows)
            throw std::runtime_error("rows or probe tables above the device-memory budget of " + std::to_string(note_audit::BUDGET_BYTES >> 30) + " GiB: call in parts");
        require_device(device);
        StreamOwner so;
        so.create();
        DevMem d_sig, d_freqs, d_sums;
        const double* src = signals;
        if (!signals_is_device) {
            d_sig.alloc(sizeof(double) * n_rows * stride);
            HIP_OK(hipMemcpyAsync(d_sig.p, signals, sizeof(double) * n_rows * stride, hipMemcpyHostToDevice, so.s));
            src = d_sig.as<double>();
        }
        const size_t slots = n_rows * n_probes;
        d_freqs.alloc(sizeof(double) * slots);
        d_sums.alloc(sizeof(double) * 2 * slots);
        std::vector<double> sums(2 * slots, 0.0);
        HIP_OK(hipMemcpyAsync(d_freqs.p, freqs, sizeof(double) * slots, hipMemcpyHostToDevice, so.s));
        note_audit::launch_dft(src, n_rows, stride, start, end, sample_rate, d_freqs.as<double>(), n_probes, d_sums.as<double>(), so.s);
        HIP_OK(hipMemcpyAsync(sums.data(), d_sums.p, sizeof(double) * 2 * slots, hipMemcpyDeviceToHost, so.s));
        HIP_OK(hipStreamSynchronize(so.s));
        const double n = (double)(end - start);                                 // signal.len() as f64
        for (size_t k = 0; k < slots; ++k) mags_out[k] = std::isnan(freqs[k]) ? 0.0 : measure::dft_magnitude(sums[2 * k], sums[2 * k + 1], n);
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_dft_magnitudes: ") + ex.what()); return -1; }
}

long long ow_intermod_audit(const ow_note_job* jobs, size_t n_jobs, const ow_intermod_cfg* cfg, ow_intermod_row* rows_out, double* audio_out,
                            size_t audio_stride) {
    try {
        const size_t n = note_audit::checked_samples(cfg, "ow_intermod_cfg.struct_size / job_size do", audio_out, audio_stride);
        if (n_jobs == 0) return (long long)n;
        note_audit::check_jobs(jobs, n_jobs, rows_out);
        const size_t start = rust_as_usize(0.5 * note_audit::SR);                                  // (0.5 * BASE_SR) as usize
        const size_t end = rust_as_usize(std::fmin(2.0 * note_audit::SR, (double)n));              // (2.0 * BASE_SR).min(signal.len() as f64) as usize
        std::vector<note_audit::Probes> probes(n_jobs);
        for (size_t i = 0; i < n_jobs; ++i) note_audit::start_intermod_row(jobs[i], start, end, rows_out[i], probes[i]);
        const bool too_short = end <= start;
        if (n == 0 || (too_short && !audio_out)) return (long long)n;
        const size_t P = OW_INTERMOD_MAX_PROBES;
        DevMem m_freqs, m_sums;
        std::vector<double> hf, hs;
        bool sized = false;
        note_audit::for_each_chunk(
            cfg->device, jobs, n_jobs, n, /*extra_bytes_per_job=*/sizeof(double) * 3 * P, audio_out, audio_stride,
            [&](size_t c0, size_t cn, const double* d_rows, size_t stride, hipStream_t st) {
                if (too_short) return;
                if (!sized) {                                    // the first chunk is the largest
                    m_freqs.alloc(sizeof(double) * cn * P);
                    m_sums.alloc(sizeof(double) * 2 * cn * P);
                    sized = true;
                }
                hf.assign(cn * P, std::nan(""));
                for (size_t i = 0; i < cn; ++i) std::copy(probes[c0 + i].freq, probes[c0 + i].freq + probes[c0 + i].count, hf.begin() + i * P);
                hs.assign(2 * cn * P, 0.0);
                HIP_OK(hipMemcpyAsync(m_freqs.p, hf.data(), sizeof(double) * cn * P, hipMemcpyHostToDevice, st));
                note_audit::launch_dft(d_rows, cn, stride, start, end, note_audit::SR, m_freqs.as<double>(), P, m_sums.as<double>(), st);
                HIP_OK(hipMemcpyAsync(hs.data(), m_sums.p, sizeof(double) * 2 * cn * P, hipMemcpyDeviceToHost, st));
            },
            [&](size_t c0, size_t cn) {
                if (too_short) return;
                for (size_t i = 0; i < cn; ++i) note_audit::finish_intermod(probes[c0 + i], hs.data() + 2 * i * P, (double)(end - start), rows_out[c0 + i]);
            });
        return (long long)n;
    } catch (const std::exception& ex) { set_err(std::string("ow_intermod_audit: ") + ex.what()); return -1; }
}

long long ow_overshoot(const ow_note_job* jobs, size_t n_jobs, const ow_overshoot_cfg* cfg, ow_overshoot_row* rows_out, double* audio_out,
                       size_t audio_stride) {
    try {
        const size_t n = note_audit::checked_samples(cfg, "ow_overshoot_cfg.struct_size / job_size do", audio_out, audio_stride);
        if (n_jobs == 0) return (long long)n;
        note_audit::check_jobs(jobs, n_jobs, rows_out);
        const owdev::OwNaWindows w = note_audit::overshoot_windows(n);
        if (n == 0) {                                            // every window empty
            const double zeros[OW_NA_MAX_WINDOWS] = {0.0, 0.0, 0.0, 0.0};
            for (size_t i = 0; i < n_jobs; ++i) note_audit::finish_overshoot(jobs[i], w, zeros, rows_out[i]);
            return 0;
        }
        DevMem m_stats;
        std::vector<double> hs;
        note_audit::for_each_chunk(
            cfg->device, jobs, n_jobs, n, /*extra_bytes_per_job=*/sizeof(double) * OW_NA_MAX_WINDOWS, audio_out, audio_stride,
            [&](size_t, size_t cn, const double* d_rows, size_t stride, hipStream_t st) {
                if (!m_stats.p) m_stats.alloc(sizeof(double) * cn * OW_NA_MAX_WINDOWS);       // the first chunk is the largest
                hs.assign(cn * OW_NA_MAX_WINDOWS, 0.0);
                note_audit::launch_windows(d_rows, cn, stride, w, m_stats.as<double>(), st);
                HIP_OK(hipMemcpyAsync(hs.data(), m_stats.p, sizeof(double) * cn * w.count, hipMemcpyDeviceToHost, st));
            },
            [&](size_t c0, size_t cn) {
                for (size_t i = 0; i < cn; ++i) note_audit::finish_overshoot(jobs[c0 + i], w, hs.data() + i * w.count, rows_out[c0 + i]);
            });
        return (long long)n;
    } catch (const std::exception& ex) { set_err(std::string("ow_overshoot: ") + ex.what()); return -1; }
}

// ---- include/openwurli_hip_test.h ----------------------------------------------------------------------------------------------------
// k_window_stats on given host rows (the entry points reach it only behind a render): out [n_rows][n_windows]
int ow_debug_window_stats(const double* signals, size_t n_rows, size_t stride, const uint32_t* starts, const uint32_t* ends, const uint32_t* kinds,
                          size_t n_windows, int device, double* out) {
    try {
        if (!signals || !starts || !ends || !kinds || !out) throw std::runtime_error("null argument");
        if (n_rows == 0 || n_windows == 0 || n_windows > OW_NA_MAX_WINDOWS) throw std::runtime_error("1.." + std::to_string(OW_NA_MAX_WINDOWS) + " windows, at least one row");
        if (n_rows > 0xffffffffull || stride > note_audit::BUDGET_BYTES / sizeof(double) / n_rows) throw std::runtime_error("too many rows");
        owdev::OwNaWindows w;
        std::memset(&w, 0, sizeof(w));
        w.count = (uint32_t)n_windows;
        for (size_t k = 0; k < n_windows; ++k) {
            if (ends[k] > stride || starts[k] > ends[k] || kinds[k] > owdev::NA_WIN_SUM_SQ) throw std::runtime_error("window " + std::to_string(k) + " out of range");
            w.start[k] = starts[k]; w.end[k] = ends[k]; w.kind[k] = kinds[k];
        }
        require_device(device);
        StreamOwner so;
        so.create();
        DevMem d_sig, d_out;
        d_sig.alloc(sizeof(double) * n_rows * stride);
        d_out.alloc(sizeof(double) * n_rows * n_windows);
        HIP_OK(hipMemcpyAsync(d_sig.p, signals, sizeof(double) * n_rows * stride, hipMemcpyHostToDevice, so.s));
        note_audit::launch_windows(d_sig.as<double>(), n_rows, stride, w, d_out.as<double>(), so.s);
        HIP_OK(hipMemcpyAsync(out, d_out.p, sizeof(double) * n_rows * n_windows, hipMemcpyDeviceToHost, so.s));
        HIP_OK(hipStreamSynchronize(so.s));
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_debug_window_stats: ") + ex.what()); return -1; }
}
// the voices' note table as k_note_table builds it: out [OW_TEST_NOTE_TABLE_FIELDS][64], field-major, note index = midi - 33
int ow_debug_note_table(double* out, int device) {
    try {
        if (!out) throw std::runtime_error("null argument");
        static_assert(OW_TEST_NOTE_TABLE_FIELDS == NT_COUNT, "openwurli_hip_test.h and ow_types.h disagree");
        OfflineCall call(device, note_audit::SR, OW_PREAMP_LEGACY8, /*note_table=*/true);
        HIP_OK(hipMemcpyAsync(out, call.nt(), sizeof(double) * NT_COUNT * 64, hipMemcpyDeviceToHost, call.st()));
        HIP_OK(hipStreamSynchronize(call.st()));
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_debug_note_table: ") + ex.what()); return -1; }
}
}  // extern "C"
