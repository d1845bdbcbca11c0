// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: `preamp-bench centroid-track`
// (tools/preamp-bench/src/main.rs:1925-2135), the spectral centroid over time, for many notes per call.
namespace {
namespace centroid {
const double SR = 44100.0;                         // BASE_SR, main.rs:27
const size_t BUDGET_BYTES = size_t(8) << 30;       // per chunk (a job takes a voice row and an output row), as the calibration sweep's
inline size_t ms_to_samples(double ms) { return rust_as_usize((ms / 1000.0) * SR); }        // main.rs:2012-2014

// which frames and bins exist (main.rs:1933-1935, 2046); throws what the entry points refuse
owdev::OwCentroidGrid make_grid(size_t len, size_t window, size_t hop, size_t end) {
    if (hop == 0) throw std::runtime_error("hop_samples is 0: the reference's frame loop would never end");
    if (window == 0) throw std::runtime_error("window_samples is 0: no bin in range");
    if (window > OW_CENTROID_MAX_WINDOW)
        throw std::runtime_error("window of " + std::to_string(window) + " samples: more than OW_CENTROID_MAX_WINDOW = " + std::to_string(OW_CENTROID_MAX_WINDOW));
    if (hop > 0xffffffffull) throw std::runtime_error("hop_samples out of range");
    const double freq_resolution = SR / (double)window;
    const size_t k_min = rust_as_usize(std::ceil(50.0 / freq_resolution));
    const size_t k_max = std::min(rust_as_usize(std::floor((SR / 4.0) / freq_resolution)), window / 2);
    if (k_min > k_max)
        throw std::runtime_error("window of " + std::to_string(window) + " samples has no bin in range (k_min " + std::to_string(k_min) + " > k_max " +
                                 std::to_string(k_max) + ")");
    // while pos + window <= len && pos + window / 2 <= end { ..; pos += hop }  (integer half)
    size_t frames = 0;
    if (window <= len && window / 2 <= end) frames = std::min((len - window) / hop, (end - window / 2) / hop) + 1;
    if (frames > 0x7fffffffull) throw std::runtime_error("too many frames");
    owdev::OwCentroidGrid g;
    g.window = (uint32_t)window; g.hop = (uint32_t)hop; g.frames = (uint32_t)frames;
    g.k_min = (uint32_t)k_min; g.k_max = (uint32_t)k_max; g.row0 = 0; g.freq_resolution = freq_resolution;
    return g;
}
// threads per workgroup: the multiple of 64 (at most 256) that wastes the fewest lanes over the bins' passes, the larger one on a tie
inline unsigned block_threads(uint32_t bins) {
    unsigned best = 64, best_cost = ~0u;
    for (unsigned t = 64; t <= 256; t += 64) {
        const unsigned cost = ((bins + t - 1) / t) * t;
        if (cost <= best_cost) { best = t; best_cost = cost; }
    }
    return best;
}
// the periodic Hann table of the command (:2021-2023), host libm
std::vector<double> hann_table(size_t n) {
    std::vector<double> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = 0.5 * (1.0 - std::cos(2.0 * 3.14159265358979323846 * (double)i / (double)n));
    return h;
}
// d_sig [rows][stride] -> d_frames [rows][g.frames], on st (no synchronisation)
void launch_frames(const double* d_sig, size_t rows, size_t stride, const double* d_hann, owdev::OwCentroidGrid g, double* d_frames, hipStream_t st) {
    if (g.frames == 0 || rows == 0) return;
    const uint32_t bins = g.k_max - g.k_min + 1;
    const size_t lds = sizeof(double) * ((size_t)g.window + bins);
    for (size_t r0 = 0; r0 < rows; r0 += 65535) {
        g.row0 = (uint32_t)r0;
        owdev::k_centroid_frames<<<dim3(g.frames, (unsigned)std::min<size_t>(65535, rows - r0)), dim3(block_threads(bins)), lds, st>>>(d_sig, stride, d_hann, g, d_frames);
        HIP_OK(hipGetLastError());
    }
}
struct Targets { double a_lo, a_hi, s_lo, s_hi, d_lo, d_hi; };
inline Targets targets(uint8_t midi) {                 // main.rs:2079-2088
    if (midi <= 48) return {600.0, 1000.0, 500.0, 800.0, -200.0, -50.0};
    if (midi <= 72) return {600.0, 1200.0, 600.0, 1000.0, -240.0, -30.0};
    return {800.0, 1600.0, 800.0, 1400.0, -250.0, -30.0};
}
// the summary of one job from its frames (:2042-2069, 2090-2129)
void summarise(uint8_t note, const double* c, const owdev::OwCentroidGrid& g, ow_centroid_row& r) {
    std::memset(&r, 0, sizeof(r));
    const Targets t = targets(note);
    r.attack_lo = t.a_lo; r.attack_hi = t.a_hi; r.sustain_lo = t.s_lo; r.sustain_hi = t.s_hi; r.drift_lo = t.d_lo; r.drift_hi = t.d_hi;
    r.frame10 = r.frame300 = -1;
    for (uint32_t j = 0; j < g.frames; ++j) {
        const size_t pos = (size_t)j * g.hop;
        const double center_ms = ((double)pos + (double)g.window / 2.0) / SR * 1000.0;      // float half
        if (r.frame10 < 0 && center_ms >= 10.0) { r.frame10 = (int32_t)j; r.c10 = c[j]; r.has_c10 = 1; }
        if (r.frame300 < 0 && center_ms >= 300.0) { r.frame300 = (int32_t)j; r.c300 = c[j]; r.has_c300 = 1; }
    }
    if (r.has_c10) r.attack_status = (r.c10 >= t.a_lo && r.c10 <= t.a_hi) ? OW_CENTROID_OK : OW_CENTROID_MISS;
    if (r.has_c300) r.sustain_status = (r.c300 >= t.s_lo && r.c300 <= t.s_hi) ? OW_CENTROID_OK : OW_CENTROID_MISS;
    if (r.has_c10 && r.has_c300) {
        r.drift = r.c300 - r.c10;
        r.drift_status = (r.drift >= t.d_lo && r.drift <= t.d_hi) ? OW_CENTROID_OK : OW_CENTROID_MISS;
    }
}
// checks of ow_centroid_cfg shared by ow_centroid_frame_count and ow_centroid_track; returns the grid, *n_out = samples per job
owdev::OwCentroidGrid checked_grid(const ow_centroid_cfg* cfg, size_t* n_out) {
    if (!cfg) throw std::runtime_error("null argument");
    if (cfg->struct_size != sizeof(ow_centroid_cfg) || cfg->job_size != sizeof(ow_centroid_job))
        throw std::runtime_error(abi_mismatch("ow_centroid_cfg.struct_size / job_size do"));
    require_legacy_chain(cfg->preamp_kind, cfg->power_amp_kind);
    const double x = cfg->duration_s * SR;               // Voice::render_note_with_scale: (duration * sample_rate) as usize
    if (!(x < 2147483648.0)) throw std::runtime_error("duration_s must give fewer than 2^31 samples");
    const size_t n = rust_as_usize(x);
    *n_out = n;
    return make_grid(n, ms_to_samples(cfg->window_ms), ms_to_samples(cfg->hop_ms), ms_to_samples(cfg->end_ms));
}
}  // namespace centroid
}  // namespace

extern "C" {
long long ow_centroid_frame_count(const ow_centroid_cfg* cfg) {
    try {
        size_t n = 0;
        return (long long)centroid::checked_grid(cfg, &n).frames;
    } catch (const std::exception& ex) { set_err(std::string("ow_centroid_frame_count: ") + ex.what()); return -1; }
}

long long ow_centroid_analyze(const double* signals, size_t n_rows, size_t stride, size_t len, size_t window_samples, size_t hop_samples,
                              size_t end_sample, int device, int signals_is_device, double* frames_out, size_t frames_stride) {
    try {
        if (len > stride) throw std::runtime_error("stride smaller than the " + std::to_string(len) + " samples of a row");
        owdev::OwCentroidGrid g = centroid::make_grid(len, window_samples, hop_samples, end_sample);
        if (g.frames == 0 || n_rows == 0) return g.frames;
        if (!signals || !frames_out) throw std::runtime_error("null argument");
        if (frames_stride < g.frames) throw std::runtime_error("frames_stride smaller than the " + std::to_string(g.frames) + " frames of a row");
        require_device(device);
        StreamOwner so;
        so.create();
        DevMem d_sig, d_hann, d_frames;
        const double* src = signals;
        if (!signals_is_device) {
            d_sig.alloc(sizeof(double) * n_rows * stride);
            HIP_OK(hipMemcpyAsync(d_sig.p, signals, sizeof(double) * n_rows * stride, hipMemcpyHostToDevice, so.s));
            src = d_sig.as<double>();
        }
        const std::vector<double> hann = centroid::hann_table(g.window);
        d_hann.alloc(sizeof(double) * hann.size());
        d_frames.alloc(sizeof(double) * n_rows * g.frames);
        HIP_OK(hipMemcpyAsync(d_hann.p, hann.data(), sizeof(double) * hann.size(), hipMemcpyHostToDevice, so.s));
        centroid::launch_frames(src, n_rows, stride, d_hann.as<double>(), g, d_frames.as<double>(), so.s);
        rows_to_host(frames_out, frames_stride, d_frames.p, g.frames, g.frames, n_rows, so.s);
        HIP_OK(hipStreamSynchronize(so.s));
        return g.frames;
    } catch (const std::exception& ex) { set_err(std::string("ow_centroid_analyze: ") + ex.what()); return -1; }
}

long long ow_centroid_track(const ow_centroid_job* jobs, size_t n_jobs, const ow_centroid_cfg* cfg, ow_centroid_row* rows_out, double* frames_out,
                            size_t frames_stride, double* audio_out, size_t audio_stride) {
    try {
        size_t n = 0;
        const owdev::OwCentroidGrid g = centroid::checked_grid(cfg, &n);
        if (frames_out && frames_stride < g.frames) throw std::runtime_error("frames_stride smaller than the " + std::to_string(g.frames) + " frames of a job");
        if (audio_out && audio_stride < n) throw std::runtime_error("audio_stride smaller than the " + std::to_string(n) + " samples of a job");
        if (n_jobs == 0) return g.frames;
        if (!jobs || !rows_out || (!frames_out && g.frames > 0)) throw std::runtime_error("null argument");
        if (n_jobs > (size_t)INT32_MAX / 64) throw std::runtime_error("too many jobs");
        for (size_t i = 0; i < n_jobs; ++i) {
            const ow_centroid_job& j = jobs[i];
            const std::string at = "job " + std::to_string(i) + ": ";
            check_note_velocity(at, j.note, j.velocity);
            check_positive_finite(at, "r_ldr", j.r_ldr);
            check_finite(at, "volume", j.volume);
            check_finite(at, "speaker", j.speaker);
            if (j.has_displacement_scale) check_finite(at, "displacement_scale", j.displacement_scale);
        }
        if (n == 0) {                                      // an empty render: no frame, both "no data" lines
            for (size_t i = 0; i < n_jobs; ++i) centroid::summarise(jobs[i].note, nullptr, g, rows_out[i]);
            return 0;
        }
        OfflineCall call(cfg->device, centroid::SR, OW_PREAMP_LEGACY8, /*note_table=*/true);   // the preamp at OVERSAMPLED_SR = 88 200 Hz
        hipStream_t st = call.st();
        const size_t stride = (size_t)row_stride((long long)n);
        const size_t row_bytes = sizeof(double) * stride;
        const size_t chunk = budget_chunk(centroid::BUDGET_BYTES, 2 * row_bytes, call.sw.centroid_chunk, n_jobs);
        DevMem m_vrec, m_jobs, m_reed, m_out, m_hann, m_frames;         // released on every exit path
        m_vrec.alloc(sizeof(double) * ((chunk + 63) / 64) * OW_VREC_DOUBLES);
        m_jobs.alloc(sizeof(owdev::OwJobDev) * chunk);
        m_reed.alloc(row_bytes * chunk);
        m_out.alloc(row_bytes * chunk);
        m_frames.alloc(sizeof(double) * chunk * std::max<size_t>(g.frames, 1));
        const std::vector<double> hann = centroid::hann_table(g.window);
        m_hann.alloc(sizeof(double) * hann.size());
        HIP_OK(hipMemcpyAsync(m_hann.p, hann.data(), sizeof(double) * hann.size(), hipMemcpyHostToDevice, st));
        const JobChainCfg cc{centroid::SR, cfg->device, OW_PREAMP_LEGACY8, OW_POWER_AMP_BEHAVIORAL, 0};
        std::vector<owdev::OwJobDev> hj;
        for (size_t c0 = 0; c0 < n_jobs; c0 += chunk) {
            const size_t cn = std::min(chunk, n_jobs - c0);
            hj.assign(cn, owdev::OwJobDev{});
            for (size_t i = 0; i < cn; ++i) {
                const ow_centroid_job& j = jobs[c0 + i];
                owdev::OwJobDev& d = hj[i];
                std::memset(&d, 0, sizeof(d));
                d.note = j.note; d.velocity = j.velocity;
                d.mlp = 0; d.no_attack_noise = 0;            // Voice::render_note_with_scale: MLP off, attack noise on (voice.rs:201-221)
                d.poweramp = j.no_poweramp ? 0 : 1; d.no_preamp = j.no_preamp ? 1 : 0;
                d.has_ds = j.has_displacement_scale ? 1 : 0; d.displacement_scale = j.displacement_scale;
                d.dc_at_ldr = 1;                             // set_ldr_resistance(r_ldr), then reset() (main.rs:1989-1991)
                d.volume = j.volume; d.speaker = j.speaker; d.r_ldr = j.r_ldr; d.tremolo_depth = 0.0;
            }
            HIP_OK(hipMemcpyAsync(m_jobs.p, hj.data(), sizeof(owdev::OwJobDev) * cn, hipMemcpyHostToDevice, st));
            owdev::k_job_voice<<<dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, st>>>(call.dK(), call.nt(), m_vrec.as<double>(), m_jobs.as<owdev::OwJobDev>(),
                                                                                      m_reed.as<double>(), (int)cn, (long long)n, (long long)stride);
            HIP_OK(hipGetLastError());
            run_job_chain(call, cc, hj, m_jobs.as<owdev::OwJobDev>(), m_reed.as<double>(), m_out.as<double>(), cn, (long long)n, (long long)stride);
            centroid::launch_frames(m_out.as<double>(), cn, stride, m_hann.as<double>(), g, m_frames.as<double>(), st);
            if (g.frames > 0) rows_to_host(frames_out + c0 * frames_stride, frames_stride, m_frames.p, g.frames, g.frames, cn, st);
            if (audio_out) rows_to_host(audio_out + c0 * audio_stride, audio_stride, m_out.p, stride, n, cn, st);
            HIP_OK(hipStreamSynchronize(st));               // the buffers are reused by the next chunk
        }
        for (size_t i = 0; i < n_jobs; ++i) centroid::summarise(jobs[i].note, frames_out ? frames_out + i * frames_stride : nullptr, g, rows_out[i]);
        return g.frames;
    } catch (const std::exception& ex) { set_err(std::string("ow_centroid_track: ") + ex.what()); return -1; }
}
}  // extern "C"
