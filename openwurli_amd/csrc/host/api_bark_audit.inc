// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: `preamp-bench bark-audit`
// (tools/preamp-bench/src/main.rs:551-664), many (note, velocity) jobs per call.  k_bark_voice renders reed and pickup, the job chain at a
// static 1 Mohm and volume 1.0 is process_oversampled, k_dft_probes reduces the pickup and the preamp rows, the host finishes.
namespace {
namespace bark {
// OW_BARK_ROW=0/1 forces the kernel of the legacy preamp; otherwise a row of sixteen lanes per solver state (k_bark_chain_row: five
// wavefronts per eight jobs) for launches of up to 4 096 jobs, the lane pair (k_job_chain<false>) above.  The threshold started as
// job_chain_row's 1 024, copied; tools/bench_bark_audit.py --sweep then measured whole calls of 0.5 s jobs, row against lane pair:
// 512 jobs 55.4 / 108.3 ms, 1 024 56.3 / 108.9, 2 048 57.8 / 110.0, 4 096 99.0 / 109.2 (the row form's workgroups take a second round
// there); nothing above 4 096 has been measured, so the lane pair keeps it.  The melange preamp always takes k_job_chain<true>.
static inline bool chain_row(const Switches& sw, size_t n_jobs) { return sw.bark_row >= 0 ? sw.bark_row == 1 : n_jobs <= 4096; }

// validated sizes of a call: samples per job, first sample of the measuring window
struct Sizes { size_t n, m0; };
Sizes checked_sizes(const ow_bark_cfg* cfg, const double* taps_out, size_t tap_stride) {
    if (!cfg) throw std::runtime_error("null argument");
    if (cfg->struct_size != sizeof(ow_bark_cfg) || cfg->job_size != sizeof(ow_note_job))
        throw std::runtime_error(abi_mismatch("ow_bark_cfg.struct_size / job_size do"));
    require_known_kinds(cfg->preamp_kind);
    if (!(std::isfinite(cfg->duration_s) && cfg->duration_s >= 0.0)) throw std::runtime_error("duration_s is not a finite non-negative number");
    if (!(std::isfinite(cfg->measure_start_s) && cfg->measure_start_s >= 0.0)) throw std::runtime_error("measure_start_s is not a finite non-negative number");
    const double x = cfg->duration_s * note_audit::SR;                  // (duration * BASE_SR) as usize, main.rs:607
    if (!(x < 2147483648.0)) throw std::runtime_error("duration_s must give fewer than 2^31 samples");
    Sizes s;
    s.n = rust_as_usize(x);
    s.m0 = rust_as_usize(cfg->measure_start_s * note_audit::SR);        // (measure_start * BASE_SR) as usize, main.rs:608
    // the reference's constants cannot reach this state (its slice would panic)
    if (s.n > 0 && s.m0 >= s.n)
        throw std::runtime_error("measure_start_s leaves no sample to measure: the window starts at " + std::to_string(s.m0) + " of " + std::to_string(s.n) + " samples");
    if (taps_out && tap_stride < s.n) throw std::runtime_error("tap_stride smaller than the " + std::to_string(s.n) + " samples of a job");
    return s;
}
// tables::pickup_displacement_scale (tables.rs:279-288) on the host, for rows no kernel ran for
double displacement_scale(int midi) {
    return calib::fclamp(0.85 * std::pow(calib::reed_compliance(midi) / calib::reed_compliance(60), 0.75), 0.02, 0.95);
}
void start_row(const ow_note_job& j, const Sizes& s, ow_bark_row& r) {
    std::memset(&r, 0, sizeof(r));
    r.note = j.note; r.velocity = j.velocity;
    r.window_start = (uint32_t)std::min(s.m0, s.n); r.window_end = (uint32_t)s.n;
    r.fundamental_hz = owdev::midi_to_freq((double)j.note);             // params.fundamental_hz: the undetuned fundamental
}
// sums: (re, im) at f0, (re, im) at 2 f0 of one row's window
void ratio(const double* sums, double n_window, double& h1, double& h2, double& h2_h1) {
    h1 = measure::dft_magnitude(sums[0], sums[1], n_window);
    h2 = measure::dft_magnitude(sums[2], sums[3], n_window);
    h2_h1 = h1 > 1e-15 ? h2 / h1 : 0.0;                                 // main.rs:625, 635
}
}  // namespace bark
}  // namespace

extern "C" {
long long ow_bark_audit(const ow_note_job* jobs, size_t n_jobs, const ow_bark_cfg* cfg, ow_bark_row* rows_out, double* taps_out, size_t tap_stride) {
    try {
        const bark::Sizes sz = bark::checked_sizes(cfg, taps_out, tap_stride);
        const size_t n = sz.n, m0 = sz.m0;
        if (n_jobs == 0) return (long long)n;
        note_audit::check_jobs(jobs, n_jobs, rows_out);
        for (size_t i = 0; i < n_jobs; ++i) bark::start_row(jobs[i], sz, rows_out[i]);
        if (n == 0) {                                                  // empty rows: every peak and magnitude is 0
            for (size_t i = 0; i < n_jobs; ++i) rows_out[i].displacement_scale = bark::displacement_scale(jobs[i].note);
            return 0;
        }
        const bool mel = cfg->preamp_kind == OW_PREAMP_MELANGE12;
        OfflineCall call(cfg->device, note_audit::SR, cfg->preamp_kind, /*note_table=*/true);
        hipStream_t st = call.st();
        const OwConsts* dK = call.dK();
        const size_t stride = (size_t)row_stride((long long)n);
        const size_t row_bytes = sizeof(double) * stride;
        const int n_rows = taps_out ? 3 : 2;
        // per job: its pickup and preamp rows (its reed row with taps), its share of a block's voice records (one block of 64 jobs), its job
        // record, its figures of k_bark_voice and its probe slots (2 frequencies, 2 rows x 2 probes x (re, im))
        const size_t job_bytes = row_bytes * (size_t)n_rows + sizeof(double) * (OW_VREC_DOUBLES / 64) + sizeof(owdev::OwJobDev) +
                                 sizeof(double) * (owdev::BARK_ST_COUNT + 2 + 8);
        const size_t chunk = budget_chunk(note_audit::BUDGET_BYTES - sizeof(double) * OW_VREC_DOUBLES, job_bytes, call.sw.bark_chunk, n_jobs);
        DevMem m_vrec, m_jobs, m_reed, m_pu, m_pre, m_stats, m_freqs, m_sums;          // released on every exit path
        m_vrec.alloc(sizeof(double) * ((chunk + 63) / 64) * OW_VREC_DOUBLES);
        m_jobs.alloc(sizeof(owdev::OwJobDev) * chunk);
        if (taps_out) m_reed.alloc(row_bytes * chunk);
        m_pu.alloc(row_bytes * chunk);
        m_pre.alloc(row_bytes * chunk);
        m_stats.alloc(sizeof(double) * owdev::BARK_ST_COUNT * chunk);
        m_freqs.alloc(sizeof(double) * 2 * chunk);
        m_sums.alloc(sizeof(double) * 8 * chunk);
        const double* settled = mel ? call.mel_settled() : nullptr;
        std::vector<owdev::OwJobDev> hj;
        std::vector<double> hf, hstats, hsums;
        // declared behind every buffer the queued work touches: on any way out, a thrown HIP error included, the stream is waited for first
        const note_audit::StreamDrain drain{st};
        const double n_window = (double)(n - m0);                      // signal.len() as f64 of the steady slice
        for (size_t c0 = 0; c0 < n_jobs; c0 += chunk) {
            const size_t cn = std::min(chunk, n_jobs - c0);
            const int ci = (int)cn;
            hj.assign(cn, owdev::OwJobDev{});
            hf.assign(2 * cn, 0.0);
            for (size_t i = 0; i < cn; ++i) {
                owdev::OwJobDev& d = hj[i];
                std::memset(&d, 0, sizeof(d));
                d.note = jobs[c0 + i].note; d.velocity = jobs[c0 + i].velocity;
                // the chain: new() + set_ldr_resistance(1e6) and no reset() is the batch job's start state for both kinds (see ow_calibrate);
                // JOB_OUT_PA_INPUT at volume 1.0: pre x 1.0 x 1.0 = pre, bit for bit
                d.volume = 1.0; d.speaker = 0.0; d.r_ldr = 1000000.0;
                hf[2 * i] = rows_out[c0 + i].fundamental_hz;
                hf[2 * i + 1] = 2.0 * rows_out[c0 + i].fundamental_hz;   // freq * 2.0, main.rs:579
            }
            hstats.assign(owdev::BARK_ST_COUNT * cn, 0.0);
            hsums.assign(8 * cn, 0.0);
            owdev::OwJobDev* d_jobs = m_jobs.as<owdev::OwJobDev>();
            HIP_OK(hipMemcpyAsync(d_jobs, hj.data(), sizeof(owdev::OwJobDev) * cn, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(m_freqs.p, hf.data(), sizeof(double) * 2 * cn, hipMemcpyHostToDevice, st));
            owdev::k_bark_voice<<<dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, st>>>(dK, call.nt(), m_vrec.as<double>(), d_jobs, m_reed.as<double>(),
                                                                                      m_pu.as<double>(), m_stats.as<double>(), ci, (long long)n,
                                                                                      (long long)m0, (long long)stride);
            HIP_OK(hipGetLastError());
            if (mel)
                owdev::k_job_chain<true><<<dim3((unsigned)((cn + 31) / 32)), dim3(64), 0, st>>>(dK, d_jobs, m_pu.as<double>(), m_pre.as<double>(), settled, ci,
                                                                                                (long long)n, (long long)stride, nullptr, owdev::JOB_OUT_PA_INPUT);
            else if (bark::chain_row(call.sw, cn))
                owdev::k_bark_chain_row<<<dim3((unsigned)((cn + 7) / 8)), dim3(320), 0, st>>>(dK, d_jobs, m_pu.as<double>(), m_pre.as<double>(), ci, (long long)n,
                                                                                             (long long)stride);
            else
                owdev::k_job_chain<false><<<dim3((unsigned)((cn + 31) / 32)), dim3(64), 0, st>>>(dK, d_jobs, m_pu.as<double>(), m_pre.as<double>(), nullptr, ci,
                                                                                                 (long long)n, (long long)stride, nullptr, owdev::JOB_OUT_PA_INPUT);
            HIP_OK(hipGetLastError());
            // dft_magnitude's sums over [m0, n) at (f0, 2 f0): the pickup rows into sums[0 .. 4 cn), the preamp rows behind them
            note_audit::launch_dft(m_pu.as<double>(), cn, stride, m0, n, note_audit::SR, m_freqs.as<double>(), 2, m_sums.as<double>(), st);
            note_audit::launch_dft(m_pre.as<double>(), cn, stride, m0, n, note_audit::SR, m_freqs.as<double>(), 2, m_sums.as<double>() + 4 * cn, st);
            HIP_OK(hipMemcpyAsync(hstats.data(), m_stats.p, sizeof(double) * owdev::BARK_ST_COUNT * cn, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(hsums.data(), m_sums.p, sizeof(double) * 8 * cn, hipMemcpyDeviceToHost, st));
            if (taps_out) {                                            // taps_out[job][0 reed | 1 pickup | 2 preamp][0..n)
                const void* src[3] = {m_reed.p, m_pu.p, m_pre.p};
                for (int k = 0; k < 3; ++k) rows_to_host(taps_out + (c0 * 3 + (size_t)k) * tap_stride, 3 * tap_stride, src[k], stride, n, cn, st);
            }
            HIP_OK(hipStreamSynchronize(st));                          // the buffers are reused by the next chunk
            for (size_t i = 0; i < cn; ++i) {
                ow_bark_row& r = rows_out[c0 + i];
                const double* s = &hstats[owdev::BARK_ST_COUNT * i];
                r.displacement_scale = s[owdev::BARK_ST_DS];
                r.reed_peak = s[owdev::BARK_ST_REED_PEAK];
                r.y_peak = r.reed_peak * r.displacement_scale;         // main.rs:615
                r.pu_peak = s[owdev::BARK_ST_PU_PEAK];
                bark::ratio(&hsums[4 * i], n_window, r.pu_h1, r.pu_h2, r.pu_h2_h1);
                bark::ratio(&hsums[4 * cn + 4 * i], n_window, r.pre_h1, r.pre_h2, r.pre_h2_h1);
            }
        }
        return (long long)n;
    } catch (const std::exception& ex) { set_err(std::string("ow_bark_audit: ") + ex.what()); return -1; }
}
}  // extern "C"
