// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the calibration sweep (`preamp-bench calibrate` /
// `sensitivity`, tools/preamp-bench/src/main.rs:1069-1395).
namespace {
// CalibrationConfig's two table functions, restated in the reference's operation order (a few scalars per point: host work).
namespace calib {
inline double fclamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }        // f64::clamp (NaN passes)
inline double midi_to_freq(int midi) { return 440.0 * std::pow(2.0, ((double)midi - 69.0) / 12.0); }   // tables.rs:37-39
inline double reed_length_mm(int midi) {                                                                // tables.rs:161-169
    const double n = fclamp((double)midi - 32.0, 1.0, 64.0);
    const double inches = (n <= 20.0) ? 3.0 - n / 20.0 : 2.0 - (n - 20.0) / 44.0;
    return inches * 25.4;
}
inline double reed_compliance(int midi) {                                                               // tables.rs:183-225
    int reed = midi - 32;
    reed = std::max(1, std::min(64, reed));
    const double width_inch = reed <= 14 ? 0.151 : reed <= 20 ? 0.127 : reed <= 42 ? 0.121 : reed <= 50 ? 0.111 : 0.098;
    double thick_inch;
    if (reed <= 16) thick_inch = 0.026;
    else if (reed <= 26) thick_inch = 0.026 + (((double)reed - 16.0) / 10.0) * (0.034 - 0.026);
    else thick_inch = 0.034;
    const double l = reed_length_mm(midi), w = width_inch * 25.4, t = thick_inch * 25.4;
    return (l * l * l) / (w * t * t * t);
}
inline double pickup_displacement_scale(int midi, const ow_calib_point& c) {                            // tables.rs:283-288
    const double cm = reed_compliance(midi);
    const double c_ref = reed_compliance(60);
    const double ds = c.ds_at_c4 * std::pow(cm / c_ref, c.ds_exponent);
    return fclamp(ds, c.ds_clamp_lo, c.ds_clamp_hi);
}
inline double pickup_rms_proxy(double ds, double f0, double fc) {                                       // tables.rs:424-441
    if (ds < 1e-10) return 0.0;
    const double r = (1.0 - std::sqrt(1.0 - ds * ds)) / ds;
    const double inv_sqrt = 1.0 / std::sqrt(1.0 - ds * ds);
    double sum_sq = 0.0, r_n = r;
    for (int n = 1; n <= 8; ++n) {
        const double cn = 2.0 * r_n * inv_sqrt;
        const double nf = (double)n * f0;
        const double hpf_n = nf / std::sqrt(nf * nf + fc * fc);
        sum_sq += (cn * hpf_n) * (cn * hpf_n);
        r_n *= r;
    }
    return std::sqrt(sum_sq);
}
inline double register_trim_db(int midi) {                                                              // tables.rs:443-481
    static const double ax[13] = {36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84};
    static const double ay[13] = {-1.3, 0.0, -1.3, 0.7, 0.2, -1.0, 0.0, 0.9, 1.2, 0.0, 1.8, 2.4, 3.6};
    const double m = (double)midi;
    if (m <= ax[0]) return ay[0];
    if (m >= ax[12]) return ay[12];
    for (int i = 0; i < 12; ++i)
        if (m <= ax[i + 1]) return ay[i] + ((m - ax[i]) / (ax[i + 1] - ax[i])) * (ay[i + 1] - ay[i]);
    return 0.0;
}
inline double velocity_exponent(int midi) {                                                             // tables.rs:535-554
    const double m = (double)midi;
    const double z = (m - 62.0) / 15.0;
    const double t = std::exp(-0.5 * (z * z));
    const double mn = (m < 62.0) ? 0.55 : 1.3;
    return mn + t * (1.7 - mn);
}
inline double velocity_scurve(double v) {                                                               // tables.rs:556-562
    const double k = 1.5;
    const double s = 1.0 / (1.0 + std::exp(-k * (v - 0.5)));
    const double s0 = 1.0 / (1.0 + std::exp(k * 0.5));
    const double s1 = 1.0 / (1.0 + std::exp(-k * 0.5));
    return (s - s0) / (s1 - s0);
}
inline double output_scale(int midi, double velocity_norm, const ow_calib_point& c) {                   // tables.rs:578-620
    const double HPF_FC = 2312.0;
    const double ds = pickup_displacement_scale(midi, c);
    const double f0 = midi_to_freq(midi);
    const double scurve_v = velocity_scurve(velocity_norm);
    const double vel_scale = std::pow(scurve_v, velocity_exponent(midi));
    const double vel_scale_c4 = std::pow(scurve_v, velocity_exponent(60));
    const double effective_ds = std::fmax(ds * vel_scale, 1e-6);
    const double effective_ds_ref = std::fmax(c.ds_at_c4 * vel_scale_c4, 1e-6);
    const double rms = pickup_rms_proxy(effective_ds, f0, HPF_FC);
    const double rms_ref = pickup_rms_proxy(effective_ds_ref, midi_to_freq(60), HPF_FC);
    const double flat_db = -20.0 * std::log10(rms / rms_ref);
    const double voicing_db = c.voicing_slope * std::fmax((double)midi - 60.0, 0.0);
    const double trim = c.zero_trim ? 0.0 : register_trim_db(midi);
    const double vel_blend = std::pow(velocity_norm, 1.3);
    const double effective_trim = trim * vel_blend;
    return std::pow(10.0, (c.target_db + flat_db + voicing_db + effective_trim) / 20.0);
}
inline double h2_h1_ratio_db(const double* m, double n) {                                                // main.rs:929-937 (the sums come from k_calib_metrics)
    const double h1 = measure::dft_magnitude(m[owdev::CALIB_MET_RE1], m[owdev::CALIB_MET_IM1], n);
    const double h2 = measure::dft_magnitude(m[owdev::CALIB_MET_RE2], m[owdev::CALIB_MET_IM2], n);
    return h1 > 1e-15 ? 20.0 * std::log10(h2 / h1) : -120.0;
}
}  // namespace calib
}  // namespace

extern "C" {
int ow_calibrate(const ow_calib_point* points, size_t n_pts, const ow_calibrate_cfg* cfg, ow_calibrate_row* rows_out, double* taps_out,
                 size_t taps_stride) {
    try {
        if (!cfg) throw std::runtime_error("null argument");
        if (cfg->struct_size != sizeof(ow_calibrate_cfg) || cfg->point_size != sizeof(ow_calib_point))
            throw std::runtime_error(abi_mismatch("ow_calibrate_cfg.struct_size / point_size do"));
        if (n_pts == 0) return 0;
        if (!points || !rows_out) throw std::runtime_error("null argument");
        require_known_kinds(cfg->preamp_kind, cfg->power_amp_kind);
        const long long n = OW_CALIB_SAMPLES;                          // (0.5 * BASE_SR) as usize, main.rs:1136,1172
        if (taps_out && taps_stride < (size_t)n) throw std::runtime_error("taps_stride smaller than " + std::to_string(n));
        if (n_pts > (size_t)INT32_MAX) throw std::runtime_error("too many points");
        const double sr = 44100.0;                                     // BASE_SR, main.rs:27
        std::vector<owdev::OwCalibDev> hp(n_pts);
        for (size_t i = 0; i < n_pts; ++i) {
            const ow_calib_point& c = points[i];
            const std::string at = "point " + std::to_string(i) + ": ";
            check_note_velocity(at, c.note, c.velocity);
            if (!(c.ds_clamp_lo <= c.ds_clamp_hi)) throw std::runtime_error(at + "ds_clamp lo > hi or NaN (f64::clamp panics)");
            hp[i].note = c.note; hp[i].velocity = c.velocity;
            hp[i].ds_actual = calib::pickup_displacement_scale(c.note, c);
            hp[i].out_scale = calib::output_scale(c.note, (double)c.velocity / 127.0, c);
            hp[i].f0 = calib::midi_to_freq(c.note);
        }
        OfflineCall call(cfg->device, sr, cfg->preamp_kind, /*note_table=*/true);
        hipStream_t st = call.st();
        const OwConsts* dK = call.dK();
        const bool mel = cfg->preamp_kind == OW_PREAMP_MELANGE12, mpa = cfg->power_amp_kind == OW_POWER_AMP_MELANGE;
        const long long stride = row_stride(n);
        const size_t row_bytes = sizeof(double) * (size_t)stride;
        const int n_rows = taps_out ? 5 : 4;
        // points per chunk: ~8 GiB of device rows at four (five with taps) rows of 0.5 s per point
        const size_t chunk = budget_chunk(size_t(8) << 30, row_bytes * (size_t)n_rows, call.sw.calib_chunk, n_pts);
        DevMem m_vrec, m_pts, m_jobs, m_rows, m_pk, m_met;            // released on every exit path
        m_vrec.alloc(sizeof(double) * ((chunk + 63) / 64) * OW_VREC_DOUBLES);
        m_pts.alloc(sizeof(owdev::OwCalibDev) * n_pts);
        m_jobs.alloc(sizeof(owdev::OwJobDev) * chunk);
        m_rows.alloc(row_bytes * chunk * (size_t)n_rows);
        m_pk.alloc(sizeof(double) * n_pts);
        m_met.alloc(sizeof(double) * n_pts * 4 * owdev::CALIB_MET_COUNT);
        owdev::OwCalibDev* d_pts = m_pts.as<owdev::OwCalibDev>();
        double* rows = m_rows.as<double>();
        double* T[5];                                                  // T1..T5 row blocks of a chunk ([chunk][stride] each)
        T[1] = rows; T[2] = rows + (size_t)chunk * stride; T[3] = rows + 2 * (size_t)chunk * stride; T[4] = rows + 3 * (size_t)chunk * stride;
        T[0] = taps_out ? rows + 4 * (size_t)chunk * stride : nullptr;
        HIP_OK(hipMemcpyAsync(d_pts, hp.data(), sizeof(owdev::OwCalibDev) * n_pts, hipMemcpyHostToDevice, st));
        // T4's jobs: `preamp-bench render`'s chain with a static 1 Mohm LDR and volume 1.0, stopped at the power amp's input
        // (JOB_OUT_PA_INPUT: pre x 1.0 x 1.0 = pre, bit for bit).  run_calibrate builds its preamp with new() + set_ldr_resistance(1e6) and no
        // reset() (main.rs:1190-1191), the batch job with new() + reset() + set_ldr_resistance: the same start state for both kinds --
        // legacy: new() solves DC at r_ldr = 1e6 with g_ldr = g_ldr_prev = 1e-6 (dk_preamp_legacy.rs:269-366), reset() solves it again at
        // the same r_ldr with w = two_w x 0.5 = w exactly (:628-640), and set_ldr_resistance(1e6) moves nothing (|1e6 - 1e6| <= 0.01,
        // :620-626); melange: new() and reset() both clone the settled state (melange_adapter.rs:22-29, 40-48, 88-93), noise off.
        std::vector<owdev::OwJobDev> hj(chunk);
        for (auto& j : hj) {
            std::memset(&j, 0, sizeof(j));
            j.poweramp = 1; j.volume = 1.0; j.speaker = cfg->speaker; j.r_ldr = 1000000.0;
        }
        HIP_OK(hipMemcpyAsync(m_jobs.p, hj.data(), sizeof(owdev::OwJobDev) * chunk, hipMemcpyHostToDevice, st));
        const double* settled = mel ? call.mel_settled() : nullptr;
        std::unique_ptr<MelPowerAmpStage> pa;
        if (mpa) pa.reset(new MelPowerAmpStage(cfg->device, st));
        const double nwin = (double)(OW_CALIB_WIN_HI - OW_CALIB_WIN_LO);
        auto copy_taps = [&](int k, size_t p0, size_t cn) {           // T(k+1) rows of the chunk -> taps_out[p][k][0..n)
            rows_to_host(taps_out + (p0 * 5 + (size_t)k) * taps_stride, 5 * taps_stride, T[k], (size_t)stride, (size_t)n, cn, st);
        };
        for (size_t p0 = 0; p0 < n_pts; p0 += chunk) {
            const size_t cn = std::min(chunk, n_pts - p0);
            const int ci = (int)cn;
            const owdev::OwCalibDev* cp = d_pts + p0;
            double* met = m_met.as<double>() + p0 * 4 * owdev::CALIB_MET_COUNT;
            owdev::k_calib_voice<<<dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, st>>>(dK, call.nt(), m_vrec.as<double>(), cp, T[0], T[1], T[2],
                                                                                         m_pk.as<double>() + p0, ci, n, stride);
            HIP_OK(hipGetLastError());
            if (taps_out) { copy_taps(0, p0, cn); copy_taps(1, p0, cn); copy_taps(2, p0, cn); }
            // T2 / T3 metrics now: the melange power amp below reuses their rows
            owdev::CalibMetRows a23{{T[1], T[2], nullptr, nullptr}};
            owdev::k_calib_metrics<<<dim3((unsigned)cn, 2), dim3(256), 0, st>>>(a23, cp, stride, sr, 1u, 0, met);
            HIP_OK(hipGetLastError());
            if (mel)
                owdev::k_job_chain<true><<<dim3((unsigned)((cn + 31) / 32)), dim3(64), 0, st>>>(dK, m_jobs.as<owdev::OwJobDev>(), T[2], T[3], settled,
                                                                                                ci, n, stride, nullptr, owdev::JOB_OUT_PA_INPUT);
            else
                owdev::k_job_chain<false><<<dim3((unsigned)((cn + 31) / 32)), dim3(64), 0, st>>>(dK, m_jobs.as<owdev::OwJobDev>(), T[2], T[3], nullptr,
                                                                                                 ci, n, stride, nullptr, owdev::JOB_OUT_PA_INPUT);
            HIP_OK(hipGetLastError());
            const unsigned ob = (unsigned)((cn + 63) / 64);
            if (mpa) {        // as run_job_chain: t4 x volume^2 -> the melange power amp, rail sag on -> speaker
                owdev::k_calib_out<<<dim3(ob), dim3(64), 0, st>>>(dK, T[3], T[1], cfg->volume, cfg->speaker, ci, n, stride, owdev::CALIB_OUT_ATT);
                pa->run(T[1], T[2], n, ci, 1, stride);
                owdev::k_calib_out<<<dim3(ob), dim3(64), 0, st>>>(dK, T[2], T[4], cfg->volume, cfg->speaker, ci, n, stride, owdev::CALIB_OUT_SPEAKER);
            } else {
                owdev::k_calib_out<<<dim3(ob), dim3(64), 0, st>>>(dK, T[3], T[4], cfg->volume, cfg->speaker, ci, n, stride, owdev::CALIB_OUT_FULL);
            }
            HIP_OK(hipGetLastError());
            owdev::CalibMetRows a45{{T[3], T[4], nullptr, nullptr}};
            owdev::k_calib_metrics<<<dim3((unsigned)cn, 2), dim3(256), 0, st>>>(a45, cp, stride, sr, 3u, 2, met);
            HIP_OK(hipGetLastError());
            if (taps_out) { copy_taps(3, p0, cn); copy_taps(4, p0, cn); }
        }
        std::vector<double> pk(n_pts), hm(n_pts * 4 * owdev::CALIB_MET_COUNT);
        HIP_OK(hipMemcpyAsync(pk.data(), m_pk.p, sizeof(double) * n_pts, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hm.data(), m_met.p, sizeof(double) * hm.size(), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (size_t i = 0; i < n_pts; ++i) {
            const ow_calib_point& c = points[i];
            const double* m2 = &hm[(i * 4 + 0) * owdev::CALIB_MET_COUNT];
            const double* m3 = &hm[(i * 4 + 1) * owdev::CALIB_MET_COUNT];
            const double* m4 = &hm[(i * 4 + 2) * owdev::CALIB_MET_COUNT];
            const double* m5 = &hm[(i * 4 + 3) * owdev::CALIB_MET_COUNT];
            ow_calibrate_row& r = rows_out[i];
            std::memset(&r, 0, sizeof(r));
            r.midi = c.note; r.velocity = c.velocity;
            r.ds_at_c4 = c.ds_at_c4; r.ds_actual = hp[i].ds_actual; r.y_peak = pk[i] * hp[i].ds_actual;       // main.rs:1175-1176
            r.t2_peak_db = measure::to_dbfs(m2[owdev::CALIB_MET_PEAK]); r.t2_rms_db = measure::rms_db(m2[owdev::CALIB_MET_SUMSQ] / nwin);
            r.t2_h2_h1_db = calib::h2_h1_ratio_db(m2, nwin);
            r.t3_peak_db = measure::to_dbfs(m3[owdev::CALIB_MET_PEAK]); r.t3_rms_db = measure::rms_db(m3[owdev::CALIB_MET_SUMSQ] / nwin);
            r.t4_peak_db = measure::to_dbfs(m4[owdev::CALIB_MET_PEAK]); r.t4_rms_db = measure::rms_db(m4[owdev::CALIB_MET_SUMSQ] / nwin);
            r.t4_h2_h1_db = calib::h2_h1_ratio_db(m4, nwin);
            r.t5_peak_db = measure::to_dbfs(m5[owdev::CALIB_MET_PEAK]); r.t5_rms_db = measure::rms_db(m5[owdev::CALIB_MET_SUMSQ] / nwin);
            r.t5_h2_h1_db = calib::h2_h1_ratio_db(m5, nwin);
            r.proxy_db = 20.0 * std::log10(hp[i].out_scale);                                                   // main.rs:1225-1232
            r.trim_db = c.zero_trim ? 0.0 : calib::register_trim_db(c.note);
            r.proxy_error_db = r.t3_rms_db - c.target_db;
            r.tanh_compression_db = r.t4_peak_db - r.t5_peak_db;
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_calibrate: ") + ex.what()); return -1; }
}
}  // extern "C"
