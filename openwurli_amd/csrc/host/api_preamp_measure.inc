// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the preamp measurements (`preamp-bench gain` /
// `sweep` / `harmonics` / `tremolo-sweep`, tools/preamp-bench/src/main.rs:150-369).
namespace {
namespace pbench {
// OW_PBENCH_ROW=0/1 forces the kernel; otherwise a row of sixteen lanes per solver state (k_pbench_row: five wavefronts per eight points)
// while the grid leaves the chip's SIMDs free, the lane pair (k_pbench<false>: one wavefront per 32 points) beyond -- as job_chain_row()
inline bool use_row(size_t n_pts, int forced) { return forced >= 0 ? forced != 0 : n_pts <= 1024; }
}  // namespace pbench
}  // namespace

extern "C" {
int ow_preamp_measure(const ow_preamp_point* points, size_t n_pts, const ow_preamp_measure_cfg* cfg, ow_preamp_measure_row* rows_out,
                      double* trace_out, size_t trace_stride) {
    try {
        if (!cfg) throw std::runtime_error("null argument");
        if (cfg->struct_size != sizeof(ow_preamp_measure_cfg) || cfg->point_size != sizeof(ow_preamp_point))
            throw std::runtime_error(abi_mismatch("ow_preamp_measure_cfg.struct_size / point_size do"));
        if (n_pts == 0) return 0;
        if (!points || !rows_out) throw std::runtime_error("null argument");
        require_known_kinds(cfg->preamp_kind);
        const long long n = OW_PBENCH_SAMPLES;
        if (trace_out && trace_stride < (size_t)n) throw std::runtime_error("trace_stride smaller than " + std::to_string(n));
        if (n_pts > (size_t)INT32_MAX) throw std::runtime_error("too many points");
        std::vector<owdev::OwPbenchDev> hp(n_pts);
        for (size_t i = 0; i < n_pts; ++i) {
            const ow_preamp_point& q = points[i];
            const std::string at = "point " + std::to_string(i) + ": ";
            check_positive_finite(at, "freq_hz", q.freq_hz); check_positive_finite(at, "amplitude", q.amplitude);
            check_positive_finite(at, "r_ldr", q.r_ldr); check_positive_finite(at, "r_reset", q.r_reset);
            hp[i].freq = q.freq_hz; hp[i].amp = q.amplitude; hp[i].r_ldr = q.r_ldr; hp[i].r_reset = q.r_reset;
        }
        OfflineCall call(cfg->device, 44100.0, cfg->preamp_kind, /*note_table=*/false);   // BASE_SR: the preamp at OVERSAMPLED_SR = 88 200 Hz (main.rs:27-28)
        hipStream_t st = call.st();
        const OwConsts* dK = call.dK();
        const Switches& sw = call.sw;
        const bool mel = cfg->preamp_kind == OW_PREAMP_MELANGE12;
        const long long stride = row_stride(n);
        const size_t row_bytes = sizeof(double) * (size_t)stride;
        // points per launch: with a trace, a device trace buffer of ~4 GiB ([chunk][stride] f64); without one nothing is kept per point
        // but its metrics -- all points in one launch
        const size_t chunk = trace_out ? budget_chunk(size_t(4) << 30, row_bytes, sw.pbench_chunk, n_pts) : budget_chunk(SIZE_MAX, 1, sw.pbench_chunk, n_pts);
        DevMem m_pts, m_met, m_trace;                                  // released on every exit path
        m_pts.alloc(sizeof(owdev::OwPbenchDev) * n_pts);
        m_met.alloc(sizeof(double) * owdev::PB_MET_COUNT * n_pts);
        if (trace_out) m_trace.alloc(row_bytes * chunk);
        HIP_OK(hipMemcpyAsync(m_pts.p, hp.data(), sizeof(owdev::OwPbenchDev) * n_pts, hipMemcpyHostToDevice, st));
        const double* settled = mel ? call.mel_settled() : nullptr;
        for (size_t p0 = 0; p0 < n_pts; p0 += chunk) {
            const size_t cn = std::min(chunk, n_pts - p0);
            const int ci = (int)cn;
            const owdev::OwPbenchDev* cp = m_pts.as<owdev::OwPbenchDev>() + p0;
            double* met = m_met.as<double>() + p0 * owdev::PB_MET_COUNT;
            double* tr = trace_out ? m_trace.as<double>() : nullptr;
            if (mel)
                owdev::k_pbench<true><<<dim3((unsigned)((cn + 31) / 32)), dim3(64), 0, st>>>(dK, cp, met, tr, settled, ci, stride);
            else if (pbench::use_row(cn, sw.pbench_row))
                owdev::k_pbench_row<<<dim3((unsigned)((cn + 7) / 8)), dim3(320), 0, st>>>(dK, cp, met, tr, ci, stride);
            else
                owdev::k_pbench<false><<<dim3((unsigned)((cn + 31) / 32)), dim3(64), 0, st>>>(dK, cp, met, tr, nullptr, ci, stride);
            HIP_OK(hipGetLastError());
            if (trace_out) rows_to_host(trace_out + p0 * trace_stride, trace_stride, tr, (size_t)stride, (size_t)n, cn, st);
        }
        std::vector<double> hm(n_pts * owdev::PB_MET_COUNT);
        HIP_OK(hipMemcpyAsync(hm.data(), m_met.p, sizeof(double) * hm.size(), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const double nh = (double)(OW_PBENCH_SAMPLES - OW_PBENCH_HARM_LO);   // signal.len() of cmd_harmonics' last quarter
        for (size_t i = 0; i < n_pts; ++i) {
            const ow_preamp_point& q = points[i];
            const double* m = &hm[i * owdev::PB_MET_COUNT];
            ow_preamp_measure_row& r = rows_out[i];
            std::memset(&r, 0, sizeof(r));
            r.freq_hz = q.freq_hz; r.amplitude = q.amplitude; r.r_ldr = q.r_ldr;
            r.gain = m[owdev::PB_MET_PEAK] / q.amplitude;                                         // measure_gain_at, main.rs:189
            r.gain_db = 20.0 * std::log10(r.gain);                                                // cmd_gain / cmd_sweep, :199, :238
            for (int k = 0; k < 5; ++k) r.h[k] = measure::dft_magnitude(m[owdev::PB_MET_RE1 + 2 * k], m[owdev::PB_MET_RE1 + 2 * k + 1], nh);
            const double h1 = r.h[0], h2 = r.h[1], h3 = r.h[2], h4 = r.h[3], h5 = r.h[4];    // cmd_harmonics, :292-298
            r.thd_pct = (std::sqrt(h2 * h2 + h3 * h3 + h4 * h4 + h5 * h5) / h1) * 100.0;
            r.h2_h3_db = h3 > 1e-15 ? 20.0 * std::log10(h2 / h3) : INFINITY;
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_preamp_measure: ") + ex.what()); return -1; }
}
}  // extern "C"
