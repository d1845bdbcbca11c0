// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the pump measurements (`preamp-bench pump-sweep` /
// `pump-trace` / `pump-spike` / `pump-step` / `pump-sinusoid`, tools/preamp-bench/src/main.rs:2329-3063).
namespace {
namespace pump {
// the chain rate build_consts makes of a host rate is the host rate doubled below 88.2 kHz (engine.rs:195): the host rate whose chain rate is `rate`
inline double host_rate_for(double rate) { return rate * 0.5 < 88200.0 ? rate * 0.5 : rate; }

// k_pump_points runs a state that was never rebuilt on OwConsts::m_s0 / m_k0 and forms S N_i from S where it is used (mel_process_lit).  That
// is the tables' own S_NI and K, bit for bit, as long as they are these sums of the table S -- true of the codegen tables and of
// build_melange_consts' rebuild (its dense sums add exact zeros); checked so that a regenerated table cannot silently change that.
void check_tables(const OwConsts& c) {
    for (int n = 0; n < 12; ++n) {
        const double s0 = c.m_s0[n][2] * PRE_N_I[0][2];
        const double s1 = c.m_s0[n][2] * PRE_N_I[1][2] + c.m_s0[n][4] * PRE_N_I[1][4] + c.m_s0[n][5] * PRE_N_I[1][5];
        const double s2 = c.m_s0[n][4] * PRE_N_I[2][4] + c.m_s0[n][7] * PRE_N_I[2][7] + c.m_s0[n][8] * PRE_N_I[2][8];
        if (s0 != c.m_sni0[n][0] || s1 != c.m_sni0[n][1] || s2 != c.m_sni0[n][2])
            throw std::runtime_error("the rate's S_NI table is not S N_i of its S table: k_pump_points cannot reproduce it");
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double sum = 0.0;
            for (int n = 0; n < 12; ++n) sum += PRE_N_V[i][n] * c.m_sni0[n][j];
            if (sum != c.m_k0[i][j]) throw std::runtime_error("the rate's K table is not N_v S_NI: k_pump_points cannot reproduce it");
        }
}

// ow_pump_row from the kernel's sums, in the reference's order of operations (pump-sweep :2412-2414, pump-spike's measure :2615-2618)
void finish_row(const double* m, uint64_t capture, ow_pump_row& r) {
    std::memset(&r, 0, sizeof r);
    const double nf = (double)capture;
    r.sum = m[owdev::PM_SUM]; r.sum_sq = m[owdev::PM_SUM_SQ]; r.min = m[owdev::PM_MIN]; r.max = m[owdev::PM_MAX];
    r.mean = r.sum / nf;
    r.std = std::sqrt(std::fmax(r.sum_sq / nf - r.mean * r.mean, 0.0));
    const uint64_t pairs = capture / 2;
    r.pair_mean = m[owdev::PM_PSUM] / (double)pairs;
    r.pair_std = std::sqrt(std::fmax(m[owdev::PM_PSUM_SQ] / (double)pairs - r.pair_mean * r.pair_mean, 0.0));
    const double raw_mean = m[owdev::PM_RAW_SUM] / (double)(2 * pairs);
    r.raw_std = std::sqrt(std::fmax(m[owdev::PM_RAW_SUM_SQ] / (double)(2 * pairs) - raw_mean * raw_mean, 0.0));
    r.extra = m[owdev::PM_EXTRA]; r.max_step = m[owdev::PM_MAX_STEP];
    r.nr_exhausted = (uint64_t)m[owdev::PM_NR]; r.be_fallbacks = (uint64_t)m[owdev::PM_BE];
    r.voltage_damps = (uint64_t)m[owdev::PM_DAMP]; r.nan_resets = (uint64_t)m[owdev::PM_NAN];
}
}  // namespace pump
}  // namespace

extern "C" {
int ow_pump_measure(const ow_pump_point* points, size_t n_pts, const ow_pump_cfg* cfg, ow_pump_row* rows_out, double* trace_out, size_t trace_stride) {
    try {
        if (!cfg) throw std::runtime_error("null argument");
        if (cfg->struct_size != sizeof(ow_pump_cfg) || cfg->point_size != sizeof(ow_pump_point))
            throw std::runtime_error(abi_mismatch("ow_pump_cfg.struct_size / point_size do"));
        if (n_pts == 0) return 0;
        if (!points || !rows_out) throw std::runtime_error("null argument");
        if (n_pts > (size_t)INT32_MAX) throw std::runtime_error("too many points");
        uint64_t cap_max = 0;
        bool any_table = false;
        for (size_t i = 0; i < n_pts; ++i) {
            const ow_pump_point& q = points[i];
            const std::string at = "point " + std::to_string(i) + ": ";
            check_positive_finite(at, "sample_rate", q.sample_rate); check_positive_finite(at, "r_settle", q.r_settle);
            check_finite(at, "in_amp", q.in_amp); check_finite(at, "in_freq", q.in_freq);
            if (q.extra_sample > 1u) throw std::runtime_error(at + "extra_sample is neither 0 nor 1");
            if (q.capture == 0) throw std::runtime_error(at + "capture is 0");
            if (q.schedule == OW_PUMP_STEP || q.schedule == OW_PUMP_RAMP) check_positive_finite(at, "r_to", q.r_to);
            else if (q.schedule == OW_PUMP_LOGCOS) { check_finite(at, "ln_mid", q.ln_mid); check_finite(at, "ln_amp", q.ln_amp); check_finite(at, "sched_freq", q.sched_freq); }
            else if (q.schedule != OW_PUMP_STATIC) throw std::runtime_error(at + "unknown schedule");
            if (q.schedule == OW_PUMP_RAMP && q.capture < 2) throw std::runtime_error(at + "capture below 2 with OW_PUMP_RAMP (the ramp divides by capture - 1)");
            if (q.settle >= (1ull << 40) || q.capture >= (1ull << 40) || q.settle + q.capture + 1 >= (1ull << 40))
                throw std::runtime_error(at + "a run of 2^40 samples or more");
            cap_max = std::max<uint64_t>(cap_max, q.capture);
            any_table = any_table || q.schedule == OW_PUMP_RAMP || q.schedule == OW_PUMP_LOGCOS;
        }
        if (trace_out && trace_stride < cap_max) throw std::runtime_error("trace_stride smaller than the largest capture (" + std::to_string(cap_max) + ")");

        // one group per distinct sample rate, each sorted by resistance (the lanes that exhaust Newton on every sample share wavefronts)
        std::vector<size_t> order(n_pts);
        for (size_t i = 0; i < n_pts; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            if (points[a].sample_rate != points[b].sample_rate) return points[a].sample_rate < points[b].sample_rate;
            return points[a].r_settle < points[b].r_settle;
        });
        const Switches sw0 = Switches::from_env();
        const long long tstride = row_stride((long long)cap_max);
        // device bytes per point: the sample-major trace and its rows, a tabulated schedule
        const size_t per_point = sizeof(double) * ((trace_out ? 2 * (size_t)tstride : 0) + (any_table ? (size_t)cap_max : 0)) + 512;
        // (with a trace at most 2^20 points per launch: k_pump_trace_rows' grid has the points in y)
        const size_t chunk = std::min<size_t>(budget_chunk(size_t(4) << 30, per_point, sw0.pump_chunk, n_pts), trace_out ? size_t(1) << 20 : SIZE_MAX);

        std::vector<owdev::OwPumpDev> hp;
        std::vector<double> sched, hm;
        for (size_t g0 = 0; g0 < n_pts;) {
            const double rate = points[order[g0]].sample_rate;
            size_t g1 = g0;
            while (g1 < n_pts && points[order[g1]].sample_rate == rate) ++g1;
            OfflineCall call(cfg->device, pump::host_rate_for(rate), OW_PREAMP_MELANGE12, /*note_table=*/false);
            {   // the constants the call uploaded, rebuilt here for the check (OfflineCall keeps its copy to itself)
                std::unique_ptr<OwConsts> hc(new OwConsts());
                owhip::build_consts(*hc, pump::host_rate_for(rate), OW_PREAMP_MELANGE12);
                if (hc->os_sr != rate) throw std::runtime_error("sample_rate " + std::to_string(rate) + " is not reachable as a chain rate");
                pump::check_tables(*hc);
            }
            hipStream_t st = call.st();
            for (size_t c0 = g0; c0 < g1; c0 += chunk) {
                const size_t cn = std::min(chunk, g1 - c0);
                hp.assign(cn, owdev::OwPumpDev());
                sched.clear();
                uint64_t cmax = 0;
                for (size_t i = 0; i < cn; ++i) {
                    const ow_pump_point& q = points[order[c0 + i]];
                    owdev::OwPumpDev& d = hp[i];
                    d.r_settle = q.r_settle; d.r_to = q.r_to; d.amp = q.in_amp;
                    d.w = 2.0 * 3.14159265358979323846 * q.in_freq / q.sample_rate;                    // two_pi_dt, main.rs:2722
                    d.settle = (long long)q.settle; d.capture = (long long)q.capture; d.extra = (int)q.extra_sample;
                    d.sched_off = (long long)sched.size();
                    d.kind = q.schedule == OW_PUMP_STATIC ? owdev::PUMP_STATIC : q.schedule == OW_PUMP_STEP ? owdev::PUMP_STEP : owdev::PUMP_TABLE;
                    if (q.schedule == OW_PUMP_RAMP) {
                        for (uint64_t k = 0; k < q.capture; ++k) {                                     // main.rs:2779-2781
                            const double t = (double)k / (double)(q.capture - 1);
                            sched.push_back(q.r_settle + (q.r_to - q.r_settle) * t);
                        }
                    } else if (q.schedule == OW_PUMP_LOGCOS) {
                        const double dt = 1.0 / q.sample_rate, omega = 2.0 * 3.14159265358979323846 * q.sched_freq;   // main.rs:2966-2967
                        for (uint64_t k = 0; k < q.capture; ++k) {                                     // :2996-2997
                            const double t = (double)k * dt;
                            sched.push_back(std::exp(q.ln_mid + q.ln_amp * std::cos(omega * t)));
                        }
                    }
                    cmax = std::max<uint64_t>(cmax, q.capture);
                }
                const unsigned blocks = (unsigned)((cn + 31) / 32);
                DevMem m_pts, m_sched, m_met, m_lu, m_tr, m_rows;              // released on every exit path
                m_pts.alloc(sizeof(owdev::OwPumpDev) * cn);
                m_sched.alloc(sizeof(double) * sched.size());
                m_met.alloc(sizeof(double) * owdev::PM_COUNT * cn);
                m_lu.alloc(sizeof(double) * 12 * 12 * 32 * blocks);
                const long long ld = row_stride((long long)cn);
                if (trace_out) {
                    m_tr.alloc(sizeof(double) * (size_t)ld * cmax);
                    m_rows.alloc(sizeof(double) * (size_t)tstride * cn);
                    HIP_OK(hipMemsetAsync(m_tr.p, 0, sizeof(double) * (size_t)ld * cmax, st));
                    HIP_OK(hipMemsetAsync(m_rows.p, 0, sizeof(double) * (size_t)tstride * cn, st));
                }
                HIP_OK(hipMemcpyAsync(m_pts.p, hp.data(), sizeof(owdev::OwPumpDev) * cn, hipMemcpyHostToDevice, st));
                if (!sched.empty()) HIP_OK(hipMemcpyAsync(m_sched.p, sched.data(), sizeof(double) * sched.size(), hipMemcpyHostToDevice, st));
                owdev::k_pump_points<<<dim3(blocks), dim3(64), 0, st>>>(call.dK(), m_pts.as<owdev::OwPumpDev>(), (int)cn, m_sched.as<double>(), m_met.as<double>(),
                                                                        trace_out ? m_tr.as<double>() : nullptr, ld, call.sw.mel_generic ? 1 : 0, m_lu.as<double>());
                HIP_OK(hipGetLastError());
                hm.resize(cn * owdev::PM_COUNT);
                HIP_OK(hipMemcpyAsync(hm.data(), m_met.p, sizeof(double) * hm.size(), hipMemcpyDeviceToHost, st));
                std::vector<double> hrows;
                if (trace_out) {
                    owdev::k_pump_trace_rows<<<dim3((unsigned)((cmax + 31) / 32), blocks), dim3(32, 8), 0, st>>>(m_tr.as<double>(), ld, (int)cn, (long long)cmax,
                                                                                                               m_rows.as<double>(), tstride);
                    HIP_OK(hipGetLastError());
                    hrows.resize((size_t)tstride * cn);
                    HIP_OK(hipMemcpyAsync(hrows.data(), m_rows.p, sizeof(double) * hrows.size(), hipMemcpyDeviceToHost, st));
                }
                HIP_OK(hipStreamSynchronize(st));
                for (size_t i = 0; i < cn; ++i) {                              // back into the caller's order
                    const size_t o = order[c0 + i];
                    pump::finish_row(&hm[i * owdev::PM_COUNT], points[o].capture, rows_out[o]);
                    if (trace_out) {
                        double* row = trace_out + o * trace_stride;
                        std::memcpy(row, &hrows[i * (size_t)tstride], sizeof(double) * (size_t)cap_max);
                    }
                }
            }
            g0 = g1;
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_pump_measure: ") + ex.what()); return -1; }
}
}  // extern "C"
