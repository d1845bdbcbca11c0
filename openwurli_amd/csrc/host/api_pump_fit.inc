// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the pump-dynamics fitter (tools/analyze_pump_dynamics.py):
// ow_pump_fit_eval (the loss of many (trace, model, parameter vector) triples per call) and ow_pump_fit (scipy's non-adaptive Nelder-Mead,
// many fits per call).  The host checks, sorts the work by (trace, model) and cuts it into wavefronts; ow_pump_fit_kernels.h does the rest.
namespace {
namespace pump_fit {
constexpr uint32_t N_MODELS = 6;

struct Problem {                 // the checked inputs that both entry points share
    const double *r, *target, *rates, *lut_r, *lut_v;
    const uint64_t* offsets;
    size_t n_traces, n_lut;
    uint32_t skip;
    uint64_t total;
};

// every refusal of the shared inputs, before any device work
Problem check_problem(const double* r, const double* target, const uint64_t* offsets, const double* rates, size_t n_traces, const double* lut_r,
                      const double* lut_v, size_t n_lut, uint32_t skip) {
    if (!r || !target || !offsets || !rates || !lut_r || !lut_v) throw std::runtime_error("null argument");
    if (n_traces == 0) throw std::runtime_error("no traces");
    if (n_traces > (size_t)INT32_MAX) throw std::runtime_error("too many traces");
    if (n_lut < 2) throw std::runtime_error("a table of fewer than 2 points");
    if (n_lut > OW_PF_MAX_LUT) throw std::runtime_error("a table of more than " + std::to_string(OW_PF_MAX_LUT) + " points");
    for (size_t i = 0; i < n_lut; ++i) {
        const std::string at = "table point " + std::to_string(i) + ": ";
        check_positive_finite(at, "lut_r", lut_r[i]);
        check_finite(at, "lut_v", lut_v[i]);
        if (i && !(lut_r[i] > lut_r[i - 1])) throw std::runtime_error(at + "lut_r is not strictly ascending");
    }
    if (offsets[0] != 0) throw std::runtime_error("offsets[0] is not 0");
    for (size_t t = 0; t < n_traces; ++t) {
        const std::string at = "trace " + std::to_string(t) + ": ";
        if (offsets[t + 1] < offsets[t]) throw std::runtime_error(at + "offsets are not ascending");
        const uint64_t n = offsets[t + 1] - offsets[t];
        if (n <= (uint64_t)skip + 1) throw std::runtime_error(at + std::to_string(n) + " samples: skip + 1 (" + std::to_string((uint64_t)skip + 1) + ") or fewer");
        if (n > (uint64_t)INT32_MAX) throw std::runtime_error(at + "longer than 2^31 - 1 samples");
        check_positive_finite(at, "sample_rate", rates[t]);
        for (uint64_t k = offsets[t]; k < offsets[t + 1]; ++k) {
            if (!(std::isfinite(r[k]) && r[k] > 0.0)) throw std::runtime_error(at + "r is not a finite positive number at sample " + std::to_string(k - offsets[t]));
            if (!std::isfinite(target[k])) throw std::runtime_error(at + "target is not finite at sample " + std::to_string(k - offsets[t]));
        }
    }
    return Problem{r, target, rates, lut_r, lut_v, offsets, n_traces, n_lut, skip, offsets[n_traces]};
}

// (trace, model, parameters) of n items, checked; n_params doubles of each row of four must be finite
void check_items(const char* what, const uint32_t* trace, const uint32_t* model, const double* params, size_t n, size_t n_traces) {
    static const int n_params[N_MODELS] = {1, 1, 2, 2, 3, 4};
    if (n > (size_t)INT32_MAX / 8) throw std::runtime_error(std::string("too many ") + what + "s");
    for (size_t i = 0; i < n; ++i) {
        const std::string at = std::string(what) + " " + std::to_string(i) + ": ";
        if (model[i] >= N_MODELS) throw std::runtime_error(at + "model " + std::to_string(model[i]) + " above 5");
        if (trace[i] >= n_traces) throw std::runtime_error(at + "trace " + std::to_string(trace[i]) + " out of range");
        for (int k = 0; k < n_params[model[i]]; ++k) check_finite(at, "parameter", params[4 * i + k]);
    }
}

// The work sorted by (trace, model), stable, and cut into wavefronts of at most `per_wave` items of one (trace, model).
// order[i]: the caller's index of sorted item i (what the kernels take as `dest`).
void pack(const uint32_t* trace, const uint32_t* model, size_t n, uint32_t per_wave, std::vector<uint32_t>& order, std::vector<owdev::OwPfWaveDev>& waves) {
    order.resize(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (trace[a] != trace[b]) return trace[a] < trace[b];
        return model[a] < model[b];
    });
    waves.clear();
    for (size_t i = 0; i < n;) {
        const uint32_t t = trace[order[i]], m = model[order[i]];
        size_t j = i;
        while (j < n && j - i < per_wave && trace[order[j]] == t && model[order[j]] == m) ++j;
        waves.push_back(owdev::OwPfWaveDev{t, m, (uint32_t)i, (uint32_t)(j - i)});
        i = j;
    }
}

// the inputs on the device: the traces, ln R and the table's value at R (k_pump_fit_prep), the table with its logarithms and slopes
struct Staged {
    StreamOwner so;
    DevMem r, target, lnr, base, traces, lut_r, lut_v, lut_ln, lut_slope, waves, params, dest;
    hipStream_t st = nullptr;
    void upload(const Problem& p, int device) {
        HIP_OK(hipSetDevice(device));
        so.create();
        st = so.s;
        std::vector<owdev::OwPfTraceDev> ht(p.n_traces);
        for (size_t t = 0; t < p.n_traces; ++t) ht[t] = owdev::OwPfTraceDev{p.offsets[t], (uint32_t)(p.offsets[t + 1] - p.offsets[t]), 0u, p.rates[t]};
        const size_t bytes = sizeof(double) * p.total, lb = sizeof(double) * p.n_lut;
        r.alloc(bytes); target.alloc(bytes); lnr.alloc(bytes); base.alloc(bytes);
        traces.alloc(sizeof(owdev::OwPfTraceDev) * p.n_traces);
        lut_r.alloc(lb); lut_v.alloc(lb); lut_ln.alloc(lb); lut_slope.alloc(lb);
        HIP_OK(hipMemcpyAsync(r.p, p.r, bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(target.p, p.target, bytes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(traces.p, ht.data(), sizeof(owdev::OwPfTraceDev) * p.n_traces, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(lut_r.p, p.lut_r, lb, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(lut_v.p, p.lut_v, lb, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));      // ht leaves scope
        owdev::k_pump_fit_lut<<<dim3(1), dim3(256), 0, st>>>(lut_r.as<double>(), lut_v.as<double>(), (int)p.n_lut, lut_ln.as<double>(), lut_slope.as<double>());
        HIP_OK(hipGetLastError());
        owdev::k_pump_fit_prep<<<dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, st>>>(r.as<double>(), p.total, lut_ln.as<double>(), lut_v.as<double>(),
                                                                                            lut_slope.as<double>(), lut_r.as<double>(), (int)p.n_lut,
                                                                                            lnr.as<double>(), base.as<double>());
        HIP_OK(hipGetLastError());
    }
    // the sorted work: its wavefront records, its parameter rows in sorted order and the caller's index of each
    void upload_work(const std::vector<owdev::OwPfWaveDev>& hw, const std::vector<uint32_t>& order, const double* rows) {
        std::vector<double> sorted(4 * order.size());
        for (size_t i = 0; i < order.size(); ++i) std::memcpy(&sorted[4 * i], rows + 4 * (size_t)order[i], 4 * sizeof(double));
        waves.alloc(sizeof(owdev::OwPfWaveDev) * hw.size());
        params.alloc(sizeof(double) * sorted.size());
        dest.alloc(sizeof(uint32_t) * order.size());
        HIP_OK(hipMemcpyAsync(waves.p, hw.data(), sizeof(owdev::OwPfWaveDev) * hw.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(params.p, sorted.data(), sizeof(double) * sorted.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(dest.p, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));      // sorted leaves scope
    }
};
}  // namespace pump_fit
}  // namespace

extern "C" {
int ow_pump_fit_eval(const double* r, const double* target, const uint64_t* offsets, const double* sample_rates, size_t n_traces, const double* lut_r,
                     const double* lut_v, size_t n_lut, const uint32_t* eval_trace, const uint32_t* eval_model, const double* eval_params, size_t n_evals,
                     uint32_t skip, int device, double* loss_out, double* pred_out, size_t pred_stride) {
    static_assert(OW_PF_MAX_LUT == 1024, "the header states the table's limit as a number");
    try {
        if (!eval_trace || !eval_model || !eval_params || !loss_out) throw std::runtime_error("null argument");
        const pump_fit::Problem p = pump_fit::check_problem(r, target, offsets, sample_rates, n_traces, lut_r, lut_v, n_lut, skip);
        pump_fit::check_items("evaluation", eval_trace, eval_model, eval_params, n_evals, n_traces);
        if (pred_out)
            for (size_t i = 0; i < n_evals; ++i)
                if (offsets[eval_trace[i] + 1] - offsets[eval_trace[i]] > pred_stride) throw std::runtime_error("pred_stride smaller than the trace of evaluation " + std::to_string(i));
        if (n_evals == 0) return 0;
        std::vector<uint32_t> order;
        std::vector<owdev::OwPfWaveDev> hw;
        pump_fit::pack(eval_trace, eval_model, n_evals, 64, order, hw);
        pump_fit::Staged s;                    // released on every exit path
        s.upload(p, device);
        s.upload_work(hw, order, eval_params);
        DevMem m_loss, m_pred;
        m_loss.alloc(sizeof(double) * n_evals);
        if (pred_out) {
            m_pred.alloc(sizeof(double) * n_evals * pred_stride);
            HIP_OK(hipMemsetAsync(m_pred.p, 0, sizeof(double) * n_evals * pred_stride, s.st));
        }
        owdev::k_pump_fit_eval<<<dim3((unsigned)hw.size()), dim3(64), 0, s.st>>>(
            s.traces.as<owdev::OwPfTraceDev>(), s.waves.as<owdev::OwPfWaveDev>(), s.params.as<double>(), s.dest.as<uint32_t>(), s.r.as<double>(),
            s.lnr.as<double>(), s.base.as<double>(), s.target.as<double>(), s.lut_ln.as<double>(), s.lut_v.as<double>(), s.lut_slope.as<double>(),
            s.lut_r.as<double>(), (int)n_lut, skip, m_loss.as<double>(), pred_out ? m_pred.as<double>() : nullptr, (uint64_t)pred_stride);
        HIP_OK(hipGetLastError());
        std::vector<double> h_loss(n_evals), h_pred(pred_out ? n_evals * pred_stride : 0);
        HIP_OK(hipMemcpyAsync(h_loss.data(), m_loss.p, sizeof(double) * n_evals, hipMemcpyDeviceToHost, s.st));
        if (pred_out) HIP_OK(hipMemcpyAsync(h_pred.data(), m_pred.p, sizeof(double) * h_pred.size(), hipMemcpyDeviceToHost, s.st));
        HIP_OK(hipStreamSynchronize(s.st));
        std::memcpy(loss_out, h_loss.data(), sizeof(double) * n_evals);      // the caller's buffers change only once everything has succeeded
        if (pred_out) std::memcpy(pred_out, h_pred.data(), sizeof(double) * h_pred.size());
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_pump_fit_eval: ") + ex.what()); return -1; }
}

int ow_pump_fit(const double* r, const double* target, const uint64_t* offsets, const double* sample_rates, size_t n_traces, const double* lut_r,
                const double* lut_v, size_t n_lut, const uint32_t* fit_trace, const uint32_t* fit_model, const double* x0, size_t n_fits, uint32_t skip,
                double xatol, double fatol, uint32_t maxiter, int device, double* x_out, double* fun_out, uint32_t* nit_out, uint32_t* nfev_out,
                uint32_t* status_out) {
    static_assert(owdev::PF_CONVERGED == 0 && owdev::PF_MAXITER == 1 && owdev::PF_START_INVALID == 2, "the header states the status codes as numbers");
    try {
        if (!fit_trace || !fit_model || !x0 || !x_out || !fun_out || !nit_out || !nfev_out || !status_out) throw std::runtime_error("null argument");
        const pump_fit::Problem p = pump_fit::check_problem(r, target, offsets, sample_rates, n_traces, lut_r, lut_v, n_lut, skip);
        pump_fit::check_items("fit", fit_trace, fit_model, x0, n_fits, n_traces);
        if (maxiter == 0) throw std::runtime_error("maxiter is 0");
        if (xatol != xatol || fatol != fatol) throw std::runtime_error("xatol / fatol is not a number");
        if (n_fits == 0) return 0;
        std::vector<uint32_t> order;
        std::vector<owdev::OwPfWaveDev> hw;
        pump_fit::pack(fit_trace, fit_model, n_fits, OW_PF_ROWS, order, hw);
        pump_fit::Staged s;                    // released on every exit path
        s.upload(p, device);
        s.upload_work(hw, order, x0);
        DevMem m_x, m_fun, m_nit, m_nfev, m_status;
        m_x.alloc(sizeof(double) * 4 * n_fits); m_fun.alloc(sizeof(double) * n_fits);
        m_nit.alloc(sizeof(uint32_t) * n_fits); m_nfev.alloc(sizeof(uint32_t) * n_fits); m_status.alloc(sizeof(uint32_t) * n_fits);
        owdev::k_pump_fit<<<dim3((unsigned)hw.size()), dim3(64), 0, s.st>>>(
            s.traces.as<owdev::OwPfTraceDev>(), s.waves.as<owdev::OwPfWaveDev>(), s.params.as<double>(), s.dest.as<uint32_t>(), s.r.as<double>(),
            s.lnr.as<double>(), s.base.as<double>(), s.target.as<double>(), s.lut_ln.as<double>(), s.lut_v.as<double>(), s.lut_slope.as<double>(),
            s.lut_r.as<double>(), (int)n_lut, skip, xatol, fatol, maxiter, m_x.as<double>(), m_fun.as<double>(), m_nit.as<uint32_t>(), m_nfev.as<uint32_t>(),
            m_status.as<uint32_t>());
        HIP_OK(hipGetLastError());
        std::vector<double> h_x(4 * n_fits), h_fun(n_fits);
        std::vector<uint32_t> h_nit(n_fits), h_nfev(n_fits), h_status(n_fits);
        HIP_OK(hipMemcpyAsync(h_x.data(), m_x.p, sizeof(double) * 4 * n_fits, hipMemcpyDeviceToHost, s.st));
        HIP_OK(hipMemcpyAsync(h_fun.data(), m_fun.p, sizeof(double) * n_fits, hipMemcpyDeviceToHost, s.st));
        HIP_OK(hipMemcpyAsync(h_nit.data(), m_nit.p, sizeof(uint32_t) * n_fits, hipMemcpyDeviceToHost, s.st));
        HIP_OK(hipMemcpyAsync(h_nfev.data(), m_nfev.p, sizeof(uint32_t) * n_fits, hipMemcpyDeviceToHost, s.st));
        HIP_OK(hipMemcpyAsync(h_status.data(), m_status.p, sizeof(uint32_t) * n_fits, hipMemcpyDeviceToHost, s.st));
        HIP_OK(hipStreamSynchronize(s.st));
        std::memcpy(x_out, h_x.data(), sizeof(double) * 4 * n_fits);         // the caller's buffers change only once everything has succeeded
        std::memcpy(fun_out, h_fun.data(), sizeof(double) * n_fits);
        std::memcpy(nit_out, h_nit.data(), sizeof(uint32_t) * n_fits);
        std::memcpy(nfev_out, h_nfev.data(), sizeof(uint32_t) * n_fits);
        std::memcpy(status_out, h_status.data(), sizeof(uint32_t) * n_fits);
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_pump_fit: ") + ex.what()); return -1; }
}
}  // extern "C"
