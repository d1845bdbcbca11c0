// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the note-on MLP's corrections given at run time --
// weight sets evaluated on the device (k_mlp_infer, ow_mlp_mfma.h), or explicit per-job corrections, fed into the batch render's note-on
// (batch_render_impl, api_offline.inc).  The reference has no such entry point: it bakes mlp_weights.rs at compile time.
static_assert(sizeof(ow_mlp_weights) == sizeof(owdev::MlpWeightsDev), "ow_mlp_weights is read by the device as MlpWeightsDev");
static_assert(sizeof(ow_mlp_weights) == sizeof(double) * 529, "2 x 16 + 16 + 16 x 16 + 16 + 16 x 11 + 11 + 11 + 11 doubles, no padding");
static_assert(sizeof(ow_mlp_corrections) == sizeof(owdev::MlpOut), "ow_mlp_corrections is read by the device as MlpOut");
namespace {

void mlp_builtin(ow_mlp_weights& w) {
    std::memcpy(w.w1, MLP_W1, sizeof w.w1); std::memcpy(w.b1, MLP_B1, sizeof w.b1);
    std::memcpy(w.w2, MLP_W2, sizeof w.w2); std::memcpy(w.b2, MLP_B2, sizeof w.b2);
    std::memcpy(w.w3, MLP_W3, sizeof w.w3); std::memcpy(w.b3, MLP_B3, sizeof w.b3);
    std::memcpy(w.target_means, MLP_TARGET_MEANS, sizeof w.target_means); std::memcpy(w.target_stds, MLP_TARGET_STDS, sizeof w.target_stds);
}

// every weight of every set is finite; the refusal names the set (what: "set ", or what the caller calls its sets) and the field
void check_weight_sets(const ow_mlp_weights* sets, size_t n_sets, const char* what = "set ", const char* field_prefix = "") {
    struct Field { const char* name; size_t offset, rows, cols; };
    static const Field fields[] = {
        {"w1", offsetof(ow_mlp_weights, w1), 16, 2},   {"b1", offsetof(ow_mlp_weights, b1), 16, 0},
        {"w2", offsetof(ow_mlp_weights, w2), 16, 16},  {"b2", offsetof(ow_mlp_weights, b2), 16, 0},
        {"w3", offsetof(ow_mlp_weights, w3), 11, 16},  {"b3", offsetof(ow_mlp_weights, b3), 11, 0},
        {"target_means", offsetof(ow_mlp_weights, target_means), 11, 0}, {"target_stds", offsetof(ow_mlp_weights, target_stds), 11, 0}};
    for (size_t s = 0; s < n_sets; ++s)
        for (const Field& f : fields) {
            const double* v = (const double*)((const char*)&sets[s] + f.offset);
            const size_t n = f.rows * (f.cols ? f.cols : 1);
            for (size_t k = 0; k < n; ++k)
                if (!std::isfinite(v[k])) {
                    const std::string idx = f.cols ? "[" + std::to_string(k / f.cols) + "][" + std::to_string(k % f.cols) + "]" : "[" + std::to_string(k) + "]";
                    throw std::runtime_error(what + std::to_string(s) + ": " + field_prefix + f.name + idx + " is not finite");
                }
        }
}

void check_corrections(const ow_mlp_corrections* corr, size_t n_jobs) {
    for (size_t j = 0; j < n_jobs; ++j) {
        const std::string at = "job " + std::to_string(j) + ": ";
        for (int h = 0; h < 5; ++h) {
            check_finite(at, ("freq_offsets_cents[" + std::to_string(h) + "]").c_str(), corr[j].freq_offsets_cents[h]);
            check_positive_finite(at, ("decay_offsets[" + std::to_string(h) + "]").c_str(), corr[j].decay_offsets[h]);   // note-on divides by it
        }
        check_finite(at, "ds_correction", corr[j].ds_correction);
    }
}

// sets (host, or nullptr = the built-in one) onto the device, on st
void upload_sets(DevMem& m, const ow_mlp_weights* sets, size_t n_sets, std::unique_ptr<ow_mlp_weights>& builtin, hipStream_t st) {
    if (!sets) { builtin.reset(new ow_mlp_weights); mlp_builtin(*builtin); sets = builtin.get(); }
    m.alloc(sizeof(ow_mlp_weights) * n_sets);
    HIP_OK(hipMemcpyAsync(m.p, sets, sizeof(ow_mlp_weights) * n_sets, hipMemcpyHostToDevice, st));
}

constexpr size_t MLP_MAX_SETS = 65535;      // the sets are the grid's y dimension

}  // namespace

extern "C" {

int ow_mlp_default_weights(ow_mlp_weights* out) {
    if (!out) { set_err("ow_mlp_default_weights: null argument"); return -1; }
    mlp_builtin(*out);
    return 0;
}

int ow_mlp_infer(const ow_mlp_weights* sets, size_t n_sets, const uint8_t* notes, const double* velocities, size_t n_points, int device,
                 ow_mlp_corrections* out, double* raw_out) {
    try {
        if (!sets && n_sets != 1) throw std::runtime_error("null argument: sets (NULL stands for the built-in set with n_sets == 1 only)");
        if (!notes || !velocities || !out) throw std::runtime_error("null argument");
        if (n_sets == 0 || n_points == 0) return 0;
        if (n_sets > MLP_MAX_SETS) throw std::runtime_error("more than 65535 weight sets in one call");
        if (n_points > 0x7FFFFFFFu - 64u || n_sets * n_points > (size_t)1 << 36) throw std::runtime_error("too many points in one call");
        if (sets) check_weight_sets(sets, n_sets);
        for (size_t i = 0; i < n_points; ++i) check_finite("point " + std::to_string(i) + ": ", "velocity", velocities[i]);
        require_device(device);
        StreamOwner so;
        so.create();
        hipStream_t st = so.s;
        std::unique_ptr<ow_mlp_weights> builtin;        // outlives its upload
        DevMem m_sets, m_notes, m_vels, m_out, m_raw;
        upload_sets(m_sets, sets, n_sets, builtin, st);
        m_notes.alloc(n_points); m_vels.alloc(sizeof(double) * n_points);
        m_out.alloc(sizeof(owdev::MlpOut) * n_sets * n_points);
        if (raw_out) m_raw.alloc(sizeof(double) * 11 * n_sets * n_points);
        HIP_OK(hipMemcpyAsync(m_notes.p, notes, n_points, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_vels.p, velocities, sizeof(double) * n_points, hipMemcpyHostToDevice, st));
        owdev::k_mlp_infer<<<dim3((unsigned)((n_points + 63) / 64), (unsigned)n_sets), dim3(64), 0, st>>>(
            m_sets.as<owdev::MlpWeightsDev>(), m_notes.as<uint8_t>(), m_vels.as<double>(), nullptr, (unsigned)n_points, nullptr, nullptr,
            m_out.as<owdev::MlpOut>(), raw_out ? m_raw.as<double>() : nullptr);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(out, m_out.p, sizeof(owdev::MlpOut) * n_sets * n_points, hipMemcpyDeviceToHost, st));
        if (raw_out) HIP_OK(hipMemcpyAsync(raw_out, m_raw.p, sizeof(double) * 11 * n_sets * n_points, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_mlp_infer: ") + ex.what()); return -1; }
}

long long ow_batch_render_corrected(const ow_job* jobs, size_t n_jobs, const ow_batch_cfg* cfg, const ow_mlp_corrections* corr, double* out,
                                    size_t stride, int out_is_device) {
    try {
        if (!corr) throw std::runtime_error("null argument: corr");
        if (jobs && n_jobs) check_corrections(corr, n_jobs);
    } catch (const std::exception& ex) { set_err(std::string("ow_batch_render_corrected: ") + ex.what()); return -1; }
    return batch_render_impl("ow_batch_render_corrected", jobs, n_jobs, cfg, out, stride, out_is_device,
                             [=](OfflineCall& call, owdev::MlpOut* d_corr) {
                                 HIP_OK(hipMemcpyAsync(d_corr, corr, sizeof(ow_mlp_corrections) * n_jobs, hipMemcpyHostToDevice, call.st()));
                             });
}

long long ow_batch_render_mlp(const ow_job* jobs, size_t n_jobs, const ow_batch_cfg* cfg, const ow_mlp_weights* sets, size_t n_sets,
                              const uint32_t* set_of_job, double* out, size_t stride, int out_is_device) {
    // the jobs grouped by weight set (a block of k_mlp_infer evaluates ONE set), scattered back by job index
    std::vector<uint32_t> set_begin, scatter;
    std::vector<uint8_t> notes, enabled;
    std::vector<double> vels;
    try {
        if (!sets && n_sets != 1) throw std::runtime_error("null argument: sets (NULL stands for the built-in set with n_sets == 1 only)");
        if (!set_of_job) throw std::runtime_error("null argument: set_of_job");
        if (n_sets == 0) throw std::runtime_error("no weight set");
        if (n_sets > MLP_MAX_SETS) throw std::runtime_error("more than 65535 weight sets in one call");
        if (jobs && n_jobs) {
            if (n_jobs > 0x7FFFFFFFu - 64u) throw std::runtime_error("too many jobs in one call");
            for (size_t j = 0; j < n_jobs; ++j)
                if (set_of_job[j] >= n_sets)
                    throw std::runtime_error("job " + std::to_string(j) + ": set_of_job " + std::to_string(set_of_job[j]) + " is not below n_sets " + std::to_string(n_sets));
            if (sets) check_weight_sets(sets, n_sets);
            set_begin.assign(n_sets + 1, 0);
            for (size_t j = 0; j < n_jobs; ++j) set_begin[set_of_job[j] + 1] += 1;
            for (size_t s = 0; s < n_sets; ++s) set_begin[s + 1] += set_begin[s];
            std::vector<uint32_t> next(set_begin.begin(), set_begin.end() - 1);
            scatter.resize(n_jobs); notes.resize(n_jobs); enabled.resize(n_jobs); vels.resize(n_jobs);
            for (size_t j = 0; j < n_jobs; ++j) {
                const uint32_t q = next[set_of_job[j]]++;
                scatter[q] = (uint32_t)j;
                notes[q] = std::min<uint8_t>(std::max<uint8_t>(jobs[j].note, OW_MIDI_LO), OW_MIDI_HI);     // the note k_job_voice strikes
                vels[q] = (double)jobs[j].velocity / 127.0;                                                // main.rs:403
                enabled[q] = jobs[j].mlp ? 1 : 0;
            }
        }
    } catch (const std::exception& ex) { set_err(std::string("ow_batch_render_mlp: ") + ex.what()); return -1; }
    return batch_render_impl("ow_batch_render_mlp", jobs, n_jobs, cfg, out, stride, out_is_device, [&](OfflineCall& call, owdev::MlpOut* d_corr) {
        hipStream_t st = call.st();
        std::unique_ptr<ow_mlp_weights> builtin;
        // the inputs are released at the end of this scope: hipFree waits for the kernel that reads them
        DevMem m_sets, m_begin, m_scatter, m_notes, m_enabled, m_vels;
        upload_sets(m_sets, sets, n_sets, builtin, st);
        m_begin.alloc(sizeof(uint32_t) * (n_sets + 1)); m_scatter.alloc(sizeof(uint32_t) * n_jobs);
        m_notes.alloc(n_jobs); m_enabled.alloc(n_jobs); m_vels.alloc(sizeof(double) * n_jobs);
        HIP_OK(hipMemcpyAsync(m_begin.p, set_begin.data(), sizeof(uint32_t) * (n_sets + 1), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_scatter.p, scatter.data(), sizeof(uint32_t) * n_jobs, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_notes.p, notes.data(), n_jobs, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_enabled.p, enabled.data(), n_jobs, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_vels.p, vels.data(), sizeof(double) * n_jobs, hipMemcpyHostToDevice, st));
        uint32_t widest = 0;
        for (size_t s = 0; s < n_sets; ++s) widest = std::max(widest, set_begin[s + 1] - set_begin[s]);
        owdev::k_mlp_infer<<<dim3((widest + 63u) / 64u, (unsigned)n_sets), dim3(64), 0, st>>>(
            m_sets.as<owdev::MlpWeightsDev>(), m_notes.as<uint8_t>(), m_vels.as<double>(), m_enabled.as<uint8_t>(), (unsigned)n_jobs,
            m_begin.as<uint32_t>(), m_scatter.as<uint32_t>(), d_corr, nullptr);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));     // the host vectors and `builtin` above were the sources of asynchronous copies
    });
}

}  // extern "C"
