// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): what the offline entry points (batch render, render-midi and the
// preamp-bench measurement commands) share -- argument checks, row geometry and chunking, the per-call device setup, the melange power amp
// as a stage of its own.  An api_*.inc says only what is particular to its command.
namespace {

// ---- refusals: the texts are part of the C-ABI's behaviour (the callers' tests match them) ------------------------------------------
void require_device(int device) {
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw std::runtime_error("no HIP device: openwurli-hip has no CPU fallback");
    HIP_OK(hipSetDevice(device));
}
// fields: which size fields disagree, with their verb ("ow_batch_cfg.struct_size / job_size do", "ow_midi_render_cfg.struct_size does")
std::string abi_mismatch(const char* fields) {
    return std::string("ABI mismatch: ") + fields + " not match this library's openwurli_hip.h (OW_ABI_VERSION " + std::to_string(OW_ABI_VERSION) + ")";
}
void require_known_kinds(int preamp_kind, int power_amp_kind = OW_POWER_AMP_BEHAVIORAL) {
    if (preamp_kind != OW_PREAMP_LEGACY8 && preamp_kind != OW_PREAMP_MELANGE12) throw std::runtime_error("unknown preamp_kind");
    if (power_amp_kind != OW_POWER_AMP_BEHAVIORAL && power_amp_kind != OW_POWER_AMP_MELANGE) throw std::runtime_error("unknown power_amp_kind");
}
// the commands whose chain is the legacy preamp and the behavioural power amp in one kernel (render-poly, centroid-track)
void require_legacy_chain(int preamp_kind, int power_amp_kind) {
    if (preamp_kind == OW_PREAMP_MELANGE12)
        throw std::runtime_error("preamp_kind OW_PREAMP_MELANGE12 is not supported: the melange preamp's reset() discards --ldr (see openwurli_hip.h)");
    if (preamp_kind != OW_PREAMP_LEGACY8) throw std::runtime_error("unknown preamp_kind");
    if (power_amp_kind == OW_POWER_AMP_MELANGE)
        throw std::runtime_error("power_amp_kind OW_POWER_AMP_MELANGE is not supported: it needs its own launch between the stages (see openwurli_hip.h)");
    if (power_amp_kind != OW_POWER_AMP_BEHAVIORAL) throw std::runtime_error("unknown power_amp_kind");
}
// at: the item's prefix, "point 3: " / "job 3: " / "chord 3: "
void check_note_velocity(const std::string& at, int note, int velocity) {
    if (note < OW_MIDI_LO || note > OW_MIDI_HI) throw std::runtime_error(at + "note " + std::to_string(note) + " outside 33..96 (the tables' range)");
    if (velocity > 127) throw std::runtime_error(at + "velocity " + std::to_string(velocity) + " above 127 (a MIDI velocity byte)");
}
void check_finite(const std::string& at, const char* name, double x) {
    if (!std::isfinite(x)) throw std::runtime_error(at + name + " is not finite");
}
void check_positive_finite(const std::string& at, const char* name, double x) {
    if (!(std::isfinite(x) && x > 0.0)) throw std::runtime_error(at + name + " is not a finite positive number");
}

// ---- lengths, rows, chunks ----------------------------------------------------------------------------------------------------------
// Rust's `f64 as usize`: NaN and negatives give 0, large values saturate
inline size_t rust_as_usize(double x) { return !(x > 0.0) ? 0 : (x >= 18446744073709551615.0 ? SIZE_MAX : (size_t)x); }
// device rows of n samples start 512 bytes apart
inline long long row_stride(long long n) { return (n + 63) / 64 * 64; }
// items per chunk: what budget_bytes of device memory hold at bytes_per_item each, at most cap of them (cap > 0: an OW_*_CHUNK switch,
// tests), no more than there are, and at least one
size_t budget_chunk(size_t budget_bytes, size_t bytes_per_item, long long cap, size_t n_items) {
    size_t c = std::max<size_t>(budget_bytes / bytes_per_item, 1);
    if (cap > 0) c = std::min(c, (size_t)cap);
    return std::max<size_t>(std::min(c, n_items), 1);
}
// bins k of numpy's frequency axis (k * val, k < nb) with f_lo <= k * val <= f_hi, numpy's own arithmetic: k_lo..k_hi inclusive; both are
// left as they are (the callers' "no bin" state, k_lo > k_hi) when the mask is empty
inline void feat_band_bins(double val, uint64_t nb, double f_lo, double f_hi, uint32_t& k_lo_out, uint32_t& k_hi_out) {
    double q = f_lo / val;
    uint64_t k = (q > 0.0 && q < (double)nb) ? (uint64_t)q : (q >= (double)nb ? nb : 0);
    while (k > 0 && (double)(k - 1) * val >= f_lo) --k;
    while (k < nb && (double)k * val < f_lo) ++k;
    const uint64_t k_lo = k;
    while (k < nb && (double)k * val <= f_hi) ++k;
    if (k > k_lo) { k_lo_out = (uint32_t)k_lo; k_hi_out = (uint32_t)(k - 1); }
}
// rows of n doubles, dev_stride_doubles apart on the device -> host rows host_stride doubles apart, on st (no synchronisation)
void rows_to_host(double* host, size_t host_stride, const void* dev, size_t dev_stride_doubles, size_t n, size_t rows, hipStream_t st) {
    HIP_OK(hipMemcpy2DAsync(host, host_stride * sizeof(double), dev, dev_stride_doubles * sizeof(double), n * sizeof(double), rows, hipMemcpyDeviceToHost, st));
}

// ---- preamp-bench's figures from a kernel's sums (main.rs:893-927, 2241-2247) -------------------------------------------------------
namespace measure {
inline double to_dbfs(double val) { return val > 1e-15 ? 20.0 * std::log10(val) : -120.0; }
inline double rms_db(double mean_sq) { return mean_sq > 0.0 ? 10.0 * std::log10(mean_sq) : -120.0; }
inline double dft_magnitude(double re, double im, double n) {
    const double a = re / n, b = im / n;
    return 2.0 * std::sqrt(a * a + b * b);
}
}  // namespace measure

// ---- one call of an offline entry point on the device -------------------------------------------------------------------------------
// Selects the device, then owns the call's stream, its OwConsts (sr, preamp_kind) on the device and, when asked for, the voices' note
// table.  The switches are read once per call.  Declare it before the call's own buffers: they are then released first (hipFree waits for
// the device), the stream after them, the host copy of the constants last.
struct OfflineCall {
    const Switches sw = Switches::from_env();
    OfflineCall(int device, double sr, int preamp_kind, bool note_table) : device_(device), hc_(new OwConsts()) {
        require_device(device);
        owhip::build_consts(*hc_, sr, preamp_kind);
        so_.create();
        m_K_.alloc(sizeof(OwConsts));
        HIP_OK(hipMemcpyAsync(m_K_.p, hc_.get(), sizeof(OwConsts), hipMemcpyHostToDevice, so_.s));
        if (note_table) {
            m_nt_.alloc(sizeof(double) * NT_COUNT * 64);
            owdev::k_note_table<<<dim3(1), dim3(64), 0, so_.s>>>(m_nt_.as<double>());
            HIP_OK(hipGetLastError());
        }
    }
    hipStream_t st() const { return so_.s; }
    const OwConsts* dK() const { return m_K_.as<OwConsts>(); }
    const double* nt() const { return m_nt_.as<double>(); }
    // the melange preamp's settled state (18 doubles: new() and reset() clone it, melange_adapter.rs:22-29, 88-93), fetched on first use
    const double* mel_settled() {
        if (!m_settled_.p) {
            m_settled_.alloc(sizeof(double) * 18);
            mel_settled_to_device(device_, m_settled_.as<double>(), so_.s);
        }
        return m_settled_.as<double>();
    }

  private:
    int device_;
    std::unique_ptr<OwConsts> hc_;       // outlives its upload
    StreamOwner so_;
    DevMem m_K_, m_nt_, m_settled_;
};

// The melange power amp (a build without `legacy-power-amp`) as a launch of its own: PowerAmp::new() is new_at_sample_rate(44 100) whatever
// the render's rate is (power_amp.rs:321-323), the 7-BJT solver with eight lanes per row (k_mpa_debug).  The caller keeps it alive until
// the stream is synchronised.
struct MelPowerAmpStage {
    MelPowerAmpStage(int device, hipStream_t st) : st_(st), hpa_(new OwPaConsts()) {
        owhip::build_pa_consts(*hpa_, 44100.0);
        d_pac_.alloc(sizeof(OwPaConsts));
        d_pas_.alloc(sizeof(double) * owdev::PAS_CIRCUIT_END);
        pa_settled_to_device(device, d_pas_.as<double>(), st);
        HIP_OK(hipMemcpyAsync(d_pac_.p, hpa_.get(), sizeof(OwPaConsts), hipMemcpyHostToDevice, st));
    }
    // in -> out, rows of n samples `stride` apart
    void run(const double* in, double* out, long long n, int rows, int rail_sag, long long stride) {
        owdev::k_mpa_debug<<<dim3((unsigned)((rows + PA_EPB - 1) / PA_EPB)), dim3(PA_WPB * 64), 0, st_>>>(d_pac_.as<OwPaConsts>(), d_pas_.as<double>(), in, out, nullptr, n,
                                                                                                         rows, rail_sag, nullptr, nullptr, nullptr, stride);
        HIP_OK(hipGetLastError());
    }

  private:
    hipStream_t st_;
    std::unique_ptr<OwPaConsts> hpa_;    // outlives its upload
    DevMem d_pac_, d_pas_;
};

}  // namespace
