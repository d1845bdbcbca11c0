// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the pickup-law study (ml/h3_analysis_v2.py):
// ow_pickup_law, the harmonics of a sine reed through clip, a pickup law, the one-pole high-pass and a DFT probe per harmonic, for many
// (carrier, law) jobs per call.  The host checks, sorts the laws by kind and cuts them into wavefronts; ow_pickup_law_kernels.h does the rest.
namespace {
namespace pickup_law {
// The laws sorted by kind, stable, and cut into wavefronts of at most 64 laws of one kind.  order[i]: the caller's index of sorted law i.
void pack(const int32_t* kinds, size_t n, std::vector<uint32_t>& order, std::vector<owdev::OwPlChunkDev>& chunks) {
    order.resize(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return kinds[a] < kinds[b]; });
    chunks.clear();
    for (size_t i = 0; i < n;) {
        const int32_t k = kinds[order[i]];
        size_t j = i;
        while (j < n && j - i < (size_t)owdev::PL_TILE && kinds[order[j]] == k) ++j;
        chunks.push_back(owdev::OwPlChunkDev{(uint32_t)k, (uint32_t)i, (uint32_t)(j - i), 0u});
        i = j;
    }
}
}  // namespace pickup_law
}  // namespace

extern "C" {
int ow_pickup_law(const double* carriers, size_t n_carriers, const int32_t* law_kinds, const double* law_params, size_t n_laws, double sample_rate,
                  uint32_t n_samples, uint32_t n_harmonics, double sensitivity, double clip, double hpf_b0, double hpf_a1, int device, double* amps_out,
                  double* y_peak_out) {
    static_assert(owdev::PL_MAX_H == OW_MAX_HARMONICS, "the kernel's accumulators are the header's harmonic limit");
    try {
        if (!carriers || !law_kinds || !law_params || !amps_out || !y_peak_out) throw std::runtime_error("null argument");
        if (n_samples < 4) throw std::runtime_error("n_samples " + std::to_string(n_samples) + ": fewer than 4");
        if (n_harmonics == 0 || n_harmonics > OW_MAX_HARMONICS)
            throw std::runtime_error("n_harmonics " + std::to_string(n_harmonics) + " outside 1.." + std::to_string(OW_MAX_HARMONICS));
        check_positive_finite("", "sample_rate", sample_rate);
        if (!(std::isfinite(clip) && clip > 0.0 && clip < 1.0)) throw std::runtime_error("clip is not inside (0, 1)");
        check_finite("", "sensitivity", sensitivity);
        check_finite("", "hpf_b0", hpf_b0);
        check_finite("", "hpf_a1", hpf_a1);
        if (n_carriers > (size_t)INT32_MAX || n_laws > (size_t)INT32_MAX) throw std::runtime_error("too many carriers or laws");
        for (size_t l = 0; l < n_laws; ++l) {
            const std::string at = "law " + std::to_string(l) + ": ";
            if (law_kinds[l] < 0 || law_kinds[l] > 2) throw std::runtime_error(at + "kind " + std::to_string(law_kinds[l]) + " outside 0..2");
            check_finite(at, "parameter", law_params[l]);
        }
        for (size_t c = 0; c < n_carriers; ++c) {
            const std::string at = "carrier " + std::to_string(c) + ": ";
            check_finite(at, "f0_hz", carriers[3 * c]);
            check_finite(at, "ds", carriers[3 * c + 1]);
            check_finite(at, "vel_scale", carriers[3 * c + 2]);
        }
        if (n_carriers == 0 || n_laws == 0) return 0;
        std::vector<uint32_t> order;
        std::vector<owdev::OwPlChunkDev> chunks;
        pickup_law::pack(law_kinds, n_laws, order, chunks);
        if (n_carriers * chunks.size() > (size_t)INT32_MAX) throw std::runtime_error("too many (carrier, law) jobs for one call");
        std::vector<double> sorted(n_laws);
        for (size_t i = 0; i < n_laws; ++i) sorted[i] = law_params[order[i]];
        const size_t n_amps = n_carriers * n_laws * (size_t)n_harmonics;

        HIP_OK(hipSetDevice(device));
        StreamOwner so;                        // released on every exit path, as the buffers are
        so.create();
        DevMem m_car, m_chunks, m_params, m_dest, m_amps, m_peak;
        m_car.alloc(sizeof(double) * 3 * n_carriers);
        m_chunks.alloc(sizeof(owdev::OwPlChunkDev) * chunks.size());
        m_params.alloc(sizeof(double) * n_laws);
        m_dest.alloc(sizeof(uint32_t) * n_laws);
        m_amps.alloc(sizeof(double) * n_amps);
        m_peak.alloc(sizeof(double) * n_carriers);
        HIP_OK(hipMemcpyAsync(m_car.p, carriers, sizeof(double) * 3 * n_carriers, hipMemcpyHostToDevice, so.s));
        HIP_OK(hipMemcpyAsync(m_chunks.p, chunks.data(), sizeof(owdev::OwPlChunkDev) * chunks.size(), hipMemcpyHostToDevice, so.s));
        HIP_OK(hipMemcpyAsync(m_params.p, sorted.data(), sizeof(double) * n_laws, hipMemcpyHostToDevice, so.s));
        HIP_OK(hipMemcpyAsync(m_dest.p, order.data(), sizeof(uint32_t) * n_laws, hipMemcpyHostToDevice, so.s));
        owdev::k_pickup_law<<<dim3((unsigned)(n_carriers * chunks.size())), dim3(owdev::PL_TILE), 0, so.s>>>(
            m_car.as<double>(), m_chunks.as<owdev::OwPlChunkDev>(), (uint32_t)chunks.size(), m_params.as<double>(), m_dest.as<uint32_t>(), (uint32_t)n_laws,
            sample_rate, n_samples, (int)n_harmonics, sensitivity, clip, hpf_b0, hpf_a1, m_amps.as<double>(), m_peak.as<double>());
        HIP_OK(hipGetLastError());
        std::vector<double> h_amps(n_amps), h_peak(n_carriers);
        HIP_OK(hipMemcpyAsync(h_amps.data(), m_amps.p, sizeof(double) * n_amps, hipMemcpyDeviceToHost, so.s));
        HIP_OK(hipMemcpyAsync(h_peak.data(), m_peak.p, sizeof(double) * n_carriers, hipMemcpyDeviceToHost, so.s));
        HIP_OK(hipStreamSynchronize(so.s));
        std::memcpy(amps_out, h_amps.data(), sizeof(double) * n_amps);      // the caller's buffers change only once everything has succeeded
        std::memcpy(y_peak_out, h_peak.data(), sizeof(double) * n_carriers);
        return 0;
    } catch (const std::exception& ex) {
        (void)hipGetLastError();               // the runtime keeps a failed call's error (a device index it does not have) until it is read:
                                               // left there, the next call's launch check would report it as its own
        set_err(std::string("ow_pickup_law: ") + ex.what());
        return -1;
    }
}
}  // extern "C"
