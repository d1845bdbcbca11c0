// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the recording side of the ML loop, many segments per
// call -- ow_goertzel_harmonics (ml/goertzel_utils.py:34-57, 106-119: k_goertzel runs the recurrences, the host plans the bins and
// finishes) and ow_interharmonic_noise (ml/compute_residuals.py:93-117: k_feat_window's windowed copy, k_feat_band_median).
namespace {
namespace harmonics {
void check_cfg(const ow_harmonics_cfg* cfg) {
    if (!cfg) throw std::runtime_error("null argument");
    if (cfg->struct_size != sizeof(ow_harmonics_cfg) || cfg->segment_size != sizeof(ow_segment))
        throw std::runtime_error(abi_mismatch("ow_harmonics_cfg.struct_size / segment_size do"));
    if (cfg->wav24_mode != OW_WAV_NONE && cfg->wav24_mode != OW_WAV_ROUND && cfg->wav24_mode != OW_WAV_TRUNCATE) throw std::runtime_error("unknown wav24_mode");
    check_positive_finite("", "sample_rate", cfg->sample_rate);
    if (!(std::isfinite(cfg->search_pct) && cfg->search_pct >= 0.0)) throw std::runtime_error("search_pct is not a finite non-negative number");
}
// the segment's length
uint32_t check_segment(const ow_segment& g, size_t i, size_t n_rows, size_t stride) {
    const std::string at = "segment " + std::to_string(i);
    if (g.row >= n_rows || g.end <= g.start || g.end > stride || g.n_harmonics > OW_MAX_HARMONICS) throw std::runtime_error(at + " out of range");
    if (g.end - g.start > (1u << 22)) throw std::runtime_error(at + " longer than 2^22 samples");
    check_finite(at + ": ", "f0", g.f0);
    return g.end - g.start;
}
// the audio on the device: the caller's buffer, or a copy of it that `own` holds
const double* device_audio(const double* audio, size_t n_rows, size_t stride, int audio_is_device, DevMem& own, hipStream_t st) {
    if (audio_is_device) return audio;
    own.alloc(sizeof(double) * n_rows * stride);
    HIP_OK(hipMemcpyAsync(own.p, audio, sizeof(double) * n_rows * stride, hipMemcpyHostToDevice, st));
    return own.as<double>();
}
}  // namespace harmonics
}  // namespace

extern "C" {
int ow_goertzel_harmonics(const double* audio, size_t n_rows, size_t stride, const ow_segment* segs, size_t n_segs, const ow_harmonics_cfg* cfg,
                          double* amps, double* coeffs_out, int32_t* bins_out) {
    static_assert(OW_MAX_HARMONICS * OW_GOERTZEL_OFFSETS <= OW_GOERTZEL_MAX_REC, "one wavefront's two slots per lane cover a segment");
    try {
        harmonics::check_cfg(cfg);
        if (n_segs == 0) return 0;
        if (!audio || !segs || !amps) throw std::runtime_error("null argument");
        const double sr = cfg->sample_rate, pct = cfg->search_pct;
        // np.linspace(-pct, pct, 11): arange(11) * step + start with step = (stop - start) / 10, the last one set to stop
        double offs[OW_GOERTZEL_OFFSETS];
        {
            const double start = -pct, stop = pct, delta = stop - start, step = delta / (double)(OW_GOERTZEL_OFFSETS - 1);
            for (int i = 0; i < OW_GOERTZEL_OFFSETS; ++i)
                offs[i] = (step == 0.0 ? (double)i / (double)(OW_GOERTZEL_OFFSETS - 1) * delta : (double)i * step) + start;
            offs[OW_GOERTZEL_OFFSETS - 1] = stop;
        }
        const size_t per_seg = (size_t)OW_MAX_HARMONICS * OW_GOERTZEL_OFFSETS;
        std::vector<owdev::OwGoertzelSegDev> hs;       // segments with at least one recurrence: one wavefront each
        std::vector<double> coeff;                     // per recurrence
        std::vector<int32_t> rec_of(n_segs * per_seg, -1);   // (segment, harmonic, offset) -> recurrence, -1: skipped
        std::vector<int32_t> bins(n_segs * per_seg, -1);
        std::vector<double> coeffs(n_segs * per_seg, 0.0);
        uint64_t q_off = 0;
        for (size_t i = 0; i < n_segs; ++i) {
            const ow_segment& g = segs[i];
            const uint32_t n = harmonics::check_segment(g, i, n_rows, stride);
            const double N = (double)n;
            owdev::OwGoertzelSegDev d;
            d.x_off = (uint64_t)g.row * stride + g.start; d.q_off = q_off; d.n = n; d.rec0 = (uint32_t)coeff.size(); d.n_rec = 0; d.pad = 0;
            for (uint32_t h = 0; h < g.n_harmonics; ++h) {
                const double fh = g.f0 * (double)(h + 1);
                if (fh >= sr / 2 - 100) continue;
                const size_t at = i * per_seg + (size_t)h * OW_GOERTZEL_OFFSETS;
                for (int o = 0; o < OW_GOERTZEL_OFFSETS; ++o) {
                    const double f = fh * (1.0 + offs[o]);
                    const double kf = std::nearbyint(f * N / sr);          // int(round(f * N / sr)): half to even
                    if (!(kf > 0.0) || kf >= (double)(n / 2)) continue;    // k <= 0 or k >= N // 2
                    const uint32_t k = (uint32_t)kf;
                    const double w = 2.0 * OW_PI * (double)k / N;
                    const double c = 2.0 * std::cos(w);
                    bins[at + o] = (int32_t)k; coeffs[at + o] = c;
                    int32_t r = -1;
                    for (int p = 0; p < o; ++p)                           // an earlier offset of this harmonic with the same bin runs for both
                        if (bins[at + p] == (int32_t)k) { r = rec_of[at + p]; break; }
                    if (r < 0) { r = (int32_t)coeff.size(); coeff.push_back(c); ++d.n_rec; }
                    rec_of[at + o] = r;
                }
            }
            if (d.n_rec) { hs.push_back(d); q_off += n; }
        }
        if (coeff.size() > (size_t)INT32_MAX) throw std::runtime_error("too many recurrences in one call");
        std::vector<double2> state(coeff.size());
        if (!hs.empty()) {
            HIP_OK(hipSetDevice(cfg->device));
            StreamOwner so;
            so.create();
            hipStream_t st = so.s;
            DevMem own_audio, m_q, m_segs, m_coeff, m_out;   // released on every exit path
            const double* d_audio = harmonics::device_audio(audio, n_rows, stride, cfg->audio_is_device, own_audio, st);
            m_segs.alloc(sizeof(owdev::OwGoertzelSegDev) * hs.size());
            m_coeff.alloc(sizeof(double) * coeff.size());
            m_out.alloc(sizeof(double2) * coeff.size());
            HIP_OK(hipMemcpyAsync(m_segs.p, hs.data(), sizeof(owdev::OwGoertzelSegDev) * hs.size(), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(m_coeff.p, coeff.data(), sizeof(double) * coeff.size(), hipMemcpyHostToDevice, st));
            const owdev::OwGoertzelSegDev* d_segs = m_segs.as<owdev::OwGoertzelSegDev>();
            const bool quant = cfg->wav24_mode != OW_WAV_NONE;
            if (quant) {
                m_q.alloc(sizeof(double) * q_off);
                owdev::k_goertzel_quant<<<dim3((unsigned)hs.size()), dim3(256), 0, st>>>(d_audio, d_segs, m_q.as<double>(), cfg->wav24_mode);
                HIP_OK(hipGetLastError());
            }
            owdev::k_goertzel<<<dim3((unsigned)hs.size()), dim3(64), 0, st>>>(quant ? m_q.as<double>() : d_audio, d_segs, quant ? 1 : 0,
                                                                             m_coeff.as<double>(), m_out.as<double2>());
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(state.data(), m_out.p, sizeof(double2) * coeff.size(), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
        }
        for (size_t i = 0; i < n_segs; ++i) {
            const ow_segment& g = segs[i];
            const double N = (double)(g.end - g.start);
            for (uint32_t h = 0; h < OW_MAX_HARMONICS; ++h) {
                double a = 0.0;
                if (h < g.n_harmonics) {
                    double best = 0.0;
                    const size_t at = i * per_seg + (size_t)h * OW_GOERTZEL_OFFSETS;
                    for (int o = 0; o < OW_GOERTZEL_OFFSETS; ++o) {
                        if (rec_of[at + o] < 0) continue;
                        const double c = coeffs[at + o], s1 = state[rec_of[at + o]].x, s2 = state[rec_of[at + o]].y;
                        const double mag = std::sqrt(s1 * s1 + s2 * s2 - c * s1 * s2) / N * 2.0;
                        if (mag > best) best = mag;
                    }
                    a = g.f0 * (double)(h + 1) >= sr / 2 - 100 ? 1e-20 : std::max(best, 1e-20);
                }
                amps[i * OW_MAX_HARMONICS + h] = a;
            }
        }
        if (coeffs_out) std::memcpy(coeffs_out, coeffs.data(), sizeof(double) * coeffs.size());
        if (bins_out) std::memcpy(bins_out, bins.data(), sizeof(int32_t) * bins.size());
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_goertzel_harmonics: ") + ex.what()); return -1; }
}

int ow_interharmonic_noise(const double* audio, size_t n_rows, size_t stride, const ow_segment* segs, size_t n_segs, const ow_harmonics_cfg* cfg,
                           double* noise) {
    static_assert(OW_NOISE_MAX_BAND_BINS == OW_BAND_MAX_BINS, "the header's limit is the kernel's");
    try {
        harmonics::check_cfg(cfg);
        if (n_segs == 0) return 0;
        if (!audio || !segs || !noise) throw std::runtime_error("null argument");
        const double sr = cfg->sample_rate;
        std::vector<owdev::OwSegDev> hs(n_segs);
        std::vector<owdev::OwBandDev> hb;
        uint64_t off = 0;
        for (size_t i = 0; i < n_segs; ++i) {
            const ow_segment& g = segs[i];
            const uint32_t n = harmonics::check_segment(g, i, n_rows, stride);
            hs[i].row = g.row; hs[i].start = g.start; hs[i].n = n; hs[i].n_harm = g.n_harmonics; hs[i].xw_off = off;
            off += n;
            const uint64_t nfft = 4ull * n, nb = nfft / 2 + 1;
            const double val = 1.0 / ((double)nfft * (1.0 / sr));        // np.fft.rfftfreq(nfft, d = 1 / sr)
            for (uint32_t h = 0; h < g.n_harmonics; ++h) {
                owdev::OwBandDev b;
                b.seg = (uint32_t)i; b.k_lo = 1; b.k_hi = 0; b.pad = 0;
                const double nf = ((double)h + 1.5) * g.f0;
                if (!(nf >= sr / 2 - 100)) feat_band_bins(val, nb, nf * 0.99, nf * 1.01, b.k_lo, b.k_hi);
                if (b.k_lo <= b.k_hi && b.k_hi - b.k_lo + 1 > OW_NOISE_MAX_BAND_BINS)
                    throw std::runtime_error("segment " + std::to_string(i) + ": the band of harmonic " + std::to_string(h + 1) + " holds " +
                                             std::to_string(b.k_hi - b.k_lo + 1) + " bins, more than OW_NOISE_MAX_BAND_BINS (" +
                                             std::to_string(OW_NOISE_MAX_BAND_BINS) + ")");
                hb.push_back(b);
            }
        }
        std::vector<double> med(hb.size());
        if (!hb.empty()) {
            HIP_OK(hipSetDevice(cfg->device));
            StreamOwner so;
            so.create();
            hipStream_t st = so.s;
            DevMem own_audio, m_xw, m_ss, m_segs, m_bands, m_med;   // released on every exit path
            const double* d_audio = harmonics::device_audio(audio, n_rows, stride, cfg->audio_is_device, own_audio, st);
            m_xw.alloc(sizeof(double) * off);
            m_ss.alloc(sizeof(double) * n_segs);
            m_segs.alloc(sizeof(owdev::OwSegDev) * n_segs);
            m_bands.alloc(sizeof(owdev::OwBandDev) * hb.size());
            m_med.alloc(sizeof(double) * hb.size());
            HIP_OK(hipMemcpyAsync(m_segs.p, hs.data(), sizeof(owdev::OwSegDev) * n_segs, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(m_bands.p, hb.data(), sizeof(owdev::OwBandDev) * hb.size(), hipMemcpyHostToDevice, st));
            owdev::k_feat_window<<<dim3((unsigned)n_segs), dim3(256), 0, st>>>(d_audio, stride, m_segs.as<owdev::OwSegDev>(), m_xw.as<double>(),
                                                                             m_ss.as<double>(), cfg->wav24_mode);
            HIP_OK(hipGetLastError());
            owdev::k_feat_band_median<<<dim3((unsigned)hb.size()), dim3(256), 0, st>>>(m_segs.as<owdev::OwSegDev>(), m_bands.as<owdev::OwBandDev>(),
                                                                                      m_xw.as<double>(), m_med.as<double>());
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(med.data(), m_med.p, sizeof(double) * hb.size(), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
        }
        size_t bi = 0;
        for (size_t i = 0; i < n_segs; ++i)
            for (uint32_t h = 0; h < OW_MAX_HARMONICS; ++h) {
                double v = 0.0;
                if (h < segs[i].n_harmonics) {
                    v = hb[bi].k_lo <= hb[bi].k_hi ? std::max(med[bi], 1e-20) : 1e-20;   // max(np.median(...), 1e-20)
                    ++bi;
                }
                noise[i * OW_MAX_HARMONICS + h] = v;
            }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_interharmonic_noise: ") + ex.what()); return -1; }
}
}  // extern "C"
