// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the analysis of tools/wurli_compare.py for many clips
// per call -- ow_stft_profile (compute_stft :46-58 with what harmonic_profile :61-78 and measure_spectral_centroid :122-127 take from S)
// and ow_frame_rms (the RMS envelopes of measure_decay :95-107 and measure_attack_time :136-147, the sum of measure_rms :130-133).
namespace {
namespace compare {
// Device memory of one chunk of clips besides what the caller holds: the clips' rows when they come from the host, the per-frame
// magnitudes (ow_stft_profile with mean_mag) or the RMS rows (ow_frame_rms).  A clip that alone needs more is refused.
const size_t BUDGET_BYTES = size_t(1) << 30;

void check_mode(int wav24_mode) {
    if (wav24_mode != OW_WAV_NONE && wav24_mode != OW_WAV_ROUND && wav24_mode != OW_WAV_TRUNCATE) throw std::runtime_error("unknown wav24_mode");
}
// n_frames = max(1, (len - n) // hop + 1) with Python's floor: a clip shorter than the frame has the one zero-padded frame
inline uint32_t frame_count(uint32_t len, uint32_t n, uint32_t hop) { return len >= n ? (len - n) / hop + 1 : 1; }

void check_lengths(const uint32_t* lengths, size_t n_clips, size_t stride) {
    for (size_t c = 0; c < n_clips; ++c)
        if (lengths[c] > stride)
            throw std::runtime_error("clip " + std::to_string(c) + ": length " + std::to_string(lengths[c]) + " beyond the stride of " + std::to_string(stride) + " samples");
}
// the clips [c0, c0 + cn) on the device: the caller's rows, or a copy that `own` holds (rebased so that clip c is row c)
const double* chunk_rows(const double* clips, size_t stride, size_t c0, size_t cn, int clips_is_device, DevMem& own, hipStream_t st) {
    if (clips_is_device) return clips;
    HIP_OK(hipMemcpyAsync(own.p, clips + c0 * stride, sizeof(double) * cn * stride, hipMemcpyHostToDevice, st));
    return own.as<double>() - c0 * stride;
}
// how many clips from c0 on fit the budget at cost(c) bytes each (at most 65 535: one grid row per clip); throws if the first does not
template <class Cost> size_t chunk_from(size_t c0, size_t n_clips, Cost cost) {
    size_t used = 0, cn = 0;
    while (c0 + cn < n_clips && cn < 65535) {
        const size_t b = cost(c0 + cn);
        if (used + b > BUDGET_BYTES) break;
        used += b; ++cn;
    }
    if (cn == 0) throw std::runtime_error("clip " + std::to_string(c0) + " alone needs more than the " + std::to_string(BUDGET_BYTES >> 20) + " MiB of device memory a chunk may take");
    return cn;
}
}  // namespace compare
}  // namespace

extern "C" {
int ow_stft_profile(const double* clips, size_t n_clips, size_t stride, const uint32_t* lengths, const double* window, uint32_t n_fft, uint32_t hop,
                    double sample_rate, int wav24_mode, int device, int clips_is_device, double* mean_mag, double* centroid) {
    try {
        if (n_fft < owdev::STFT_MIN_FFT || n_fft > owdev::STFT_MAX_FFT || (n_fft & (n_fft - 1)) != 0)
            throw std::runtime_error("n_fft of " + std::to_string(n_fft) + " is not a power of two in " + std::to_string(owdev::STFT_MIN_FFT) + ".." + std::to_string(owdev::STFT_MAX_FFT));
        if (hop == 0) throw std::runtime_error("hop is 0: the reference's frame loop would never end");
        compare::check_mode(wav24_mode);
        check_positive_finite("", "sample_rate", sample_rate);
        if (n_clips == 0) return 0;
        if (!clips || !lengths || !window || (!mean_mag && !centroid)) throw std::runtime_error("null argument");
        if (n_clips > 0x7fffffffull) throw std::runtime_error("too many clips");
        compare::check_lengths(lengths, n_clips, stride);
        const uint32_t M = n_fft / 2;
        uint32_t log2_m = 0;
        while ((1u << log2_m) < M) ++log2_m;
        std::vector<uint32_t> nf(n_clips);
        for (size_t c = 0; c < n_clips; ++c) nf[c] = compare::frame_count(lengths[c], n_fft, hop);
        const size_t row_bytes = clips_is_device ? 0 : sizeof(double) * stride;
        const size_t frame_bytes = sizeof(double) * ((mean_mag ? (size_t)M + 1 : 0) + 1);
        require_device(device);
        StreamOwner so;
        so.create();
        hipStream_t st = so.s;
        DevMem m_rows, m_len, m_nf, m_off, m_win, m_tw, m_mags, m_cent, m_mean, m_centroid;   // released on every exit path
        m_len.alloc(sizeof(uint32_t) * n_clips);
        m_nf.alloc(sizeof(uint32_t) * n_clips);
        m_off.alloc(sizeof(uint64_t) * n_clips);
        m_win.alloc(sizeof(double) * n_fft);
        m_tw.alloc(sizeof(double2) * (M + 1));
        if (mean_mag) m_mean.alloc(sizeof(double) * n_clips * (M + 1));
        if (centroid) m_centroid.alloc(sizeof(double) * n_clips);
        HIP_OK(hipMemcpyAsync(m_len.p, lengths, sizeof(uint32_t) * n_clips, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_nf.p, nf.data(), sizeof(uint32_t) * n_clips, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_win.p, window, sizeof(double) * n_fft, hipMemcpyHostToDevice, st));
        owdev::k_stft_twiddles<<<dim3((M + 1 + 255) / 256), dim3(256), 0, st>>>(m_tw.as<double2>(), n_fft);
        HIP_OK(hipGetLastError());
        const size_t lds = owdev::stft_lds_bytes(n_fft);
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(owdev::k_stft_frames), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const unsigned threads = std::min(256u, std::max(64u, M / 4));
        std::vector<uint64_t> off(n_clips);
        owdev::OwStftGrid g;
        g.n_fft = n_fft; g.log2_m = log2_m; g.hop = hop; g.clip0 = 0; g.wav24_mode = wav24_mode; g.want_mag = mean_mag ? 1 : 0;
        g.freq_val = 1.0 / ((double)n_fft * (1.0 / sample_rate));            // np.fft.rfftfreq(n_fft, 1.0 / sr)
        size_t rows_cap = 0, frames_cap = 0;
        for (size_t c0 = 0; c0 < n_clips;) {
            const size_t cn = compare::chunk_from(c0, n_clips, [&](size_t c) { return row_bytes + frame_bytes * nf[c]; });
            uint64_t frames = 0;
            uint32_t most = 0;
            for (size_t c = c0; c < c0 + cn; ++c) { off[c] = frames; frames += nf[c]; most = std::max(most, nf[c]); }
            if (!clips_is_device && cn > rows_cap) { m_rows.alloc(sizeof(double) * cn * stride); rows_cap = cn; }
            if (frames > frames_cap) {
                if (mean_mag) m_mags.alloc(sizeof(double) * frames * (M + 1));
                m_cent.alloc(sizeof(double) * frames);
                frames_cap = frames;
            }
            HIP_OK(hipMemcpyAsync(m_off.as<uint64_t>() + c0, off.data() + c0, sizeof(uint64_t) * cn, hipMemcpyHostToDevice, st));
            const double* d_rows = compare::chunk_rows(clips, stride, c0, cn, clips_is_device, m_rows, st);
            g.clip0 = (uint32_t)c0;
            owdev::k_stft_frames<<<dim3(most, (unsigned)cn), dim3(threads), lds, st>>>(d_rows, stride, m_len.as<uint32_t>(), m_nf.as<uint32_t>(), m_off.as<uint64_t>(),
                                                                                      m_win.as<double>(), m_tw.as<double2>(), g, mean_mag ? m_mags.as<double>() : nullptr,
                                                                                      m_cent.as<double>());
            HIP_OK(hipGetLastError());
            owdev::k_stft_reduce<<<dim3((M + 2 + 255) / 256, (unsigned)cn), dim3(256), 0, st>>>(m_mags.as<double>(), m_cent.as<double>(), m_nf.as<uint32_t>(), m_off.as<uint64_t>(),
                                                                                               (uint32_t)c0, M, m_mean.as<double>(), m_centroid.as<double>());
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(st));               // the chunk's buffers are reused by the next one
            c0 += cn;
        }
        if (mean_mag) HIP_OK(hipMemcpyAsync(mean_mag, m_mean.p, sizeof(double) * n_clips * (M + 1), hipMemcpyDeviceToHost, st));
        if (centroid) HIP_OK(hipMemcpyAsync(centroid, m_centroid.p, sizeof(double) * n_clips, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_stft_profile: ") + ex.what()); return -1; }
}

int ow_frame_rms(const double* clips, size_t n_clips, size_t stride, const uint32_t* lengths, uint32_t frame_len, uint32_t hop, int wav24_mode,
                 int device, int clips_is_device, double* rms, size_t frames_stride, uint32_t* n_frames, double* sum_sq) {
    try {
        if (frame_len == 0) throw std::runtime_error("frame_len is 0");
        if (hop == 0) throw std::runtime_error("hop is 0: the reference's frame loop would never end");
        compare::check_mode(wav24_mode);
        if (n_clips == 0) return 0;
        if (!clips || !lengths || !rms || !n_frames) throw std::runtime_error("null argument");
        if (n_clips > 0x7fffffffull) throw std::runtime_error("too many clips");
        compare::check_lengths(lengths, n_clips, stride);
        std::vector<uint32_t> nf(n_clips);
        for (size_t c = 0; c < n_clips; ++c) {
            nf[c] = compare::frame_count(lengths[c], frame_len, hop);
            if (nf[c] > frames_stride)
                throw std::runtime_error("clip " + std::to_string(c) + ": frames_stride smaller than its " + std::to_string(nf[c]) + " frames");
        }
        const size_t clip_bytes = (clips_is_device ? 0 : sizeof(double) * stride) + sizeof(double) * frames_stride;
        require_device(device);
        StreamOwner so;
        so.create();
        hipStream_t st = so.s;
        DevMem m_rows, m_len, m_nf, m_rms, m_sum;           // released on every exit path
        m_len.alloc(sizeof(uint32_t) * n_clips);
        m_nf.alloc(sizeof(uint32_t) * n_clips);
        if (sum_sq) m_sum.alloc(sizeof(double) * n_clips);
        HIP_OK(hipMemcpyAsync(m_len.p, lengths, sizeof(uint32_t) * n_clips, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_nf.p, nf.data(), sizeof(uint32_t) * n_clips, hipMemcpyHostToDevice, st));
        size_t cap = 0;
        for (size_t c0 = 0; c0 < n_clips;) {
            const size_t cn = compare::chunk_from(c0, n_clips, [&](size_t) { return clip_bytes; });
            if (cn > cap) {
                if (!clips_is_device) m_rows.alloc(sizeof(double) * cn * stride);
                m_rms.alloc(sizeof(double) * cn * frames_stride);
                cap = cn;
            }
            uint32_t most = 0;
            for (size_t c = c0; c < c0 + cn; ++c) most = std::max(most, nf[c]);
            const double* d_rows = compare::chunk_rows(clips, stride, c0, cn, clips_is_device, m_rows, st);
            HIP_OK(hipMemsetAsync(m_rms.p, 0, sizeof(double) * cn * frames_stride, st));      // frames a clip does not have read 0.0
            owdev::k_frame_rms<<<dim3(most, (unsigned)cn), dim3(256), 0, st>>>(d_rows, stride, m_len.as<uint32_t>(), m_nf.as<uint32_t>(), (uint32_t)c0, frame_len, hop,
                                                                             wav24_mode, m_rms.as<double>(), frames_stride);
            HIP_OK(hipGetLastError());
            if (sum_sq) {
                owdev::k_clip_sum_sq<<<dim3((unsigned)cn), dim3(256), 0, st>>>(d_rows, stride, m_len.as<uint32_t>(), (uint32_t)c0, wav24_mode, m_sum.as<double>());
                HIP_OK(hipGetLastError());
            }
            HIP_OK(hipMemcpyAsync(rms + c0 * frames_stride, m_rms.p, sizeof(double) * cn * frames_stride, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));               // the chunk's buffers are reused by the next one
            c0 += cn;
        }
        if (sum_sq) HIP_OK(hipMemcpyAsync(sum_sq, m_sum.p, sizeof(double) * n_clips, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::memcpy(n_frames, nf.data(), sizeof(uint32_t) * n_clips);
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_frame_rms: ") + ex.what()); return -1; }
}
}  // extern "C"
