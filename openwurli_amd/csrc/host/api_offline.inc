// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: render_note, batch render, WAV writers, feature stage.
extern "C" {
// ---- offline ------------------------------------------------------------------------------------
static long long render_note_impl(uint8_t midi, double velocity, double dur_s, double sample_rate, int device, double* out, size_t cap, const double* ds);
long long ow_render_note(uint8_t midi, double velocity, double dur_s, double sample_rate, int device, double* out, size_t cap) {
    return render_note_impl(midi, velocity, dur_s, sample_rate, device, out, cap, nullptr);
}
long long ow_render_note_with_scale(uint8_t midi, double velocity, double dur_s, double sample_rate, double displacement_scale, int device,
                                    double* out, size_t cap) {
    return render_note_impl(midi, velocity, dur_s, sample_rate, device, out, cap, &displacement_scale);
}
double ow_normalize_scale(const double* samples, size_t n) {     // main.rs:505-511
    double peak = 0.0;
    for (size_t i = 0; samples && i < n; ++i) peak = std::fmax(peak, std::fabs(samples[i]));
    return peak > 0.7 ? 0.7 / peak : 1.0;
}
static long long render_note_impl(uint8_t midi, double velocity, double dur_s, double sample_rate, int device, double* out, size_t cap, const double* ds) {
    try {
        // a voices-only pool: no chain state, no Twin-T settle, and render_range launches the voice kernels alone
        std::unique_ptr<ow_pool> guard(pool_create(sample_rate, 1, device, OW_PREAMP_LEGACY8, OW_POWER_AMP_BEHAVIORAL, OW_TREMOLO_TWIN_T, true));
        ow_pool* p = guard.get();
        ow_engine* e = p->engines[0].get();
        // Voice::render_note: seed = midi * 2654435761, MLP off, no note clamping beyond the table range (voice.rs:206-207)
        const uint8_t note = std::min<uint8_t>(std::max<uint8_t>(midi, OW_MIDI_LO), OW_MIDI_HI);
        e->vm->has_voice |= 1ull; e->set_state(0, OW_VOICE_HELD); e->vm->midi_of[0] = note;
        e->sync_masks(0);
        push_op(e, OP_NOTE_ON, 0, note, false, (uint32_t)midi * 2654435761u, velocity);
        if (ds) push_op(e, OP_SET_DS, 0, note, false, 0, *ds);      // voice.set_displacement_scale(scale) right after note_on (voice.rs:210-212)
        const size_t n = rust_as_usize(dur_s * sample_rate);
        const size_t chunk_len = p->Lcap;            // OW_MAX_BLOCK for a pool of one: few launches, few synchronisations
        std::vector<double> chunk(chunk_len);
        size_t done = 0;
        while (done < n) {
            const size_t len = std::min<size_t>(chunk_len, n - done);
            render_range(p, 0, 1, len, true);
            HIP_OK(hipStreamSynchronize(p->stream));
            // no cleanup_voices here: render_note keeps rendering the voice for the whole duration; only the kernel choice of the
            // next chunk follows the device status (onset ramp / attack noise still running -> general kernel again)
            {
                const uint8_t tr = p->h_eout[0].transient != 0u;
                if (p->h_eout[0].transient == 2u) throw std::runtime_error("voice dispatch: a voice in a transient phase was sent to the steady kernel");
                if (tr != p->transient[0]) { p->transient[0] = tr; p->lists_valid = false; }
            }
            if (ow_pool_read_voice_sum(p, chunk.data(), len, len) != 0) throw std::runtime_error(g_err);
            for (size_t i = 0; i < len && done + i < cap; ++i) out[done + i] = chunk[i];
            done += len;
        }
        return (long long)n;      // the note's length; min(n, cap) samples were written (header contract)
    } catch (const std::exception& ex) { set_err(std::string("ow_render_note: ") + ex.what()); return -1; }
}

// The batch render behind ow_batch_render and its two siblings with corrections given at run time (api_mlp.inc).  fill_corr empty:
// every job's note-on infers its own corrections from the built-in constants (ow_batch_render, the launches it always made).
// Otherwise the voices read job j's corrections from a device table of n_jobs entries, which fill_corr fills on the call's stream.
using FillCorr = std::function<void(OfflineCall&, owdev::MlpOut*)>;
static long long batch_render_impl(const char* who, const ow_job* jobs, size_t n_jobs, const ow_batch_cfg* cfg, double* out, size_t stride, int out_is_device,
                                   const FillCorr& fill_corr) {
    try {
        if (!jobs || !cfg || !out || n_jobs == 0) throw std::runtime_error("null argument");
        if (cfg->struct_size != sizeof(ow_batch_cfg) || cfg->job_size != sizeof(ow_job)) throw std::runtime_error(abi_mismatch("ow_batch_cfg.struct_size / job_size do"));
        require_known_kinds(cfg->preamp_kind);                                    // (power_amp_kind: by run_job_chain)
        const size_t n = rust_as_usize(cfg->duration_s * cfg->sample_rate);       // (duration * sample_rate) as usize, main.rs:411
        if (n == 0) return 0;
        if (stride < n) throw std::runtime_error("stride smaller than the job length");
        OfflineCall call(cfg->device, cfg->sample_rate, cfg->preamp_kind, /*note_table=*/true);
        std::vector<owdev::OwJobDev> hj(n_jobs);
        for (size_t i = 0; i < n_jobs; ++i) {
            hj[i].note = jobs[i].note; hj[i].velocity = jobs[i].velocity; hj[i].mlp = jobs[i].mlp; hj[i].poweramp = jobs[i].poweramp;
            hj[i].no_preamp = jobs[i].no_preamp ? 1 : 0; hj[i].no_attack_noise = jobs[i].no_attack_noise ? 1 : 0;
            hj[i].has_ds = jobs[i].has_displacement_scale ? 1 : 0; hj[i].dc_at_ldr = 0;
            hj[i].volume = jobs[i].volume; hj[i].speaker = jobs[i].speaker; hj[i].r_ldr = jobs[i].r_ldr;
            hj[i].tremolo_depth = jobs[i].tremolo_depth; hj[i].displacement_scale = jobs[i].displacement_scale;
        }
        const size_t vblocks = (n_jobs + 63) / 64;
        hipStream_t st = call.st();
        DevMem m_vrec, m_jobs, m_reed, m_out;              // released on every exit path
        m_vrec.alloc(sizeof(double) * vblocks * OW_VREC_DOUBLES);
        m_jobs.alloc(sizeof(owdev::OwJobDev) * n_jobs);
        m_reed.alloc(sizeof(double) * n_jobs * stride);      // same row stride as the output: the chain kernels index both with it
        if (!out_is_device) m_out.alloc(sizeof(double) * n_jobs * stride);
        const OwConsts* dK = call.dK(); const double* d_nt = call.nt(); double* d_vrec = m_vrec.as<double>();
        owdev::OwJobDev* d_jobs = m_jobs.as<owdev::OwJobDev>(); double* d_reed = m_reed.as<double>();
        double* d_out = out_is_device ? out : m_out.as<double>();
        HIP_OK(hipMemcpyAsync(d_jobs, hj.data(), sizeof(owdev::OwJobDev) * n_jobs, hipMemcpyHostToDevice, st));
        DevMem m_corr;
        const owdev::MlpOut* d_corr = nullptr;
        if (fill_corr) {
            m_corr.alloc(sizeof(owdev::MlpOut) * n_jobs);
            fill_corr(call, m_corr.as<owdev::MlpOut>());
            d_corr = m_corr.as<owdev::MlpOut>();
        }
        const JobChainCfg cc{cfg->sample_rate, cfg->device, cfg->preamp_kind, cfg->power_amp_kind, cfg->no_rail_sag};
        // Voices and chain side by side when the chain is the plain legacy one and leaves room on the chip: a job's run time is serial
        // latency in both kernels, so the 13 % the voices take are hidden behind the chain instead of in front of it.
        const bool overlap = job_chain_is_plain_legacy(cc, hj) && job_voice_overlap(call.sw, n_jobs);
        DevMem m_prog;
        StreamOwner so2;
        Event ev_ready, ev_voice;
        int* d_prog = nullptr;
        if (overlap) {
            m_prog.alloc(sizeof(int) * (vblocks + 1));                 // progress of every voice block + the chain's "gave up waiting" flag
            d_prog = m_prog.as<int>();
            HIP_OK(hipMemsetAsync(d_prog, 0, sizeof(int) * (vblocks + 1), st));
            so2.create(); ev_ready.create(); ev_voice.create();
            HIP_OK(hipEventRecord(ev_ready, st));
            HIP_OK(hipStreamWaitEvent(so2.s, ev_ready, 0));
            owdev::k_job_voice<<<dim3((unsigned)vblocks), dim3(64), 0, so2.s>>>(dK, d_nt, d_vrec, d_jobs, d_reed, (int)n_jobs, (long long)n, (long long)stride, d_prog, d_corr);
            HIP_OK(hipGetLastError());
            HIP_OK(hipEventRecord(ev_voice, so2.s));
        } else {
            owdev::k_job_voice<<<dim3((unsigned)vblocks), dim3(64), 0, st>>>(dK, d_nt, d_vrec, d_jobs, d_reed, (int)n_jobs, (long long)n, (long long)stride, nullptr, d_corr);
            HIP_OK(hipGetLastError());
        }
        run_job_chain(call, cc, hj, d_jobs, d_reed, d_out, n_jobs, (long long)n, (long long)stride, d_prog);
        if (overlap) {
            HIP_OK(hipStreamWaitEvent(st, ev_voice, 0));
            int gave_up = 0;
            HIP_OK(hipMemcpyAsync(&gave_up, d_prog + vblocks, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            if (gave_up) run_job_chain(call, cc, hj, d_jobs, d_reed, d_out, n_jobs, (long long)n, (long long)stride);   // the voices are complete now
        }
        if (!out_is_device) HIP_OK(hipMemcpyAsync(out, d_out, sizeof(double) * n_jobs * stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return (long long)n;
    } catch (const std::exception& ex) { set_err(std::string(who) + ": " + ex.what()); return -1; }
}
long long ow_batch_render(const ow_job* jobs, size_t n_jobs, const ow_batch_cfg* cfg, double* out, size_t stride, int out_is_device) {
    return batch_render_impl("ow_batch_render", jobs, n_jobs, cfg, out, stride, out_is_device, FillCorr());
}

void* ow_device_alloc(size_t bytes, int device) {
    void* ptr = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&ptr, bytes ? bytes : 1) != hipSuccess) { set_err("ow_device_alloc: hipMalloc failed"); return nullptr; }
    return ptr;
}
void ow_device_free(void* ptr, int device) {
    if (ptr && hipSetDevice(device) == hipSuccess) hipFree(ptr);
}

void* ow_host_alloc(size_t bytes, int device) {
    void* ptr = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipHostMalloc(&ptr, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { set_err("ow_host_alloc: hipHostMalloc failed"); return nullptr; }
    void* dptr = nullptr;
    if (hipHostGetDevicePointer(&dptr, ptr, 0) != hipSuccess) dptr = nullptr;
    try { host_block_register(ptr, bytes ? bytes : 1, dptr); } catch (...) {}
    return ptr;
}
void ow_host_free(void* ptr, int device) {
    if (!ptr) return;
    host_block_forget(ptr);
    if (hipSetDevice(device) == hipSuccess) hipHostFree(ptr);
}

// ---- ML-pipeline stage after the batch render ---------------------------------------------------------------
int ow_wav24_quantize(const double* samples, size_t n, double scale, int mode, int32_t* out) {
    if ((!samples || !out) && n) { set_err("ow_wav24_quantize: null argument"); return -1; }
    if (mode != OW_WAV_ROUND && mode != OW_WAV_TRUNCATE) { set_err("ow_wav24_quantize: unknown mode"); return -1; }
    const double mx = 8388607.0;
    for (size_t i = 0; i < n; ++i) {
        double v;
        if (mode == OW_WAV_ROUND) {          // main.rs:951-954: round half away from zero, saturating cast, clamp
            v = std::round(samples[i] * scale * mx);
        } else {                             // reed-renderer main.rs:119-123: clamp to +-1, scale, truncate toward zero
            const double c = samples[i] < -1.0 ? -1.0 : (samples[i] > 1.0 ? 1.0 : samples[i]);
            v = std::trunc(c * mx);
        }
        if (!(v == v)) v = 0.0;              // Rust `as i32`: NaN -> 0
        out[i] = (int32_t)(v < -mx ? -mx : (v > mx ? mx : v));
    }
    return 0;
}

int ow_wav24_write(const char* path, const double* samples, size_t n, uint32_t sample_rate, double scale, int mode) {
    if (!path || (!samples && n)) { set_err("ow_wav24_write: null argument"); return -1; }
    std::vector<int32_t> q(n);
    if (ow_wav24_quantize(samples, n, scale, mode, q.data()) != 0) return -1;
    const uint32_t data_bytes = (uint32_t)(n * 3);
    std::vector<uint8_t> buf;
    buf.reserve(68 + data_bytes + 1);
    auto u16 = [&](uint32_t v) { buf.push_back((uint8_t)v); buf.push_back((uint8_t)(v >> 8)); };
    auto u32 = [&](uint32_t v) { u16(v & 0xFFFFu); u16(v >> 16); };
    auto tag = [&](const char* t) { buf.insert(buf.end(), t, t + 4); };
    tag("RIFF"); u32(4 + (8 + 40) + (8 + data_bytes + (data_bytes & 1))); tag("WAVE");
    tag("fmt "); u32(40);
    u16(0xFFFE);                 // WAVE_FORMAT_EXTENSIBLE
    u16(1);                      // channels
    u32(sample_rate);
    u32(sample_rate * 3);        // bytes per second
    u16(3);                      // block align
    u16(24);                     // bits per sample (container)
    u16(22);                     // cbSize
    u16(24);                     // valid bits
    u32(0x4);                    // channel mask: front centre
    static const uint8_t pcm_guid[16] = {0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
    buf.insert(buf.end(), pcm_guid, pcm_guid + 16);
    tag("data"); u32(data_bytes);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t v = (uint32_t)q[i];
        buf.push_back((uint8_t)v); buf.push_back((uint8_t)(v >> 8)); buf.push_back((uint8_t)(v >> 16));
    }
    if (data_bytes & 1) buf.push_back(0);
    FILE* f = std::fopen(path, "wb");
    if (!f) { set_err(std::string("ow_wav24_write: cannot open ") + path); return -2; }
    const bool ok = std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (std::fclose(f) != 0 || !ok) { set_err(std::string("ow_wav24_write: short write to ") + path); return -3; }
    return 0;
}

int ow_extract_harmonics(const double* audio, size_t n_rows, size_t stride, double sample_rate, const ow_segment* segs, size_t n_segs,
                         double search_pct, int wav24_mode, int device, int audio_is_device, double* amps, double* freqs, double* rms) {
    try {
        if (!audio || !segs || !amps || !freqs) throw std::runtime_error("null argument");
        if (wav24_mode != OW_WAV_NONE && wav24_mode != OW_WAV_ROUND && wav24_mode != OW_WAV_TRUNCATE) throw std::runtime_error("unknown wav24_mode");
        if (!(sample_rate > 0.0) || !(search_pct >= 0.0)) throw std::runtime_error("invalid sample rate or search band");
        if (n_segs == 0) return 0;
        std::vector<owdev::OwSegDev> hs(n_segs);
        std::vector<owdev::OwBinsDev> hb;
        std::vector<double> vals(n_segs);
        uint64_t off = 0;
        for (size_t i = 0; i < n_segs; ++i) {
            const ow_segment& g = segs[i];
            if (g.row >= n_rows || g.end <= g.start || g.end > stride || g.n_harmonics > OW_MAX_HARMONICS)
                throw std::runtime_error("segment " + std::to_string(i) + " out of range");
            const uint32_t n = g.end - g.start;
            if (n > (1u << 22)) throw std::runtime_error("segment longer than 2^22 samples");
            hs[i].row = g.row; hs[i].start = g.start; hs[i].n = n; hs[i].n_harm = g.n_harmonics; hs[i].xw_off = off;
            off += n;
            // numpy's axis: rfftfreq(nfft, d = 1/sr) = arange(nfft/2 + 1) * (1 / (nfft * d)); mask = (axis >= f_lo) & (axis <= f_hi)
            const uint64_t nfft = 4ull * n, nb = nfft / 2 + 1;
            const double val = 1.0 / ((double)nfft * (1.0 / sample_rate));
            vals[i] = val;
            for (uint32_t h = 0; h < g.n_harmonics; ++h) {
                owdev::OwBinsDev b;
                b.seg = (uint32_t)i; b.k_lo = 1; b.k_hi = 0; b.pad = 0;
                const double fh = g.f0 * (double)(h + 1);
                if (!(fh >= sample_rate / 2 - 100)) {
                    const double f_lo = fh * (1.0 - search_pct), f_hi = fh * (1.0 + search_pct);
                    feat_band_bins(val, nb, f_lo, f_hi, b.k_lo, b.k_hi);
                }
                hb.push_back(b);
            }
        }
        HIP_OK(hipSetDevice(device));
        StreamOwner so;
        so.create();
        hipStream_t st = so.s;
        DevMem own_audio, m_xw, m_ss, m_segs, m_bins, m_peaks;   // released on every exit path
        const double* d_audio = audio;
        if (!audio_is_device) {
            own_audio.alloc(sizeof(double) * n_rows * stride);
            HIP_OK(hipMemcpyAsync(own_audio.p, audio, sizeof(double) * n_rows * stride, hipMemcpyHostToDevice, st));
            d_audio = own_audio.as<double>();
        }
        m_xw.alloc(sizeof(double) * std::max<uint64_t>(off, 1));
        m_ss.alloc(sizeof(double) * n_segs);
        m_segs.alloc(sizeof(owdev::OwSegDev) * n_segs);
        double* d_xw = m_xw.as<double>(); double* d_ss = m_ss.as<double>();
        owdev::OwSegDev* d_segs = m_segs.as<owdev::OwSegDev>();
        HIP_OK(hipMemcpyAsync(d_segs, hs.data(), sizeof(owdev::OwSegDev) * n_segs, hipMemcpyHostToDevice, st));
        owdev::k_feat_window<<<dim3((unsigned)n_segs), dim3(256), 0, st>>>(d_audio, stride, d_segs, d_xw, d_ss, wav24_mode);
        std::vector<owdev::OwPeakDev> peaks(hb.size());
        if (!hb.empty()) {
            m_bins.alloc(sizeof(owdev::OwBinsDev) * hb.size());
            m_peaks.alloc(sizeof(owdev::OwPeakDev) * hb.size());
            HIP_OK(hipMemcpyAsync(m_bins.p, hb.data(), sizeof(owdev::OwBinsDev) * hb.size(), hipMemcpyHostToDevice, st));
            owdev::k_feat_peaks<<<dim3((unsigned)hb.size()), dim3(256), 0, st>>>(d_segs, m_bins.as<owdev::OwBinsDev>(), d_xw, m_peaks.as<owdev::OwPeakDev>());
            HIP_OK(hipMemcpyAsync(peaks.data(), m_peaks.p, sizeof(owdev::OwPeakDev) * hb.size(), hipMemcpyDeviceToHost, st));
        }
        std::vector<double> ss(n_segs);
        HIP_OK(hipMemcpyAsync(ss.data(), d_ss, sizeof(double) * n_segs, hipMemcpyDeviceToHost, st));
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));
        size_t bi = 0;
        for (size_t i = 0; i < n_segs; ++i) {
            const double N = (double)hs[i].n;
            for (uint32_t h = 0; h < OW_MAX_HARMONICS; ++h) {
                double a = 0.0, f = 0.0;
                if (h < hs[i].n_harm) {
                    const owdev::OwBinsDev& b = hb[bi];
                    if (b.k_lo <= b.k_hi) {
                        a = std::hypot(peaks[bi].re, peaks[bi].im) * 2.0 / N / 0.5;   // np.abs(rfft) * 2.0 / N / 0.5
                        f = (double)peaks[bi].k * vals[i];
                    } else { a = 1e-20; f = segs[i].f0 * (double)(h + 1); }
                    ++bi;
                }
                amps[i * OW_MAX_HARMONICS + h] = a; freqs[i * OW_MAX_HARMONICS + h] = f;
            }
            if (rms) rms[i] = std::max(std::sqrt(ss[i] / N), 1e-20);
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_extract_harmonics: ") + ex.what()); return -1; }
}

}  // extern "C"
