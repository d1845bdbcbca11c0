// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: recorded-note intake, stages 1 and 2 of the ML loop --
// ow_isolation_score (ml/score_isolation.py:36-167: k_isolation_score walks the pairs, the host builds the collision table, lays the
// targets out one wavefront per 64 notes of a file and turns masks into collision scores), ow_isolation_collision_table
// (harmonic_collision_check, :69-102, for every pair of MIDI numbers) and ow_clip_bounds (ml/extract_notes.py:43-64: k_clip_bounds).
namespace {
namespace isolation {
// harmonic_collision_check(target, [other]) for all 128 x 128 pairs: bit h of table[target * 128 + other] is set while harmonic h + 1 of
// the target is clean.  IEEE multiply, divide, max, min and compare on the caller's frequencies: the reference's bits.
void iso_collision_table(const double* freq, double ratio_limit, uint8_t* table) {
    for (int t = 0; t < 128; ++t)
        for (int o = 0; o < 128; ++o) {
            uint8_t m = 0;
            for (int ht = 0; ht < 8; ++ht) {
                const double fh = freq[t] * (double)(ht + 1);
                bool clean = true;
                for (int ho = 0; ho < 8 && clean; ++ho) {
                    const double fo = freq[o] * (double)(ho + 1);
                    const double hi = fo > fh ? fo : fh, lo = fo < fh ? fo : fh;         // max(fh, fh_other), min(fh, fh_other)
                    const double ratio = hi / (1e-6 > lo ? 1e-6 : lo);
                    if (ratio < ratio_limit) clean = false;
                }
                if (clean) m |= (uint8_t)(1u << ht);
            }
            table[t * 128 + o] = m;
        }
}
void check_tables(const double* freq, double ratio_limit) {
    if (!freq) throw std::runtime_error("null argument");
    for (int i = 0; i < 128; ++i) check_finite("midi_freq[" + std::to_string(i) + "]: ", "value", freq[i]);
    check_finite("", "collision_ratio", ratio_limit);
}
}  // namespace isolation
}  // namespace

extern "C" {
int ow_isolation_collision_table(const double* midi_freq, double collision_ratio, uint8_t* table) {
    try {
        if (!table) throw std::runtime_error("null argument");
        isolation::check_tables(midi_freq, collision_ratio);
        isolation::iso_collision_table(midi_freq, collision_ratio, table);
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_isolation_collision_table: ") + ex.what()); return -1; }
}

int ow_isolation_score(const ow_iso_note* notes, size_t n_notes, const uint64_t* file_first, size_t n_files, const ow_iso_cfg* cfg,
                       double* temporal, double* collision, double* dominance, uint8_t* mask) {
    static_assert(sizeof(owdev::OwIsoNoteDev) == 64, "one record is two 32-byte scalar requests");
    try {
        if (!cfg) throw std::runtime_error("null argument");
        if (cfg->struct_size != sizeof(ow_iso_cfg) || cfg->note_size != sizeof(ow_iso_note))
            throw std::runtime_error(abi_mismatch("ow_iso_cfg.struct_size / note_size do"));
        if (cfg->kernel_ms_out) *cfg->kernel_ms_out = 0.0;
        if (n_notes == 0) return 0;
        if (!notes || !file_first || !temporal || !collision || !dominance || !mask || !cfg->decay_rate) throw std::runtime_error("null argument");
        isolation::check_tables(cfg->midi_freq, cfg->collision_ratio);
        for (int i = 0; i < 128; ++i) check_finite("decay_rate[" + std::to_string(i) + "]: ", "value", cfg->decay_rate[i]);
        if (n_notes > (size_t)1 << 30) throw std::runtime_error("more than 2^30 notes in one call");
        if (n_files == 0 || file_first[0] != 0 || file_first[n_files] != n_notes) throw std::runtime_error("file ranges do not cover the notes: file_first[0] must be 0 and file_first[n_files] n_notes");
        for (size_t f = 0; f < n_files; ++f)
            if (file_first[f + 1] < file_first[f] || file_first[f + 1] > n_notes) throw std::runtime_error("file " + std::to_string(f) + ": range is not ascending");
        std::vector<owdev::OwIsoNoteDev> hn(n_notes);
        for (size_t i = 0; i < n_notes; ++i) {
            const ow_iso_note& s = notes[i];
            const std::string at = "note " + std::to_string(i) + ": ";
            if (s.midi_note < 0 || s.midi_note > 127) throw std::runtime_error(at + "midi_note outside 0..127");
            check_finite(at, "onset_s", s.onset_s); check_finite(at, "offset_s", s.offset_s); check_finite(at, "amplitude", s.amplitude);
            check_finite(at, "window_start", s.window_start); check_finite(at, "window_end", s.window_end);
            owdev::OwIsoNoteDev& d = hn[i];
            d.onset = s.onset_s; d.offset = s.offset_s; d.amp = s.amplitude; d.rate = cfg->decay_rate[s.midi_note];
            d.ws = s.window_start; d.we = s.window_end; d.key = s.id_key; d.midi = s.midi_note; d.score = s.score != 0;
            temporal[i] = 0.0; collision[i] = 0.0; dominance[i] = 0.0; mask[i] = 0;
        }
        std::vector<owdev::OwIsoWaveDev> hw;                  // a file's targets start on a wavefront boundary: no wavefront mixes files
        for (size_t f = 0; f < n_files; ++f)
            for (uint64_t b = file_first[f]; b < file_first[f + 1]; b += 64) {
                bool any = false;
                for (uint64_t i = b; i < std::min<uint64_t>(b + 64, file_first[f + 1]); ++i) any = any || hn[i].score;
                if (any) hw.push_back(owdev::OwIsoWaveDev{(uint32_t)file_first[f], (uint32_t)file_first[f + 1], (uint32_t)b, 0});
            }
        if (hw.empty()) return 0;
        std::vector<uint8_t> by_target(128 * 128), by_other(128 * 128);
        isolation::iso_collision_table(cfg->midi_freq, cfg->collision_ratio, by_target.data());
        for (int t = 0; t < 128; ++t)
            for (int o = 0; o < 128; ++o) by_other[o * 128 + t] = by_target[t * 128 + o];
        HIP_OK(hipSetDevice(cfg->device));
        StreamOwner so;
        so.create();
        hipStream_t st = so.s;
        DevMem m_notes, m_waves, m_table, m_temp, m_dom, m_mask;   // released on every exit path
        Event ev0, ev1;
        m_notes.alloc(sizeof(owdev::OwIsoNoteDev) * n_notes);
        m_waves.alloc(sizeof(owdev::OwIsoWaveDev) * hw.size());
        m_table.alloc(by_other.size());
        m_temp.alloc(sizeof(double) * n_notes); m_dom.alloc(sizeof(double) * n_notes); m_mask.alloc(n_notes);
        HIP_OK(hipMemcpyAsync(m_notes.p, hn.data(), sizeof(owdev::OwIsoNoteDev) * n_notes, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_waves.p, hw.data(), sizeof(owdev::OwIsoWaveDev) * hw.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_table.p, by_other.data(), by_other.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(m_temp.p, 0, sizeof(double) * n_notes, st));
        HIP_OK(hipMemsetAsync(m_dom.p, 0, sizeof(double) * n_notes, st));
        HIP_OK(hipMemsetAsync(m_mask.p, 0, n_notes, st));
        if (cfg->kernel_ms_out) { ev0.create(hipEventDefault); ev1.create(hipEventDefault); HIP_OK(hipEventRecord(ev0.e, st)); }
        owdev::k_isolation_score<<<dim3((unsigned)hw.size()), dim3(64), 0, st>>>(m_notes.as<owdev::OwIsoNoteDev>(), m_waves.as<owdev::OwIsoWaveDev>(),
                                                                               m_table.as<uint8_t>(), m_temp.as<double>(), m_dom.as<double>(),
                                                                               m_mask.as<uint8_t>());
        HIP_OK(hipGetLastError());
        if (cfg->kernel_ms_out) HIP_OK(hipEventRecord(ev1.e, st));
        HIP_OK(hipMemcpyAsync(temporal, m_temp.p, sizeof(double) * n_notes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(dominance, m_dom.p, sizeof(double) * n_notes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(mask, m_mask.p, n_notes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (cfg->kernel_ms_out) {
            float ms = 0.0f;
            HIP_OK(hipEventElapsedTime(&ms, ev0.e, ev1.e));
            *cfg->kernel_ms_out = (double)ms;
        }
        for (size_t i = 0; i < n_notes; ++i) {
            if (!hn[i].score) continue;
            double clean = 0.0;                               // np.sum(weights[harmonic_mask]) / np.sum(weights): small integers, exact
            for (int h = 0; h < 8; ++h)
                if (mask[i] >> h & 1) clean += h < 4 ? 2.0 : 1.0;
            collision[i] = clean / 12.0;
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_isolation_score: ") + ex.what()); return -1; }
}

int ow_clip_bounds(const double* clips, size_t n_clips, size_t stride, const uint32_t* lengths, double onset_frac, double offset_frac, int device,
                   double* peak, int64_t* first, int64_t* last) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the kernel's index type is the header's");
    try {
        if (n_clips == 0) return 0;
        if (!clips || !lengths || !peak || !first || !last) throw std::runtime_error("null argument");
        check_finite("", "onset_frac", onset_frac); check_finite("", "offset_frac", offset_frac);
        if (stride == 0 || n_clips > (size_t)INT32_MAX) throw std::runtime_error("stride of 0 or more than 2^31 - 1 clips");
        for (size_t c = 0; c < n_clips; ++c)
            if (lengths[c] > stride) throw std::runtime_error("clip " + std::to_string(c) + ": length " + std::to_string(lengths[c]) + " exceeds the stride " + std::to_string(stride));
        HIP_OK(hipSetDevice(device));
        StreamOwner so;
        so.create();
        hipStream_t st = so.s;
        DevMem m_x, m_len, m_peak, m_first, m_last;           // released on every exit path
        m_x.alloc(sizeof(double) * n_clips * stride);
        m_len.alloc(sizeof(uint32_t) * n_clips);
        m_peak.alloc(sizeof(double) * n_clips); m_first.alloc(sizeof(int64_t) * n_clips); m_last.alloc(sizeof(int64_t) * n_clips);
        HIP_OK(hipMemcpyAsync(m_x.p, clips, sizeof(double) * n_clips * stride, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_len.p, lengths, sizeof(uint32_t) * n_clips, hipMemcpyHostToDevice, st));
        owdev::k_clip_bounds<<<dim3((unsigned)n_clips), dim3(OW_CLIP_THREADS), 0, st>>>(m_x.as<double>(), stride, m_len.as<uint32_t>(), onset_frac, offset_frac,
                                                                                      m_peak.as<double>(), m_first.as<long long>(), m_last.as<long long>());
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(peak, m_peak.p, sizeof(double) * n_clips, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(first, m_first.p, sizeof(int64_t) * n_clips, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(last, m_last.p, sizeof(int64_t) * n_clips, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_clip_bounds: ") + ex.what()); return -1; }
}
}  // extern "C"
