// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: `preamp-bench render-poly`
// (tools/preamp-bench/src/main.rs:1397-1592), the chord intermodulation measurement, for many chords per call.
namespace {
namespace poly {
// device rows a chord takes: its n voice rows plus final, separate_sum, residual
inline size_t chord_rows(const ow_poly_chord& c) { return (size_t)c.n_notes + 3; }
const size_t BUDGET_BYTES = size_t(8) << 30;      // per chunk, as the calibration sweep's
}  // namespace poly
}  // namespace

extern "C" {
long long ow_render_poly(const ow_poly_chord* chords, size_t n_chords, const ow_poly_cfg* cfg, ow_poly_row* rows_out, double* final_out,
                         double* separate_sum_out, double* residual_out, size_t out_stride) {
    try {
        if (!cfg) throw std::runtime_error("null argument");
        if (cfg->struct_size != sizeof(ow_poly_cfg) || cfg->chord_size != sizeof(ow_poly_chord))
            throw std::runtime_error(abi_mismatch("ow_poly_cfg.struct_size / chord_size do"));
        require_legacy_chain(cfg->preamp_kind, cfg->power_amp_kind);
        const double sr = 44100.0;                                     // BASE_SR, main.rs:27
        // (duration * BASE_SR) as usize (main.rs:1422); the window slice [8820, min(88200, n)) panics in the reference unless n > 8820 (:1516-1520)
        const size_t nu = rust_as_usize(cfg->duration_s * sr);
        const long long n = nu < 2147483648ull ? (long long)nu : 0;
        if (n <= OW_POLY_WIN_LO)
            throw std::runtime_error("duration_s must give more than " + std::to_string(OW_POLY_WIN_LO) + " (and fewer than 2^31) samples: the measurement window starts there");
        const bool any_audio = final_out || separate_sum_out || residual_out;
        if (any_audio && out_stride < (size_t)n) throw std::runtime_error("stride smaller than the " + std::to_string(n) + " samples of a chord");
        if (n_chords == 0) return n;
        if (!chords || !rows_out) throw std::runtime_error("null argument");
        if (n_chords > (size_t)INT32_MAX / 64) throw std::runtime_error("too many chords");
        for (size_t i = 0; i < n_chords; ++i) {
            const ow_poly_chord& c = chords[i];
            const std::string at = "chord " + std::to_string(i) + ": ";
            if (c.n_notes < 1 || c.n_notes > OW_POLY_MAX_NOTES)
                throw std::runtime_error(at + "n_notes " + std::to_string(c.n_notes) + " outside 1.." + std::to_string(OW_POLY_MAX_NOTES));
            for (int k = 0; k < c.n_notes; ++k) check_note_velocity(at, c.notes[k], c.velocities[k]);
            check_positive_finite(at, "r_ldr", c.r_ldr);
            check_finite(at, "volume", c.volume);
            check_finite(at, "speaker", c.speaker);
        }
        OfflineCall call(cfg->device, sr, OW_PREAMP_LEGACY8, /*note_table=*/true);   // the preamp at OVERSAMPLED_SR = 88 200 Hz (main.rs:27-28, 132-148)
        hipStream_t st = call.st();
        const OwConsts* dK = call.dK();
        const Switches& sw = call.sw;
        const long long stride = row_stride(n);
        const size_t row_bytes = sizeof(double) * (size_t)stride;
        // chunks: runs of chords in call order whose rows (n voice rows + three result rows each) fit the budget, OW_POLY_CHUNK chords at most
        std::vector<size_t> cuts{0};
        size_t max_chords = 0, max_voices = 0;
        {
            size_t rows = 0, voices = 0;
            for (size_t i = 0; i < n_chords; ++i) {
                const size_t cnt = i - cuts.back();
                const bool full = cnt > 0 && ((rows + poly::chord_rows(chords[i])) * row_bytes > poly::BUDGET_BYTES || (sw.poly_chunk > 0 && cnt >= (size_t)sw.poly_chunk));
                if (full) { cuts.push_back(i); rows = 0; voices = 0; }
                rows += poly::chord_rows(chords[i]);
                voices += chords[i].n_notes;
                max_chords = std::max(max_chords, i + 1 - cuts.back());
                max_voices = std::max(max_voices, voices);
            }
            cuts.push_back(n_chords);
        }
        DevMem m_vrec, m_voices, m_chords, m_slots, m_reed, m_fin, m_sep, m_res, m_met;   // released on every exit path
        m_vrec.alloc(sizeof(double) * ((max_voices + 63) / 64) * OW_VREC_DOUBLES);
        m_voices.alloc(sizeof(owdev::OwPolyVoiceDev) * max_voices);
        m_chords.alloc(sizeof(owdev::OwPolyChordDev) * max_chords);
        m_slots.alloc(sizeof(owdev::OwPolySlotDev) * 32 * max_chords);  // at most one wavefront per chord
        m_reed.alloc(row_bytes * max_voices);
        if (final_out) m_fin.alloc(row_bytes * max_chords);
        if (separate_sum_out) m_sep.alloc(row_bytes * max_chords);
        if (residual_out) m_res.alloc(row_bytes * max_chords);
        m_met.alloc(sizeof(double) * owdev::POLY_MET_COUNT * n_chords);
        const long long win_hi = std::min<long long>(OW_POLY_WIN_HI, n);     // (2.0 * BASE_SR).min(n_samples as f64) as usize, main.rs:1517
        std::vector<owdev::OwPolyVoiceDev> hv;
        std::vector<owdev::OwPolyChordDev> hch;
        std::vector<owdev::OwPolySlotDev> hs;
        for (size_t q = 0; q + 1 < cuts.size(); ++q) {
            const size_t c0 = cuts[q], cn = cuts[q + 1] - c0;
            hv.clear(); hch.clear(); hs.clear();
            int used = 32;                                             // slots taken in the wavefront being filled (32: open a new one)
            for (size_t i = 0; i < cn; ++i) {
                const ow_poly_chord& c = chords[c0 + i];
                owdev::OwPolyChordDev d;
                std::memset(&d, 0, sizeof(d));
                d.volume = c.volume; d.speaker = c.speaker; d.r_ldr = c.r_ldr;
                d.n_notes = c.n_notes; d.no_poweramp = c.no_poweramp ? 1 : 0; d.voice_row0 = (int32_t)hv.size();
                hch.push_back(d);
                for (int k = 0; k < c.n_notes; ++k) {                  // (note as u32).wrapping_mul(2654435761).wrapping_add(i as u32), main.rs:1437-1439
                    owdev::OwPolyVoiceDev v;
                    std::memset(&v, 0, sizeof(v));
                    v.note = c.notes[k]; v.velocity = c.velocities[k]; v.seed = (uint32_t)c.notes[k] * 2654435761u + (uint32_t)k;
                    hv.push_back(v);
                }
                // no chord straddles a wavefront: its n + 1 chains take adjacent slots of one
                if (used + c.n_notes + 1 > 32) {
                    hs.resize(hs.size() + 32, owdev::OwPolySlotDev{-1, 0});
                    used = 0;
                }
                owdev::OwPolySlotDev* blk = hs.data() + hs.size() - 32;
                for (int k = 0; k <= c.n_notes; ++k) blk[used + k] = owdev::OwPolySlotDev{(int32_t)i, k};
                used += c.n_notes + 1;
            }
            const size_t nv = hv.size(), nblocks = hs.size() / 32;
            HIP_OK(hipMemcpyAsync(m_voices.p, hv.data(), sizeof(owdev::OwPolyVoiceDev) * nv, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(m_chords.p, hch.data(), sizeof(owdev::OwPolyChordDev) * cn, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(m_slots.p, hs.data(), sizeof(owdev::OwPolySlotDev) * hs.size(), hipMemcpyHostToDevice, st));
            owdev::k_poly_voice<<<dim3((unsigned)((nv + 63) / 64)), dim3(64), 0, st>>>(dK, call.nt(), m_vrec.as<double>(), m_voices.as<owdev::OwPolyVoiceDev>(),
                                                                                        m_reed.as<double>(), (int)nv, n, stride);
            HIP_OK(hipGetLastError());
            owdev::k_poly_chain<<<dim3((unsigned)nblocks), dim3(64), 0, st>>>(dK, m_chords.as<owdev::OwPolyChordDev>(), m_slots.as<owdev::OwPolySlotDev>(),
                                                                              m_reed.as<double>(), m_fin.as<double>(), m_sep.as<double>(), m_res.as<double>(),
                                                                              m_met.as<double>() + c0 * owdev::POLY_MET_COUNT, n, stride, win_hi);
            HIP_OK(hipGetLastError());
            auto copy_rows = [&](double* host, const DevMem& m) {
                if (host) rows_to_host(host + c0 * out_stride, out_stride, m.p, (size_t)stride, (size_t)n, cn, st);
            };
            copy_rows(final_out, m_fin); copy_rows(separate_sum_out, m_sep); copy_rows(residual_out, m_res);
            HIP_OK(hipStreamSynchronize(st));                          // the host vectors are refilled for the next chunk
        }
        std::vector<double> hm(n_chords * owdev::POLY_MET_COUNT);
        HIP_OK(hipMemcpyAsync(hm.data(), m_met.p, sizeof(double) * hm.size(), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const double nwin = (double)(win_hi - OW_POLY_WIN_LO);         // signal.len() of the window slices
        for (size_t i = 0; i < n_chords; ++i) {
            const double* m = &hm[i * owdev::POLY_MET_COUNT];
            ow_poly_row& r = rows_out[i];
            std::memset(&r, 0, sizeof(r));
            r.peak = m[owdev::POLY_MET_PEAK];
            r.residual_peak = m[owdev::POLY_MET_RES_PEAK];
            for (int k = 0; k < 3; ++k) {
                r.win_peak[k] = m[owdev::POLY_MET_WPK + k];
                r.win_mean_sq[k] = m[owdev::POLY_MET_WSS + k] / nwin;                 // rms_db's mean_sq, main.rs:921
                r.peak_db[k] = measure::to_dbfs(r.win_peak[k]);                          // :1522-1524
                r.rms_db[k] = measure::rms_db(r.win_mean_sq[k]);                         // :1525-1527
            }
            r.intermod_ratio_db = r.rms_db[0] - r.rms_db[2];                          // :1575
        }
        return n;
    } catch (const std::exception& ex) { set_err(std::string("ow_render_poly: ") + ex.what()); return -1; }
}
}  // extern "C"
