// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: library / pool entry points, host blocks, taps, trajectory control and persistence, MIDI bursts.

extern "C" {

int ow_abi_version(void) { return OW_ABI_VERSION; }
const char* ow_last_error(void) { return g_err.c_str(); }
void ow_clear_error(void) { g_err.clear(); }

ow_pool* ow_pool_new(double sample_rate, size_t n_engines, int device, int preamp_kind) {
    try { return pool_create(sample_rate, n_engines, device, preamp_kind); }
    catch (const std::exception& ex) { set_err(std::string("ow_pool_new: ") + ex.what()); return nullptr; }
}
ow_pool* ow_pool_new_kinds(double sample_rate, size_t n_engines, int device, int preamp_kind, int power_amp_kind, int tremolo_kind) {
    try { return pool_create(sample_rate, n_engines, device, preamp_kind, power_amp_kind, tremolo_kind); }
    catch (const std::exception& ex) { set_err(std::string("ow_pool_new_kinds: ") + ex.what()); return nullptr; }
}
ow_pool* ow_pool_new_with(double sample_rate, size_t n_engines, int device, int preamp_kind, int power_amp_kind) {
    try { return pool_create(sample_rate, n_engines, device, preamp_kind, power_amp_kind); }
    catch (const std::exception& ex) { set_err(std::string("ow_pool_new_with: ") + ex.what()); return nullptr; }
}
void ow_pool_free(ow_pool* p) { delete p; }
size_t ow_pool_size(const ow_pool* p) { return p ? p->I : 0; }
ow_engine* ow_pool_engine(ow_pool* p, size_t i) { return (p && i < p->I) ? p->engines[i].get() : nullptr; }
ow_pool* ow_engine_pool(ow_engine* e) { return e ? e->pool : nullptr; }
void* ow_pool_stream(ow_pool* p) { return p ? (void*)p->stream : nullptr; }
void ow_pool_set_profiling(ow_pool* p, int on) { if (p) p->profiling = on != 0; }
void ow_pool_last_kernel_ms(const ow_pool* p, float ms[5]) { for (int i = 0; i < 5; ++i) ms[i] = p ? p->last_ms[i] : 0.f; }

int ow_pool_set_sample_rate(ow_pool* p, double sr) {
    if (!p || !(sr > 0.0)) return -1;
    try {
        HIP_OK(hipSetDevice(p->device));
        upload_consts(p, sr, p->hc.preamp_kind);
        for (auto& en : p->engines) {
            en->sr = sr;
            en->noise_on = false; en->thermal_gain = 1.0;   // set_sample_rate builds a new DkPreamp (engine.rs:276): noise off, gain 1.0
            en->rail_sag = true;                            // ... and a new PowerAmp (engine.rs:279): rail sag back on
            en->touch();
        }
        // voices keep their records (the reference keeps Voice objects too, engine.rs:272-286), chain objects are rebuilt
        std::vector<double> d0(p->I);
        for (size_t i = 0; i < p->I; ++i) d0[i] = p->engines[i]->depth.target;
        chain_init_range(p, 0, (int)p->I, INIT_RATE, d0);
        warm_up_range(p, 0, (int)p->I);
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_pool_set_sample_rate: ") + ex.what()); return -1; }
}

void ow_pool_reset(ow_pool* p) {
    if (!p) return;
    guarded("ow_pool_reset", [&] {
        HIP_OK(hipSetDevice(p->device));
        for (auto& en : p->engines) engine_host_reset(en.get());
        chain_init_range(p, 0, (int)p->I, INIT_RESET, std::vector<double>(p->I, 0.0));
        warm_up_range(p, 0, (int)p->I);
    });
}

void ow_pool_ensure_buffer_capacity(ow_pool* p, size_t n) {
    if (!p || n <= p->Lcap) return;
    guarded("ow_pool_ensure_buffer_capacity", [&] {
        HIP_OK(hipSetDevice(p->device));
        HIP_OK(hipStreamSynchronize(p->stream));
        alloc_stream_buffers(p, n);
    });
}

void ow_pool_render(ow_pool* p, float* out_host, size_t out_stride, size_t len) {
    if (!p || len == 0) return;
    const bool ok = guarded("ow_pool_render", [&] {
        HIP_OK(hipSetDevice(p->device));
        if (p->inject_faults > 0) { --p->inject_faults; throw std::runtime_error("injected fault (ow_test_inject_render_faults)"); }
        const bool hostprof = p->sw.host_profile;
        auto t0 = std::chrono::steady_clock::now();
        render_range(p, 0, (int)p->I, len, true, out_host, out_stride);
        steal_countdown_early(p, len);
        auto t1 = std::chrono::steady_clock::now();
        HIP_OK(hipStreamSynchronize(p->stream));
        auto t2 = std::chrono::steady_clock::now();
        post_render_host(p, 0, (int)p->I, len);
        auto t3 = std::chrono::steady_clock::now();
        collect_profile(p);
        if (p->d_vm && p->vm_bursts && p->vm_host_dirty && p->stream_copy && !p->vm_download_pending) {   // see ow_pool::ev_vm_up
            if (p->vm_upload_inflight) HIP_OK(hipStreamWaitEvent(p->stream_copy, p->ev_vm_up, 0));
            __atomic_store_n(&p->vm_host_dirty, (uint8_t)0, __ATOMIC_RELAXED);
            HIP_OK(hipMemcpyAsync(p->d_vm, p->h_vm, sizeof(OwVm) * p->I, hipMemcpyHostToDevice, p->stream_copy));
            HIP_OK(hipEventRecord(p->ev_vm_up, p->stream_copy));
            p->vm_upload_inflight = true;
        }
        auto t4 = std::chrono::steady_clock::now();
        if (hostprof) {
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            double* acc = p->hostprof_acc;
            acc[0] += ms(t0, t1); acc[1] += ms(t1, t2); acc[2] += ms(t2, t3); acc[3] += ms(t3, t4);
            if (ms(t0, t1) > 2.0 || ms(t2, t3) > 1.0)      // the blocks around a re-strike: where the host time between the kernels goes
                std::fprintf(stderr, "hostprof block %ld len %zu: launch %.3f wait %.3f post %.3f ms\n", p->hostprof_cnt, len, ms(t0, t1), ms(t1, t2), ms(t2, t3));
            if (++p->hostprof_cnt % 50 == 0) { std::fprintf(stderr, "hostprof I=%zu: launch %.3f wait %.3f post %.3f profile %.3f ms (mean of 50)\n", p->I, acc[0] / 50, acc[1] / 50, acc[2] / 50, acc[3] / 50); acc[0] = acc[1] = acc[2] = acc[3] = 0; }
        }
        p->last_len = len;
    });
    if (!ok) {
        // queued note events / setter targets of engines the failed render did not get to pack must survive: the next block scans again
        __atomic_store_n(&p->dirty_any, (uint8_t)1, __ATOMIC_RELAXED);
        p->args_stale = true; p->lists_valid = false; p->steal_counted = false;
        // "never fails, degrades to silence" (SURVEY 8b; engine.rs:450-458 does the same for numeric failure): every row of the
        // caller's block is written.  Drain the stream first so that an output copy already queued cannot land after the zeros.
        for (hipStream_t s : {(hipStream_t)p->stream, (hipStream_t)p->stream_trem, (hipStream_t)p->stream_copy}) if (s) hipStreamSynchronize(s);
        if (out_host && out_stride >= len)
            for (size_t e = 0; e < p->I; ++e) std::memset(out_host + e * out_stride, 0, len * sizeof(float));
        if (p->d_out && len <= p->Lcap) { hipMemset(p->d_out, 0, sizeof(float) * len * p->I); p->out_ld = len; }   // the HBM copy of the block too
    }
}

const float* ow_pool_device_output(const ow_pool* p, size_t* stride) {
    if (!p) return nullptr;
    if (stride) *stride = p->out_ld;
    return p->d_out;
}

// Shared tremolo trajectory of (device, the chain rate of host rate `sample_rate`): make its first `seconds` exist now (blocking), e.g.
// when a host instantiates the plugin, so that no engine ever waits for the single oscillator that extends it.  Returns the number of
// samples the store holds afterwards, <0 on error.
long long ow_tremolo_prefetch(double sample_rate, int device, double seconds) {
    try {
        if (!(sample_rate > 0.0) || !(seconds >= 0.0)) throw std::runtime_error("bad argument");
        HIP_OK(hipSetDevice(device));
        std::unique_ptr<OwConsts> hc(new OwConsts()), k48(new OwConsts());
        owhip::build_consts(*hc, sample_rate, OW_PREAMP_LEGACY8);
        owhip::build_consts(*k48, 24000.0, OW_PREAMP_LEGACY8);
        const Switches sw = Switches::from_env();
        std::shared_ptr<TremTraj> t = traj_acquire(device, *hc, *k48, sw.trem_cache);
        const size_t want = (size_t)std::min(seconds * hc->os_sr, (double)t->cap_max);
        t->grow_to(want);                                    // instantiation time: the place to allocate
        hipEvent_t ev;
        { std::lock_guard<std::mutex> lk(t->mu); ev = t->cover(want, 0); }
        if (ev) HIP_OK(hipEventSynchronize(ev));
        std::lock_guard<std::mutex> lk(t->mu);
        return (long long)std::max(t->done, std::min(want, t->len));     // (the store may hold more: the background lead)
    } catch (const std::exception& ex) { set_err(std::string("ow_tremolo_prefetch: ") + ex.what()); return -1; }
}

// ---- trajectory persistence (ow_tremolo_export / ow_tremolo_import) -----------------------------------------------------------------
// The reference's expensive start-up states are in-process caches (OnceLock: dk_preamp/melange_adapter.rs:12-29; Tremolo::new settles in
// its constructor, tremolo.rs:92-102), paid once per process.  Here the analogue of that cost is the trajectory itself: a fresh process
// that renders offline faster than the one oscillator steps waits for it.  A host may therefore keep the store across processes: export
// writes r_ldr[0 .. L) (L = the store's length cut to a checkpoint boundary), the checkpoints, the fallback list and the settled rows;
// import loads them into the store of (device, chain rate) -- after checking that THIS library would have produced them: same build, same
// tremolo constants, payload checksum, and the first and the last 4 096-sample segment regenerated on the device by the product kernel
// from the file's own settled rows / checkpoint and compared bit for bit (samples and the checkpoint behind them).
namespace {
struct TrajFileHeader {
    char magic[8];                  // "OWTRAJ1\0"
    uint32_t abi, ck;               // OW_ABI_VERSION, OW_TRAJ_CK
    uint64_t build_id, consts_hash, rate_bits, len, be_settle, payload_sum;
    double settled[18];
    uint64_t reserved[4];
};
uint64_t fnv64(const void* data, size_t bytes, uint64_t h = 0xCBF29CE484222325ull) {
    const unsigned char* b = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}
uint64_t words_sum(const void* data, size_t bytes, uint64_t h) {     // order-dependent mix over 64-bit words (payloads are arrays of 8-byte items)
    const uint64_t* w = static_cast<const uint64_t*>(data);
    for (size_t i = 0; i < bytes / 8; ++i) { h ^= w[i]; h *= 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
    return h;
}
uint64_t traj_build_id() { static const char stamp[] = "openwurli-hip " __DATE__ " " __TIME__; return fnv64(stamp, sizeof stamp) ^ (uint64_t)OW_ABI_VERSION; }
uint64_t traj_consts_hash(const OwConsts& c) {
    uint64_t h = fnv64(c.t_a_neg, sizeof c.t_a_neg);
    h = fnv64(c.t_s, sizeof c.t_s, h); h = fnv64(c.t_k, sizeof c.t_k, h); h = fnv64(c.t_s_ni, sizeof c.t_s_ni, h);
    h = fnv64(c.t_a_neg_be, sizeof c.t_a_neg_be, h); h = fnv64(c.t_s_be, sizeof c.t_s_be, h); h = fnv64(c.t_k_be, sizeof c.t_k_be, h);
    h = fnv64(c.t_s_ni_be, sizeof c.t_s_ni_be, h);
    const double tail[4] = {c.ldr_attack, c.ldr_release, c.ln_r_max, c.ln_min_minus_max};
    return fnv64(tail, sizeof tail, h);
}
struct FileCloser { std::FILE* f = nullptr; ~FileCloser() { if (f) std::fclose(f); } };
// oscillator rows (I = 1 layout) in front of sample k * OW_TRAJ_CK, from checkpoint k (v[7] ip[4] ipp[4] env) and the sample before it
void traj_state_from_ckpt(const double* ck, double r_before, double* rows) {
    for (int i = 0; i < 7; ++i) rows[CS_T_V + i] = ck[i];
    for (int i = 0; i < 4; ++i) { rows[CS_T_I + i] = ck[7 + i]; rows[CS_T_IP + i] = ck[11 + i]; }
    rows[CS_T_ENV] = ck[15]; rows[CS_T_RLDR] = r_before;
    const uint64_t z = 0; std::memcpy(&rows[CS_T_BE], &z, 8);
}
}  // namespace

long long ow_tremolo_export(double sample_rate, int device, const char* path) {
    try {
        if (!(sample_rate > 0.0) || !path) throw std::runtime_error("bad argument");
        HIP_OK(hipSetDevice(device));
        std::unique_ptr<OwConsts> hc(new OwConsts()), k48(new OwConsts());
        owhip::build_consts(*hc, sample_rate, OW_PREAMP_LEGACY8);
        owhip::build_consts(*k48, 24000.0, OW_PREAMP_LEGACY8);
        const Switches sw = Switches::from_env();
        std::shared_ptr<TremTraj> t = traj_acquire(device, *hc, *k48, sw.trem_cache);
        TrajFileHeader h;
        std::memset(&h, 0, sizeof h);
        std::memcpy(h.magic, "OWTRAJ1", 8);
        h.abi = OW_ABI_VERSION; h.ck = OW_TRAJ_CK; h.build_id = traj_build_id(); h.consts_hash = traj_consts_hash(*hc);
        std::memcpy(&h.rate_bits, &hc->os_sr, 8);
        std::vector<double> r, ck;
        std::vector<unsigned long long> be(1 + OW_TRAJ_BE_CAP);
        {
            std::lock_guard<std::mutex> lk(t->mu);
            HIP_OK(hipStreamSynchronize(t->stream));                   // everything enqueued has been produced
            const size_t L = t->len / OW_TRAJ_CK * OW_TRAJ_CK;
            if (L == 0) throw std::runtime_error("the store holds less than one checkpoint segment");
            h.len = L; h.be_settle = t->be_settle;
            r.resize(L); ck.resize((L / OW_TRAJ_CK + 1) * OW_TRAJ_CKD);
            HIP_OK(hipMemcpy(r.data(), t->d_r, sizeof(double) * L, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(ck.data(), t->d_ckpt, sizeof(double) * ck.size(), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(be.data(), t->d_be, sizeof(unsigned long long) * be.size(), hipMemcpyDeviceToHost));
        }
        // events of samples beyond L belong to what is not exported
        { size_t k = 0; const size_t n = (size_t)std::min<unsigned long long>(be[0], OW_TRAJ_BE_CAP);
          for (size_t i = 0; i < n; ++i) if (be[1 + i] < h.len) be[1 + k++] = be[1 + i];
          for (size_t i = k; i < OW_TRAJ_BE_CAP; ++i) be[1 + i] = ~0ull;
          be[0] = k; }
        traj_state_from_ckpt(ck.data(), 1000000.0, h.settled);         // the settled rows ARE checkpoint 0 (the cell at rest: r_ldr = 1 MOhm)
        std::memcpy(&h.settled[17], &h.be_settle, 8);
        h.payload_sum = words_sum(be.data(), sizeof(unsigned long long) * be.size(), words_sum(ck.data(), sizeof(double) * ck.size(), words_sum(r.data(), sizeof(double) * r.size(), 0x0123456789ABCDEFull)));
        FileCloser fc;
        fc.f = std::fopen(path, "wb");
        if (!fc.f) throw std::runtime_error(std::string("cannot open ") + path);
        if (std::fwrite(&h, sizeof h, 1, fc.f) != 1 || std::fwrite(r.data(), sizeof(double), r.size(), fc.f) != r.size() ||
            std::fwrite(ck.data(), sizeof(double), ck.size(), fc.f) != ck.size() || std::fwrite(be.data(), sizeof(unsigned long long), be.size(), fc.f) != be.size())
            throw std::runtime_error("short write");
        return (long long)h.len;
    } catch (const std::exception& ex) { (void)hipGetLastError(); set_err(std::string("ow_tremolo_export: ") + ex.what()); return -1; }
}

long long ow_tremolo_import(double sample_rate, int device, const char* path) {
    try {
        if (!(sample_rate > 0.0) || !path) throw std::runtime_error("bad argument");
        HIP_OK(hipSetDevice(device));
        std::unique_ptr<OwConsts> hc(new OwConsts()), k48(new OwConsts());
        owhip::build_consts(*hc, sample_rate, OW_PREAMP_LEGACY8);
        owhip::build_consts(*k48, 24000.0, OW_PREAMP_LEGACY8);
        FileCloser fc;
        fc.f = std::fopen(path, "rb");
        if (!fc.f) throw std::runtime_error(std::string("cannot open ") + path);
        TrajFileHeader h;
        if (std::fread(&h, sizeof h, 1, fc.f) != 1 || std::memcmp(h.magic, "OWTRAJ1", 8) != 0) throw std::runtime_error("not a trajectory file");
        uint64_t rate_bits; std::memcpy(&rate_bits, &hc->os_sr, 8);
        if (h.abi != OW_ABI_VERSION || h.ck != OW_TRAJ_CK || h.build_id != traj_build_id()) throw std::runtime_error("written by another build of the library");
        if (h.rate_bits != rate_bits) throw std::runtime_error("written for another chain rate");
        if (h.consts_hash != traj_consts_hash(*hc)) throw std::runtime_error("written with other tremolo constants");
        const size_t L = (size_t)h.len;
        if (L == 0 || L % OW_TRAJ_CK != 0 || L > (size_t)4.0e9) throw std::runtime_error("bad length");
        std::vector<double> r(L), ck((L / OW_TRAJ_CK + 1) * OW_TRAJ_CKD);
        std::vector<unsigned long long> be(1 + OW_TRAJ_BE_CAP);
        if (std::fread(r.data(), sizeof(double), r.size(), fc.f) != r.size() || std::fread(ck.data(), sizeof(double), ck.size(), fc.f) != ck.size() ||
            std::fread(be.data(), sizeof(unsigned long long), be.size(), fc.f) != be.size())
            throw std::runtime_error("truncated file");
        if (h.payload_sum != words_sum(be.data(), sizeof(unsigned long long) * be.size(), words_sum(ck.data(), sizeof(double) * ck.size(), words_sum(r.data(), sizeof(double) * r.size(), 0x0123456789ABCDEFull))))
            throw std::runtime_error("checksum mismatch");
        // ---- would this library have produced it?  Segment 0 from the file's settled rows, the last segment from its checkpoint.
        {
            DevMem dk, dstate, dr, dck, dbe;
            dk.alloc(sizeof(OwConsts)); dstate.alloc(sizeof(double) * 18); dr.alloc(sizeof(double) * (OW_TRAJ_CK + 64));
            const size_t nck = TremTraj::ckpt_doubles(L);
            dck.alloc(sizeof(double) * nck); dbe.alloc(sizeof(unsigned long long) * (1 + OW_TRAJ_BE_CAP));
            HIP_OK(hipMemcpy(dk.p, hc.get(), sizeof(OwConsts), hipMemcpyHostToDevice));
            std::vector<double> got(OW_TRAJ_CK), gck(OW_TRAJ_CKD);
            const size_t K = L / OW_TRAJ_CK;
            for (int pass = 0; pass < 2; ++pass) {
                const size_t seg = pass == 0 ? 0 : K - 1;
                if (pass == 1 && seg == 0) break;
                double rows[18];
                if (seg == 0) { std::memcpy(rows, h.settled, sizeof rows); const uint64_t z = 0; std::memcpy(&rows[17], &z, 8); }
                else traj_state_from_ckpt(ck.data() + seg * OW_TRAJ_CKD, r[seg * OW_TRAJ_CK - 1], rows);
                HIP_OK(hipMemcpy(dstate.p, rows, sizeof rows, hipMemcpyHostToDevice));
                HIP_OK(hipMemset(dbe.p, 0, sizeof(unsigned long long) * (1 + OW_TRAJ_BE_CAP)));
                owdev::k_trem_traj_extend_row<<<dim3(1), dim3(64)>>>(dk.as<OwConsts>(), dstate.as<double>(), dr.as<double>(), (long long)(seg * OW_TRAJ_CK),
                                                                      (long long)OW_TRAJ_CK, dck.as<double>(), dbe.as<unsigned long long>());
                HIP_OK(hipGetLastError());
                HIP_OK(hipMemcpy(got.data(), dr.p, sizeof(double) * OW_TRAJ_CK, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(gck.data(), dck.as<double>() + (seg + 1) * OW_TRAJ_CKD, sizeof(double) * OW_TRAJ_CKD, hipMemcpyDeviceToHost));
                if (std::memcmp(got.data(), r.data() + seg * OW_TRAJ_CK, sizeof(double) * OW_TRAJ_CK) != 0 ||
                    std::memcmp(gck.data(), ck.data() + (seg + 1) * OW_TRAJ_CKD, sizeof(double) * OW_TRAJ_CKD) != 0)
                    throw std::runtime_error("the regenerated segment differs from the file's");
            }
        }
        // ---- the settled rows spare the new store its settle; then the store takes what it does not have yet
        const Switches sw = Switches::from_env();
        if (sw.trem_cache) {
            TremSettled ts;
            std::memcpy(ts.rows, h.settled, sizeof ts.rows);
            std::lock_guard<std::mutex> lk(g_mel_mu);
            g_trem_settled.emplace(std::make_pair(device, rate_bits), ts);        // (an existing entry stays: it was computed here)
        }
        std::shared_ptr<TremTraj> t = traj_acquire(device, *hc, *k48, sw.trem_cache);
        if (t->be_settle != h.be_settle) throw std::runtime_error("settled state differs from this library's");
        if (L > t->cap_max) throw std::runtime_error("longer than the store's configured capacity (ow_tremolo_configure)");
        t->grow_to(L);
        std::lock_guard<std::mutex> lk(t->mu);
        HIP_OK(hipStreamSynchronize(t->stream));
        if (L > t->cap) throw std::runtime_error("the store could not grow to the file's length");
        if (L <= t->len) return 0;                                         // the store already holds more
        const size_t from = t->len / OW_TRAJ_CK * OW_TRAJ_CK;               // whole segments from the checkpoint at or below the store's end (same bits where they overlap)
        HIP_OK(hipMemcpy(t->d_r + from, r.data() + from, sizeof(double) * (L - from), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(t->d_ckpt + from / OW_TRAJ_CK * OW_TRAJ_CKD, ck.data() + from / OW_TRAJ_CK * OW_TRAJ_CKD, sizeof(double) * (L / OW_TRAJ_CK - from / OW_TRAJ_CK + 1) * OW_TRAJ_CKD, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(t->d_be, be.data(), sizeof(unsigned long long) * be.size(), hipMemcpyHostToDevice));
        double rows[18];
        traj_state_from_ckpt(ck.data() + L / OW_TRAJ_CK * OW_TRAJ_CKD, r[L - 1], rows);
        HIP_OK(hipMemcpy(t->d_state, rows, sizeof rows, hipMemcpyHostToDevice));
        t->len = L; t->done = L;
        t->target = std::max(t->target, L);
        return (long long)L;
    } catch (const std::exception& ex) { (void)hipGetLastError(); set_err(std::string("ow_tremolo_import: ") + ex.what()); return -1; }
}

// Capacity and lead of the trajectory stores of `device` (seconds of audio): capacity_seconds = how old an engine may grow (time since
// new / reset / set_sample_rate) before it leaves the shared trajectory for an oscillator of its own (default 1 800; <= 0 restores it);
// lead_seconds = how far the store is kept ahead of its oldest reader in the background (default 60; 0 = only the block ahead; < 0
// restores the default).  The buffers are NOT reserved at that size: a store starts at 150 s (115 MB at 96 kHz; all of it for pools of
// >= 4 096 engines) and doubles on a helper thread well before a reader gets there.  Applies to stores created afterwards (a store is
// created by the first engine of its device and chain rate) and raises / lowers the limits of the existing ones.  0 on success.
int ow_tremolo_configure(int device, double capacity_seconds, double lead_seconds) {
    try {
        std::vector<std::shared_ptr<TremTraj>> live;
        {
            std::lock_guard<std::mutex> lk(g_traj_mu);
            TrajConfig& c = g_traj_cfg[device];
            c.seconds = capacity_seconds > 0.0 ? capacity_seconds : 0.0;
            c.lead = lead_seconds >= 0.0 ? lead_seconds : -1.0;
            for (auto& kv : traj_registry()) if (kv.first.first == device) live.push_back(kv.second);
        }
        for (auto& t : live) {
            std::lock_guard<std::mutex> lk(t->mu);
            const double secs = capacity_seconds > 0.0 ? capacity_seconds : OW_TRAJ_DEFAULT_SECONDS, lead = lead_seconds >= 0.0 ? lead_seconds : OW_TRAJ_DEFAULT_LEAD;
            const size_t want = ((size_t)std::min(secs * t->os_sr, 4.0e9) + OW_TRAJ_CK - 1) / OW_TRAJ_CK * OW_TRAJ_CK;
            t->cap_max = std::max(want, t->cap);             // never below what is already allocated (engines may stand there)
            t->lead = (size_t)std::min(lead * t->os_sr, (double)t->cap_max);
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_tremolo_configure: ") + ex.what()); return -1; }
}

int ow_pool_read_voice_sum(ow_pool* p, double* out_host, size_t out_stride, size_t len) {
    if (!p || !out_host || len > p->Lcap) return -1;
    try {
        HIP_OK(hipSetDevice(p->device));
        const size_t I = p->I;
        std::vector<double> a(I * len), b(I * len);
        HIP_OK(hipMemcpy2D(a.data(), len * sizeof(double), p->d_sum, p->Lcap * sizeof(double), len * sizeof(double), I, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy2D(b.data(), len * sizeof(double), p->d_sum + I * p->Lcap, p->Lcap * sizeof(double), len * sizeof(double), I, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < I; ++e) {
            const OwEngineArgs& ar = p->h_args[e];
            for (size_t n = 0; n < len; ++n) {
                double x = 0.0;
                if (!p->h_eout[e].sum_nonfinite) {
                    if (ar.main_mask) x = a[e * len + n];
                    if (ar.steal_mask) x += b[e * len + n];
                }
                out_host[e * out_stride + n] = x;
            }
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_pool_read_voice_sum: ") + ex.what()); return -1; }
}

int ow_pool_read_preamp_out(ow_pool* p, double* out_host, size_t out_stride, size_t n_os) {
    if (!p || !out_host || n_os > 2 * p->Lcap) return -1;
    try {
        HIP_OK(hipSetDevice(p->device));
        const size_t I = p->I;
        std::vector<double> a(I * n_os);
        HIP_OK(hipMemcpy(a.data(), p->d_pre, sizeof(double) * I * n_os, hipMemcpyDeviceToHost));  // [n_os][I]
        for (size_t e = 0; e < I; ++e)
            for (size_t n = 0; n < n_os; ++n) out_host[e * out_stride + n] = a[n * I + e];
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_pool_read_preamp_out: ") + ex.what()); return -1; }
}

int ow_pool_read_tremolo_r(ow_pool* p, double* out_host, size_t out_stride, size_t n_os) {
    if (!p || !out_host || n_os > 2 * p->Lcap) return -1;
    try {
        HIP_OK(hipSetDevice(p->device));
        const size_t I = p->I;
        std::vector<double> a(I * n_os);
        const double* src = p->d_rbuf + (size_t)p->rb_cur * (2 * p->Lcap * I);   // the half the last block consumed, [n_os][I]
        HIP_OK(hipMemcpy(a.data(), src, sizeof(double) * I * n_os, hipMemcpyDeviceToHost));
        std::vector<double> tr;
        if (p->traj && p->n_on_traj) {     // engines on the shared trajectory: the n_os samples below their present t
            if ((long long)n_os > p->last_n_os) throw std::runtime_error("more samples than the last block consumed");
            // (the samples the last block consumed are complete -- its kernels waited for them; no wait for the store's stream, which
            // the background extension keeps busy)
            HIP_OK(hipStreamSynchronize(p->stream));
            DevMem g;
            g.alloc(sizeof(double) * I * n_os);
            const double* base;
            { std::lock_guard<std::mutex> lk(p->traj->mu); base = p->traj->d_r; }
            // the block consumed [t_end - last_n_os, t_end); its first n_os samples are asked for
            owdev::k_trem_traj_gather<<<dim3((unsigned)((I * n_os + 255) / 256)), dim3(256), 0, p->stream>>>(
                base + p->trem_clock - (p->last_n_os - (long long)n_os), p->d_birth, (int)I, (long long)n_os, g.as<double>());
            HIP_OK(hipGetLastError());
            tr.resize(I * n_os);
            HIP_OK(hipMemcpyAsync(tr.data(), g.p, sizeof(double) * I * n_os, hipMemcpyDeviceToHost, p->stream));
            HIP_OK(hipStreamSynchronize(p->stream));
        }
        for (size_t e = 0; e < I; ++e) {
            if (!tr.empty() && p->h_birth[e] != OW_OFF_TRAJ) { std::memcpy(out_host + e * out_stride, tr.data() + e * n_os, sizeof(double) * n_os); continue; }
            for (size_t n = 0; n < n_os; ++n) out_host[e * out_stride + n] = a[n * I + p->h_lead[e]];   // the column of the engine's phase group
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_pool_read_tremolo_r: ") + ex.what()); return -1; }
}
}  // extern "C"
