// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): tremolo phase groups, chain (re)initialisation, kernel choice of a block, voice lists, render_range and its phases, post-render bookkeeping, pool life cycle.
namespace {
// ---- tremolo phase groups (see ow_pool) ---------------------------------------------------------------------------------
void trem_groups_changed(ow_pool* p) {
    HIP_OK(hipMemcpyAsync(p->d_lead, p->h_lead, sizeof(uint32_t) * p->I, hipMemcpyHostToDevice, p->stream));
    p->lead_list_valid = false;
    p->split_e0 = p->split_ne = -1;
}
// After this no group has members on both sides of the boundary of [e0, e0+ne): a straddling group is cut in two, the part that
// loses the leader gets its lowest member as the new leader together with a copy of the 18 tremolo rows.  Init / reset / warm-up of
// a sub-range then only touch groups that lie wholly inside it.  O(I) host work, on reset-class calls only.
void trem_split_at_range(ow_pool* p, int e0, int ne) {
    const uint32_t I = (uint32_t)p->I, lo = (uint32_t)e0, hi = (uint32_t)(e0 + ne);
    if (ne >= (int)I || (p->split_e0 == e0 && p->split_ne == ne)) return;
    const uint32_t NONE = 0xFFFFFFFFu;
    bool straddle = false;
    std::fill(p->grp_in.begin(), p->grp_in.end(), NONE);
    std::fill(p->grp_out.begin(), p->grp_out.end(), NONE);
    for (uint32_t e = 0; e < I; ++e) {
        const uint32_t x = p->h_lead[e];
        uint32_t& slot = (e >= lo && e < hi) ? p->grp_in[x] : p->grp_out[x];
        if (slot == NONE) slot = e;                    // ascending scan: the first one found is the lowest
    }
    size_t n_copy = 0;
    for (uint32_t x = 0; x < I; ++x) {
        if (p->grp_in[x] == NONE || p->grp_out[x] == NONE) continue;
        straddle = true;
        const bool x_inside = x >= lo && x < hi;
        const uint32_t fresh = x_inside ? p->grp_out[x] : p->grp_in[x];     // leader of the part that loses x
        p->h_copy[n_copy] = x; p->h_copy[I + n_copy] = fresh; ++n_copy;
    }
    if (straddle) {
        invalidate_spec(p);                             // the oscillator rows must be the committed ones before they are copied
        HIP_OK(hipStreamSynchronize(p->stream));
        for (uint32_t e = 0; e < I; ++e) {
            const uint32_t x = p->h_lead[e];
            if (p->grp_in[x] == NONE || p->grp_out[x] == NONE) continue;
            const bool e_inside = e >= lo && e < hi, x_inside = x >= lo && x < hi;
            if (e_inside != x_inside) p->h_lead[e] = x_inside ? p->grp_out[x] : p->grp_in[x];
        }
        HIP_OK(hipMemcpyAsync(p->d_copy, p->h_copy, sizeof(uint32_t) * n_copy, hipMemcpyHostToDevice, p->stream));
        HIP_OK(hipMemcpyAsync(p->d_copy + I, p->h_copy + I, sizeof(uint32_t) * n_copy, hipMemcpyHostToDevice, p->stream));
        owdev::k_trem_copy_rows<<<dim3((unsigned)((n_copy + 63) / 64)), dim3(64), 0, p->stream>>>(p->d_cs, (int)I, p->d_copy, p->d_copy + I, (int)n_copy);
        trem_groups_changed(p);
        HIP_OK(hipStreamSynchronize(p->stream));
    }
    p->split_e0 = e0; p->split_ne = ne;
}
// Compact list of the group leaders inside [e0, e0+ne) (groups do not straddle the range: trem_split_at_range) -> d_leaders.
// Engines on the shared trajectory have no oscillator of their own and are not listed.
void trem_leader_list(ow_pool* p, int e0, int ne) {
    if (p->lead_list_valid && p->lead_e0 == e0 && p->lead_ne == ne) return;
    if (p->stream_trem) HIP_OK(hipStreamSynchronize(p->stream_trem));   // a kernel still reading the old list (rare path: groups or range changed)
    int n = 0;
    const bool traj = p->traj != nullptr;
    for (int k = 0; k < ne; ++k)
        if (p->h_lead[e0 + k] == (uint32_t)(e0 + k) && !(traj && p->h_birth[e0 + k] != OW_OFF_TRAJ)) p->h_leaders[n++] = (uint32_t)(e0 + k);
    HIP_OK(hipMemcpy(p->d_leaders, p->h_leaders, sizeof(uint32_t) * std::max(n, 1), hipMemcpyHostToDevice));
    p->n_lead = n; p->lead_e0 = e0; p->lead_ne = ne; p->lead_list_valid = true;
}

// min over the engines on the trajectory of birth[e] (the oldest decides how far the store must reach); O(I), reset-class calls only
void traj_recount(ow_pool* p) {
    long long mn = p->trem_clock; size_t n = 0;
    for (size_t e = 0; e < p->I; ++e) if (p->h_birth[e] != OW_OFF_TRAJ) { mn = std::min(mn, p->h_birth[e]); ++n; }
    p->min_birth = mn; p->n_on_traj = n;
}
void traj_upload_births(ow_pool* p, int e0, int ne) {     // synchronous: h_birth is pageable and changes again right away
    HIP_OK(hipStreamSynchronize(p->stream));              // a k_trem_birth_shift of a sub-range render still queued would shift the new values again
    HIP_OK(hipMemcpy(p->d_birth + e0, p->h_birth.data() + e0, sizeof(long long) * (size_t)ne, hipMemcpyHostToDevice));
}

// Engines of [e0, e0+ne) whose next block would run past the end of the store leave the trajectory: each gets its own oscillator rows,
// rebuilt from the checkpoint below its t and stepped up to it (k_trem_from_ckpt, < OW_TRAJ_CK steps), and is a phase group of one from
// here on (per-group oscillator, as in rounds 1-3).  Cold: once in an engine's life, after OW_TREM_TRAJ_SECONDS without a reset.
void trem_evict(ow_pool* p, int e0, int ne, int n_os) {
    TremTraj* T = p->traj.get();
    std::vector<uint32_t> eng; std::vector<long long> tp;
    long long tmax = 0;
    for (int k = 0; k < ne; ++k) {
        const long long b = p->h_birth[e0 + k];
        if (b == OW_OFF_TRAJ || (size_t)(p->trem_clock - b) + (size_t)n_os <= T->cap_max) continue;
        eng.push_back((uint32_t)(e0 + k)); tp.push_back(p->trem_clock - b); tmax = std::max(tmax, p->trem_clock - b);
    }
    if (eng.empty()) return;
    invalidate_spec(p);
    HIP_OK(hipStreamSynchronize(p->stream));
    hipEvent_t ev;
    { std::lock_guard<std::mutex> lk(T->mu); ev = T->cover((size_t)tmax, 0); }
    if (ev) HIP_OK(hipEventSynchronize(ev));
    std::vector<unsigned long long> be(eng.size());
    {
        const std::vector<unsigned long long> events = T->be_events();
        for (size_t i = 0; i < eng.size(); ++i) be[i] = T->be_count_at(tp[i], events);
    }
    // scratch reserved at pool creation (d_evict: [I] engines as u64 | [I] t | [I] fallback counts): no allocation on this path
    uint32_t* de = (uint32_t*)p->d_evict.p; long long* dt = (long long*)(p->d_evict + p->I); unsigned long long* db = p->d_evict + 2 * p->I;
    HIP_OK(hipMemcpy(de, eng.data(), sizeof(uint32_t) * eng.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dt, tp.data(), sizeof(long long) * eng.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(db, be.data(), sizeof(unsigned long long) * eng.size(), hipMemcpyHostToDevice));
    const double* tr; const double* tc;
    { std::lock_guard<std::mutex> lk(T->mu); tr = T->d_r; tc = T->d_ckpt; }
    owdev::k_trem_from_ckpt<<<dim3((unsigned)((eng.size() + 63) / 64)), dim3(64), 0, p->stream>>>(p->dK, tr, tc, p->d_cs, (int)p->I, de, dt, db, (int)eng.size());
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(p->stream));
    for (uint32_t e : eng) { p->h_birth[e] = OW_OFF_TRAJ; p->h_lead[e] = e; }
    traj_upload_births(p, e0, ne);
    traj_recount(p);
    trem_groups_changed(p);
    HIP_OK(hipStreamSynchronize(p->stream));
}

void chain_init_range(ow_pool* p, int e0, int ne, int mode, const std::vector<double>& depth0) {
    invalidate_spec(p);
    HIP_OK(hipStreamSynchronize(p->stream));
    const int I = (int)p->I;
    const bool on_traj = p->traj != nullptr;
    if (on_traj) {
        // Tremolo::new / reset: the cell starts at t = 0 of the shared trajectory (its settled state IS Tremolo::new's) -- nothing to settle,
        // nothing to copy; an engine that had left the trajectory for its own oscillator comes back
        for (int k = 0; k < ne; ++k) {
            if (p->h_birth[e0 + k] == OW_OFF_TRAJ) p->lead_list_valid = false;
            p->h_birth[e0 + k] = p->trem_clock;
            p->h_lead[e0 + k] = (uint32_t)(e0 + k);
        }
        traj_upload_births(p, e0, ne);
        traj_recount(p);
    } else {
        // the range's engines get identical fresh tremolo states below: cut them out of the groups they shared with engines outside the
        // range (those keep their oscillator), then make the range one group led by its first engine
        trem_split_at_range(p, e0, ne);
        for (int k = 0; k < ne; ++k) p->h_lead[e0 + k] = (uint32_t)e0;
        trem_groups_changed(p);
        p->split_e0 = e0; p->split_ne = ne;
        trem_leader_list(p, e0, ne);
    }
    if (mode == INIT_RESET) {
        // reset() snaps every smoother to ITS target (engine.rs:245-249), and LinearSmoother::set_target stores the target at once
        // (engine.rs:86-99) -- also for a setter call the device has not seen yet because no block was rendered since.  Hand the
        // host targets to the kernel; the retarget requests themselves are dropped by engine_host_reset.
        for (int k = 0; k < ne; ++k) {
            const ow_engine* en = p->engines[e0 + k].get();
            p->h_snap[0 * p->I + e0 + k] = en->depth.target; p->h_snap[1 * p->I + e0 + k] = en->spk.target; p->h_snap[2 * p->I + e0 + k] = en->volume.target;
        }
        for (int r = 0; r < 3; ++r)
            HIP_OK(hipMemcpyAsync(p->d_snap + (size_t)r * p->I + e0, p->h_snap + (size_t)r * p->I + e0, sizeof(double) * ne, hipMemcpyHostToDevice, p->stream));
    }
    // depth0: one value per engine of the range (Tremolo::new(depth)); the kernel takes a scalar, so group equal values
    int i = 0;
    while (i < ne) {
        int j = i + 1;
        while (j < ne && depth0[j] == depth0[i]) ++j;
        owdev::k_chain_init<<<dim3((j - i + 63) / 64), dim3(64), 0, p->stream>>>(p->dK, p->d_cs, p->d_snap, I, e0 + i, j - i, mode, depth0[i]);
        i = j;
    }
    if (p->hc.preamp_kind == OW_PREAMP_MELANGE12)   // DkPreamp::new / reset of the melange adapter: settled state at the chain rate
        owdev::k_mel_init<<<dim3((2 * ne + 63) / 64), dim3(64), 0, p->stream>>>(p->d_cs, p->d_mel_settled, p->d_noise, I, e0, ne);
    if (p->power_amp_kind == OW_POWER_AMP_MELANGE)  // PowerAmp::new_at_sample_rate (new / set_sample_rate) or PowerAmp::reset (reset keeps last_good)
        owdev::k_mpa_init<<<dim3((ne + 63) / 64), dim3(64), 0, p->stream>>>(p->dPa, p->d_pa_settled, p->d_pa, I, e0, ne, mode != INIT_RESET ? 1 : 0);
    if (!on_traj && p->tremolo_kind != OW_TREMOLO_LEGACY_LFO) {   // (legacy-tremolo build: nothing to settle, the LFO starts at phase 0, k_chain_init)
        // the range is one phase group led by e0: Tremolo::new's settle (tremolo.rs:92-102) for that one oscillator
        if (p->sw.trem_cache) {
            trem_settled_rows(p->device, p->hc.os_sr, p->dK, p->dK48, p->d_trem_settled, p->d_zero, p->stream, true);
            owdev::k_trem_load_settled<<<dim3(1), dim3(64), 0, p->stream>>>(p->d_cs, I, e0, p->d_trem_settled);
        } else {
            const long long n_settle = (long long)owhip::sat_u32(p->hc.os_sr * 2.0);
            owdev::k_tremolo_wide<true><<<dim3(1), dim3(64), 0, p->stream>>>(p->dK48, p->d_cs, nullptr, I, 50LL, p->d_leaders, 1);
            owdev::k_tremolo_wide<true><<<dim3(1), dim3(64), 0, p->stream>>>(p->dK, p->d_cs, nullptr, I, n_settle, p->d_leaders, 1);
        }
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(p->stream));   // the tremolo stream picks these rows up next (init-time sync)
}

void upload_consts(ow_pool* p, double sr, int preamp_kind) {
    invalidate_spec(p);
    owhip::build_consts(p->hc, sr, preamp_kind);
    p->hc.tremolo_kind = (uint32_t)p->tremolo_kind;
    OwConsts k48;
    owhip::build_consts(k48, 24000.0, preamp_kind);  // os_sr = 48 kHz -> codegen-rate tremolo matrices
    k48.tremolo_kind = (uint32_t)p->tremolo_kind;
    HIP_OK(hipMemcpyAsync(p->dK, &p->hc, sizeof(OwConsts), hipMemcpyHostToDevice, p->stream));
    HIP_OK(hipMemcpyAsync(p->dK48, &k48, sizeof(OwConsts), hipMemcpyHostToDevice, p->stream));
    // the shared trajectory of this (device, chain rate); the callers (pool_create, set_sample_rate) re-initialise every engine next
    p->traj.reset();
    if (!p->voices_only && p->tremolo_kind == OW_TREMOLO_TWIN_T && p->sw.trem_traj) {
        // a store that cannot be had (no room for it on a crowded device) is not an error: the pool runs one oscillator per phase
        // group, as under OW_TREM_TRAJ=0 -- the same samples
        try { p->traj = traj_acquire(p->device, p->hc, k48, p->sw.trem_cache, p->I); }
        catch (const std::exception& ex) { p->traj.reset(); (void)hipGetLastError(); std::fprintf(stderr, "openwurli-hip: no tremolo trajectory store (%s): per-group oscillators\n", ex.what()); }
    }
    if (!p->traj) { std::fill(p->h_birth.begin(), p->h_birth.end(), OW_OFF_TRAJ); if (p->d_birth) traj_upload_births(p, 0, (int)p->I); p->n_on_traj = 0; }
    if (p->power_amp_kind == OW_POWER_AMP_MELANGE) {
        std::unique_ptr<OwPaConsts> hpa(new OwPaConsts());
        owhip::build_pa_consts(*hpa, p->hc.os_sr);          // the amp runs at the chain rate (engine.rs:207-213)
        HIP_OK(hipMemcpyAsync(p->dPa, hpa.get(), sizeof(OwPaConsts), hipMemcpyHostToDevice, p->stream));
        HIP_OK(hipStreamSynchronize(p->stream));
    }
    HIP_OK(hipStreamSynchronize(p->stream));
}

// Host threads worth starting: the CPU count capped by the cgroup CPU quota (cpu.max "quota period").  A container limited
// to 16 CPUs on a 256-thread host gets throttled for whole scheduler periods when 64 threads burst at once.
static size_t effective_cpus() {
    static const size_t cached = [] {
    size_t n = std::thread::hardware_concurrency();
    if (n == 0) n = 1;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[32] = {0};
        long long period = 0;
        if (std::fscanf(f, "%31s %lld", quota, &period) == 2 && period > 0 && std::strcmp(quota, "max") != 0) {
            const long long q = std::atoll(quota);
            if (q > 0) n = std::min<size_t>(n, (size_t)std::max<long long>(1, q / period));
        }
        std::fclose(f);
    }
    // one process per GPU (torchrun sets LOCAL_WORLD_SIZE): the ranks of a node share the quota, so each takes its share of the
    // threads -- eight ranks bursting 16 threads each into a 16-CPU quota get throttled for whole scheduler periods
    if (const char* lws = std::getenv("LOCAL_WORLD_SIZE")) { const long w = std::atol(lws); if (w > 1) n = std::max<size_t>(1, n / (size_t)w); }
    if (const char* env = std::getenv("OW_HOST_THREADS")) { const long v = std::atol(env); if (v >= 1 && v <= 256) n = (size_t)v; }
    return n;
    }();
    return cached;
}
size_t Workers::host_threads() { return std::min<size_t>(effective_cpus(), OW_MAX_SLICES); }

// see ow_pool::dev_ops_applied
void vm_settle_applied(ow_pool* p) {
    p->dev_ops_applied = false;
    const uint32_t lo = p->applied_lo, hi = p->applied_hi;
    const size_t T = hi - lo >= 16384 ? std::min<size_t>(effective_cpus(), 32) : 1;
    const uint32_t per = (uint32_t)((hi - lo + T - 1) / T);
    auto slice = [&](size_t t) {
        const uint32_t k1 = std::min(hi, lo + (uint32_t)(t + 1) * per);
        for (uint32_t e = lo + (uint32_t)t * per; e < k1; ++e)
            if (p->h_vm[e].n_dev_ops) { p->h_vm[e].n_dev_ops = 0u; p->transient[e] = 1; }
    };
    Workers::get().each(T, slice);
    p->lists_valid = false;
    if (p->d_prev_tr) p->attn_resync = true;      // p->transient moved without the device's copy
}

// ---- which kernels a block gets ------------------------------------------------------------------------------------------------
// Pure functions of the latched switches, the pool's build and the block's size: no pool, no device (ow_test_block_plan and
// tests/test_block_plan_host.py pin the table).  A tri-state switch forces its choice with 0 / 1 and leaves it to the size rule at -1.
static inline bool forced_or(int sw, bool by_size) { return sw >= 0 ? sw == 1 : by_size; }
// OW_TREM_WIDE: pools this small leave SIMDs idle, and the oscillator's serial latency is their block time: four lanes per oscillator
// (ow_trem_wide.h).  (OW_TREM_SERIAL, measured with lane = group at 131 072 oscillators: serialised in front of the voices 31.8 ms per
// block -- voices 12.8, tremolo 9.1 on an empty chip --, overlapped 29.7 ms; the serialised schedule is how the two kernels' own times
// are measured, profiles/.)
static inline bool trem_wide(const Switches& sw, int n_lead) { return forced_or(sw.trem_wide, n_lead <= 16384); }
// OW_PREAMP_WIDE: legacy preamp with a quad per solver state (k_preamp_wide): while the pool leaves most SIMDs empty the kernel's time is
// the serial latency of one sample, which the quad shortens; beyond ~4 096 engines the lane-pair kernel's lower instruction count wins
static inline bool preamp_wide(const Switches& sw, int ne) { return forced_or(sw.preamp_wide, ne <= 4096); }
static inline bool eout_attention(const ow_pool* p, int ne) { return p->d_attn && forced_or(p->sw.eout_attn, ne >= 8192); }

// What launch_chain runs between the voice sums and the preamp rows (PREAMP_*) or the finished rows (CHAIN_*: output stage included).
enum ChainKernel { CHAIN_NONE, CHAIN_ROW_OS_8, CHAIN_ROW_OS_16, CHAIN_ROW_8, CHAIN_ROW_16, CHAIN_FUSED_OS, CHAIN_FUSED, CHAIN_STREAM,
                   PREAMP_MEL_ENG, PREAMP_MEL_COL, PREAMP_MEL_LIT, PREAMP_MEL, PREAMP_WIDE, PREAMP_PAIR, PREAMP_LANE };
enum PostKernel { POST_NONE, POST_MPA, POST_PAIR, POST_OS, POST_BASE };
static const char* const CHAIN_KERNEL_NAME[] = {"", "k_chain_row<true,8>", "k_chain_row<true,16>", "k_chain_row<false,8>", "k_chain_row<false,16>",
                                                "k_chain_fused<true>", "k_chain_fused<false>", "k_chain_stream", "k_preamp_mel_eng", "k_preamp_mel_col",
                                                "k_preamp_mel_lit", "k_preamp_mel", "k_preamp_wide", "k_preamp_pair", "k_preamp"};
static const char* const POST_KERNEL_NAME[] = {"", "k_post_mpa", "k_post<false,true>", "k_post<true>", "k_post<false>"};
static inline bool chain_has_output_stage(ChainKernel k) { return k >= CHAIN_ROW_OS_8 && k <= CHAIN_STREAM; }

ChainKernel choose_chain(const Switches& sw, int preamp_kind, int power_amp_kind, bool oversample, bool ml_sparse_ok, int ne, int L, bool to_pinned_block) {
    if (ne <= 0) return CHAIN_NONE;
    const bool legacy = preamp_kind == OW_PREAMP_LEGACY8 && power_amp_kind == OW_POWER_AMP_BEHAVIORAL;
    const bool wide = preamp_wide(sw, ne);
    // OW_CHAIN_FUSED: the output stage in the same launch behind the quad preamp (k_chain_fused, ow_chain_wide.h): legacy preamp + behavioural
    // power amp only.  (Measured by pool size, tools/probe_row_crossover.py, ms per 512-sample block: 2 048 engines fused 1.99 / two launches
    // 2.37; 4 096 engines 2.97 / 2.59 -- 512 two-wavefront workgroups are the last that find their SIMDs free.)
    if (legacy && forced_or(sw.chain_fused, wide && ne <= 2048)) {
        // OW_CHAIN_ROW: ... with one solver state per row of sixteen lanes (ow_chain_row.h: four preamp wavefronts + the output-stage one per
        // eight engines) while every preamp wavefront has a SIMD of its own; blocks of up to 128 samples keep eight rows in flight
        if (!forced_or(sw.chain_row, ne <= 1024)) return oversample ? CHAIN_FUSED_OS : CHAIN_FUSED;
        if (oversample) return L <= 128 ? CHAIN_ROW_OS_8 : CHAIN_ROW_OS_16;
        return L <= 128 ? CHAIN_ROW_8 : CHAIN_ROW_16;
    }
    // k_chain_stream (ow_chain_stream.h): legacy preamp + behavioural amp, oversampled chain, pools too big for the quad kernels: preamp and
    // output stage alternate per 64-sample chunk in one launch.  Default: when the block goes to a pinned host block (the point of it: no
    // copy trails the launch); OW_CHAIN_STREAM=1 always.
    if (legacy && oversample && !wide && forced_or(sw.chain_stream, to_pinned_block)) return CHAIN_STREAM;
    if (preamp_kind == OW_PREAMP_MELANGE12) {
        // The default kernel re-factors the 12x12 system for every sample whose R_ldr moved, operation for operation like the reference
        // (ow_melange_col.h).  OW_MEL_RANK1=1 selects the rank-one (Sherman-Morrison) kernel instead: mathematically the same, but without the
        // LU's rounding noise, i.e. up to 1.8e-7 V away from the reference while R_ldr moves fast (DESIGN.md deviation 6); OW_MEL_LDS=1 the
        // round-2 literal kernel (S of every engine in LDS; also what a chain rate without the compiled-in sparsity pattern gets);
        // OW_MEL_GENERIC=1 the literal kernels without their fast path.  OW_MEL_ENG=1: lane = engine (ow_melange_eng.h: the rebuild once per
        // engine instead of once per solver state).  Bit-identical; measured 39.2 against 40.4 ms per 131 072-engine block and 45 against
        // 21 ms at 65 536 (one wavefront per SIMD): not the default.
        if (sw.mel_rank1) return PREAMP_MEL;
        if (!ml_sparse_ok || sw.mel_lds) return PREAMP_MEL_LIT;
        return sw.mel_eng ? PREAMP_MEL_ENG : PREAMP_MEL_COL;
    }
    if (wide) return PREAMP_WIDE;
    // OW_PREAMP_PAIR: lane = engine, main and shadow state in one lane: half the wavefronts, two per SIMD from 131 072 engines
    return forced_or(sw.preamp_pair, ne >= 131072) ? PREAMP_PAIR : PREAMP_LANE;
}
PostKernel choose_post(const Switches& sw, int power_amp_kind, bool oversample, int ne, ChainKernel chain) {
    if (ne <= 0 || chain == CHAIN_NONE || chain_has_output_stage(chain)) return POST_NONE;
    if (power_amp_kind == OW_POWER_AMP_MELANGE) return POST_MPA;
    if (!oversample) return POST_BASE;
    return forced_or(sw.post_pair, ne >= 131072) ? POST_PAIR : POST_OS;       // OW_POST_PAIR: lane = engine (two wavefronts per SIMD without it)
}
// Melange power amp: engines dispatched by falling demand (OW_PA_SORT=0: in index order -- the same samples, tested) when the block has more
// engines than k_post_mpa holds on the chip at once: two workgroups of PA_EPB per CU (LDS).  Reads a device attribute: not part of the choice above.
static int power_amp_resident_engines(const ow_pool* p) {
    if (p->sw.pa_sort == 2) return PA_EPB;      // '2': order every block of more than one workgroup (tests)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device) != hipSuccess || cus <= 0) cus = 256;
    return cus * 2 * PA_EPB;
}

// Deal the sounding voices of engines [e0, e0+ne) into wavefront-sized blocks (see ow_kernels.h, "Packed dispatch").
// general = engines whose status after the previous block reported a transient phase, or that receive ops in this block (a note-on
// starts an onset ramp and an attack-noise burst, a note-off a damper phase; nothing else starts one).
void build_voice_lists(ow_pool* p, int e0, int ne) {
    // Big ranges are cut into T engine slices that are packed independently (each slice starts on a block boundary, so at most
    // T - 1 blocks are less full than they could be): pass 1 sizes the three lists of every slice, a prefix sum places them,
    // pass 2 writes the entries.
    const size_t T = ne >= 16384 ? std::min<size_t>(effective_cpus(), 32) : 1;
    // slices start on multiples of 32 engines, like the chain kernels' workgroups
    const int per = (int)(((ne + T - 1) / T + 31) / 32 * 32);
    // entry offsets of a slice in the four lists; h: pass-1 hashes of the slice
    struct Fill { uint32_t s = 0, g = 0, t = 0, a = 0; uint64_t h[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}; };
    Fill size[OW_MAX_SLICES], start[OW_MAX_SLICES + 1];        // T <= 32
    auto pack = [&](size_t t, uint32_t* S, uint32_t* G, uint32_t* Tl, uint32_t* A, Fill& f) {   // a null list: count (and hash) only
        auto pad = [](uint32_t* a, uint32_t& n) { while (n & 63u) { if (a) a[n] = 0xFFFFFFFFu; ++n; } };
        auto put_l = [&](int list, uint32_t* a, uint32_t& n, uint32_t e, uint64_t mask, bool own_block) {
            const uint32_t pc = (uint32_t)__builtin_popcountll(mask);
            if (own_block || (n & 63u) + pc > 64u) pad(a, n);
            if (a) for (uint64_t m = mask; m; m &= m - 1) a[n++] = (e << 6) | (uint32_t)__builtin_ctzll(m);
            else {
                n += pc;
                uint64_t* h = f.h[list];
                h[0] = (h[0] ^ ((uint64_t)e * 0x9E3779B97F4A7C15ull + mask)) * 0xFF51AFD7ED558CCDull;
                h[1] = (h[1] + mask * 0xC2B2AE3D27D4EB4Full + e) * 0x9FB21C651E98DF25ull + (h[1] >> 29);
            }
        };
        auto put = [&](uint32_t* a, uint32_t& n, uint32_t e, uint64_t mask, bool own_block) {
            put_l(&n == &f.s ? 0 : (&n == &f.g ? 1 : (&n == &f.t ? 2 : 3)), a, n, e, mask, own_block);
        };
        const int k1 = std::min(ne, (int)(t + 1) * per);
        for (int k = (int)t * per; k < k1; ++k) {
            const uint32_t e = (uint32_t)(e0 + k);
            const OwEngineArgs& a = p->h_args[e];
            if (a.main_mask) {
                if (p->sw.force_general) put(G, f.g, e, a.main_mask, false);
                else if (p->transient[e] || a.op_count) {
                    // in a transient phase, or about to be (ops pending).  A slot voice only damps while its slot is Releasing (the damper
                    // starts with the release, engine.rs:340-374): an engine without releasing slot voices is inside onset ramps / attack
                    // noise at most -- the attack variant of the steady kernel, 1.2-1.7 x its price instead of the general kernel's 2.6 x
                    const bool damping = (p->h_vm[e].st_mask[OW_VOICE_RELEASING] & a.main_mask) != 0ull;
                    if (!damping && p->sw.voice_attack) put(A, f.a, e, a.main_mask, false);
                    else put(G, f.g, e, a.main_mask, false);
                } else put(S, f.s, e, a.main_mask, false);
            }
            if (a.steal_mask) put(Tl, f.t, e, a.steal_mask, true);   // one engine per block: the crossfade early-out is per engine
        }
        pad(S, f.s); pad(G, f.g); pad(Tl, f.t); pad(A, f.a);
    };
    auto pass1 = [&](size_t t) { pack(t, nullptr, nullptr, nullptr, nullptr, size[t]); };
    Workers::get().each(T, pass1);
    for (size_t t = 0; t < T; ++t) { start[t + 1].s = start[t].s + size[t].s; start[t + 1].g = start[t].g + size[t].g; start[t + 1].t = start[t].t + size[t].t; start[t + 1].a = start[t].a + size[t].a; }
    const uint32_t fs = start[T].s, fg = start[T].g, fl = start[T].t, fa = start[T].a;
    // a list whose (engine, mask) sequence, slices and range are the ones its device copy was packed from is left alone: after a
    // whole-pool re-strike the attack and steal lists of the 128-sample sub-block serve the next block(s) as they are
    ow_pool::VoiceList* const vls[4] = {&p->vl_steady, &p->vl_general, &p->vl_steal, &p->vl_attack};
    const uint32_t fill[4] = {fs, fg, fl, fa};
    bool keep[4];
    for (int l = 0; l < 4; ++l) {
        uint64_t sig[3] = {0x243F6A8885A308D3ull ^ (uint64_t)T, 0x13198A2E03707344ull ^ (uint64_t)per, ((uint64_t)(uint32_t)e0 << 32) | (uint32_t)ne};
        for (size_t t = 0; t < T; ++t) {
            const uint32_t n_t = l == 0 ? size[t].s : (l == 1 ? size[t].g : (l == 2 ? size[t].t : size[t].a));
            sig[0] = (sig[0] * 0x100000001B3ull) ^ size[t].h[l][0] ^ ((uint64_t)n_t << 17);
            sig[1] = (sig[1] * 0xD6E8FEB86659FD93ull) + size[t].h[l][1] + n_t;
        }
        ow_pool::VoiceList& vl = *vls[l];
        keep[l] = fill[l] != 0 && vl.sig_valid && vl.n_blocks == fill[l] / 64 && vl.sig[0] == sig[0] && vl.sig[1] == sig[1] && vl.sig[2] == sig[2];
        // the signature only stands for the DEVICE copy once that copy has been enqueued (below): if anything throws in between, no list keeps
        // a signature whose upload never happened
        vl.sig[0] = sig[0]; vl.sig[1] = sig[1]; vl.sig[2] = sig[2]; vl.sig_valid = keep[l];
        vl.n_blocks = fill[l] / 64;
    }
    auto pass2 = [&](size_t t) {
        Fill f;   // slice-local counters: the slice regions start on block boundaries, so padding decisions match pass 1
        pack(t, keep[0] ? nullptr : p->vl_steady.h + start[t].s, keep[1] ? nullptr : p->vl_general.h + start[t].g,
             keep[2] ? nullptr : p->vl_steal.h + start[t].t, keep[3] ? nullptr : p->vl_attack.h + start[t].a, f);
    };
    if (!((keep[0] || !fs) && (keep[1] || !fg) && (keep[2] || !fl) && (keep[3] || !fa))) Workers::get().each(T, pass2);
    hipStream_t st = p->stream;
    for (int l = 0; l < 4; ++l)
        if (fill[l] && !keep[l]) {
            HIP_OK(hipMemcpyAsync(vls[l]->d, vls[l]->h, sizeof(uint32_t) * fill[l], hipMemcpyHostToDevice, st));
            vls[l]->sig_valid = true;
        }
    p->lists_e0 = e0; p->lists_ne = ne;
}

// one oscillator per phase group of the range (p->d_leaders, trem_leader_list)
static void launch_tremolo(ow_pool* p, hipStream_t tt, double* rbuf, int n_os) {
    const int I = (int)p->I, nl = p->n_lead;
    if (p->tremolo_kind == OW_TREMOLO_LEGACY_LFO) owdev::k_tremolo_lfo<<<dim3((nl + 63) / 64), dim3(64), 0, tt>>>(p->dK, p->d_cs, rbuf, I, (long long)n_os, p->d_leaders, nl, 0LL);
    else if (trem_wide(p->sw, nl)) owdev::k_tremolo_wide<false><<<dim3((nl + 15) / 16), dim3(64), 0, tt>>>(p->dK, p->d_cs, rbuf, I, (long long)n_os, p->d_leaders, nl);
    else owdev::k_tremolo<<<dim3((nl + 63) / 64), dim3(64), 0, tt>>>(p->dK, p->d_cs, rbuf, I, n_os, p->d_leaders, nl);
}

// ---- one block: the phases of render_range, in the order of DESIGN.md 4.1 ----------------------------------------------------------
struct Block {
    int e0 = 0, ne = 0, L = 0, n_os = 0;     // engines [e0, e0+ne), samples at the host rate / at the chain rate
    size_t len = 0;
    bool whole = false;                      // the whole pool
    bool chain = false;                      // false: a voices-only pool (ow_render_note) stops at the voice sums
    float* out_host = nullptr;               // rows go to out_host[(e - e0) * out_stride] ...
    size_t out_stride = 0;
    float* out_direct = nullptr;             // ... written by the output stage itself: the target's device address when it lies in a pinned block of ow_host_alloc
    owdev::OwTremSrc tsrc{nullptr, nullptr, nullptr, nullptr};   // where the chain kernels read this block's R_ldr
};

// min over the range's engines on the trajectory of birth[e]
static long long range_min_birth(const ow_pool* p, int e0, int ne) {
    long long mn = p->trem_clock;
    for (int k = 0; k < ne; ++k) if (p->h_birth[e0 + k] != OW_OFF_TRAJ) mn = std::min(mn, p->h_birth[e0 + k]);
    return mn;
}
// Engines on the shared trajectory read r_ldr[t .. t + n_os) at their own t = clock - birth: make the store reach the oldest one's block
// (nothing to do unless this pool holds the process's oldest engine), plus one block ahead on the store's own stream.  Returns the event
// the chain has to wait for (nullptr: the samples are there).
static hipEvent_t traj_cover_block(ow_pool* p, Block& b) {
    const int e0 = b.e0, ne = b.ne, n_os = b.n_os;
    long long mn = b.whole ? p->min_birth : range_min_birth(p, e0, ne);
    if ((size_t)(p->trem_clock - mn) + (size_t)n_os > p->traj->cap_max) { trem_evict(p, e0, ne, n_os); mn = range_min_birth(p, e0, ne); }
    size_t need = (size_t)(p->trem_clock - mn) + (size_t)n_os;
    bool ask = false, must = false, feed = false;
    {
        std::lock_guard<std::mutex> lk(p->traj->mu);
        must = need > p->traj->cap;                        // the helper did not get there in time (it is asked a lead + 30 s before)
        if (!must && p->traj->wants_growth(need)) { p->traj->grow_requested = true; ask = true; }
    }
    if (must) {                                            // cold: allocates on this thread, like the reference's buffer auto-grow
        try { p->traj->grow_to(std::max(need, p->traj->cap * 2)); }
        catch (const std::exception& ex) {
            // no memory for a longer store (a crowded device): it stays as long as it is -- as the helper thread's failure path decides --
            // and the engines that have outgrown it continue on oscillators of their own instead of retrying the allocation every block
            (void)hipGetLastError();
            { std::lock_guard<std::mutex> lk(p->traj->mu); p->traj->cap_max = p->traj->cap; p->traj->grow_requested = false; }
            std::fprintf(stderr, "openwurli-hip: tremolo trajectory store stays at %zu samples (%s)\n", p->traj->cap, ex.what());
            trem_evict(p, e0, ne, n_os);
            need = (size_t)(p->trem_clock - range_min_birth(p, e0, ne)) + (size_t)n_os;
        }
    }
    if (ask) traj_grower().ask(p->traj);
    hipEvent_t ready;
    {
        std::lock_guard<std::mutex> lk(p->traj->mu);
        ready = p->traj->cover(need, (size_t)n_os, p->I < 4096 ? p->traj->lead : 0, &feed);
        b.tsrc.traj = p->traj->d_r + p->trem_clock;        // (under the lock: a growth swaps the buffer)
    }
    if (feed) traj_grower().feed(p->traj);
    return ready;
}

// Engines with an oscillator of their own (phase groups): this block's R_ldr is already there if the block-ahead speculation hit; then
// the next block's, speculatively.  Returns the half of rbuf (index of ev_trem) the chain has to wait for, -1: no oscillator ran.
static int trem_block(ow_pool* p, Block& b) {
    const int e0 = b.e0, ne = b.ne, n_os = b.n_os;
    hipStream_t tt = p->stream_trem;
    const size_t rb_half = (size_t)2 * p->Lcap * p->I;
    const bool hit = b.chain && p->spec.valid && p->spec.e0 == e0 && p->spec.ne == ne && p->spec.n_os == n_os;
    if (p->spec.valid && !hit) {   // mis-speculated (different block length / engine range): roll the oscillator back
        HIP_OK(hipMemcpyAsync(p->d_cs, p->d_trem_backup, sizeof(double) * 18 * p->I, hipMemcpyDeviceToDevice, tt));
        p->spec.valid = false;
    }
    if (b.chain) {
        // a sub-range advances on its own: its engines leave the phase groups they share with engines outside it (no-op for the whole pool
        // and for a range that was just initialised); then the oscillators to run are the group leaders inside the range
        if (p->n_on_traj < p->I) trem_split_at_range(p, e0, ne);
        trem_leader_list(p, e0, ne);
        if (hit) {
            p->rb_cur ^= 1;            // the half the speculation filled
        } else if (p->n_lead > 0) {
            launch_tremolo(p, tt, p->d_rbuf + p->rb_cur * rb_half, n_os);
            HIP_OK(hipEventRecord(p->ev_trem[p->rb_cur], tt));
        }
    }
    const bool own_osc = b.chain && p->n_lead > 0;
    b.tsrc.rbuf = p->d_rbuf + p->rb_cur * rb_half;
    // The oscillators of the NEXT block go first: they need nothing from the host, so they run while the host packs ops and voice lists,
    // and their wavefronts (one per SIMD at 65 536 of them) are resident before the voice kernel fills the rest.  (k_apply_ops is
    // register-capped so that it fits beside them.)  Back up the oscillator rows, then run ahead into the other half.
    if (own_osc) {
        const int nxt = p->rb_cur ^ 1;
        HIP_OK(hipMemcpyAsync(p->d_trem_backup, p->d_cs, sizeof(double) * 18 * p->I, hipMemcpyDeviceToDevice, tt));
        if (p->profiling) HIP_OK(hipEventRecord(p->ev[6], tt));
        launch_tremolo(p, tt, p->d_rbuf + nxt * rb_half, n_os);
        if (p->profiling) HIP_OK(hipEventRecord(p->ev[7], tt));
        HIP_OK(hipEventRecord(p->ev_trem[nxt], tt));
        p->spec.valid = true; p->spec.e0 = e0; p->spec.ne = ne; p->spec.n_os = n_os;
    } else if (b.chain && p->profiling) { HIP_OK(hipEventRecord(p->ev[6], tt)); HIP_OK(hipEventRecord(p->ev[7], tt)); }
    // OW_TREM_SERIAL=1 (measurement switch, see trem_wide): the voices of this block wait for the block-ahead oscillators
    if (own_osc && p->sw.trem_serial) HIP_OK(hipStreamWaitEvent(p->stream, p->ev_trem[p->rb_cur ^ 1], 0));
    return own_osc || hit ? p->rb_cur : -1;
}

// Per-engine args + ops: only engines whose host state changed are touched (the rest keep their uploaded args; a steady-state step of
// a large pool does no per-engine host work here).  Large pools split the range over host threads: slice t counts its pending ops, a
// prefix sum places the slices in h_ops, then every slice packs its own engines (a 65536-engine re-strike moves ~8 M ops; one thread
// took ~100 ms for it).
struct Packed { bool any_dirty = false; size_t n_ops = 0; uint32_t n_act = 0; bool any_main = false, any_steal = false; };
static Packed pack_args_and_ops(ow_pool* p, const Block& b) {
    const int e0 = b.e0, ne = b.ne;
    Packed r;
    // A steady block of the whole pool -- no engine touched since the last one -- skips the per-engine scans below (0.2 ms at 131 072)
    const bool untouched = b.whole && !__atomic_load_n(&p->dirty_any, __ATOMIC_RELAXED) && !p->args_stale && p->any_cache_valid;
    if (b.whole) __atomic_store_n(&p->dirty_any, (uint8_t)0, __ATOMIC_RELAXED);   // engines touched from here on belong to the next block
    size_t n_dirty = 0;
    if (!untouched) for (int k = 0; k < ne; ++k) n_dirty += p->dirty[e0 + k];     // dirty[] holds 0/1
    size_t T = (n_dirty >= 4096) ? std::min<size_t>(effective_cpus(), 32) : 1;
    const int per = (int)((ne + T - 1) / T);
    size_t cnt[OW_MAX_SLICES + 1] = {0};
    uint8_t dirty_t[OW_MAX_SLICES] = {0};
    auto count_slice = [&](size_t t) {
        size_t c = 0; uint8_t d = 0;
        const int k1 = std::min(ne, (int)(t + 1) * per);
        for (int k = (int)t * per; k < k1; ++k) {
            if (!p->dirty[e0 + k]) continue;
            d = 1;
            c += p->engines[e0 + k]->ops.size();
        }
        cnt[t + 1] = c; dirty_t[t] = d;
    };
    if (!untouched) Workers::get().each(T, count_slice);
    for (size_t t = 0; t < T; ++t) { r.any_dirty = r.any_dirty || dirty_t[t]; cnt[t + 1] += cnt[t]; }
    r.n_ops = cnt[T];
    ensure_ops_capacity(p, r.n_ops);
    if (r.any_dirty || p->args_stale) {
        auto pack_slice = [&](size_t t) {
            size_t op_pos = cnt[t];
            const int k1 = std::min(ne, (int)(t + 1) * per);
            for (int k = (int)t * per; k < k1; ++k) {
                OwEngineArgs& a = p->h_args[e0 + k];
                if (!p->dirty[e0 + k]) {
                    if (a.op_count || a.set_flags) { a.op_count = 0; a.set_flags = 0; }
                    continue;
                }
                ow_engine* en = p->engines[e0 + k].get();
                // engine.rs:471-473: a Free slot renders nothing unless it still carries a steal voice
                a.main_mask = en->vm->main_mask; a.steal_mask = en->vm->steal_mask;
                a.noise_on = en->noise_on ? 1u : 0u; a.thermal_gain = en->thermal_gain;
                a.pa_flags = en->rail_sag ? 1u : 0u;
                a.op_begin = (uint32_t)op_pos;
                a.op_count = (uint32_t)en->ops.size();
                if (!en->ops.empty()) std::memcpy(p->h_ops + op_pos, en->ops.data(), sizeof(OwOp) * en->ops.size());
                if (const uint32_t nd = en->vm->n_dev_ops) {
                    // the engine's queue was (also) written on the device (k_vm_events): it stays where it is; ops the host queued
                    // behind it are appended there after the upload (rare: single events between a burst and the render)
                    if (!en->ops.empty()) {
                        const uint32_t room = OW_VM_OPS_MAX - nd, nh = (uint32_t)std::min<size_t>(en->ops.size(), room);
                        if (nh < en->ops.size()) {
                            // Only with OW_MIDI_APPLY_EARLY=0 (a burst's queue left for this render), a burst that filled the engine's 192
                            // entries and single events behind it: the tail does not fit the device queue.  Counted and reported -- the
                            // default schedule applies a burst's queue inside ow_pool_midi and never gets here with nd != 0.
                            const uint64_t lost = g_ops_dropped.fetch_add(en->ops.size() - nh) + (en->ops.size() - nh);
                            if (lost == en->ops.size() - nh)
                                std::fprintf(stderr, "openwurli-hip: engine %zu: %zu queued slot ops do not fit behind a device-side MIDI burst (OW_MIDI_APPLY_EARLY=0) and are dropped\n",
                                             (size_t)(e0 + k), en->ops.size() - nh);
                        }
                        std::lock_guard<std::mutex> lk(p->op_tails_mu);
                        p->op_tails.push_back({(uint32_t)op_pos, (uint32_t)((e0 + k) * OW_VM_OPS_MAX) + nd, nh});
                        a.op_count = nd + nh;
                    } else a.op_count = nd;
                    a.op_begin = 0x80000000u | (uint32_t)((e0 + k) * OW_VM_OPS_MAX);
                    en->vm->n_dev_ops = 0;
                    if (!p->vm_host_dirty) p->vm_host_dirty = 1;
                }
                op_pos += en->ops.size();
                if (!en->ops.empty()) { en->ops.clear(); __atomic_fetch_sub(&p->host_ops_any, 1u, __ATOMIC_RELAXED); }
                a.set_flags = 0;
                if (en->depth.pending) { a.set_flags |= 1u; a.depth_target = en->depth.pending_value; en->depth.pending = false; }
                if (en->spk.pending)   { a.set_flags |= 2u; a.spk_target = en->spk.pending_value;     en->spk.pending = false; }
                if (en->volume.pending){ a.set_flags |= 4u; a.vol_target = en->volume.pending_value;  en->volume.pending = false; }
                p->dirty[e0 + k] = 0;
            }
        };
        Workers::get().each(T, pack_slice);
    }
    // One parallel pass over the args of the range (13 MB at 131 072 engines: ~1 ms per walk on one thread, and the blocks after a
    // whole-pool re-strike used to take two): does any engine sound, and which engines have ops (slice t lists its own into its part of
    // h_op_engines; the parts are closed up below).
    r.any_main = p->any_main_c; r.any_steal = p->any_steal_c;
    if (!untouched) {
        const size_t TA = ne >= 16384 ? std::min<size_t>(effective_cpus(), 32) : 1;
        const int per_a = (int)((ne + TA - 1) / TA);
        uint32_t act_n[OW_MAX_SLICES] = {0};
        uint8_t any_m[OW_MAX_SLICES] = {0}, any_s[OW_MAX_SLICES] = {0};
        auto scan_slice = [&](size_t t) {
            const int k0 = (int)t * per_a, k1 = std::min(ne, (int)(t + 1) * per_a);
            uint32_t n = 0; uint8_t m = 0, sl = 0;
            uint32_t* dst = p->h_op_engines + k0;
            for (int k = k0; k < k1; ++k) {
                const OwEngineArgs& a = p->h_args[e0 + k];
                m |= a.main_mask != 0; sl |= a.steal_mask != 0;
                if (a.op_count) dst[n++] = (uint32_t)(e0 + k);
            }
            act_n[t] = n; any_m[t] = m; any_s[t] = sl;
        };
        Workers::get().each(TA, scan_slice);
        r.any_main = false; r.any_steal = false;
        for (size_t t = 0; t < TA; ++t) {
            r.any_main |= any_m[t] != 0; r.any_steal |= any_s[t] != 0;
            if (act_n[t] && r.n_act != (uint32_t)(t * per_a)) std::memmove(p->h_op_engines + r.n_act, p->h_op_engines + t * per_a, sizeof(uint32_t) * act_n[t]);
            r.n_act += act_n[t];
        }
        if (b.whole) { p->any_main_c = r.any_main; p->any_steal_c = r.any_steal; p->any_cache_valid = true; }
    }
    return r;
}

static void upload_and_apply_ops(ow_pool* p, const Block& b, const Packed& pk) {
    const int e0 = b.e0, ne = b.ne;
    hipStream_t st = p->stream;
    // args carry one-shot fields (ops, setter targets): upload when anything changed, and once more afterwards to clear them
    if (pk.any_dirty || p->args_stale) {
        HIP_OK(hipMemcpyAsync(p->d_args + e0, p->h_args + e0, sizeof(OwEngineArgs) * ne, hipMemcpyHostToDevice, st));
        p->args_stale = pk.any_dirty;
    }
    HIP_OK(hipMemsetAsync(p->d_eout + e0, 0, sizeof(OwEngineOut) * ne, st));
    if (p->profiling) HIP_OK(hipEventRecord(p->ev[0], st));
    if (pk.n_ops || p->dev_ops_pending) {
        if (pk.n_ops) HIP_OK(hipMemcpyAsync(p->d_ops, p->h_ops, sizeof(OwOp) * pk.n_ops, hipMemcpyHostToDevice, st));
        for (const ow_pool::OpTail& t : p->op_tails)
            HIP_OK(hipMemcpyAsync(p->d_ops_fix + t.dst, p->d_ops + t.src, sizeof(OwOp) * t.n, hipMemcpyDeviceToDevice, st));
        p->op_tails.clear();
        // one block per engine that has ops (listed by the scan of pack_args_and_ops; an untouched range has none)
        if (pk.n_act) {
            HIP_OK(hipMemcpyAsync(p->d_op_engines, p->h_op_engines, sizeof(uint32_t) * pk.n_act, hipMemcpyHostToDevice, st));
            owdev::k_apply_ops<<<dim3(pk.n_act), dim3(64), 0, st>>>(p->dK, p->d_nt, p->d_vrec, p->d_args, p->d_ops, p->d_op_engines, p->d_ops_fix);
        }
        if (b.whole) p->dev_ops_pending = false;
    }
    if (p->profiling) HIP_OK(hipEventRecord(p->ev[1], st));
}

// The voice kernels over the packed lists (build_voice_lists).  Returns whether a steady launch will report its jitter grids (d_skew_seen).
static bool launch_voices(ow_pool* p, const Block& b) {
    const int I = (int)p->I, L = b.L, Lcap = (int)p->Lcap;
    hipStream_t s = p->stream;
    const unsigned bs = p->vl_steady.n_blocks, bg = p->vl_general.n_blocks, bt = p->vl_steal.n_blocks, ba = p->vl_attack.n_blocks;
    if (ba) owdev::k_voice_steady<false, 1><<<dim3(ba), dim3(64), 0, s>>>(p->dK, p->d_vrec, p->vl_attack.d, p->d_sum, p->d_eout, I, L, Lcap, nullptr);
    if (bs) {
        // voices on more than one jitter grid in some wavefront of the previous steady launch: the skewed variant (same samples)
        if (p->sw.voice_skew && p->skew_next)
            owdev::k_voice_steady<true><<<dim3(bs), dim3(64), 0, s>>>(p->dK, p->d_vrec, p->vl_steady.d, p->d_sum, p->d_eout, I, L, Lcap, p->d_skew_seen);
        else
            owdev::k_voice_steady<false><<<dim3(bs), dim3(64), 0, s>>>(p->dK, p->d_vrec, p->vl_steady.d, p->d_sum, p->d_eout, I, L, Lcap, p->d_skew_seen);
    }
    if (bg) {
        // the release variant of the steady kernel takes the blocks whose voices are all past onset and noise (each block decides by
        // itself, voice_steal_takes: what is left in this list are engines with a damping voice); k_voice (pass | 4) renders the others
        const bool rel = p->sw.voice_release && !p->sw.force_general;      // (force_general measures k_voice itself)
        if (rel) owdev::k_voice_steady<false, 3><<<dim3(bg), dim3(64), 0, s>>>(p->dK, p->d_vrec, p->vl_general.d, p->d_sum, p->d_eout, I, L, Lcap, nullptr);
        owdev::k_voice<<<dim3(bg), dim3(64), 0, s>>>(p->dK, p->d_vrec, p->vl_general.d, p->d_sum, p->d_eout, I, L, Lcap, rel ? 4 : 0);
    }
    if (bt) {
        // the steal variant of the steady kernel takes the engines whose steal voices are past onset and noise (each block decides
        // by itself, voice_steal_takes); k_voice (pass | 4) renders the others
        if (p->sw.voice_steal) owdev::k_voice_steady<false, 2><<<dim3(bt), dim3(64), 0, s>>>(p->dK, p->d_vrec, p->vl_steal.d, p->d_sum, p->d_eout, I, L, Lcap, nullptr);
        owdev::k_voice<<<dim3(bt), dim3(64), 0, s>>>(p->dK, p->d_vrec, p->vl_steal.d, p->d_sum, p->d_eout, I, L, Lcap, p->sw.voice_steal ? 5 : 1);
    }
    return bs != 0;
}

// Voice sums -> preamp rows, or (CHAIN_*) -> finished rows.  Returns whether the rows went straight into the caller's pinned block.
static bool launch_chain(ow_pool* p, const Block& b, ChainKernel kernel) {
    const int I = (int)p->I, L = b.L, Lcap = (int)p->Lcap, e0 = b.e0, ne = b.ne;
    hipStream_t s = p->stream;
    const owdev::OwTremSrc& tsrc = b.tsrc;
    const dim3 per8((ne + 7) / 8), per32((ne + 31) / 32), per64((ne + 63) / 64), per512((ne + 511) / 512);   // per512: eight wavefronts of 64 engines (ow_wave_turns.h)
    const int generic = p->sw.mel_generic ? 1 : 0;
    switch (kernel) {
    case CHAIN_NONE: break;
    case CHAIN_ROW_OS_8: owdev::k_chain_row<true, 8><<<per8, dim3(320), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_out, I, L, Lcap, L, e0, ne); break;
    case CHAIN_ROW_OS_16: owdev::k_chain_row<true, 16><<<per8, dim3(320), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_out, I, L, Lcap, L, e0, ne); break;
    case CHAIN_ROW_8: owdev::k_chain_row<false, 8><<<per8, dim3(320), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_out, I, L, Lcap, L, e0, ne); break;
    case CHAIN_ROW_16: owdev::k_chain_row<false, 16><<<per8, dim3(320), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_out, I, L, Lcap, L, e0, ne); break;
    case CHAIN_FUSED_OS: owdev::k_chain_fused<true><<<per8, dim3(128), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_out, I, L, Lcap, L, e0, ne); break;
    case CHAIN_FUSED: owdev::k_chain_fused<false><<<per8, dim3(128), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_out, I, L, Lcap, L, e0, ne); break;
    case CHAIN_STREAM:
        owdev::k_chain_stream<<<per32, dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_out, I, L, Lcap, L, e0, ne, b.out_direct, b.out_stride);
        return b.out_direct != nullptr;
    case PREAMP_MEL_ENG:
        owdev::k_preamp_mel_eng<<<per64, dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_mel_settled, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_noise, I, L, Lcap, e0, ne, generic, p->d_mel_lu, p->mel_lu_ld);
        break;
    case PREAMP_MEL_COL:
        owdev::k_preamp_mel_col<<<per32, dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_mel_settled, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_noise, I, L, Lcap, e0, ne, generic, p->d_mel_lu, p->mel_lu_ld);
        break;
    case PREAMP_MEL_LIT:
        owdev::k_preamp_mel_lit<<<per32, dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_mel_settled, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_noise, I, L, Lcap, e0, ne, generic, p->d_mel_lu);
        break;
    case PREAMP_MEL: owdev::k_preamp_mel<<<per32, dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_mel_settled, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, p->d_noise, I, L, Lcap, e0, ne); break;
    case PREAMP_WIDE: owdev::k_preamp_wide<<<per8, dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, I, L, Lcap, e0, ne); break;
    case PREAMP_PAIR: owdev::k_preamp_pair<<<per512, dim3(512), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, I, L, Lcap, e0, ne); break;
    case PREAMP_LANE: owdev::k_preamp<<<per32, dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_sum, tsrc, p->d_pre, I, L, Lcap, e0, ne); break;
    }
    return false;
}

// Preamp rows -> finished rows.  Returns whether they went straight into the caller's pinned block.
static bool launch_output_stage(ow_pool* p, const Block& b, PostKernel kernel) {
    const int I = (int)p->I, L = b.L, e0 = b.e0, ne = b.ne;
    hipStream_t s = p->stream;
    switch (kernel) {
    case POST_NONE: return false;                // voice sums only / the output stage ran inside the chain kernel
    case POST_MPA: {
        // more engines than the chip holds at once: dispatch them by falling demand of their last block (see k_post_mpa); below that every
        // wavefront is resident from the start, the block lasts as long as its slowest engine and the order cannot matter
        const bool ordered = p->sw.pa_sort != 0 && ne > power_amp_resident_engines(p);
        if (ordered) {
            const uint32_t total = (uint32_t)b.n_os;
            HIP_OK(hipMemsetAsync(p->d_pa_hist, 0, sizeof(uint32_t) * PA_ORDER_CLASSES, s));
            owdev::k_pa_order_hist<<<dim3((ne + 255) / 256), dim3(256), 0, s>>>(p->d_pa_demand, e0, ne, total, p->d_pa_hist);
            owdev::k_pa_order_scan<<<dim3(1), dim3(PA_ORDER_CLASSES), 0, s>>>(p->d_pa_hist);
            owdev::k_pa_order_scatter<<<dim3((ne + 255) / 256), dim3(256), 0, s>>>(p->d_pa_demand, e0, ne, total, p->d_pa_hist, p->d_pa_order);
        }
        owdev::k_post_mpa<<<dim3((ne + PA_EPB - 1) / PA_EPB), dim3(PA_WPB * 64), 0, s>>>(p->dK, p->dPa, p->d_pa_settled, p->d_cs, p->d_pa, p->d_args, p->d_eout, p->d_pre, p->d_out,
                                                                                     p->d_pa_tap, I, L, L, e0, ne, ordered ? p->d_pa_order : nullptr, p->d_pa_demand);
        return false;
    }
    case POST_PAIR: owdev::k_post<false, true><<<dim3((ne + 511) / 512), dim3(512), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_pre, p->d_out, I, L, L, e0, ne, b.out_direct, b.out_stride); break;
    case POST_OS: owdev::k_post<true><<<dim3((ne + 31) / 32), dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_pre, p->d_out, I, L, L, e0, ne, b.out_direct, b.out_stride); break;
    case POST_BASE: owdev::k_post<false><<<dim3((ne + 63) / 64), dim3(64), 0, s>>>(p->dK, p->d_cs, p->d_args, p->d_eout, p->d_pre, p->d_out, I, L, L, e0, ne, b.out_direct, b.out_stride); break;
    }
    return b.out_direct != nullptr;
}

// the block's rows to the caller's host buffer, unless the output stage stored them there itself
static void deliver_rows(ow_pool* p, const Block& b) {
    const float* src = p->d_out + (size_t)b.e0 * b.len;
    if (b.out_stride == b.len) HIP_OK(hipMemcpyAsync(b.out_host, src, sizeof(float) * b.len * (size_t)b.ne, hipMemcpyDeviceToHost, p->stream));
    else HIP_OK(hipMemcpy2DAsync(b.out_host, b.out_stride * sizeof(float), src, b.len * sizeof(float), b.len * sizeof(float), (size_t)b.ne, hipMemcpyDeviceToHost, p->stream));
}

// the trajectory clock, the steady launch's report and the block's status on their way to the host (post_render_host reads them after the sync)
static void finish_block(ow_pool* p, const Block& b, bool steady_launched) {
    const int e0 = b.e0, ne = b.ne, n_os = b.n_os;
    hipStream_t st = p->stream;
    if (b.chain && p->traj) {          // the engines of the range are n_os samples further along the trajectory
        if (b.whole) p->trem_clock += n_os;
        else {
            for (int k = 0; k < ne; ++k) if (p->h_birth[e0 + k] != OW_OFF_TRAJ) { p->h_birth[e0 + k] -= n_os; p->min_birth = std::min(p->min_birth, p->h_birth[e0 + k]); }
            owdev::k_trem_birth_shift<<<dim3((ne + 255) / 256), dim3(256), 0, st>>>(p->d_birth, e0, ne, -(long long)n_os);
        }
    }
    p->last_n_os = n_os;
    HIP_OK(hipGetLastError());
    if (steady_launched) {
        HIP_OK(hipMemcpyAsync(p->h_skew_seen, p->d_skew_seen, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        p->skew_pending = true;
    }
    if (eout_attention(p, ne)) {
        if (p->attn_resync) {
            std::memcpy(p->h_prev_tr, p->transient.data(), p->I);
            HIP_OK(hipMemcpyAsync(p->d_prev_tr, p->h_prev_tr, p->I, hipMemcpyHostToDevice, st));
            p->attn_resync = false;
        }
        owdev::k_eout_attention<<<dim3((ne + 255) / 256), dim3(256), 0, st>>>(p->d_eout, p->d_args, p->d_prev_tr, e0, ne, p->d_attn);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(p->h_attn, p->d_attn, sizeof(uint64_t) * ((ne + 63) / 64), hipMemcpyDeviceToHost, st));
        p->attn_pending = true;
    } else {
        HIP_OK(hipMemcpyAsync(p->h_eout + e0, p->d_eout + e0, sizeof(OwEngineOut) * ne, hipMemcpyDeviceToHost, st));
        p->attn_pending = false;
    }
}

// One render of `len` samples for engines [e0, e0+ne).  with_voices=false skips the voice kernels
// (warm-up of engines whose voices were just freed).
// out_host != nullptr: rows [e0, e0+ne) of the block are copied to out_host[(e - e0) * out_stride].
void render_range(ow_pool* p, int e0, int ne, size_t len, bool with_voices, float* out_host = nullptr, size_t out_stride = 0) {
    if (len > p->Lcap) { HIP_OK(hipStreamSynchronize(p->stream)); alloc_stream_buffers(p, len); }  // auto-grow, engine.rs:430 (also after a grow that failed: Lcap 0)
    p->out_ld = len;
    hipStream_t st = p->stream;
    auto profile_mark = [&](int i) { if (p->profiling) HIP_OK(hipEventRecord(p->ev_stage[i], st)); };
    vm_wait_download(p);                     // a burst applied on the device: the host's copy of the voice-pool states is complete from here on
    Block b;
    b.e0 = e0; b.ne = ne; b.len = len; b.L = (int)len; b.n_os = b.L * (p->hc.oversample ? 2 : 1);
    b.whole = e0 == 0 && ne == (int)p->I;
    b.chain = !p->voices_only;
    b.out_host = out_host; b.out_stride = out_stride;
    b.tsrc = owdev::OwTremSrc{nullptr, p->d_lead, nullptr, p->d_birth};
    // ---- tremolo: CdS cell resistance of this block, from the shared trajectory and / or the pool's own oscillators
    const hipEvent_t traj_ready = b.chain && p->traj ? traj_cover_block(p, b) : nullptr;
    const int trem_half = trem_block(p, b);
    // ---- host state of the engines -> device
    const Packed pk = pack_args_and_ops(p, b);
    upload_and_apply_ops(p, b, pk);
    // ---- voices
    const bool voices = with_voices && (pk.any_main || pk.any_steal);
    if (voices) {
        // the lists depend on masks, pending ops (any_dirty) and the transient flags of the previous block (post_render_host)
        if (!p->lists_valid || pk.any_dirty || p->lists_e0 != e0 || p->lists_ne != ne) build_voice_lists(p, e0, ne);
        p->lists_valid = !pk.any_dirty;     // engines with ops were classified "general" for this block only
        if (p->vl_steady.n_blocks) HIP_OK(hipMemsetAsync(p->d_skew_seen, 0, sizeof(uint32_t), st));
    }
    // A target inside a pinned block of ow_host_alloc is written by the output stage itself (it is mapped into the device's address space)
    if (out_host && p->sw.out_direct != 0 && out_stride >= len && ne > 0)
        b.out_direct = (float*)host_block_device_ptr(out_host, sizeof(float) * ((size_t)(ne - 1) * out_stride + len));
    profile_mark(0);
    const bool steady_launched = voices && launch_voices(p, b);
    profile_mark(1);
    // ---- chain: preamp and output stage, once this block's R_ldr is there
    if (trem_half >= 0) HIP_OK(hipStreamWaitEvent(st, p->ev_trem[trem_half], 0));
    if (traj_ready) HIP_OK(hipStreamWaitEvent(st, traj_ready, 0));
    profile_mark(2);
    const ChainKernel chain = !b.chain ? CHAIN_NONE
        : choose_chain(p->sw, (int)p->hc.preamp_kind, p->power_amp_kind, p->hc.oversample != 0, p->hc.ml_sparse_ok != 0, ne, b.L, b.out_direct != nullptr);
    bool delivered = launch_chain(p, b, chain);
    profile_mark(3);
    delivered |= launch_output_stage(p, b, choose_post(p->sw, p->power_amp_kind, p->hc.oversample != 0, ne, chain));
    profile_mark(4);
    if (out_host && ne > 0 && !delivered) deliver_rows(p, b);
    finish_block(p, b, steady_launched);
}

// host bookkeeping of ONE engine after a block: steal-fade countdown (engine.rs:490-493), NaN-guard frees (engine.rs:499-521,
// culprits identified in the same pass) and cleanup_voices (engine.rs:592-602)
// slot.steal_fade.saturating_sub(len) and the drop of a steal voice whose crossfade has ended (engine.rs:490-493): needs nothing from the
// block's status, so a whole-pool render does it for every engine while the kernels run (steal_countdown_early) instead of after them
void engine_steal_countdown(ow_engine* en, uint32_t l32) {
    OwVm& v = *en->vm;
    if (!v.steal_mask) return;
    vm_host_changed(en);
    for (uint64_t m = v.steal_mask; m; m &= m - 1) {
        const int s = __builtin_ctzll(m);
        v.steal_fade[s] = v.steal_fade[s] > l32 ? v.steal_fade[s] - l32 : 0u;
        if (v.steal_fade[s] == 0) { v.has_steal &= ~(1ull << s); en->sync_masks(s); }
    }
}
void engine_post_render(ow_engine* en, uint32_t l32, const OwEngineOut& o, bool steal_counted = false) {
    OwVm& v = *en->vm;
    vm_host_changed(en);
    if (!steal_counted) engine_steal_countdown(en, l32);
    if (o.sum_nonfinite) {
        en->nan_guard_fires += 1;
        for (int s = 0; s < OW_MAX_VOICES; ++s) {
            const uint64_t b = 1ull << s;
            if ((o.bad_main >> s) & 1ull) { en->set_state(s, OW_VOICE_FREE); v.has_voice &= ~b; }
            if ((o.bad_steal >> s) & 1ull) { v.has_steal &= ~b; v.steal_fade[s] = 0; }
            en->sync_masks(s);
        }
    }
    if (o.out_nonfinite) en->output_nan_resets += 1;
    for (uint64_t m = o.silent_mask & v.main_mask; m; m &= m - 1) {
        const int s = __builtin_ctzll(m);
        if (en->state_of(s) != OW_VOICE_FREE && ((v.has_voice >> s) & 1ull)) { en->set_state(s, OW_VOICE_FREE); v.has_voice &= ~(1ull << s); en->sync_masks(s); }
    }
}

// Second render of the voice-sum NaN guard (engine.rs:496-521).  When a block's voice sum was non-finite the reference zeroes the sum and
// renders every voice the engine still has AGAIN, freeing the ones whose output is non-finite; the survivors have then advanced 2 * len
// samples.  engine_post_render has already freed the voices that were non-finite in the first pass and dropped the steal voices whose
// crossfade ended (the reference drops those at the end of the first pass, before the guard looks); here the survivors are stepped by
// another `len` samples (k_voice in guard mode: same stepping, nothing summed), voices that turn non-finite in that second pass are freed
// too, and the status the block leaves behind (silent voices, transient phases) is the status after the second pass.  Cold path.
void engine_guard_second_pass_result(ow_engine* en, const OwEngineOut& o) {
    OwVm& v = *en->vm;
    vm_host_changed(en);
    for (int s = 0; s < OW_MAX_VOICES; ++s) {
        const uint64_t b = 1ull << s;
        bool touched = false;
        if ((o.bad_main >> s) & 1ull) { en->set_state(s, OW_VOICE_FREE); v.has_voice &= ~b; touched = true; }
        if ((o.bad_steal >> s) & 1ull) { v.has_steal &= ~b; v.steal_fade[s] = 0; touched = true; }
        if (touched) en->sync_masks(s);
    }
    for (uint64_t m = o.silent_mask & v.main_mask; m; m &= m - 1) {     // cleanup_voices sees the twice-advanced voices (engine.rs:461)
        const int s = __builtin_ctzll(m);
        if (en->state_of(s) != OW_VOICE_FREE && ((v.has_voice >> s) & 1ull)) { en->set_state(s, OW_VOICE_FREE); v.has_voice &= ~(1ull << s); en->sync_masks(s); }
    }
}
void guard_second_pass(ow_pool* p, const uint32_t* engs, size_t n_eng, size_t len) {
    hipStream_t st = p->stream;
    uint32_t nm = 0, ns = 0;          // entries; one block per engine and list
    for (size_t i = 0; i < n_eng; ++i) {
        const ow_engine* en = p->engines[engs[i]].get();
        auto put = [&](uint32_t* a, uint32_t& n, uint64_t mask) {
            if (!mask) return;
            for (uint64_t m = mask; m; m &= m - 1) a[n++] = (engs[i] << 6) | (uint32_t)__builtin_ctzll(m);
            while (n & 63u) a[n++] = 0xFFFFFFFFu;
        };
        put(p->vl_general.h, nm, en->vm->main_mask);
        put(p->vl_steal.h, ns, en->vm->steal_mask);
    }
    p->lists_valid = false;           // the list buffers were borrowed
    p->vl_general.sig_valid = false; p->vl_steal.sig_valid = false;
    // the guarded engines' status blocks: ONE clear, ONE gather and ONE transfer for the whole set (a bad parameter broadcast to a big
    // pool can put every engine here: 131 072 engines used to mean 262 144 runtime calls on the audio thread).  engs is pinned
    // (h_op_engines) and d_op_engines is free between renders.
    const unsigned nb = (unsigned)((n_eng + 255) / 256);
    HIP_OK(hipMemcpyAsync(p->d_op_engines, engs, sizeof(uint32_t) * n_eng, hipMemcpyHostToDevice, st));
    owdev::k_eout_clear_list<<<dim3(nb), dim3(256), 0, st>>>(p->d_eout, p->d_op_engines, (int)n_eng);
    const int I = (int)p->I, L = (int)len, Lcap = (int)p->Lcap;
    if (nm) {
        HIP_OK(hipMemcpyAsync(p->vl_general.d, p->vl_general.h, sizeof(uint32_t) * nm, hipMemcpyHostToDevice, st));
        owdev::k_voice<<<dim3(nm / 64), dim3(64), 0, st>>>(p->dK, p->d_vrec, p->vl_general.d, p->d_sum, p->d_eout, I, L, Lcap, 2);
    }
    if (ns) {
        HIP_OK(hipMemcpyAsync(p->vl_steal.d, p->vl_steal.h, sizeof(uint32_t) * ns, hipMemcpyHostToDevice, st));
        owdev::k_voice<<<dim3(ns / 64), dim3(64), 0, st>>>(p->dK, p->d_vrec, p->vl_steal.d, p->d_sum, p->d_eout, I, L, Lcap, 3);
    }
    owdev::k_eout_gather_list<<<dim3(nb), dim3(256), 0, st>>>(p->d_eout, p->d_op_engines, (int)n_eng, p->d_eout_packed);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(p->h_eout_packed, p->d_eout_packed, sizeof(OwEngineOut) * n_eng, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n_eng; ++i) {
        OwEngineOut& o = p->h_eout[engs[i]];
        o = p->h_eout_packed[i];
        engine_guard_second_pass_result(p->engines[engs[i]].get(), o);
        p->transient[engs[i]] = o.transient != 0u;
        o.sum_nonfinite = 1u;         // the block's voice sum stays "zeroed by the guard" for ow_pool_read_voice_sum
    }
}

// host bookkeeping after the block has been rendered (needs h_eout; call after stream sync)
// The steal-fade countdown of a whole-pool block while its kernels run (ow_pool_render, between the launches and the stream sync).
// After a whole-pool re-strike that is 64 counters and masks per engine over 120 MB of state: 2-3 ms on sixteen threads, GPU idle, when
// done after the block.  post_render_host then skips it (p->steal_counted).
void steal_countdown_early(ow_pool* p, size_t len) {
    p->steal_counted = false;
    const int ne = (int)p->I;
    if (!p->any_steal_c || !p->any_cache_valid || ne < 16384) return;
    const uint32_t l32 = (uint32_t)std::min<size_t>(len, 0xFFFFFFFFull);
    const size_t T = std::min<size_t>(effective_cpus(), 32);
    const int per = (int)((ne + T - 1) / T);
    auto slice = [&](size_t t) {
        const int k1 = std::min(ne, (int)(t + 1) * per);
        for (int k = (int)t * per; k < k1; ++k)
            if (p->h_args[k].steal_mask) engine_steal_countdown(p->engines[k].get(), l32);
    };
    Workers::get().each(T, slice);
    p->steal_counted = true;
}

void post_render_host(ow_pool* p, int e0, int ne, size_t len) {
    if (p->skew_pending) { p->skew_pending = false; p->skew_next = *p->h_skew_seen != 0u; }
    const uint32_t l32 = (uint32_t)std::min<size_t>(len, 0xFFFFFFFFull);
    const bool steal_counted = p->steal_counted;
    p->steal_counted = false;
    // what one engine's status block asks of the host; returns bit 0 = the voice lists changed, bit 1 = misdispatch, bit 2 = voice-sum guard
    auto one = [&](int e) -> uint8_t {
        const OwEngineOut& o = p->h_eout[e];
        const OwEngineArgs& a = p->h_args[e];
        uint8_t r = 0;
        if (o.transient == 2u) r |= 2;
        const uint8_t tr = o.transient != 0u;
        if (tr != p->transient[e]) { p->transient[e] = tr; r |= 1; }
        // fast path on the contiguous status/args arrays: nothing to book-keep for this engine
        if ((steal_counted || !a.steal_mask) && !(o.silent_mask & a.main_mask) && !o.sum_nonfinite && !o.out_nonfinite) return r;
        if (o.sum_nonfinite) r |= 4;
        engine_post_render(p->engines[e].get(), l32, o, steal_counted);
        return r;
    };
    auto second_pass = [&] {   // voice-sum NaN guard fired somewhere: the reference's second render pass for those engines
        uint32_t* engs = p->h_op_engines;     // pinned scratch of I entries, free between renders
        size_t n = 0;
        for (int k = 0; k < ne; ++k) if (p->h_eout[e0 + k].sum_nonfinite) engs[n++] = (uint32_t)(e0 + k);
        guard_second_pass(p, engs, n, len);
    };
    if (p->attn_pending) {
        // the block left one bit per engine (k_eout_attention): nothing set = nothing to do, the usual case of a big pool
        p->attn_pending = false;
        const int words = (ne + 63) / 64;
        size_t count = 0;
        for (int w = 0; w < words; ++w) count += (size_t)__builtin_popcountll(p->h_attn[w]);
        if (p->eout_all_live) { std::memset(p->h_eout, 0, sizeof(OwEngineOut) * p->I); p->eout_all_live = false; }
        else for (uint32_t e : p->eout_live) std::memset(&p->h_eout[e], 0, sizeof(OwEngineOut));
        p->eout_live.clear();
        if (count == 0) return;
        HIP_OK(hipMemcpyAsync(p->h_eout + e0, p->d_eout + e0, sizeof(OwEngineOut) * ne, hipMemcpyDeviceToHost, p->stream));
        HIP_OK(hipStreamSynchronize(p->stream));
        if (count * 8 <= (size_t)ne) {
            uint8_t r = 0;
            for (int w = 0; w < words; ++w)
                for (uint64_t m = p->h_attn[w]; m; m &= m - 1) {
                    const int e = e0 + w * 64 + __builtin_ctzll(m);
                    r |= one(e);
                    p->eout_live.push_back((uint32_t)e);
                }
            if (r & 1) p->lists_valid = false;
            if (r & 2) set_err("voice dispatch: an engine in a transient phase was sent to the steady kernel");
            if (r & 4) { second_pass(); p->attn_resync = true; }
            return;
        }
        p->eout_all_live = true;               // many engines (a whole-pool re-strike): the sliced scan below
    } else if (p->d_attn) {
        p->eout_all_live = true;
    }
    // engines are independent: after a whole-pool re-strike every engine has 64 steal fades to count down and 64 masks to
    // update (40 ms on one thread for 65 536 engines), so large ranges are cut into slices like the MIDI and op packing are
    const size_t T = ne >= 16384 ? std::min<size_t>(effective_cpus(), 32) : 1;
    const int per = (int)((ne + T - 1) / T);
    uint8_t res[OW_MAX_SLICES] = {0};
    auto slice = [&](size_t t) {
        const int k1 = std::min(ne, (int)(t + 1) * per);
        uint8_t r = 0;
        for (int k = (int)t * per; k < k1; ++k) r |= one(e0 + k);
        res[t] = r;
    };
    // a steady block of a big pool has (almost) nothing to do per engine, which is not worth starting threads for (~0.1 ms): estimate
    // the engines with steal fades / silent voices from every 64th one and go parallel from ~8 000 of them
    long need = 0;
    if (T > 1)
        for (int k = 0; k < ne; k += 64)
            need += p->h_args[e0 + k].steal_mask != 0 || (p->h_eout[e0 + k].silent_mask & p->h_args[e0 + k].main_mask) != 0;
    const bool busy = need * 64 > 8192;
    if (T == 1 || !busy) {
        for (size_t t = 0; t < T; ++t) slice(t);
    } else {
        Workers::get().each(T, slice);
    }
    uint8_t r = 0;
    for (size_t t = 0; t < T; ++t) r |= res[t];
    if (r & 1) { p->lists_valid = false; if (p->d_prev_tr) p->attn_resync = true; }    // p->transient moved without the device's copy
    if (r & 2) set_err("voice dispatch: an engine in a transient phase was sent to the steady kernel");
    if (r & 4) { second_pass(); if (p->d_prev_tr) p->attn_resync = true; }
}

void collect_profile(ow_pool* p) {
    if (!p->profiling) return;
    if (p->voices_only) { p->last_ms[2] = 0.f; }
    else hipEventSynchronize(p->ev[7]);   // in a small pool the block-ahead tremolo outlasts the audio stream; profiling waits for it, a normal render does not
    hipEventElapsedTime(&p->last_ms[0], p->ev[0], p->ev[1]);   // ops
    if (!p->voices_only) hipEventElapsedTime(&p->last_ms[2], p->ev[6], p->ev[7]);   // tremolo (own stream)
    hipEventElapsedTime(&p->last_ms[1], p->ev_stage[0], p->ev_stage[1]);   // voices
    hipEventElapsedTime(&p->last_ms[3], p->ev_stage[2], p->ev_stage[3]);   // preamp (or the whole chain kernel)
    hipEventElapsedTime(&p->last_ms[4], p->ev_stage[3], p->ev_stage[4]);   // output stage
}

// WurliEngine::warm_up (engine.rs:261-270): 0.6 s of render() in 512-sample blocks
void warm_up_range(ow_pool* p, int e0, int ne) {
    const size_t total = (size_t)owhip::sat_u32(p->hc.sr * 0.6);
    size_t done = 0;
    while (done < total) {
        const size_t len = std::min<size_t>(512, total - done);
        render_range(p, e0, ne, len, true);
        HIP_OK(hipStreamSynchronize(p->stream));
        post_render_host(p, e0, ne, len);
        done += len;
    }
}

void engine_host_reset(ow_engine* en) {  // host half of WurliEngine::reset (engine.rs:231-244)
    vm_host_current(en); vm_host_changed(en);
    const uint8_t mlp = en->vm->mlp_enabled;
    vm_init(*en->vm);                          // every slot Free, no voices, age counter 0, sustain up; nothing queued on the device either
    en->vm->mlp_enabled = mlp;                 // (a parameter, not state: reset() does not touch it)
    en->touch();
    if (!en->ops.empty()) { en->ops.clear(); if (en->host_ops_any) __atomic_fetch_sub(en->host_ops_any, 1u, __ATOMIC_RELAXED); }
    // snap_to(target): a pending retarget would ramp; the device snaps current := target, so drop the ramp request
    en->volume.pending = en->depth.pending = en->spk.pending = false;
}

void push_op(ow_engine* en, uint8_t type, int slot, uint8_t note, bool mlp, uint32_t seed, double vel) { en->push(type, slot, note, mlp, seed, vel); }

ow_pool* pool_create(double sample_rate, size_t n_engines, int device, int preamp_kind, int power_amp_kind = OW_POWER_AMP_BEHAVIORAL,
                     int tremolo_kind = OW_TREMOLO_TWIN_T, bool voices_only = false, bool no_traj) {
    if (!(sample_rate > 0.0) || n_engines == 0) throw std::runtime_error("invalid sample rate or engine count");
    if (tremolo_kind != OW_TREMOLO_TWIN_T && tremolo_kind != OW_TREMOLO_LEGACY_LFO) throw std::runtime_error("unknown tremolo_kind");
    require_known_kinds(preamp_kind, power_amp_kind);
    require_device(device);
    std::unique_ptr<ow_pool> owner(new ow_pool());     // a throw below releases everything acquired so far
    ow_pool* p = owner.get();
    p->device = device;
    p->I = n_engines;
    p->power_amp_kind = power_amp_kind;
    p->tremolo_kind = tremolo_kind;
    p->voices_only = voices_only;
    p->stream.create();             // main, tremolo, copy: see ow_pool::stream
    p->stream_trem.create();
    p->stream_copy.create();
    for (auto& e : p->ev) e.create(hipEventDefault);
    for (auto& e : p->ev_stage) e.create(hipEventDefault);
    for (auto& e : p->ev_trem) e.create();
    p->d_trem_backup.alloc(18 * n_engines);
    p->d_trem_settled.alloc(18);
    p->d_zero.alloc(1);
    HIP_OK(hipMemsetAsync(p->d_zero, 0, sizeof(uint32_t), p->stream));
    p->d_birth.alloc(n_engines);
    p->d_evict.alloc(3 * n_engines);
    p->h_birth.assign(n_engines, OW_OFF_TRAJ);
    p->sw = Switches::from_env();
    if (no_traj) p->sw.trem_traj = false;
    p->dK.alloc(1);
    p->dK48.alloc(1);
    p->d_nt.alloc(NT_COUNT * 64);
    p->d_vrec.alloc(n_engines * 2 * OW_VREC_DOUBLES);
    p->d_cs.alloc(CS_COUNT * n_engines);
    p->d_args.alloc(n_engines);
    p->d_eout.alloc(n_engines);
    p->h_args.alloc(n_engines);
    p->h_vm.alloc(n_engines);
    p->ev_vm.create(); p->ev_vm_events.create(); p->ev_vm_up.create();
    p->h_eout.alloc(n_engines);
    p->d_eout_packed.alloc(n_engines); p->h_eout_packed.alloc(n_engines);
    p->d_skew_seen.alloc(1);
    HIP_OK(hipMemset(p->d_skew_seen, 0, sizeof(uint32_t)));
    p->h_skew_seen.alloc(1);
    *p->h_skew_seen = 0u;
    if (n_engines >= 64) {      // status summary of big ranges (k_eout_attention)
        p->d_attn.alloc((n_engines + 63) / 64); p->h_attn.alloc((n_engines + 63) / 64);
        p->d_prev_tr.alloc(n_engines);
        HIP_OK(hipMemset(p->d_prev_tr, 0, n_engines));
        p->h_prev_tr.alloc(n_engines);
        p->eout_live.reserve(n_engines / 8 + 64);       // the summary path lists at most ne / 8 engines: nothing grows on the render path
    }
    for (ow_pool::VoiceList* vl : {&p->vl_steady, &p->vl_general, &p->vl_steal, &p->vl_attack}) {   // worst case: one block per engine
        vl->d.alloc(64 * n_engines); vl->h.alloc(64 * n_engines);
    }
    p->transient.assign(n_engines, 0);
    p->d_lead.alloc(n_engines); p->h_lead.alloc(n_engines);
    p->d_leaders.alloc(n_engines); p->h_leaders.alloc(n_engines);
    p->d_copy.alloc(2 * n_engines); p->h_copy.alloc(2 * n_engines);
    p->grp_in.assign(n_engines, 0); p->grp_out.assign(n_engines, 0);
    for (size_t i = 0; i < n_engines; ++i) p->h_lead[i] = (uint32_t)i;   // singletons until the chain state is replicated below
    p->d_snap.alloc(3 * n_engines); p->h_snap.alloc(3 * n_engines);
    ensure_ops_capacity(p, (size_t)3 * OW_MAX_VOICES * n_engines);   // a whole-keyboard re-strike of every engine: no allocation in render
    Workers::get();                                                  // start the host worker threads now, not inside the first render
    p->d_op_engines.alloc(n_engines); p->h_op_engines.alloc(n_engines);
    std::memset(p->h_args, 0, sizeof(OwEngineArgs) * n_engines);
    std::memset(p->h_eout, 0, sizeof(OwEngineOut) * n_engines);
    HIP_OK(hipMemsetAsync(p->d_vrec, 0, sizeof(double) * n_engines * 2 * OW_VREC_DOUBLES, p->stream));
    HIP_OK(hipMemsetAsync(p->d_cs, 0, sizeof(double) * CS_COUNT * n_engines, p->stream));
    alloc_stream_buffers(p, n_engines == 1 ? (size_t)OW_MAX_BLOCK : (size_t)1024);  // engine.rs:25 MAX_BLOCK_SIZE for a lone engine
    if (power_amp_kind == OW_POWER_AMP_MELANGE) {
        p->dPa.alloc(1);
        p->d_pa.alloc(owdev::PAS_COUNT * n_engines);
        HIP_OK(hipMemsetAsync(p->d_pa, 0, sizeof(double) * owdev::PAS_COUNT * n_engines, p->stream));
        p->d_pa_settled.alloc(owdev::PAS_CIRCUIT_END);
        pa_settled_to_device(device, p->d_pa_settled, p->stream);
        p->d_pa_demand.alloc(n_engines);
        HIP_OK(hipMemsetAsync(p->d_pa_demand, 0, sizeof(uint32_t) * n_engines, p->stream));
        p->d_pa_order.alloc(n_engines);
        p->d_pa_hist.alloc(PA_ORDER_CLASSES);
    }
    upload_consts(p, sample_rate, preamp_kind);
    owdev::k_note_table<<<dim3(1), dim3(64), 0, p->stream>>>(p->d_nt);
    if (preamp_kind == OW_PREAMP_MELANGE12) {
        p->d_mel_settled.alloc(18);
        // LU workspace of the generic rebuild (the fallback of both literal kernels): the column-streamed kernel wants one [144] column
        // per lane = (engine, state), lane-minor, + 32 spare engines for the masked lanes of a last partial wavefront; the LDS-matrix
        // kernel one [144][32] slab per workgroup
        p->mel_lu_ld = 2 * (n_engines + 32);
        p->d_mel_lu.alloc(144 * std::max<size_t>(p->mel_lu_ld, 32 * ((size_t)(n_engines + 31) / 32 + OW_MAX_SLICES + 1)));
        mel_settled_to_device(device, p->d_mel_settled, p->stream);
        // Noise streams: the reference clones one process-wide state whose RNGs were seeded from the clock (master seed 0,
        // gen_preamp.rs:1512-1521 via melange_adapter.rs:12-29), so every engine of a process starts on the same streams.
        p->d_noise.alloc(NZ_COUNT * n_engines);
        HIP_OK(hipMemsetAsync(p->d_noise, 0, sizeof(double) * NZ_COUNT * n_engines, p->stream));
        std::vector<uint64_t> seeds(n_engines, process_noise_seed());
        HIP_OK(hipMemcpyAsync(p->d_noise + (size_t)NZ_SEED * n_engines, seeds.data(), sizeof(uint64_t) * n_engines, hipMemcpyHostToDevice, p->stream));
        HIP_OK(hipStreamSynchronize(p->stream));
    }
    p->engines.resize(n_engines);
    p->dirty.assign(n_engines, 1);
    for (size_t i = 0; i < n_engines; ++i) {
        ow_engine* en = (p->engines[i] = std::make_unique<ow_engine>()).get();
        en->pool = p;
        en->index = i;
        en->dirty = &p->dirty[i]; en->dirty_any = &p->dirty_any;
        en->vm = &p->h_vm[i];
        vm_init(*en->vm);
        en->host_ops_any = &p->host_ops_any;
        en->sr = sample_rate;
        // Room for a whole-keyboard re-strike (damper + move-to-steal + note-on per key) from the start: growing 65 536 op lists
        // from 64 to 192 entries inside the first re-strike cost 180 ms of reallocation and page faults on the MIDI threads
        // (later ones take 8 ms).  Same reason as ensure_buffer_capacity: no allocation where the events arrive.
        en->ops.reserve(3 * OW_MAX_VOICES);
    }
    if (voices_only) {          // Voice::render_note has no chain (voice.rs:191-221): nothing to initialise, nothing to settle
        for (size_t i = 0; i < n_engines; ++i) p->h_lead[i] = 0u;
        HIP_OK(hipStreamSynchronize(p->stream));
        return owner.release();
    }
    // WurliEngine::new for engine 0 on the device, then replicate (every engine of a fresh pool is identical)
    chain_init_range(p, 0, 1, INIT_NEW, std::vector<double>(1, 0.5));
    if (n_engines > 1)
        owdev::k_chain_replicate<<<dim3((unsigned)((n_engines + 63) / 64)), dim3(64), 0, p->stream>>>(p->d_cs, (int)n_engines, 0, 0, (int)n_engines);
    if (power_amp_kind == OW_POWER_AMP_MELANGE && n_engines > 1)          // the amp state is not part of the replicated chain rows
        owdev::k_mpa_init<<<dim3((unsigned)((n_engines + 63) / 64)), dim3(64), 0, p->stream>>>(p->dPa, p->d_pa_settled, p->d_pa, (int)n_engines, 0, (int)n_engines, 1);
    if (p->traj) {                    // every engine at t = 0 of the shared trajectory
        for (size_t i = 0; i < n_engines; ++i) { p->h_birth[i] = p->trem_clock; p->h_lead[i] = (uint32_t)i; }
        traj_upload_births(p, 0, (int)n_engines);
        traj_recount(p);
    } else {
        for (size_t i = 0; i < n_engines; ++i) p->h_lead[i] = 0u;         // identical oscillators: one tremolo phase group led by engine 0
    }
    trem_groups_changed(p);
    if (p->d_noise)   // the replicated chain state does not carry the noise columns: seed every engine's streams
        owdev::k_mel_noise_seed<<<dim3((unsigned)((n_engines + 63) / 64)), dim3(64), 0, p->stream>>>(p->d_noise, (int)n_engines, 0, (int)n_engines);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(p->stream));
    return owner.release();
}

template <typename F>
bool guarded(const char* what, F&& f) {  // realtime entry points never fail: record the error, degrade; false = it failed
    try { f(); return true; }
    catch (const std::exception& ex) { set_err(std::string(what) + ": " + ex.what()); std::fprintf(stderr, "openwurli-hip: %s: %s\n", what, ex.what()); return false; }
}

}  // namespace
