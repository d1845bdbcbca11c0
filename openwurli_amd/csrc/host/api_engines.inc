// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: the WurliEngine API (engine.rs).
extern "C" {
// ---- engines ------------------------------------------------------------------------------------
ow_engine* ow_engine_new(double sample_rate, int device, int preamp_kind) {
    ow_pool* p = ow_pool_new(sample_rate, 1, device, preamp_kind);
    if (!p) return nullptr;
    p->engines[0]->owns_pool = true;
    return p->engines[0].get();
}
ow_engine* ow_engine_new_kinds(double sample_rate, int device, int preamp_kind, int power_amp_kind, int tremolo_kind) {
    ow_pool* p = ow_pool_new_kinds(sample_rate, 1, device, preamp_kind, power_amp_kind, tremolo_kind);
    if (!p) return nullptr;
    p->engines[0]->owns_pool = true;
    return p->engines[0].get();
}
ow_engine* ow_engine_new_with(double sample_rate, int device, int preamp_kind, int power_amp_kind) {
    ow_pool* p = ow_pool_new_with(sample_rate, 1, device, preamp_kind, power_amp_kind);
    if (!p) return nullptr;
    p->engines[0]->owns_pool = true;
    return p->engines[0].get();
}
void ow_engine_free(ow_engine* e) { if (e && e->owns_pool) delete e->pool; }
// engine.rs:406-420.  No-ops / zeros on the behavioural amp, which has no separable rails (power_amp.rs:262-272).
void ow_engine_set_rail_sag(ow_engine* e, int on) {
    if (!e || !e->pool || e->pool->power_amp_kind != OW_POWER_AMP_MELANGE) return;
    if (e->rail_sag != (on != 0)) { e->rail_sag = on != 0; e->touch(); }
}
int ow_engine_rail_sag_enabled(const ow_engine* e) { return (e && e->pool && e->pool->power_amp_kind == OW_POWER_AMP_MELANGE && e->rail_sag) ? 1 : 0; }
void ow_engine_power_amp_diag(const ow_engine* e, ow_power_amp_diag* d) {
    if (!d) return;
    std::memset(d, 0, sizeof *d);
    d->rail_pos_volts = 22.5; d->rail_neg_volts = 22.5;
    if (!e || !e->pool || e->pool->power_amp_kind != OW_POWER_AMP_MELANGE) return;
    ow_pool* p = e->pool;
    double col[owdev::PAS_COUNT];
    if (hipSetDevice(p->device) != hipSuccess) return;
    hipStreamSynchronize(p->stream);
    if (hipMemcpy2D(col, sizeof(double), p->d_pa + e->index, sizeof(double) * p->I, sizeof(double), owdev::PAS_COUNT, hipMemcpyDeviceToHost) != hipSuccess) return;
    auto u64 = [&](int r) { uint64_t b; std::memcpy(&b, &col[r], 8); return b; };
    d->clamp_count = u64(owdev::PAS_CLAMP); d->nr_max_iter_count = u64(owdev::PAS_NRMAX); d->peak_output_volts = col[owdev::PAS_PEAK];
    d->nan_resets = u64(owdev::PAS_NAN); d->guard_resets = u64(owdev::PAS_GUARD);
    if (e->rail_sag) { d->rail_pos_volts = col[owdev::PAS_RAILP]; d->rail_neg_volts = col[owdev::PAS_RAILN]; }
}

void ow_engine_set_sample_rate(ow_engine* e, double sr) {
    if (!e) return;
    // engines of a pool share one rate (lane = engine kernels read one constant block): the whole pool follows
    ow_pool_set_sample_rate(e->pool, sr);
}

void ow_engine_reset(ow_engine* e) {
    if (!e) return;
    guarded("ow_engine_reset", [&] {
        ow_pool* p = e->pool;
        HIP_OK(hipSetDevice(p->device));
        engine_host_reset(e);
        chain_init_range(p, (int)e->index, 1, INIT_RESET, std::vector<double>(1, 0.0));
        warm_up_range(p, (int)e->index, 1);
    });
}

void ow_engine_warm_up(ow_engine* e) {
    if (!e) return;
    guarded("ow_engine_warm_up", [&] { HIP_OK(hipSetDevice(e->pool->device)); warm_up_range(e->pool, (int)e->index, 1); });
}

void ow_engine_ensure_buffer_capacity(ow_engine* e, size_t n) { if (e) ow_pool_ensure_buffer_capacity(e->pool, n); }

// (the state machine itself: ow_vm.h -- the same functions run on the device for bursts, k_vm_events)
void ow_engine_note_on(ow_engine* e, uint8_t note_in, float velocity) {  // engine.rs:299-338
    if (!e) return;
    vm_host_current(e); vm_host_changed(e);
    vm_note_on(*e->vm, *e, note_in, velocity, owhip::sat_u32(e->sr * 0.005));
    e->mark();
}
void ow_engine_note_off(ow_engine* e, uint8_t note_in) {  // engine.rs:340-359
    if (!e) return;
    vm_host_current(e); vm_host_changed(e);
    vm_note_off(*e->vm, *e, note_in);
}
void ow_engine_set_sustain(ow_engine* e, int held) {  // engine.rs:361-374
    if (!e) return;
    vm_host_current(e); vm_host_changed(e);
    vm_set_sustain(*e->vm, *e, held != 0);
}

void ow_engine_set_volume(ow_engine* e, double v) { if (e) { e->volume.set_target(v); if (e->volume.pending) e->touch(); } }
void ow_engine_set_tremolo_depth(ow_engine* e, double d) { if (e) { e->depth.set_target(d); if (e->depth.pending) e->touch(); } }
void ow_engine_set_speaker_character(ow_engine* e, double c) { if (e) { e->spk.set_target(c); if (e->spk.pending) e->touch(); } }
void ow_engine_set_mlp_enabled(ow_engine* e, int on) { if (e) { vm_host_current(e); e->vm->mlp_enabled = on != 0 ? 1 : 0; vm_host_changed(e); } }
// Thermal noise of the melange preamp's main state; no-ops on the legacy solver (dk_preamp_legacy.rs:262-265)
void ow_engine_set_noise_enabled(ow_engine* e, int on) {
    if (!e || !e->pool || e->pool->hc.preamp_kind != OW_PREAMP_MELANGE12) return;
    if (e->noise_on != (on != 0)) { e->noise_on = on != 0; e->touch(); }
}
void ow_engine_set_noise_gain(ow_engine* e, double gain) {
    if (!e || !e->pool || e->pool->hc.preamp_kind != OW_PREAMP_MELANGE12) return;
    if (e->thermal_gain != gain) { e->thermal_gain = gain; e->touch(); }
}
void ow_engine_set_noise_seed(ow_engine* e, uint64_t seed) {
    if (!e || !e->pool || !e->pool->d_noise) return;
    guarded("ow_engine_set_noise_seed", [&] {
        ow_pool* p = e->pool;
        HIP_OK(hipSetDevice(p->device));
        const uint64_t resolved = seed ? seed : process_noise_seed();
        HIP_OK(hipMemcpyAsync(p->d_noise + (size_t)NZ_SEED * p->I + e->index, &resolved, sizeof resolved, hipMemcpyHostToDevice, p->stream));
        owdev::k_mel_noise_seed<<<dim3(1), dim3(64), 0, p->stream>>>(p->d_noise, (int)p->I, (int)e->index, 1);
        HIP_OK(hipStreamSynchronize(p->stream));
    });
}

void ow_engine_render(ow_engine* e, float* out, size_t len) {
    if (!e || !out || len == 0) return;
    if (e->pool->I != 1) { set_err("ow_engine_render: engine belongs to a multi-engine pool; use ow_pool_render"); std::memset(out, 0, len * sizeof(float)); return; }
    ow_pool_render(e->pool, out, len, len);      // writes silence itself when the render fails
}

void ow_engine_get_diag(const ow_engine* e, ow_diag* d) {
    if (!e || !d) return;
    std::memset(d, 0, sizeof *d);
    vm_host_current(e);
    const OwVm& v = *e->vm;
    d->active_voices = (uint32_t)__builtin_popcountll(~v.st_mask[OW_VOICE_FREE]);
    d->held_voices = (uint32_t)__builtin_popcountll(v.st_mask[OW_VOICE_HELD]);
    d->sustained_voices = (uint32_t)__builtin_popcountll(v.st_mask[OW_VOICE_SUSTAINED]);
    d->releasing_voices = (uint32_t)__builtin_popcountll(v.st_mask[OW_VOICE_RELEASING]);
    d->steal_voices = (uint32_t)__builtin_popcountll(v.has_steal);
    d->sustain_held = v.sustain_held ? 1 : 0;
    d->nan_guard_fires = e->nan_guard_fires;
    d->output_nan_resets = e->output_nan_resets;
    ow_pool* p = e->pool;
    double diag = 0.0;
    if (p && hipSetDevice(p->device) == hipSuccess &&
        hipMemcpy(&diag, p->d_cs + (size_t)CS_DIAG * p->I + e->index, sizeof(double), hipMemcpyDeviceToHost) == hipSuccess) {
        uint64_t bits;
        std::memcpy(&bits, &diag, 8);
        d->preamp_nan_resets = (uint32_t)(bits >> 32);
        double be = 0.0;   // counts the block-ahead samples too
        if (p->traj && p->h_birth[e->index] != OW_OFF_TRAJ) {
            d->tremolo_be_fallbacks = p->traj->be_count_at(p->trem_clock - p->h_birth[e->index]);
        } else if (hipMemcpy(&be, p->d_cs + (size_t)CS_T_BE * p->I + p->h_lead[e->index], sizeof(double), hipMemcpyDeviceToHost) == hipSuccess) {
            std::memcpy(&bits, &be, 8);
            d->tremolo_be_fallbacks = bits;
        }
    }
}
int ow_engine_slot_state(const ow_engine* e, int slot) { vm_host_current(e); return (e && slot >= 0 && slot < OW_MAX_VOICES) ? e->state_of(slot) : -1; }
int ow_engine_slot_note(const ow_engine* e, int slot) { vm_host_current(e); return (e && slot >= 0 && slot < OW_MAX_VOICES) ? e->vm->midi_of[slot] : -1; }
int ow_engine_has_steal_voice_for(const ow_engine* e, uint8_t note) {
    if (!e) return 0;
    vm_host_current(e);
    for (int i = 0; i < OW_MAX_VOICES; ++i) if (e->vm->midi_of[i] == note && ((e->vm->has_steal >> i) & 1ull)) return 1;
    return 0;
}

static void midi_apply_one(ow_pool* p, const ow_midi_event& ev) {
    ow_engine* e = p->engines[ev.engine].get();
    switch (ev.type) {
        case 0: ow_engine_note_on(e, ev.note, ev.value); break;
        case 1: ow_engine_note_off(e, ev.note); break;
        case 2: ow_engine_set_sustain(e, ev.value >= 0.5f); break;
        default: break;
    }
}

// A burst on the device (ow_vm.h / ow_vm_kernels.h).  The list must be grouped by engine (the usual layout of a batched script; verified
// by the caller) and the ops it queues must fit the engines' fixed queues; false = not taken (the host path does it).
static bool midi_burst_on_device(ow_pool* p, const ow_midi_event* ev, size_t n) {
    const size_t I = p->I;
    HIP_OK(hipSetDevice(p->device));
    hipStream_t st = p->stream;
    if (!p->d_vm) {                                                // first burst: the device side of the state machine (instantiation-class work)
        DevBuf<OwVm> vm; DevBuf<OwOp> ops_fix; DevBuf<uint32_t> ev_begin, vm_ovf; PinBuf<uint32_t> h_vm_ovf;
        vm.alloc(I); ops_fix.alloc(OW_VM_OPS_MAX * I); ev_begin.alloc(2 * I); vm_ovf.alloc(1); h_vm_ovf.alloc(1);
        // all five or none: a burst that fails here leaves d_vm unset, and the next one sets up again
        p->d_vm = std::move(vm); p->d_ops_fix = std::move(ops_fix); p->d_ev_begin = std::move(ev_begin); p->d_vm_ovf = std::move(vm_ovf); p->h_vm_ovf = std::move(h_vm_ovf);
        p->vm_host_dirty = 1;
    }
    if (__atomic_load_n(&p->host_ops_any, __ATOMIC_RELAXED)) return false;   // ops queued on the host come first in their engines' queues: host path
    // the events: straight from the caller's block when it is pinned (ow_host_alloc), else through a pinned staging copy made by the workers
    const ow_midi_event* src = (const ow_midi_event*)host_block_device_ptr(ev, sizeof(ow_midi_event) * n) ? ev : nullptr;
    if (n > p->ev_cap) {
        p->ev_cap = 0;                                                              // until both exist
        const size_t cap = std::max<size_t>(n, (size_t)2 * OW_MAX_VOICES * I);      // a whole-keyboard re-strike of every engine
        p->d_ev.alloc(cap); p->h_ev.alloc(cap);
        p->ev_cap = cap;
    }
    if (!src) {
        const size_t T = std::min<size_t>(effective_cpus(), OW_MAX_SLICES);
        auto copy = [&](size_t t) { const size_t a = n * t / T, b = n * (t + 1) / T; std::memcpy(p->h_ev + a, ev + a, sizeof(ow_midi_event) * (b - a)); };
        Workers::get().each(T, copy);
        src = p->h_ev;
    }
    vm_wait_download(p);
    const uint32_t e_lo = std::min<uint32_t>(ev[0].engine, (uint32_t)I), e_hi = std::min<uint32_t>(ev[n - 1].engine + 1u, (uint32_t)I);
    if (e_lo >= e_hi) return false;                                // nothing addressed to this pool -- if the list is grouped, which only the host path checks here
    if (p->vm_upload_inflight) { HIP_OK(hipStreamWaitEvent(st, p->ev_vm_up, 0)); p->vm_upload_inflight = false; }
    if (p->vm_host_dirty) {
        HIP_OK(hipMemcpyAsync(p->d_vm, p->h_vm, sizeof(OwVm) * I, hipMemcpyHostToDevice, st));
        p->vm_host_dirty = 0;
    }
    HIP_OK(hipMemcpyAsync(p->d_ev, src, sizeof(ow_midi_event) * n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(p->d_ev_begin, 0, sizeof(uint32_t) * 2 * I, st));
    HIP_OK(hipMemsetAsync(p->d_vm_ovf, 0, sizeof(uint32_t), st));
    owdev::k_vm_index<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(p->d_ev, n, p->d_ev_begin, p->d_ev_begin + I, (uint32_t)I, p->d_vm_ovf);
    const uint32_t fade = owhip::sat_u32(p->engines[0]->sr * 0.005);
    owdev::k_vm_events<<<dim3((e_hi - e_lo + 63) / 64), dim3(64), 0, st>>>(p->d_vm, p->d_ev, p->d_ev_begin, p->d_ev_begin + I, p->d_ops_fix, e_lo, e_hi, fade, p->d_vm_ovf);
    HIP_OK(hipGetLastError());
    // a queue that overflowed (more than OW_VM_OPS_MAX slot ops for one engine between two renders) lost ops, a list that is not grouped
    // by engine (bit 1, k_vm_index) was cut into meaningless slices: nothing of this burst is kept -- the host's copy of the states is
    // still the one from before it -- and the host path replays it
    HIP_OK(hipMemcpyAsync(p->h_vm_ovf, p->d_vm_ovf, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipEventRecord(p->ev_vm_events, st));
    HIP_OK(hipStreamSynchronize(st));
    if (*p->h_vm_ovf) { p->vm_host_dirty = 1; return false; }
    // the states come back on a stream of their own (126 MB for 131 072 engines, 2.3 ms), and the queues are applied AT ONCE beside that
    // (Voice::note_on builds its voice when it is called, voice.rs:28-110; the next render used to start with this launch): the 14.5 ms
    // of a whole-pool re-strike's k_apply_ops now cover the download and the host's packing, scanning and list building for the block
    // that follows.  Ops the host had queued before the burst keep it off this path altogether (above); ops it queues afterwards are
    // applied by the next render, behind these, as before.
    hipStream_t sc = p->stream_copy ? p->stream_copy : st;
    if (sc != st) HIP_OK(hipStreamWaitEvent(sc, p->ev_vm_events, 0));
    HIP_OK(hipMemcpyAsync(p->h_vm + e_lo, p->d_vm + e_lo, sizeof(OwVm) * (e_hi - e_lo), hipMemcpyDeviceToHost, sc));
    HIP_OK(hipEventRecord(p->ev_vm, sc));
    p->vm_download_pending = true;
    std::memset(p->dirty.data() + e_lo, 1, e_hi - e_lo);           // masks / queues of these engines changed: the next render packs them
    __atomic_store_n(&p->dirty_any, (uint8_t)1, __ATOMIC_RELAXED);
    // From here on the burst IS applied to the states (the download will overwrite the host's copy): whatever fails below, the caller must
    // not replay the list on the host.  A failed early application leaves the queues to the next render, as OW_MIDI_APPLY_EARLY=0 does.
    bool early = false, launched = false;
    if (p->sw.midi_apply_early && sc != st) {
        try {
            owdev::k_apply_ops<<<dim3(e_hi - e_lo), dim3(64), 0, st>>>(p->dK, p->d_nt, p->d_vrec, nullptr, nullptr, nullptr, p->d_ops_fix, p->d_vm, (int)e_lo);
            HIP_OK(hipGetLastError());
            launched = true;
            // the queue lengths go back to zero only when the download has them: the host recognises the engines of this burst by them
            // (vm_settle_applied); a short k_apply_ops -- a burst of note-offs -- would otherwise finish, and clear, under the copy
            HIP_OK(hipStreamWaitEvent(st, p->ev_vm, 0));
            owdev::k_vm_clear_dev_ops<<<dim3((e_hi - e_lo + 255) / 256), dim3(256), 0, st>>>(p->d_vm, e_lo, e_hi);
            HIP_OK(hipGetLastError());
            early = true;
        } catch (const std::exception& ex) {
            (void)hipGetLastError();
            set_err(std::string("ow_pool_midi (device burst, early application): ") + ex.what());
        }
    }
    if (early || launched) { p->dev_ops_applied = true; p->applied_lo = e_lo; p->applied_hi = e_hi; }
    else p->dev_ops_pending = true;
    p->vm_bursts += 1;
    return true;
}

void ow_pool_midi(ow_pool* p, const ow_midi_event* ev, size_t n) {
    if (!p || !ev) return;
    // Engines are independent state machines: large event lists are applied by the persistent host workers, each slice owning a
    // contiguous range of engines and walking the list in array order (per-engine order is what matters).  No allocation here.
    size_t T = std::min<size_t>(effective_cpus(), OW_MAX_SLICES);
    if (p->sw.midi_threads) T = (size_t)p->sw.midi_threads;
    if (n < 4096 || p->I < 2 * T) T = 1;
    vm_wait_download(p);
    const bool want_device = n > 0 && !p->voices_only && (p->sw.midi_device == 1 || (p->sw.midi_device < 0 && p->I >= 8192 && n >= 65536));
    if (want_device) {     // (whether the list is grouped by engine is checked on the device too: no walk over 200 MB of events here)
        bool done = false;
        guarded("ow_pool_midi (device burst)", [&] { done = midi_burst_on_device(p, ev, n); });
        if (done) return;
    }
    if (T == 1) {
        for (size_t i = 0; i < n; ++i) if (ev[i].engine < p->I) midi_apply_one(p, ev[i]);
        return;
    }
    // Fast path: a list grouped by engine (non-decreasing engine index, the usual layout of a batched script) is cut into T
    // contiguous slices at engine boundaries, so each slice touches only its own events.  The grouping is verified first, in
    // parallel; an ungrouped list falls back to every slice scanning the whole list for its engine range.
    uint8_t ok[OW_MAX_SLICES];
    auto verify = [&](size_t t) {
        const size_t i0 = std::max<size_t>(n * t / T, 1), i1 = n * (t + 1) / T;
        uint8_t good = 1;
        for (size_t i = i0; i < i1; ++i) good &= (uint8_t)(ev[i].engine >= ev[i - 1].engine);
        ok[t] = good;
    };
    Workers::get().each(T, verify);
    bool grouped = true;
    for (size_t t = 0; t < T; ++t) grouped = grouped && ok[t];
    if (grouped) {
        size_t cut[OW_MAX_SLICES + 1];
        cut[0] = 0; cut[T] = n;
        for (size_t t = 1; t < T; ++t) {   // first event of the engine that owns position n*t/T belongs to the slice on the right
            size_t i = n * t / T;
            const uint32_t eng = ev[i].engine;
            i = (size_t)(std::lower_bound(ev, ev + i, eng, [](const ow_midi_event& a, uint32_t b) { return a.engine < b; }) - ev);
            cut[t] = std::max(i, cut[t - 1]);
        }
        auto apply = [&](size_t t) {
            for (size_t i = cut[t]; i < cut[t + 1]; ++i) if (ev[i].engine < p->I) midi_apply_one(p, ev[i]);
        };
        Workers::get().each(T, apply);
    } else {
        const size_t per = (p->I + T - 1) / T;
        auto apply = [&](size_t t) {
            const uint32_t lo = (uint32_t)(t * per), hi = (uint32_t)std::min(p->I, (t + 1) * per);
            for (size_t i = 0; i < n; ++i) if (ev[i].engine >= lo && ev[i].engine < hi) midi_apply_one(p, ev[i]);
        };
        Workers::get().each(T, apply);
    }
}
}  // extern "C"
