// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): ow_engine / ow_pool: the host side of one engine and of a pool.

struct ow_engine {
    ow_pool* pool = nullptr;
    size_t index = 0;
    bool owns_pool = false;
    // VoiceSlot[64] + pool counters (engine.rs:39-62): plain data shared with the device (ow_vm.h).  An engine of a pool points into the
    // pool's pinned array (a burst of events applied on the device is copied back into it wholesale); a device-less test engine owns one.
    OwVm* vm = nullptr;
    OwVm own_vm;
    ow_engine() { vm_init(own_vm); vm = &own_vm; }
    int state_of(int s) const { return vm_state_of(*vm, s); }
    void set_state(int s, int st) { vm_set_state(*vm, s, st); }
    bool rail_sag = true;           // melange power amp: rail sag (PowerAmp::new_at_sample_rate starts with it on, power_amp.rs:335-346)
    bool noise_on = false;          // melange preamp thermal noise (engine.rs:394-400); DkPreamp::new starts with off / 1.0
    double thermal_gain = 1.0;
    HostSmoother volume{0.5}, depth{0.5}, spk{0.0};
    uint64_t nan_guard_fires = 0, output_nan_resets = 0;
    std::vector<OwOp> ops;  // pending slot ops queued on the host, applied at the start of the next render (behind the device-queued ones)
    double sr = 0.0;            // host sample rate (steal crossfade length, engine.rs:318)
    uint8_t* dirty = nullptr;   // -> pool->dirty[index]: engine has pending ops / setter targets / changed masks
    uint8_t* dirty_any = nullptr;   // -> pool->dirty_any: some engine of the pool is dirty (lets a steady block skip the per-engine scans)
    uint32_t* host_ops_any = nullptr; // -> pool->host_ops_any: NUMBER of engines that hold host-queued ops (a burst then stays on the host: queue order)
    // (test before set: sixteen MIDI threads storing to the one shared byte on every event bounce its cache line -- 520 ms instead of 40 for
    // a 16.7 M-event re-strike; a read of an already-set flag stays shared)
    void mark() { if (dirty) { *dirty = 1; if (!__atomic_load_n(dirty_any, __ATOMIC_RELAXED)) __atomic_store_n(dirty_any, (uint8_t)1, __ATOMIC_RELAXED); } }
    void sync_masks(int s) { vm_sync_masks(*vm, s); mark(); }
    void touch() { mark(); }
    // Sink of the shared state machine on the host: the engine's own op list
    void push(uint8_t type, int slot, uint8_t note, bool mlp, uint32_t seed, double vel) {
        OwOp op;
        op.type = type; op.slot = (uint8_t)slot; op.note = note; op.mlp = mlp ? 1 : 0; op.seed = seed; op.velocity = vel;
        ops.push_back(op);
        if (host_ops_any && ops.size() == 1) __atomic_fetch_add(host_ops_any, 1u, __ATOMIC_RELAXED);     // once per engine and block, not per event
        mark();
    }
};

struct ow_pool {
    int device = 0;
    size_t I = 0;
    size_t Lcap = 0;
    OwConsts hc{};
    // Every device resource below is an owning member (host_base.inc) and releases itself in ~ow_pool, in reverse order of declaration:
    // the streams come first so that they go last, after every buffer and event.
    // Created in this order (pool_create): the runtime deals streams onto the hardware queues in creation order, and the oscillator must
    // not share a queue with the audio stream.
    StreamOwner stream;                // voices -> preamp -> output stage
    StreamOwner stream_trem;           // tremolo oscillator: no audio input (tremolo.rs:121), runs beside the voices
    StreamOwner stream_copy;           // copies beside the kernels: state download of a device MIDI burst, background state upload after a block
    Event ev_trem[2];                  // one per rbuf half
    // The tremolo oscillator is produced one block ahead (speculating that the next block has the same length); the
    // tremolo rows of the chain state are backed up first so a mis-speculation can be rolled back.
    DevBuf<double> d_trem_backup;      // [18][I]
    int rb_cur = 0;                    // rbuf half holding the R samples of the block being rendered
    struct { bool valid = false; int e0 = 0, ne = 0, n_os = 0; } spec;
    DevBuf<OwConsts> dK;        // constants at the pool's rates
    DevBuf<OwConsts> dK48;      // tremolo codegen-rate matrices for CircuitState::warmup
    DevBuf<double> d_nt;
    DevBuf<double> d_vrec;
    DevBuf<double> d_cs;
    int power_amp_kind = 0;           // OW_POWER_AMP_BEHAVIORAL / OW_POWER_AMP_MELANGE
    int tremolo_kind = 0;             // OW_TREMOLO_TWIN_T / OW_TREMOLO_LEGACY_LFO (the reference's `legacy-tremolo` cargo feature)
    DevBuf<OwPaConsts> dPa;           // melange power amp: constants at the chain rate
    DevBuf<double> d_pa;              // melange power amp: per-engine state, [PAS_COUNT][I]
    DevBuf<double> d_pa_settled;      // settled circuit state (PAS_CIRCUIT_END doubles), power_amp.rs:288-296
    DevBuf<double> d_pa_tap;          // test tap: amp output per chain-rate sample, [2 * Lcap][I] (ow_test_pool_enable_power_amp_tap)
    DevBuf<uint32_t> d_pa_demand;     // [I] Newton passes of the engine's last block (k_post_mpa), 0 = not rendered yet
    DevBuf<uint32_t> d_pa_order;      // [I] engines of a launch range by falling demand (k_pa_order_*)
    DevBuf<uint32_t> d_pa_hist;       // [256] class counts / cursors of the range
    size_t pa_tap_cap = 0;
    DevBuf<double> d_mel_settled;     // melange preamp: settled codegen-rate state (18 doubles)
    size_t mel_lu_ld = 0;             // column-streamed literal kernel: lanes per row of d_mel_lu
    DevBuf<double> d_mel_lu;          // literal kernel: LU workspace of the generic rebuild, [ceil(I/32) + OW_MAX_SLICES + 1][12][12][32]
    DevBuf<double> d_noise;           // melange preamp: thermal-noise state of the main solver states, [NZ_COUNT][I]
    DevBuf<double> d_sum;
    DevBuf<double> d_rbuf;
    DevBuf<double> d_pre;
    DevBuf<float> d_out;
    size_t out_ld = 0;                // row stride of d_out for the block it holds: rows are packed at the block length, so that the copy of
                                      // a block to the host is ONE linear transfer (copy engine) instead of a pitched one (blit kernel)
    DevBuf<OwEngineArgs> d_args;
    DevBuf<OwEngineOut> d_eout;
    DevBuf<OwOp> d_ops;
    size_t ops_cap = 0;
    PinBuf<OwEngineArgs> h_args;      // pinned
    PinBuf<OwEngineOut> h_eout;       // pinned
    // Status summary of a block (big pools): k_eout_attention marks the engines whose status block the host has to look at (a voice
    // fell silent, a steal fade is running, a guard fired, the transient flag changed); the host copies one bit per engine and fetches
    // the status blocks themselves only when a bit is set -- a steady block of 131 072 engines then costs the host 16 KB instead of a
    // 5 MB copy and a 131 072-entry scan.
    DevBuf<uint32_t> d_skew_seen;     // k_voice_steady: some wavefront of the launch held voices on more than one 16-sample jitter grid
    PinBuf<uint32_t> h_skew_seen;     // pinned
    bool skew_next = false, skew_pending = false;   // variant of the next steady launch; a report is on its way
    DevBuf<uint64_t> d_attn;          // [ceil(I / 64)]
    PinBuf<uint64_t> h_attn;          // pinned
    DevBuf<uint8_t> d_prev_tr;        // [I] transient flag the host knows (p->transient)
    PinBuf<uint8_t> h_prev_tr;        // pinned staging of p->transient for a resync
    bool attn_pending = false;        // the block just rendered left its summary in h_attn instead of its status blocks in h_eout
    bool attn_resync = true;          // d_prev_tr has to be refreshed from p->transient before the next summary
    bool eout_all_live = true;        // a block went through the status-block path: any h_eout entry may hold something
    std::vector<uint32_t> eout_live;  // engines whose h_eout entry holds something other than "nothing happened" (cleared next block)
    uint8_t dirty_any = 1;            // some dirty[] entry may be set (engines set it; a whole-pool render clears it)
    bool any_cache_valid = false, any_main_c = false, any_steal_c = false;   // any_main / any_steal of the last whole-pool render
    DevBuf<OwEngineOut> d_eout_packed;      // [I] status blocks of a list of engines, packed (voice-sum NaN guard's second pass)
    PinBuf<OwEngineOut> h_eout_packed;      // pinned
    PinBuf<OwOp> h_ops;               // pinned
    // Voice-pool states (ow_vm.h): h_vm is what the engines' host state machine works on; a burst of events (ow_pool_midi on a big pool) is
    // applied to d_vm by k_vm_events and copied back.  vm_host_dirty: the host changed some state since d_vm was last written.
    PinBuf<OwVm> h_vm;                // pinned [I]
    DevBuf<OwVm> d_vm;                // [I], allocated with the first burst
    DevBuf<OwOp> d_ops_fix;           // [I][OW_VM_OPS_MAX] op queues written by the device
    PinBuf<ow_midi_event> h_ev;       // pinned staging of a burst's events (lists that are not in a pinned block themselves)
    DevBuf<ow_midi_event> d_ev;
    size_t ev_cap = 0;
    DevBuf<uint32_t> d_ev_begin;      // [2][I] slice of every engine in the burst's list
    uint8_t vm_host_dirty = 1;
    uint32_t host_ops_any = 0;        // engines that hold host-queued ops (counted where a queue becomes non-empty / is drained: a host that mixes
                                      // single-engine events with partial renders gets the device bursts back as soon as the queues are empty)
    DevBuf<uint32_t> d_vm_ovf;        // a device queue overflowed during the burst (the burst is then replayed on the host)
    PinBuf<uint32_t> h_vm_ovf;        // pinned
    bool vm_download_pending = false; // d_vm -> h_vm is in flight (ev_vm)
    Event ev_vm;
    Event ev_vm_events;   // k_vm_events of the last burst has finished (the download waits for it on its own stream)
    // Once a pool has taken a burst on the device, the host's copy of the states goes up again in the BACKGROUND whenever a block's
    // book-keeping has changed it (end of ow_pool_render, copy stream, beside the next block's kernels): the next burst then finds the
    // device's copy current instead of starting with 126 MB of upload.  A host change while that copy is in flight sets vm_host_dirty
    // again (vm_host_changed comes first), and the burst uploads as before.
    Event ev_vm_up;
    bool vm_upload_inflight = false;
    // The last burst's queues were applied at once (k_apply_ops launched by ow_pool_midi, beside the download of the states): the engines
    // of [applied_lo, applied_hi) whose downloaded state still says "n_dev_ops queued" have nothing queued any more -- vm_wait_download
    // settles that on the host's copy and marks them as inside a note-on's phases for the next block's dispatch.
    bool dev_ops_applied = false;
    uint32_t applied_lo = 0, applied_hi = 0;
    bool dev_ops_pending = false;     // some engine's next ops sit in d_ops_fix
    uint64_t vm_bursts = 0;           // bursts that went through the device (test hook)
    struct OpTail { uint32_t src, dst, n; };   // host-queued ops of an engine that also has device-queued ones: appended on the device
    std::vector<OpTail> op_tails;
    std::mutex op_tails_mu;
    // Packed voice dispatch (ow_kernels.h): lane = sounding voice.  Three block lists of (engine << 6 | slot) entries, rebuilt when a
    // mask, a pending op or a transient flag changed: steady slot voices, slot voices of engines in a transient phase, steal voices.
    // sig: signature of the (engine, mask) sequence the device copy was packed from (two independent 64-bit hashes + layout); a rebuild that
    // arrives at the same signature leaves the list alone (the blocks after a whole-pool re-strike repack 33 MB per list otherwise)
    struct VoiceList { PinBuf<uint32_t> h; DevBuf<uint32_t> d; uint32_t n_blocks = 0; uint64_t sig[3] = {0, 0, 0}; bool sig_valid = false; };
    VoiceList vl_steady, vl_general, vl_steal, vl_attack;     // vl_attack: engines inside onset ramps / attack noise whose slot voices are not damping (k_voice_steady<false, 1>)
    std::vector<uint8_t> transient;   // per engine: device status after the previous block (OwEngineOut::transient)
    bool lists_valid = false;
    int lists_e0 = -1, lists_ne = -1;
    Event ev_stage[5];                // profiling: before voices, after voices, before preamp, after preamp, after post
    DevBuf<uint32_t> d_op_engines;    // engines that have pending ops this block (k_apply_ops runs one block per entry)
    PinBuf<uint32_t> h_op_engines;    // pinned, I entries
    std::vector<std::unique_ptr<ow_engine>> engines;   // the C-ABI hands out the (stable) ow_engine* inside
    std::vector<uint8_t> dirty;       // per engine: host state changed since the args were last uploaded
    bool args_stale = true;           // device args still hold one-shot fields of the previous block
    // Tremolo phase groups: engines whose Twin-T / CdS state is bit-identical (everything since their last chain init happened in
    // lock-step) share ONE oscillator: the group's leader (its lowest engine index) carries the 18 tremolo rows of the chain state and
    // owns a column of rbuf, the other members read that column.  A fresh pool is one group; ow_engine_reset / ow_engine_warm_up of a
    // single engine split it off (per-engine fallback), a whole-pool reset / rate change merges everything again.
    PinBuf<uint32_t> h_lead;          // pinned [I]: leader engine of every engine
    DevBuf<uint32_t> d_lead;
    PinBuf<uint32_t> h_leaders;       // pinned [I]: compact list of the leaders inside the range being rendered
    DevBuf<uint32_t> d_leaders;
    PinBuf<uint32_t> h_copy;          // pinned [2][I]: (src, dst) pairs for k_trem_copy_rows
    DevBuf<uint32_t> d_copy;
    std::vector<uint32_t> grp_in, grp_out;   // scratch of trem_split_at_range (first member inside / outside the range, per leader)
    int n_lead = 0, lead_e0 = -1, lead_ne = -1;
    bool lead_list_valid = false;     // d_leaders matches (lead_e0, lead_ne) and the current groups
    int split_e0 = -1, split_ne = -1; // range for which "no group straddles the range boundary" is known to hold
    DevBuf<double> d_snap;            // [3][I] smoother targets (depth, speaker, volume) handed to k_chain_init on reset
    PinBuf<double> h_snap;            // pinned
    DevBuf<double> d_trem_settled;    // staging of one cached settled Twin-T state (18 doubles), see trem_settled_rows
    DevBuf<uint32_t> d_zero;          // one zero (leader list {0} of the I = 1 settle scratch)
    // Shared trajectory (TremTraj): engines of a Twin-T pool read r_ldr[t] of ONE process-wide sequence at t = trem_clock - birth[e].
    // trem_clock advances with every whole-pool block; a sub-range rendered on its own shifts the births of its engines instead.
    // birth == OW_OFF_TRAJ: the engine left the trajectory (older than the store's cap) and owns a phase group of one.
    std::shared_ptr<TremTraj> traj;
    long long trem_clock = 0;
    long long min_birth = 0;          // over the engines on the trajectory (the oldest one decides how far the store must reach)
    size_t n_on_traj = 0;
    std::vector<long long> h_birth;   // [I]
    DevBuf<long long> d_birth;
    DevBuf<unsigned long long> d_evict;      // [3][I] scratch of trem_evict (engine list, positions, fallback counts): render never allocates
    long long last_n_os = 0;          // chain-rate samples of the last rendered block (ow_pool_read_tremolo_r)
    Switches sw;                      // latched at creation
    bool voices_only = false;         // ow_render_note: the pool renders voice sums only -- no chain state, no tremolo / preamp / output kernels
    int inject_faults = 0;            // test hook (openwurli_hip_test.h): the next n renders fail before their first launch
    bool steal_counted = false;       // the block in flight had its steal fades counted down while its kernels ran (steal_countdown_early)
    double hostprof_acc[4] = {0, 0, 0, 0};
    long hostprof_cnt = 0;
    bool profiling = false;
    Event ev[8];
    float last_ms[5] = {0, 0, 0, 0, 0};
    size_t last_len = 0;
    ~ow_pool();                       // (host_settle.inc) drains the streams; the members release themselves after that
};
