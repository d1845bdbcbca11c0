// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): voice-pool mirror synchronisation, process-wide settled states (melange preamp / power amp, Twin-T).
namespace {

// The host mirror of the voice-pool states is current (a burst applied on the device is copied back asynchronously: wait for it), and
// the host is about to change / has changed one of them (the device copy is stale until the next burst uploads them again).
void vm_settle_applied(ow_pool* p);
void vm_wait_download(ow_pool* p) {
    if (p && p->vm_download_pending) { hipEventSynchronize(p->ev_vm); p->vm_download_pending = false; if (p->dev_ops_applied) vm_settle_applied(p); }
}
void vm_host_current(const ow_engine* e) { if (e && e->pool) vm_wait_download(e->pool); }
void vm_host_changed(ow_engine* e) { if (e && e->pool && !__atomic_load_n(&e->pool->vm_host_dirty, __ATOMIC_RELAXED)) __atomic_store_n(&e->pool->vm_host_dirty, (uint8_t)1, __ATOMIC_RELAXED); }

// Drop a pending block-ahead tremolo result: restore the oscillator rows it advanced and drain the tremolo stream.
void invalidate_spec(ow_pool* p) {
    if (p->spec.valid) {
        hipMemcpyAsync(p->d_cs, p->d_trem_backup, sizeof(double) * 18 * p->I, hipMemcpyDeviceToDevice, p->stream_trem);
        p->spec.valid = false;
    }
    if (p->stream_trem) hipStreamSynchronize(p->stream_trem);
}

// Block buffers for `cap` samples.  The pool stands at capacity 0 from the moment the old ones are released until all the new ones exist:
// a grow that fails leaves a pool whose next render grows again (len > Lcap) instead of launching on buffers that are gone.
void alloc_stream_buffers(ow_pool* p, size_t cap) {
    invalidate_spec(p);
    p->Lcap = 0;
    p->d_sum.reset(); p->d_rbuf.reset(); p->d_pre.reset(); p->d_out.reset();
    const size_t I = p->I;
    p->d_sum.alloc(2 * I * cap);
    p->d_rbuf.alloc(2 * (2 * cap * I));   // two halves (current block, block ahead)
    p->d_pre.alloc(2 * cap * I);
    p->d_out.alloc(I * cap);
    HIP_OK(hipMemsetAsync(p->d_out, 0, sizeof(float) * I * cap, p->stream));
    if (p->d_pa_tap) p->d_pa_tap.alloc(2 * cap * I);      // the test tap follows the block capacity
    p->Lcap = cap;
}

// Op staging (pinned + device).  pool_create sizes it for a whole-keyboard re-strike of EVERY engine in one block (damper +
// move-to-steal + note-on per key = 192 ops of 16 B per engine), so ow_pool_render never gets here with n > ops_cap unless more
// than that was queued between two renders -- the only case in which a render allocates (like the reference's buffer auto-grow).
void ensure_ops_capacity(ow_pool* p, size_t n) {
    if (n <= p->ops_cap) return;
    size_t cap = std::max<size_t>(n, std::max<size_t>(p->ops_cap * 2, 256));
    p->ops_cap = 0;                        // until both exist: a failed allocation leaves a pool that grows again
    p->d_ops.alloc(cap);
    p->h_ops.alloc(cap);
    p->ops_cap = cap;
}

// Settled state of the melange preamp (melange_adapter.rs:12-20): rate-independent (always computed at the 48 kHz codegen
// tables), so it is produced once per device by k_mel_settle and cached, like the reference's OnceLock.
std::mutex g_mel_mu;
std::map<int, std::vector<double>> g_mel_settled;
void mel_settled_to_device(int device, double* d_dst, hipStream_t st) {
    // the process-wide mutex guards the maps only: a cached state is copied out under it and transferred after it is released (a pool
    // with a long queued stream must not hold up every other thread's pool creation / reset)
    std::vector<double> h;
    { std::lock_guard<std::mutex> lk(g_mel_mu); auto it = g_mel_settled.find(device); if (it != g_mel_settled.end()) h = it->second; }
    if (h.empty()) {
        OwConsts k48;
        owhip::build_consts(k48, 24000.0, OW_PREAMP_MELANGE12);   // os_sr = 48 kHz -> codegen tables
        DevMem dk;
        dk.alloc(sizeof(OwConsts));
        HIP_OK(hipMemcpyAsync(dk.p, &k48, sizeof(OwConsts), hipMemcpyHostToDevice, st));
        owdev::k_mel_settle<<<dim3(1), dim3(64), 0, st>>>(dk.as<OwConsts>(), d_dst);
        h.resize(18);
        HIP_OK(hipMemcpyAsync(h.data(), d_dst, sizeof(double) * 18, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::lock_guard<std::mutex> lk(g_mel_mu);
        g_mel_settled[device] = h;          // two threads racing here computed the same bits
        return;
    }
    HIP_OK(hipMemcpyAsync(d_dst, h.data(), sizeof(double) * 18, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
}

// Settled state of the melange power amp (power_amp.rs:288-296): always computed with the codegen-rate matrices, once per device.
std::map<int, std::vector<double>> g_pa_settled;
void pa_settled_to_device(int device, double* d_dst, hipStream_t st) {
    std::vector<double> h;
    { std::lock_guard<std::mutex> lk(g_mel_mu); auto it = g_pa_settled.find(device); if (it != g_pa_settled.end()) h = it->second; }
    if (h.empty()) {
        std::unique_ptr<OwPaConsts> h88(new OwPaConsts());
        owhip::build_pa_consts(*h88, PA_SAMPLE_RATE);
        DevMem dk;
        dk.alloc(sizeof(OwPaConsts));
        HIP_OK(hipMemcpyAsync(dk.p, h88.get(), sizeof(OwPaConsts), hipMemcpyHostToDevice, st));
        owdev::k_mpa_settle<<<dim3(1), dim3(64), 0, st>>>(dk.as<OwPaConsts>(), d_dst);
        HIP_OK(hipGetLastError());
        h.resize(owdev::PAS_CIRCUIT_END);
        HIP_OK(hipMemcpyAsync(h.data(), d_dst, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::lock_guard<std::mutex> lk(g_mel_mu);
        g_pa_settled[device] = h;
        return;
    }
    HIP_OK(hipMemcpyAsync(d_dst, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
}

// Settled state of the Twin-T oscillator (Tremolo::new: CircuitState::default's 50 warm-up steps at the codegen matrices, then 2 s of
// oscillator steps at the chain rate, tremolo.rs:92-102).  It depends on nothing but the chain rate, and it is 192 050 strictly serial
// solver steps -- 0.9 s on one wavefront -- which every pool creation, reset and rate change used to pay.  The reference caches its
// expensive settles the same way (OnceLock: melange_adapter.rs:12-29, power_amp.rs:283-299).  Keyed by (device, chain rate); the cached
// rows are what the product kernels produced on the first use, so a hit is bit-identical to a fresh settle
// (tests/test_gpu_boundary.py::test_settled_tremolo_cache_is_bit_identical).  OW_TREM_CACHE=0 disables it.
// OW_TREM_ROW=0: the quad-lane oscillator step (ow_trem_wide.h) for the settle and the shared trajectory instead of the row step
// (ow_trem_row.h).  Same samples either way (tests/test_gpu_trajectory.py); read once per process.
bool trem_row_enabled() { static const bool on = Switches::flag("OW_TREM_ROW", 1) != 0; return on; }
struct TremSettled { double rows[18]; };       // rows 0..16 after the settle; [17] = BE fallbacks the settle itself counted (u64 bits)
std::map<std::pair<int, uint64_t>, TremSettled> g_trem_settled;

// Settled rows for (device, chain rate), from the cache or by running the settle on `st` with the product kernels (k_tremolo_wide<true>:
// 50 steps at the codegen matrices, 2 s at the chain rate) in the 18-row scratch `d_state` (I = 1 layout).  use_cache = false: always
// settle, never store (OW_TREM_CACHE=0).  On return d_state holds the settled rows with row 17 = the settle's own fallback count.
TremSettled trem_settled_rows(int device, double os_sr, const OwConsts* dK, const OwConsts* dK48, double* d_state, const uint32_t* d_zero, hipStream_t st,
                              bool use_cache) {
    uint64_t rate_bits; std::memcpy(&rate_bits, &os_sr, 8);
    const std::pair<int, uint64_t> key(device, rate_bits);
    TremSettled t;
    if (use_cache) {
        bool hit = false;
        { std::lock_guard<std::mutex> lk(g_mel_mu); auto it = g_trem_settled.find(key); if (it != g_trem_settled.end()) { t = it->second; hit = true; } }
        if (hit) {     // copied out under the lock; the transfer and its sync run without it
            HIP_OK(hipMemcpyAsync(d_state, t.rows, sizeof(double) * 18, hipMemcpyHostToDevice, st));
            HIP_OK(hipStreamSynchronize(st));
            return t;
        }
    }
    const long long n_settle = (long long)owhip::sat_u32(os_sr * 2.0);
    owdev::k_trem_state_dc<<<dim3(1), dim3(64), 0, st>>>(d_state);
    if (trem_row_enabled()) {      // one system per wavefront (ow_trem_row.h): bit-identical, ~0.55 x the time
        owdev::k_trem_settle_row<<<dim3(1), dim3(64), 0, st>>>(dK48, d_state, 50LL);
        owdev::k_trem_settle_row<<<dim3(1), dim3(64), 0, st>>>(dK, d_state, n_settle);
    } else {
        owdev::k_tremolo_wide<true><<<dim3(1), dim3(64), 0, st>>>(dK48, d_state, nullptr, 1, 50LL, d_zero, 1);
        owdev::k_tremolo_wide<true><<<dim3(1), dim3(64), 0, st>>>(dK, d_state, nullptr, 1, n_settle, d_zero, 1);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(t.rows, d_state, sizeof(double) * 18, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (use_cache) { std::lock_guard<std::mutex> lk(g_mel_mu); g_trem_settled[key] = t; }
    return t;
}
}  // namespace

ow_pool::~ow_pool() {      // also of a pool that pool_create gave up half-way: whatever exists is drained, then the members release themselves
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    invalidate_spec(this);                                   // (drains the tremolo stream)
    if (stream_copy) hipStreamSynchronize(stream_copy);
}
