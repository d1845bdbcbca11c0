// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): errors, device buffers, persistent host workers, latched switches.
namespace {

thread_local std::string g_err;
void set_err(const std::string& s) { g_err = s; }

// Master seed 0 of the reference = "entropy from the system clock" (gen_preamp.rs:1512-1521), taken once per process because
// every preamp clones one cached state (melange_adapter.rs:12-29).  OW_NOISE_SEED overrides it (reproducible runs).
uint64_t process_noise_seed() {
    static const uint64_t seed = []() -> uint64_t {
        if (const char* env = std::getenv("OW_NOISE_SEED")) { const unsigned long long v = std::strtoull(env, nullptr, 0); if (v) return (uint64_t)v; }
        const uint64_t t = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
        return t ? t : (uint64_t)0x0123456789ABCDEFull;
    }();
    return seed;
}

#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// Pinned host blocks handed out by ow_host_alloc: mapped into the device's address space, so the output stage of a big pool can store a
// rendered block straight into the caller's buffer (no d_out -> host copy trailing the last kernel).  render looks a target up here;
// anything else (pageable memory, blocks pinned by somebody else) takes the staged copy.
std::mutex g_host_mu;
struct HostBlock { size_t bytes; void* dptr; };
std::map<uintptr_t, HostBlock> g_host_blocks;
void host_block_register(void* ptr, size_t bytes, void* dptr) { std::lock_guard<std::mutex> lk(g_host_mu); g_host_blocks[(uintptr_t)ptr] = HostBlock{bytes, dptr}; }
void host_block_forget(void* ptr) { std::lock_guard<std::mutex> lk(g_host_mu); g_host_blocks.erase((uintptr_t)ptr); }
// device address of [ptr, ptr + bytes) when it lies inside one registered block, else nullptr
void* host_block_device_ptr(const void* ptr, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_blocks.upper_bound((uintptr_t)ptr);
    if (it == g_host_blocks.begin()) return nullptr;
    --it;
    const uintptr_t off = (uintptr_t)ptr - it->first;
    if (!it->second.dptr || off > it->second.bytes || bytes > it->second.bytes - off) return nullptr;
    return (char*)it->second.dptr + off;
}

// Owning handles: device buffer, pinned host buffer, event, stream.  Each is move-only, releases on every exit path, and is the ONE place
// that acquires and releases its kind of resource.  Every acquisition passes acquiring() first and counts itself afterwards -- the two
// test hooks ow_test_fail_acquire_after / ow_test_live_resources (openwurli_hip_test.h); neither happens during a steady render.
std::atomic<uint64_t> g_live_resources{0};
thread_local int g_fail_acquire_after = -1;
void acquiring() {
    if (g_fail_acquire_after >= 0 && g_fail_acquire_after-- == 0) throw std::runtime_error("ow_test_fail_acquire_after: injected acquisition failure");
}
void live(int d) { g_live_resources.fetch_add((uint64_t)(int64_t)d, std::memory_order_relaxed); }
#define OW_OWNER(T, h)                                                                 \
    T() = default;                                                                     \
    T(T&& o) noexcept : h(o.h) { o.h = nullptr; }                                      \
    T& operator=(T&& o) noexcept { std::swap(h, o.h); return *this; } /* o releases what this held */ \
    ~T() { reset(); }
struct DevMem {
    void* p = nullptr;
    OW_OWNER(DevMem, p)
    void reset() { if (p) { hipFree(p); p = nullptr; live(-1); } }
    void alloc(size_t bytes) { reset(); acquiring(); HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 8))); live(1); }
    void* release() { void* q = p; if (q) live(-1); p = nullptr; return q; }     // hands the buffer to an owner outside these types (TremTraj)
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct PinMem {
    void* p = nullptr;
    OW_OWNER(PinMem, p)
    void reset() { if (p) { hipHostFree(p); p = nullptr; live(-1); } }
    void alloc(size_t bytes) { reset(); acquiring(); HIP_OK(hipHostMalloc(&p, bytes)); live(1); }
};
// n elements of T in device (DevBuf) / pinned host (PinBuf) memory; reads as the raw T* wherever one is expected
template <class T, class Mem> struct Typed : Mem {
    void alloc(size_t n) { Mem::alloc(sizeof(T) * n); }
    operator T*() const { return static_cast<T*>(this->p); }
};
template <class T> using DevBuf = Typed<T, DevMem>;
template <class T> using PinBuf = Typed<T, PinMem>;
struct Event {
    hipEvent_t e = nullptr;
    OW_OWNER(Event, e)
    void reset() { if (e) { hipEventDestroy(e); e = nullptr; live(-1); } }
    void create(unsigned flags = hipEventDisableTiming) { reset(); acquiring(); HIP_OK(hipEventCreateWithFlags(&e, flags)); live(1); }
    operator hipEvent_t() const { return e; }
};
struct StreamOwner {
    hipStream_t s = nullptr;
    OW_OWNER(StreamOwner, s)
    void reset() { if (s) { hipStreamDestroy(s); s = nullptr; live(-1); } }
    void create(unsigned flags = hipStreamNonBlocking) { reset(); acquiring(); HIP_OK(hipStreamCreateWithFlags(&s, flags)); live(1); }
    operator hipStream_t() const { return s; }
};

// Persistent host worker threads.  The realtime entry points (ow_pool_render, ow_pool_midi) must not allocate once capacity is
// ensured (SURVEY.md 8b: nih-plug's assert_process_allocs; engine.rs:288-297), and starting a std::thread allocates its state
// block and a stack: big pools therefore cut their per-engine host work into slices that run on these threads, started once
// per process and parked on a condition variable in between.  run() hands out slice indices from an atomic counter; the
// caller works too.  No std::function, no heap: the job is a function pointer + context pointer.
class Workers {
  public:
    static Workers& get() { static Workers w; return w; }
    // fn(ctx, t) for t in [0, T); returns when all slices are done.  One dispatch at a time (callers of different pools serialise).
    void run(size_t T, void (*fn)(void*, size_t), void* ctx) {
        // run() is not re-entered from inside a slice by anything in this library; if it ever is (in_slice_ set on this thread), the nested
        // call runs its slices inline -- std::mutex::try_lock on a mutex the calling thread already owns would be undefined behaviour.
        if (T <= 1 || th_.empty() || in_slice_) { for (size_t t = 0; t < T; ++t) fn(ctx, t); return; }
        // One dispatch at a time.  A second caller (another pool rendering on another audio thread) does NOT wait for the workers -- a
        // realtime thread blocked on a mutex that lower-priority work holds is a priority inversion -- it runs its slices itself, one
        // after the other: the same work as a single-threaded pass over the range (the slices partition it), i.e. the cost of a host with
        // one core, not a wait of unknown length.  Two pools of >= 16 384 engines rendering concurrently from two audio threads is the only
        // configuration that gets here.
        std::unique_lock<std::mutex> one(dispatch_mu_, std::try_to_lock);
        if (!one.owns_lock()) { for (size_t t = 0; t < T; ++t) fn(ctx, t); return; }
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = fn; ctx_ = ctx; total_ = T; next_.store(0); done_ = 0; ++gen_;
        }
        cv_.notify_all();
        size_t mine = 0;
        in_slice_ = true;
        for (size_t t; (t = next_.fetch_add(1)) < T; ++mine) fn(ctx, t);
        in_slice_ = false;
        std::unique_lock<std::mutex> lk(mu_);
        done_ += mine;
        cv_done_.wait(lk, [&] { return done_ == total_ && active_ == 0; });
        fn_ = nullptr;
    }
    template <class F> void each(size_t T, F& f) { run(T, [](void* c, size_t t) { (*static_cast<F*>(c))(t); }, &f); }
    size_t threads() const { return th_.size() + 1; }

  private:
    Workers() {
        size_t n = host_threads();
        for (size_t i = 1; i < n; ++i) th_.emplace_back([this] { loop(); });
    }
    ~Workers() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    static size_t host_threads();
    void loop() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            void (*fn)(void*, size_t) = fn_;
            void* ctx = ctx_;
            const size_t T = total_;
            if (!fn) continue;
            ++active_;
            lk.unlock();
            size_t mine = 0;
            in_slice_ = true;
            for (size_t t; (t = next_.fetch_add(1)) < T; ++mine) fn(ctx, t);
            in_slice_ = false;
            lk.lock();
            done_ += mine;
            --active_;
            if (done_ == total_ && active_ == 0) cv_done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_, dispatch_mu_;
    std::condition_variable cv_, cv_done_;
    void (*fn_)(void*, size_t) = nullptr;
    void* ctx_ = nullptr;
    size_t total_ = 0, done_ = 0, active_ = 0;
    std::atomic<size_t> next_{0};
    uint64_t gen_ = 0;
    bool stop_ = false;
    static thread_local bool in_slice_;
};
thread_local bool Workers::in_slice_ = false;
#define OW_MAX_SLICES 64   // upper bound of the slices one dispatch is cut into (scratch arrays live on the stack)

struct HostSmoother {  // host mirror of LinearSmoother::target only (the 1e-9 acceptance test, engine.rs:86-89)
    double target;
    bool pending = false;
    double pending_value = 0.0;
    void set_target(double t) {
        if (std::fabs(t - target) < 1e-9) return;
        target = t;
        pending = true;
        pending_value = t;
    }
};

// Measurement and test switches.  Every OW_* environment variable that selects between kernel paths is read ONCE, when a pool is
// created or an offline entry point is called (std::getenv is neither realtime-safe nor safe against a concurrent setenv in the host),
// and kept there; the render path only looks at the latched copy.  ow_test_pool_set_switch (openwurli_hip_test.h) changes one on a live pool.
// Kinds, and what a switch takes from its environment variable (by the first character, Switches::flag's rule; SW_COUNT: the whole number;
// anything outside lo..hi leaves the default) and from set():
//   SW_BOOL 0 / 1 (set: value != 0)   SW_TRI -1 = by size / 0 / 1 (set: negative -> -1, else value != 0)   SW_RANGE, SW_COUNT lo..hi (set refuses the rest)
enum SwitchKind { SW_BOOL, SW_TRI, SW_RANGE, SW_COUNT };
static bool switch_from_env(const char* env, SwitchKind kind, long long lo, long long hi, long long* v) {
    const char* e = env ? std::getenv(env) : nullptr;
    if (!e || !e[0]) return false;
    *v = kind == SW_COUNT ? std::atoll(e) : (long long)(e[0] - '0');
    return *v >= lo && *v <= hi;
}
static bool switch_from_set(SwitchKind kind, long long lo, long long hi, long long* v) {
    if (kind == SW_BOOL) *v = *v != 0;
    else if (kind == SW_TRI) *v = *v < 0 ? -1 : (*v != 0);
    return *v >= lo && *v <= hi;
}
// THE table of switches, one row each: member type, name (the member; what the test hooks and ow_test_block_plan call it), default,
// environment variable (nullptr: none), kind, lo, hi, settable (false: it shapes a pool at creation or belongs to the offline entry
// points -- environment only).  Everything below the table is generated from it.
#define OW_SWITCH_TABLE(X) \
    X(int, trem_wide, -1, "OW_TREM_WIDE", SW_TRI, -1, 1, true)                         /* -1: by pool size */ \
    X(int, preamp_wide, -1, "OW_PREAMP_WIDE", SW_TRI, -1, 1, true)                     /* -1: by pool size */ \
    X(int, chain_fused, -1, "OW_CHAIN_FUSED", SW_TRI, -1, 1, true)                     /* preamp + output stage as one launch (k_chain_fused); -1: whenever the quad preamp is used */ \
    X(bool, trem_serial, false, "OW_TREM_SERIAL", SW_BOOL, 0, 1, true)                 /* 1: block-ahead oscillators in front of the voices instead of beside them */ \
    X(bool, trem_cache, true, "OW_TREM_CACHE", SW_BOOL, 0, 1, false)                   /* 0: no process-wide settled-state cache */ \
    X(bool, trem_traj, true, "OW_TREM_TRAJ", SW_BOOL, 0, 1, false)                     /* 0: no shared trajectory, one oscillator per phase group (rounds 1-3) */ \
    X(bool, mel_rank1, false, "OW_MEL_RANK1", SW_BOOL, 0, 1, true)                     /* the melange preamp kernels: see choose_chain */ \
    X(bool, mel_lds, false, "OW_MEL_LDS", SW_BOOL, 0, 1, true)                         \
    X(bool, mel_generic, false, "OW_MEL_GENERIC", SW_BOOL, 0, 1, true)                 \
    X(int, mel_eng, 0, "OW_MEL_ENG", SW_BOOL, 0, 1, true)                              /* 1: lane = engine melange kernel (k_preamp_mel_eng; measured -3 % at 131 072 engines, 2x slower at 65 536) */ \
    X(bool, voice_skew, true, "OW_VOICE_SKEW", SW_BOOL, 0, 1, true)                    /* 0: the steady voice kernel without skewed lane clocks (one jitter grid per wavefront assumed) */ \
    X(int, pa_sort, 1, "OW_PA_SORT", SW_RANGE, 0, 2, true)                             /* 0 never, 1 when the block exceeds the chip, 2 always */ \
    X(int, eout_attn, -1, "OW_EOUT_ATTN", SW_TRI, -1, 1, true)                         /* status summary instead of the status blocks (k_eout_attention); -1: ranges of >= 8 192 engines */ \
    X(int, midi_device, -1, "OW_MIDI_DEVICE", SW_TRI, -1, 1, true)                     /* bursts of ow_pool_midi applied on the device (k_vm_events) never / whenever the list allows; -1: pools of >= 8 192 engines, >= 65 536 events */ \
    X(int, midi_apply_early, 1, "OW_MIDI_APPLY_EARLY", SW_BOOL, 0, 1, true)            /* 0: the queues of a device burst wait for the next render's k_apply_ops */ \
    X(int, voice_release, 1, "OW_VOICE_RELEASE", SW_BOOL, 0, 1, true)                  /* 0: no release variant of the steady voice kernel (k_voice renders every engine with a damping voice) */ \
    X(int, voice_steal, 1, "OW_VOICE_STEAL", SW_BOOL, 0, 1, true)                      /* 0: no steal variant of the steady voice kernel (k_voice renders every crossfade) */ \
    X(int, voice_attack, 1, "OW_VOICE_ATTACK", SW_BOOL, 0, 1, true)                    /* 0: no attack variant of the steady voice kernel (engines in onset / noise phases go to the general kernel) */ \
    X(bool, force_general, false, nullptr, SW_BOOL, 0, 1, true)                        /* test / probe hook: every engine's slot voices go to the general voice kernel (what it costs without any phase active) */ \
    X(int, chain_row, -1, "OW_CHAIN_ROW", SW_TRI, -1, 1, true)                         /* the fused chain launch with one solver state per row of sixteen lanes (k_chain_row) never / whenever the chain is fused; -1: ranges of <= 1 024 engines */ \
    X(int, chain_stream, -1, "OW_CHAIN_STREAM", SW_TRI, -1, 1, true)                   /* preamp + output stage of a big oversampled pool as one launch (k_chain_stream); -1: when the block goes to a pinned host block */ \
    X(int, post_pair, -1, "OW_POST_PAIR", SW_TRI, -1, 1, true)                         /* the oversampled output stage with lane = engine (k_post<false, true>) never / always; -1: ranges of >= 131 072 engines (two wavefronts per SIMD without the lane pair) */ \
    X(int, preamp_pair, -1, "OW_PREAMP_PAIR", SW_TRI, -1, 1, true)                     /* the legacy preamp on the lane path with lane = engine, main and shadow state in one lane (k_preamp_pair) never / always; -1: ranges of >= 131 072 engines */ \
    X(int, out_direct, -1, "OW_OUT_DIRECT", SW_TRI, -1, 1, true)                       /* output stage stores straight into a pinned host block (ow_host_alloc) instead of d_out + copy; -1: default */ \
    X(bool, host_profile, false, "OW_HOST_PROFILE", SW_BOOL, 0, 1, true)               /* 1: ow_pool_render prints launch / wait / post of every slow block */ \
    X(int, midi_threads, 0, "OW_MIDI_THREADS", SW_COUNT, 1, 64, false)                 \
    X(long long, calib_chunk, 0, "OW_CALIB_CHUNK", SW_COUNT, 1, LLONG_MAX, false)      /* at most n points per chunk of ow_calibrate (tests); 0: the device-memory budget alone */ \
    X(long long, pbench_chunk, 0, "OW_PBENCH_CHUNK", SW_COUNT, 1, LLONG_MAX, false)    /* at most n points per launch of ow_preamp_measure (tests); 0: one launch, or the trace budget */ \
    X(long long, poly_chunk, 0, "OW_POLY_CHUNK", SW_COUNT, 1, LLONG_MAX, false)        /* at most n chords per chunk of ow_render_poly (tests); 0: the device-memory budget alone */ \
    X(long long, centroid_chunk, 0, "OW_CENTROID_CHUNK", SW_COUNT, 1, LLONG_MAX, false) /* at most n jobs per chunk of ow_centroid_track (tests); 0: the device-memory budget alone */ \
    X(long long, note_audit_chunk, 0, "OW_NOTE_AUDIT_CHUNK", SW_COUNT, 1, LLONG_MAX, false) /* at most n jobs per chunk of ow_intermod_audit / ow_overshoot (tests); 0: the device-memory budget alone */ \
    X(long long, pump_chunk, 0, "OW_PUMP_CHUNK", SW_COUNT, 1, LLONG_MAX, false)        /* at most n points per launch of ow_pump_measure (tests); 0: the device-memory budget alone */ \
    X(int, pbench_row, -1, "OW_PBENCH_ROW", SW_TRI, -1, 1, false)                      /* force the lane-pair / row kernel of ow_preamp_measure (legacy); -1: by grid size */ \
    X(int, chain_wide, -1, "OW_CHAIN_WIDE", SW_TRI, -1, 1, false)                      /* job paths (host_jobs_chain.inc): a quad of lanes per preamp state never / always; -1: up to 8 192 jobs */ \
    X(int, job_fused, -1, "OW_JOB_FUSED", SW_TRI, -1, 1, false)                        /* ... as preamp | output stage on two wavefronts (k_job_chain_fused) never / always; -1: up to 4 096 jobs */ \
    X(bool, job_overlap, true, "OW_JOB_OVERLAP", SW_BOOL, 0, 1, false)                 /* 0: the batch render's voices in front of the fused chain instead of beside it */ \
    X(int, job_row, -1, "OW_JOB_ROW", SW_TRI, -1, 1, false)                            /* ... with a row of sixteen lanes per solver state (k_job_chain_row) never / always; -1: up to 1 024 jobs */ \
    X(long long, bark_chunk, 0, "OW_BARK_CHUNK", SW_COUNT, 1, LLONG_MAX, false)        /* at most n jobs per chunk of ow_bark_audit (tests); 0: the device-memory budget alone */ \
    X(int, bark_row, -1, "OW_BARK_ROW", SW_TRI, -1, 1, false)                          /* force the lane-pair / row chain kernel of ow_bark_audit (legacy); -1: launches of up to 4 096 jobs take the row */
struct Switches {
#define X(type, name, dflt, env, kind, lo, hi, settable) type name = dflt;
    OW_SWITCH_TABLE(X)
#undef X
    static int flag(const char* name, int dflt) { const char* e = std::getenv(name); return (e && e[0]) ? (e[0] - '0') : dflt; }
    static Switches from_env() {
        Switches w;
        long long v;
#define X(type, name, dflt, env, kind, lo, hi, settable) if (switch_from_env(env, kind, lo, hi, &v)) w.name = (type)v;
        OW_SWITCH_TABLE(X)
#undef X
        return w;
    }
    bool set(const char* n, int value) {       // false: unknown name, not settable, or a value the switch refuses
        long long v = value;
#define X(type, name, dflt, env, kind, lo, hi, settable) if (!std::strcmp(n, #name)) { if (!(settable) || !switch_from_set(kind, lo, hi, &v)) return false; name = (type)v; return true; }
        OW_SWITCH_TABLE(X)
#undef X
        return false;
    }
    bool get(const char* n, int* value) const {
#define X(type, name, dflt, env, kind, lo, hi, settable) if (!std::strcmp(n, #name)) { *value = (int)std::min<long long>((long long)name, 0x7FFFFFFF); return true; }
        OW_SWITCH_TABLE(X)
#undef X
        return false;
    }
};

struct TremTraj;   // shared Twin-T / CdS trajectory of one (device, chain rate), below
std::atomic<uint64_t> g_ops_dropped{0};      // slot ops that found no room behind a device-side burst (render_range; OW_MIDI_APPLY_EARLY=0 only)

}  // namespace
