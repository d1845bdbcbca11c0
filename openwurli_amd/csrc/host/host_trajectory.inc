// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): the shared Twin-T / CdS trajectory store (TremTraj), its helper thread, traj_acquire.
namespace {
// ---- shared Twin-T / CdS trajectory --------------------------------------------------------------------------------------------------
// Tremolo::process reads no audio and no depth (tremolo.rs:121-146) and every Tremolo::new / reset leaves the same settled state
// (:83-102, :192-216): r_ldr[t], t = process() calls since the cell was built, is one deterministic sequence per chain rate.  The store
// holds it in HBM once per (device, chain rate) for the life of the process; the engine with the largest t extends it with ONE oscillator
// (k_trem_traj_extend, a single wavefront on the store's own stream), every other engine of every pool reads it.  288 GB of HBM is what
// makes this the natural layout: 0.77 MB per second of audio at 96 kHz, OW_TREM_TRAJ_SECONDS (default 1800) of it reserved up front so
// that render never allocates.  Engines that grow older than that leave the store for an oscillator of their own (trem_evict).
struct TremTraj {
    int device = 0;
    double os_sr = 0.0;
    std::mutex mu;                    // guards len / cap / buffers / marks / enqueues on `stream`; held for host-side enqueue work only
    StreamOwner stream;               // (first: released last, after the buffers and marks)
    DevBuf<OwConsts> dK;              // constants at the chain rate (the tremolo fields are all the kernels read)
    double* d_r = nullptr;            // [cap + 64]; plain, like d_ckpt: a growth swaps them and retires the old ones
    DevBuf<double> d_state;           // [18] oscillator rows at sample `len`
    double* d_ckpt = nullptr;         // [cap / OW_TRAJ_CK + 2][OW_TRAJ_CKD]
    DevBuf<unsigned long long> d_be;  // [1 + OW_TRAJ_BE_CAP]
    DevBuf<uint32_t> d_zero;          // leaders = {0} for the settle kernels
    size_t cap = 0, len = 0;          // cap: samples the buffers hold; len: samples produced or enqueued for production
    size_t cap_max = 0;               // configured capacity (ow_tremolo_configure / OW_TREM_TRAJ_SECONDS): the buffers grow up to it, an engine
                                      // older than this leaves the store (trem_evict)
    size_t lead = 0;                  // samples the store is kept ahead of a fast reader (a small pool) by the feeder thread
    size_t target = 0;                // where the feeder is taking the store (<= cap)
    size_t reader_end = 0, reader_block = 1024;   // furthest sample a fast reader asked for, and its block (feeder back-off)
    std::chrono::steady_clock::time_point reader_seen{};
    size_t done = 0;                  // samples known to be complete (a recorded mark was seen finished)
    uint64_t be_settle = 0;           // fallbacks the settle itself counted (what a fresh CircuitState carries after Tremolo::new)
    static constexpr int NMARK = 16;
    struct Mark { size_t end = 0; Event ev; } mark[NMARK];
    int head = 0;
    bool grow_requested = false;      // the helper thread has been asked to double the buffers
    std::vector<void*> retired;       // buffers a growth replaced: kernels launched before the swap may still read them, so they are only
                                      // freed at the NEXT growth (minutes of audio later) or with the store
    ~TremTraj() {
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        if (d_r) hipFree(d_r); if (d_ckpt) hipFree(d_ckpt);
        for (void* q : retired) hipFree(q);
    }
    static size_t ckpt_doubles(size_t c) { return (size_t)OW_TRAJ_CKD * (c / OW_TRAJ_CK + 2); }
    // Buffers for `new_cap` samples: allocate (no lock held: hipMalloc may take milliseconds), then under the lock copy what exists on the
    // store's stream -- behind every extension already enqueued -- and swap.  Readers that fetch the new pointer wait for the copy's mark.
    void grow_to(size_t new_cap) {
        new_cap = std::min((new_cap + OW_TRAJ_CK - 1) / OW_TRAJ_CK * OW_TRAJ_CK, cap_max);
        { std::lock_guard<std::mutex> lk(mu); if (new_cap <= cap) { grow_requested = false; return; } }
        HIP_OK(hipSetDevice(device));
        DevMem nr, nc;                                     // released on every exit path until the swap below takes them over
        nr.alloc(sizeof(double) * (new_cap + 64));
        nc.alloc(sizeof(double) * ckpt_doubles(new_cap));
        std::vector<void*> to_free;                        // hipFree drains the whole device: never under `mu` (a render thread in cover() would wait for it)
        {
            std::lock_guard<std::mutex> lk(mu);
            if (new_cap <= cap) { grow_requested = false; return; }
            to_free.swap(retired);                         // replaced one growth ago
            HIP_OK(hipMemcpyAsync(nr.p, d_r, sizeof(double) * (len + 64 <= cap + 64 ? len + 64 : cap + 64), hipMemcpyDeviceToDevice, stream));
            HIP_OK(hipMemcpyAsync(nc.p, d_ckpt, sizeof(double) * ckpt_doubles(cap), hipMemcpyDeviceToDevice, stream));
            Mark& m = mark[head];
            head = (head + 1) % NMARK;
            HIP_OK(hipEventRecord(m.ev, stream));
            m.end = len;
            retired.push_back(d_r); retired.push_back(d_ckpt);
            d_r = (double*)nr.release(); d_ckpt = (double*)nc.release(); cap = new_cap;
            done = 0;                                      // everything has to be waited for again (the copy)
            for (Mark& o : mark) if (&o != &m && o.end <= len) o.end = 0;     // older marks stand for data in the old buffer
            grow_requested = false;
        }
        for (void* q : to_free) hipFree(q);
    }
    // callers hold mu
    void extend_to(size_t end) {
        end = std::min(end, cap);
        if (end <= len) return;
        if (trem_row_enabled()) owdev::k_trem_traj_extend_row<<<dim3(1), dim3(64), 0, stream>>>(dK, d_state, d_r + len, (long long)len, (long long)(end - len), d_ckpt, d_be);
        else owdev::k_trem_traj_extend<<<dim3(1), dim3(64), 0, stream>>>(dK, d_state, d_r + len, (long long)len, (long long)(end - len), d_ckpt, d_be);
        HIP_OK(hipGetLastError());
        Mark& m = mark[head];
        head = (head + 1) % NMARK;
        HIP_OK(hipEventRecord(m.ev, stream));
        m.end = end;
        len = end;
    }
    // extension launches not known to have finished (their marks)
    int in_flight() {
        int n = 0;
        for (Mark& m : mark) if (m.end > done) { if (hipEventQuery(m.ev) == hipSuccess) done = std::max(done, m.end); else ++n; }
        return n;
    }
    // Make samples [0, end) exist (enqueue what is missing on the store's stream), then keep the store `ahead` samples further (one block:
    // what the next render will ask for).  lead_for > 0: the caller is a reader that can outrun real time (a small pool): the store's
    // target moves to end + lead_for and the feeder thread (TrajGrower) keeps the oscillator running towards it -- two short launches in
    // flight at a time, whether or not anybody renders meanwhile.  (Deep queues do not work here: a consumer stream that waits for a mark
    // of this stream was measured to resume only when everything enqueued on it had finished -- with a second of oscillator steps queued,
    // every block of a pool at the frontier waited 0.4 s.)  Returns true in *feed when the feeder has something new to do.
    // Returns the event a consumer stream has to wait for before it reads [0, end), or nullptr when they are known to be complete.  (The
    // event may be re-recorded by a later extension before the consumer waits on it: it then stands for a longer prefix -- still sufficient.)
    hipEvent_t cover(size_t end, size_t ahead, size_t lead_for = 0, bool* feed = nullptr) {
        end = std::min(end, cap);
        extend_to(end);
        hipEvent_t wait = nullptr;
        if (end > done) {
            const Mark* best = nullptr;
            for (const Mark& m : mark) if (m.end >= end && (!best || m.end < best->end)) best = &m;
            if (best) {
                if (hipEventQuery(best->ev) == hipSuccess) done = std::max(done, best->end);
                else wait = best->ev;
            }
        }
        if (ahead) extend_to(end + ahead);
        if (lead_for) {
            const size_t t = std::min(end + lead_for, cap);
            if (t > target) { target = t; if (feed && len < target) *feed = true; }
            reader_end = std::max(reader_end, end);
            if (ahead) reader_block = ahead;
            reader_seen = std::chrono::steady_clock::now();
        }
        return wait;
    }
    // Feeder thread: one more short launch towards `target` when fewer than two are in flight; true while there is more to do.
    // It stands back while a reader renders right behind the frontier (a pool that outruns the oscillator): such a reader enqueues exactly
    // the block ahead it needs (`ahead` above), and anything the feeder put in front of that would only be more for it to wait for.  The
    // lead is built whenever readers are further back or idle -- between a host's instantiation and its first block, between blocks of
    // a host paced at real time.
    bool feed_step() {
        std::lock_guard<std::mutex> lk(mu);
        const size_t t = std::min(target, cap);
        if (len >= t) return false;
        const bool reader_active = reader_end > 0 && std::chrono::steady_clock::now() - reader_seen < std::chrono::milliseconds(20);
        if (reader_active && len < reader_end + 8 * reader_block) return true;
        if (in_flight() < 2) extend_to(std::min(len + 2048, t));
        return len < t;
    }
    // the store should soon be longer than its buffers are (callers hold mu)
    bool wants_growth(size_t end) const { return cap < cap_max && !grow_requested && std::max(end, target) + (size_t)(30.0 * os_sr) > cap; }
    // the recorded fallback events ([0] = count, [1 + k] = sample index), one transfer however many engines ask
    // No wait for the store's stream (the background extension keeps it busy for seconds at a time): whoever asks stands at a t whose
    // samples a FINISHED launch produced, so the events below t are in memory; entries a running launch has counted but not yet written
    // read as ~0 (the list is initialised to all ones) and lie above every t.
    std::vector<unsigned long long> be_events() {
        std::vector<unsigned long long> h(1 + OW_TRAJ_BE_CAP, 0ull);
        if (hipMemcpy(h.data(), d_be, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) != hipSuccess) std::fill(h.begin(), h.end(), 0ull);
        return h;
    }
    // fallback count of an engine standing at sample t (diag): the settle's own + the recorded events below t
    uint64_t be_count_at(long long t, const std::vector<unsigned long long>& h) const {
        uint64_t n = be_settle;
        const size_t k = (size_t)std::min<unsigned long long>(h[0], OW_TRAJ_BE_CAP);
        for (size_t i = 0; i < k; ++i) n += h[1 + i] < (unsigned long long)std::max<long long>(t, 0);
        if (h[0] > OW_TRAJ_BE_CAP) n += h[0] - OW_TRAJ_BE_CAP;     // beyond the list: counted, not placed
        return n;
    }
    uint64_t be_count_at(long long t) { return be_count_at(t, be_events()); }
};
std::mutex g_traj_mu;
// The registry is LEAKED on purpose (never destroyed): a static map's destructor would run ~TremTraj -- HIP calls -- during exit(),
// after the HIP runtime and any profiler attached to it have begun to shut down (rocprofv3 aborts there and the process hangs).  Stores
// die when ow_test_clear_settle_caches drops them and the last pool lets go; at process exit the driver reclaims the memory.
using TrajMap = std::map<std::pair<int, uint64_t>, std::shared_ptr<TremTraj>>;
TrajMap& traj_registry() { static TrajMap* m = new TrajMap(); return *m; }

// ow_tremolo_configure: capacity / lead of the stores of a device (seconds of audio at the chain rate); what is not configured comes from
// OW_TREM_TRAJ_SECONDS / OW_TREM_TRAJ_LEAD_SECONDS, then the defaults.
struct TrajConfig { double seconds = 0.0, lead = -1.0; };
std::map<int, TrajConfig> g_traj_cfg;      // guarded by g_traj_mu
constexpr double OW_TRAJ_DEFAULT_SECONDS = 1800.0, OW_TRAJ_DEFAULT_LEAD = 60.0, OW_TRAJ_FIRST_SECONDS = 150.0;

// Buffers grow on a helper thread (hipMalloc is no work for a thread that renders): cover() asks when the store comes within lead + 30 s
// of the end of its buffers, the helper doubles them.  One thread per process, started with the first store, parked on a condition
// variable; leaked like the registry (it must not touch the runtime while the process exits).
struct TrajGrower {
    // fixed tables: feed() / ask() are called from render, and the thread's own rounds run while hosts audit allocations -- nothing here
    // touches the heap (weak_ptr copies only count references)
    static constexpr int CAP = 16;
    std::mutex mu;
    std::condition_variable cv;
    std::weak_ptr<TremTraj> todo[CAP];     // stores whose buffers should double
    std::weak_ptr<TremTraj> fed[CAP];      // stores on their way to their target
    int n_todo = 0, n_fed = 0;
    bool stopping = false, parked = false;
    static bool same(const std::weak_ptr<TremTraj>& a, const std::weak_ptr<TremTraj>& b) { return !a.owner_before(b) && !b.owner_before(a); }
    void ask(const std::shared_ptr<TremTraj>& t) {
        { std::lock_guard<std::mutex> lk(mu); if (n_todo < CAP) todo[n_todo++] = t; }
        cv.notify_one();
    }
    void feed(const std::shared_ptr<TremTraj>& t) {
        {
            std::lock_guard<std::mutex> lk(mu);
            const std::weak_ptr<TremTraj> w(t);
            for (int i = 0; i < n_fed; ++i) if (same(fed[i], w)) return;          // already on the list
            if (n_fed == CAP) return;                                            // (sixteen chain rates x devices being fed at once: the renders' own block ahead remains)
            fed[n_fed++] = w;
        }
        cv.notify_one();
    }
    void stop() {       // from the exit handler: the thread makes no further runtime call once this returns (or after 2 s)
        std::unique_lock<std::mutex> lk(mu);
        stopping = true;
        cv.notify_all();
        cv.wait_for(lk, std::chrono::seconds(2), [&] { return parked; });
    }
    void run() {
        for (;;) {
            std::weak_ptr<TremTraj> grow[CAP], feeding[CAP];
            int n_grow = 0, n_feeding = 0;
            {
                std::unique_lock<std::mutex> lk(mu);
                if (stopping) { parked = true; cv.notify_all(); for (;;) cv.wait(lk); }
                if (n_fed == 0) cv.wait(lk, [&] { return stopping || n_todo > 0 || n_fed > 0; });
                else cv.wait_for(lk, std::chrono::milliseconds(1));      // a launch of 2 048 steps lasts ~5 ms: look again soon
                if (stopping) { parked = true; cv.notify_all(); for (;;) cv.wait(lk); }
                for (int i = 0; i < n_todo; ++i) { grow[n_grow++] = todo[i]; todo[i].reset(); }
                n_todo = 0;
                for (int i = 0; i < n_fed; ++i) feeding[n_feeding++] = fed[i];
            }
            for (int i = 0; i < n_grow; ++i)
                if (std::shared_ptr<TremTraj> t = grow[i].lock()) {
                    try { size_t c; { std::lock_guard<std::mutex> lk(t->mu); c = t->cap; } t->grow_to(c * 2); }
                    catch (const std::exception& ex) { (void)hipGetLastError(); std::lock_guard<std::mutex> lk(t->mu); t->cap_max = t->cap; t->grow_requested = false;
                                                       std::fprintf(stderr, "openwurli-hip: tremolo trajectory store stays at %zu samples (%s)\n", t->cap, ex.what()); }
                }
            bool more[CAP] = {false};
            for (int i = 0; i < n_feeding; ++i)
                if (std::shared_ptr<TremTraj> t = feeding[i].lock()) {
                    try {
                        if (hipSetDevice(t->device) == hipSuccess) more[i] = t->feed_step();
                        bool ask_grow = false;
                        { std::lock_guard<std::mutex> lk(t->mu); if (t->wants_growth(t->len)) { t->grow_requested = true; ask_grow = true; } }
                        if (ask_grow) { std::lock_guard<std::mutex> lk(mu); if (n_todo < CAP) todo[n_todo++] = t; }
                    } catch (const std::exception&) { (void)hipGetLastError(); more[i] = false; }
                }
            {
                std::lock_guard<std::mutex> lk(mu);
                // stores that were added while this round ran stay; the ones this round finished go
                int k = 0;
                for (int i = 0; i < n_fed; ++i) {
                    bool was = false, stays = false;
                    for (int j = 0; j < n_feeding; ++j) if (same(fed[i], feeding[j])) { was = true; stays = more[j]; }
                    if (!was || stays) { if (k != i) fed[k] = fed[i]; ++k; }
                }
                for (int i = k; i < n_fed; ++i) fed[i].reset();
                n_fed = k;
            }
        }
    }
};
TrajGrower& traj_grower() {
    static TrajGrower* g = [] {
        TrajGrower* x = new TrajGrower();
        std::thread([x] { x->run(); }).detach();
        // exit(): handlers run in reverse order of registration, so this one -- registered long after the HIP runtime's own -- parks the
        // thread before the runtime starts to come down (a launch or an event query during teardown crashes the process)
        std::atexit([] { traj_grower().stop(); });
        return x;
    }();
    return *g;
}

// the store of (device, hc.os_sr), created (and settled) on first use.  n_engines: size of the pool that asks -- a big pool reserves the
// whole configured capacity at once (render never waits for a growth), a small one starts with 150 s (115 MB at 96 kHz) and grows.
std::shared_ptr<TremTraj> traj_acquire(int device, const OwConsts& hc, const OwConsts& k48, bool use_settle_cache, size_t n_engines = 1) {
    uint64_t rate_bits; std::memcpy(&rate_bits, &hc.os_sr, 8);
    const std::pair<int, uint64_t> key(device, rate_bits);
    std::shared_ptr<TremTraj> t;
    {
    std::lock_guard<std::mutex> lk(g_traj_mu);
    TrajMap& g_traj = traj_registry();
    auto it = g_traj.find(key);
    if (it != g_traj.end()) t = it->second;
    else {
    t = std::make_shared<TremTraj>();
    t->device = device; t->os_sr = hc.os_sr;
    TrajConfig cfg;
    { auto c = g_traj_cfg.find(device); if (c != g_traj_cfg.end()) cfg = c->second; }
    double seconds = cfg.seconds > 0.0 ? cfg.seconds : OW_TRAJ_DEFAULT_SECONDS, lead = cfg.lead >= 0.0 ? cfg.lead : OW_TRAJ_DEFAULT_LEAD;
    if (!(cfg.seconds > 0.0)) if (const char* env = std::getenv("OW_TREM_TRAJ_SECONDS")) { const double v = std::atof(env); if (v > 0.0) seconds = v; }
    if (!(cfg.lead >= 0.0)) if (const char* env = std::getenv("OW_TREM_TRAJ_LEAD_SECONDS")) { const double v = std::atof(env); if (v >= 0.0) lead = v; }
    const double want = std::min(seconds * hc.os_sr, 4.0e9);
    t->cap_max = ((size_t)want + OW_TRAJ_CK - 1) / OW_TRAJ_CK * OW_TRAJ_CK;
    t->lead = (size_t)std::min(lead * hc.os_sr, (double)t->cap_max);
    const size_t first = n_engines >= 4096 ? t->cap_max : std::min(t->cap_max, ((size_t)(OW_TRAJ_FIRST_SECONDS * hc.os_sr) + OW_TRAJ_CK - 1) / OW_TRAJ_CK * OW_TRAJ_CK);
    t->cap = first;
    t->stream.create();
    for (auto& m : t->mark) m.ev.create();
    DevMem r, ck;
    t->dK.alloc(1);
    r.alloc(sizeof(double) * (t->cap + 64)); t->d_r = (double*)r.release();
    t->d_state.alloc(18);
    ck.alloc(sizeof(double) * TremTraj::ckpt_doubles(t->cap)); t->d_ckpt = (double*)ck.release();
    t->d_be.alloc(1 + OW_TRAJ_BE_CAP);
    t->d_zero.alloc(1);
    HIP_OK(hipMemsetAsync(t->d_be, 0xFF, sizeof(unsigned long long) * (1 + OW_TRAJ_BE_CAP), t->stream));
    HIP_OK(hipMemsetAsync(t->d_be, 0, sizeof(unsigned long long), t->stream));
    HIP_OK(hipMemsetAsync(t->d_zero, 0, sizeof(uint32_t), t->stream));
    HIP_OK(hipMemcpyAsync(t->dK, &hc, sizeof(OwConsts), hipMemcpyHostToDevice, t->stream));
    DevMem dk48;
    dk48.alloc(sizeof(OwConsts));
    HIP_OK(hipMemcpyAsync(dk48.p, &k48, sizeof(OwConsts), hipMemcpyHostToDevice, t->stream));
    const TremSettled ts = trem_settled_rows(device, hc.os_sr, t->dK, dk48.as<OwConsts>(), t->d_state, t->d_zero, t->stream, use_settle_cache);
    std::memcpy(&t->be_settle, &ts.rows[17], 8);
    HIP_OK(hipMemsetAsync(t->d_state + 17, 0, sizeof(double), t->stream));   // the trajectory's own events go to d_be
    HIP_OK(hipStreamSynchronize(t->stream));
    g_traj[key] = t;
    traj_grower();                                                        // the helper thread exists before any render could need it
    }
    }
    // (outside the registry lock) a big pool on a store that was created small: all of it now, where allocating is allowed
    if (n_engines >= 4096) t->grow_to(t->cap_max);
    // a small pool can outrun the one oscillator: it starts to run ahead right away, fed by the helper thread, so that a host that never
    // calls ow_tremolo_prefetch finds its first blocks' samples waiting.  (A big pool renders far slower than the oscillator steps and
    // only ever needs the block ahead that its own renders enqueue.)
    if (n_engines < 4096) {
        bool feed = false;
        { std::lock_guard<std::mutex> lk(t->mu); t->cover(0, 0, t->lead, &feed); }
        if (feed) traj_grower().feed(t);
    }
    return t;
}
}  // namespace
