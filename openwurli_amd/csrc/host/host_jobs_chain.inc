// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): kernel choice for the job paths and the job chain (batch render, render-midi).
namespace {
enum { INIT_NEW = 1, INIT_RATE = 2, INIT_RESET = 0 };

// Job paths (batch render, render-midi): a quad of lanes per preamp state (ow_chain_wide.h) while the jobs are too few to fill the
// chip with one lane pair each -- their run time is then the chain's serial latency.  OW_CHAIN_WIDE=0/1 forces the choice (the
// parity test compares the two kernels bit for bit).  These switches are read with the rest of the call's Switches, once per call.
static inline bool chain_wide(const Switches& sw, size_t n_jobs) { return sw.chain_wide >= 0 ? sw.chain_wide == 1 : n_jobs <= 8192; }
// OW_JOB_FUSED=0: the quad job chain as one wavefront (k_job_chain_wide) instead of preamp | output stage on two (k_job_chain_fused)
// (two wavefronts of 400+ registers per eight jobs: 512 workgroups fill the chip, more of them take a second round -- 8 192 jobs measured
// 319 against 191 ms -- so the fused form is for up to 4 096 jobs)
static inline bool job_chain_fused(const Switches& sw, size_t n_jobs) { return chain_wide(sw, n_jobs) && (sw.job_fused >= 0 ? sw.job_fused == 1 : n_jobs <= 4096); }
// The batch render may run the voices of its jobs BESIDE this chain (ow_batch_render: k_job_voice on a second stream publishes its
// progress, k_job_chain_fused waits chunk by chunk): only while the chain's workgroups leave SIMDs free for the voice kernel -- 2 048 jobs
// are 256 workgroups of two one-per-SIMD wavefronts, half the chip -- so that the producer can always be scheduled.  OW_JOB_OVERLAP=0: never.
static inline bool job_voice_overlap(const Switches& sw, size_t n_jobs) { return sw.job_overlap && job_chain_fused(sw, n_jobs) && n_jobs <= 2048; }
// OW_JOB_ROW=0: the fused job chain with a quad per solver state (k_job_chain_fused) instead of a row of sixteen lanes (k_job_chain_row:
// five wavefronts per eight jobs -- while they all find a SIMD of their own beside the voice kernel)
static inline bool job_chain_row(const Switches& sw, size_t n_jobs) { return sw.job_row >= 0 ? sw.job_row == 1 : n_jobs <= 1024; }
static void launch_job_chain_legacy(const Switches& sw, const OwConsts* dK, const owdev::OwJobDev* d_jobs, const double* d_in, double* d_out, size_t n_jobs,
                                    long long n, long long stride, hipStream_t st, const int* voice_prog = nullptr) {
    const bool wide = chain_wide(sw, n_jobs), fused = job_chain_fused(sw, n_jobs);
    if (voice_prog && !fused) throw std::runtime_error("job chain: overlap with the voices needs the fused chain");
    int* const gave_up = voice_prog ? const_cast<int*>(voice_prog) + (n_jobs + 63) / 64 : nullptr;
    if (fused && job_chain_row(sw, n_jobs))
        owdev::k_job_chain_row<<<dim3((unsigned)((n_jobs + 7) / 8)), dim3(320), 0, st>>>(dK, d_jobs, d_in, d_out, (int)n_jobs, n, stride, voice_prog, gave_up);
    else if (fused)
        owdev::k_job_chain_fused<<<dim3((unsigned)((n_jobs + 7) / 8)), dim3(128), 0, st>>>(dK, d_jobs, d_in, d_out, (int)n_jobs, n, stride, voice_prog, gave_up);
    else if (wide)
        owdev::k_job_chain_wide<<<dim3((unsigned)((n_jobs + 7) / 8)), dim3(64), 0, st>>>(dK, d_jobs, d_in, d_out, (int)n_jobs, n, stride);
    else
        owdev::k_job_chain<false><<<dim3((unsigned)((n_jobs + 31) / 32)), dim3(64), 0, st>>>(dK, d_jobs, d_in, d_out, nullptr, (int)n_jobs, n, stride);
}

ow_pool* pool_create(double sample_rate, size_t n_engines, int device, int preamp_kind, int power_amp_kind, int tremolo_kind, bool voices_only, bool no_traj = false);

// The chain of the job paths (`preamp-bench render` / `render-midi`, tools/preamp-bench/src/main.rs:413-497, 1880-1890) for n_jobs rows
// of voice signal d_in -> d_out (both [n_jobs][stride]), with everything the commands' flags can ask for:
//   * --tremolo-depth > 0 on some job: ONE Twin-T stream for the call (Tremolo::new settles every job's oscillator to the same state,
//     and the oscillator takes no input), produced by the product's own tremolo kernel from a freshly built pool of one; each job
//     applies its own depth divider;
//   * the melange preamp (`--features melange-preamp` build) through k_job_chain<true>;
//   * the melange power amp (a build without `legacy-power-amp`): PowerAmp::new() is new_at_sample_rate(44 100) whatever the render's
//     rate is (power_amp.rs:321-323), it runs at the BASE rate on preamp x volume^2 -- as its own launch (MelPowerAmpStage) between the
//     chain kernel and the speaker stage.
// `call` is the entry point's OfflineCall at cfg.sample_rate / cfg.preamp_kind: its stream, constants and switches.
struct JobChainCfg { double sample_rate; int device, preamp_kind, power_amp_kind, no_rail_sag; };
// true when run_job_chain will take the plain legacy chain (launch_job_chain_legacy) for these jobs
static bool job_chain_is_plain_legacy(const JobChainCfg& cfg, const std::vector<owdev::OwJobDev>& hj) {
    if (cfg.preamp_kind != OW_PREAMP_LEGACY8) return false;
    bool any_pa = false;
    for (const auto& j : hj) {
        if ((j.tremolo_depth > 0.0 && !j.no_preamp) || j.no_preamp || j.dc_at_ldr) return false;
        any_pa = any_pa || j.poweramp;
    }
    return !(cfg.power_amp_kind == OW_POWER_AMP_MELANGE && any_pa);
}
void run_job_chain(OfflineCall& call, const JobChainCfg& cfg, const std::vector<owdev::OwJobDev>& hj, const owdev::OwJobDev* d_jobs, const double* d_in,
                   double* d_out, size_t n_jobs, long long n, long long stride, const int* voice_prog = nullptr) {
    require_known_kinds(cfg.preamp_kind, cfg.power_amp_kind);
    const OwConsts* dK = call.dK();
    hipStream_t st = call.st();
    bool any_trem = false, any_special = false, any_pa = false;
    for (const auto& j : hj) {
        any_trem = any_trem || (j.tremolo_depth > 0.0 && !j.no_preamp);
        any_special = any_special || j.no_preamp || j.dc_at_ldr;      // dc_at_ldr (centroid-track): only k_job_chain knows it
        any_pa = any_pa || j.poweramp;
    }
    const bool mpa = cfg.power_amp_kind == OW_POWER_AMP_MELANGE && any_pa;
    DevMem d_r, d_att, d_amp;
    std::shared_ptr<TremTraj> traj;
    const double* trem = nullptr;
    if (any_trem) {
        // Tremolo::new(depth, preamp rate) without a warm-up: every job's cell starts at t = 0 of the shared trajectory of this chain rate
        const bool os = cfg.sample_rate < 88200.0;
        const long long n_os = n * (os ? 2 : 1);
        const Switches& sw = call.sw;
        if (sw.trem_traj) {
            std::unique_ptr<OwConsts> hc(new OwConsts()), k48(new OwConsts());
            owhip::build_consts(*hc, cfg.sample_rate, OW_PREAMP_LEGACY8);
            owhip::build_consts(*k48, 24000.0, OW_PREAMP_LEGACY8);
            traj = traj_acquire(cfg.device, *hc, *k48, sw.trem_cache);
            if ((size_t)n_os <= traj->cap_max) {
                traj->grow_to((size_t)n_os);                 // (offline entry point: allocating here is fine; no-op when the buffers reach that far)
                hipEvent_t ev;
                { std::lock_guard<std::mutex> lk(traj->mu); ev = traj->cover((size_t)n_os, 0); trem = traj->d_r; }
                if (ev) HIP_OK(hipStreamWaitEvent(st, ev, 0));
            }
        }
        if (!trem) {                                        // longer than the store: one oscillator for this call, from a pool of one
            d_r.alloc(sizeof(double) * (size_t)n_os);
            std::unique_ptr<ow_pool> g(pool_create(cfg.sample_rate, 1, cfg.device, OW_PREAMP_LEGACY8, OW_POWER_AMP_BEHAVIORAL, OW_TREMOLO_TWIN_T, false, /*no_traj=*/true));
            // the fresh pool's oscillator rows are Tremolo::new's settled state; n_os steps of Tremolo::process, R written per step
            owdev::k_tremolo_wide<false><<<dim3(1), dim3(64), 0, g->stream>>>(g->dK, g->d_cs, d_r.as<double>(), 1, n_os, g->d_leaders, 1);
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(g->stream));
            trem = d_r.as<double>();
        }
    }
    double* chain_out = d_out;
    if (mpa) {
        d_att.alloc(sizeof(double) * n_jobs * (size_t)stride);
        d_amp.alloc(sizeof(double) * n_jobs * (size_t)stride);
        chain_out = d_att.as<double>();
    }
    const int out_mode = mpa ? owdev::JOB_OUT_PA_INPUT : owdev::JOB_OUT_FINAL;
    if (cfg.preamp_kind == OW_PREAMP_MELANGE12) {
        owdev::k_job_chain<true><<<dim3((unsigned)((n_jobs + 31) / 32)), dim3(64), 0, st>>>(dK, d_jobs, d_in, chain_out, call.mel_settled(), (int)n_jobs, n, stride,
                                                                                            trem, out_mode);
    } else if (!any_trem && !any_special && !mpa) {
        launch_job_chain_legacy(call.sw, dK, d_jobs, d_in, chain_out, n_jobs, n, stride, st, voice_prog);
    } else {
        owdev::k_job_chain<false><<<dim3((unsigned)((n_jobs + 31) / 32)), dim3(64), 0, st>>>(dK, d_jobs, d_in, chain_out, nullptr, (int)n_jobs, n, stride, trem, out_mode);
    }
    HIP_OK(hipGetLastError());
    if (mpa) {
        MelPowerAmpStage pa(cfg.device, st);
        pa.run(d_att.as<double>(), d_amp.as<double>(), n, (int)n_jobs, cfg.no_rail_sag ? 0 : 1, stride);
        owdev::k_job_speaker<<<dim3((unsigned)((n_jobs + 63) / 64)), dim3(64), 0, st>>>(dK, d_jobs, d_att.as<double>(), d_amp.as<double>(), d_out, (int)n_jobs, n, stride);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));      // the stage and the staging buffers go out of scope
    }
    HIP_OK(hipStreamSynchronize(st));
}
}  // namespace
