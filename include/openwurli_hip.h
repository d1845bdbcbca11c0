/* openwurli-hip: C-ABI of the MI355X (gfx950) render core for the OpenWurli DSP hot path.
 *
 * This is the drop-in boundary: plain C, opaque handles, raw pointers and sizes.  Each entry
 * point replaces one item of the `openwurli-dsp` Rust public API that the nih-plug shell,
 * tools/reed-renderer and tools/preamp-bench call today (citations into /root/reference/).
 * A Rust facade with the reference's method names forwards 1:1.
 *
 * Conventions kept from the reference: one thread drives an engine; realtime
 * calls never fail (bad input is clamped, numeric failure degrades to silence + counters);
 * render() does not allocate once ensure_buffer_capacity() has been called; output is mono f32.
 * Only constructors and the offline entry points report errors (NULL / negative return).
 *
 * A *pool* is the MI355X-native unit: I independent engines at one sample rate that render in
 * lock-step: one lane per sounding voice (packed across engines) in the voice kernels, one lane
 * per engine in the chain kernels.  An `ow_engine*` is one engine of a pool;
 * `ow_engine_new` creates a pool of one.
 */
#ifndef OPENWURLI_HIP_H
#define OPENWURLI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ow_pool ow_pool;
typedef struct ow_engine ow_engine;

/* Version of this header's struct layouts and signatures.  ow_abi_version() returns the value the library was built with; a binding
 * checks it once after loading.  The by-pointer configuration structs (ow_batch_cfg, ow_midi_render_cfg) additionally carry their own
 * size in their first field, and ow_batch_cfg / ow_calibrate_cfg / ow_preamp_measure_cfg / ow_poly_cfg / ow_centroid_cfg the size of one ow_job / ow_calib_point / ow_preamp_point / ow_poly_chord /
 * ow_centroid_job: a caller built
 * against another header is refused ("ABI mismatch",
 * negative return) instead of having fields read past the end of what it passed. */
#define OW_ABI_VERSION 8
int ow_abi_version(void);

/* VoiceState, crates/openwurli-dsp/src/engine.rs:30-37 */
enum { OW_VOICE_FREE = 0, OW_VOICE_HELD = 1, OW_VOICE_SUSTAINED = 2, OW_VOICE_RELEASING = 3 };
/* preamp solver selection: cargo features of crates/openwurli-dsp/Cargo.toml:9-17 become a runtime enum */
enum { OW_PREAMP_LEGACY8 = 0, OW_PREAMP_MELANGE12 = 1 };
/* power amp selection (crates/openwurli-dsp/Cargo.toml:9-17: `legacy-power-amp` is a default feature; a `--no-default-features` build
 * gets the melange-generated 7-BJT Class-AB solver with rail dynamics, power_amp.rs:279-465 + gen_power_amp.rs) */
enum { OW_POWER_AMP_BEHAVIORAL = 0, OW_POWER_AMP_MELANGE = 1 };
/* tremolo oscillator selection (crates/openwurli-dsp/Cargo.toml:18 `legacy-tremolo`, tremolo.rs:8,53-57,80-90,170-178): the default is the
 * melange-generated Twin-T circuit; the legacy build replaces it by a half-wave rectified 5.63 Hz sine LFO in front of the same CdS model */
enum { OW_TREMOLO_TWIN_T = 0, OW_TREMOLO_LEGACY_LFO = 1 };

/* Introspection block (engine.rs:606-670 test/inspection helpers + diag counters of the solvers). */
typedef struct ow_diag {
    uint32_t active_voices, held_voices, sustained_voices, releasing_voices, steal_voices;
    uint32_t sustain_held;
    uint64_t nan_guard_fires;        /* engine.rs:662-664 */
    uint64_t tremolo_be_fallbacks;   /* gen_tremolo.rs diag_be_fallback_count */
    uint64_t preamp_nan_resets;      /* dk_preamp_legacy.rs:610-615 */
    uint64_t output_nan_resets;      /* engine.rs:450-458 */
} ow_diag;

/* Last error message of the calling thread ("" if none).  The realtime calls return void and never fail (the reference's contract,
 * SURVEY.md 8b): when one of them had to degrade (silence, dropped request) the reason is left here; it stays until the next
 * error replaces it or ow_clear_error() is called. */
const char* ow_last_error(void);
void ow_clear_error(void);

/* ---- pools ------------------------------------------------------------------------------ */
/* n_engines >= 1 engines at `sample_rate` on HIP device `device`.  Like WurliEngine::new
 * (engine.rs:194-229) the engines are NOT warmed up; call ow_pool_set_sample_rate or
 * ow_engine_set_sample_rate (what the plugin's initialize() does, plugin/src/lib.rs:96-97). */
ow_pool* ow_pool_new(double sample_rate, size_t n_engines, int device, int preamp_kind);       /* behavioural power amp */
ow_pool* ow_pool_new_with(double sample_rate, size_t n_engines, int device, int preamp_kind, int power_amp_kind);
ow_pool* ow_pool_new_kinds(double sample_rate, size_t n_engines, int device, int preamp_kind, int power_amp_kind, int tremolo_kind);
void ow_pool_free(ow_pool*);
size_t ow_pool_size(const ow_pool*);
ow_engine* ow_pool_engine(ow_pool*, size_t index);
ow_pool* ow_engine_pool(ow_engine*);              /* the pool an engine belongs to (a pool of one for ow_engine_new) */
/* WurliEngine::set_sample_rate for every engine of the pool (engine.rs:272-286): rebuilds the chain, 0.6 s warm-up. */
int ow_pool_set_sample_rate(ow_pool*, double sample_rate);
/* WurliEngine::reset for every engine (engine.rs:231-251). */
void ow_pool_reset(ow_pool*);
void ow_pool_ensure_buffer_capacity(ow_pool*, size_t max_samples);
/* Render `len` samples on every engine.  out_host: [n_engines][out_stride] f32 (out_stride >= len) or NULL to
 * leave the block in HBM (see ow_pool_device_output).  Blocking; never fails. */
void ow_pool_render(ow_pool*, float* out_host, size_t out_stride, size_t len);
/* Sample-accurate MIDI for many engines in one call: the plugin's handle_event (plugin/src/lib.rs:49-62)
 * applied in array order.  type 0 = NoteOn(note, value=velocity 0..1), 1 = NoteOff(note), 2 = sustain (value >= 0.5 = held).
 * Only the order of the events of one engine matters.  Large lists are applied by several host threads; a list grouped by engine
 * (non-decreasing `engine`) is cut into per-thread slices, any other order makes every thread scan the whole list.
 * A grouped list of >= 65 536 events on a pool of >= 8 192 engines is applied ON THE DEVICE (the voice-pool state machine of
 * engine.rs:299-374 / 569-590 one lane per engine; a list in a block of ow_host_alloc is read where it lies), and its note-ons build
 * their voices before the call returns, as Voice::note_on does (voice.rs:28-110); every other list queues its slot ops for the next
 * render.  Same states, same samples either way (OW_MIDI_DEVICE=0 / OW_MIDI_APPLY_EARLY=0 switch the two steps off). */
typedef struct ow_midi_event {
    uint32_t engine;
    uint8_t type;
    uint8_t note;
    uint16_t reserved;
    float value;
} ow_midi_event;
void ow_pool_midi(ow_pool*, const ow_midi_event* events, size_t n_events);
/* Device pointer of the last rendered block, f32 [n_engines][*stride]; *stride = the length of that block (rows are packed). */
const float* ow_pool_device_output(const ow_pool*, size_t* stride);
/* Stage-wise taps of the last rendered block, copied to host (parity tests): voice sum f64 [n_engines][len]. */
int ow_pool_read_voice_sum(ow_pool*, double* out_host, size_t out_stride, size_t len);
/* Preamp output (main - shadow, before the power amp) of the last block at the chain rate: f64 [n_engines][n_os],
 * n_os = len * (oversampled ? 2 : 1). */
int ow_pool_read_preamp_out(ow_pool*, double* out_host, size_t out_stride, size_t n_os);
/* CdS-cell resistance R[n] the tremolo produced for the last block (before the depth divider), chain rate: f64 [n_engines][n_os]. */
int ow_pool_read_tremolo_r(ow_pool*, double* out_host, size_t out_stride, size_t n_os);
/* The Twin-T / CdS tremolo cell takes no audio and no depth (tremolo.rs:121-146) and Tremolo::new / reset always leave the same settled
 * state (:83-102,:192-216), so its resistance r_ldr[t] is one sequence per chain rate.  The library computes it once per (device, chain
 * rate) into HBM -- the engine with the largest t extends it with a single oscillator, every engine of every pool of the process reads it
 * at its own t -- instead of one oscillator per engine.  Bit-identical to per-engine oscillators (tests/test_gpu_trajectory.py).
 * The store runs ahead of its oldest reader in the background from the moment it exists (Tremolo::new settles inside the constructor,
 * tremolo.rs:83-102: nothing for the host to call), a lead of 60 s of audio by default, on its own stream, one wavefront.  Its buffers
 * start at 150 s of audio (115 MB at 96 kHz; pools of >= 4 096 engines take the whole capacity at once) and double on a helper thread
 * long before a reader gets to their end; an engine older than the capacity (default 1 800 s since its new / reset / set_sample_rate)
 * continues on an oscillator of its own -- same samples, one oscillator per such engine.  OW_TREM_TRAJ=0 when a pool is created: no
 * trajectory for that pool.
 * ow_tremolo_configure: capacity and lead, in seconds of audio, of the stores of `device` (<= 0 / < 0: back to the defaults, which
 * OW_TREM_TRAJ_SECONDS / OW_TREM_TRAJ_LEAD_SECONDS override).  Applies to stores created afterwards and re-limits the existing ones
 * (never below what they hold).  Nothing is reserved by this call.  0 on success.
 * ow_tremolo_prefetch: make the first `seconds` of the trajectory for host rate `sample_rate` exist now (blocking; optional -- a host
 * that wants its first block after instantiation to find everything in place).  Returns the samples known complete, <0 on error. */
int ow_tremolo_configure(int device, double capacity_seconds, double lead_seconds);
long long ow_tremolo_prefetch(double sample_rate, int device, double seconds);
/* Keeping the trajectory ACROSS PROCESSES -- the counterpart of the reference's in-process start-up caches (the OnceLock settles of
 * dk_preamp/melange_adapter.rs:12-29; Tremolo::new's own settle, tremolo.rs:92-102), which a new process pays again.  Optional.
 * ow_tremolo_export: write what the store of (device, chain rate of host rate `sample_rate`) holds, cut to a 4 096-sample checkpoint
 * boundary, to `path` (8 bytes per chain sample).  Returns the samples written, <0 on error.
 * ow_tremolo_import: load such a file into the store (created if it does not exist yet; its 2 s settle is taken from the file too).  The
 * file is only accepted when THIS library would have produced it: same build id, same chain rate, same tremolo constants, payload
 * checksum, and its first and last checkpoint segments regenerated on the device by the product kernel and compared bit for bit.
 * Returns the samples the store took from the file (0: it already held more), <0 when the file is rejected (ow_last_error says why;
 * the store is untouched and extends itself as usual).  Call it where allocating is allowed (instantiation). */
long long ow_tremolo_export(double sample_rate, int device, const char* path);
long long ow_tremolo_import(double sample_rate, int device, const char* path);
/* HIP stream the pool launches on (hipStream_t as void*), for event timing by the caller. */
void* ow_pool_stream(ow_pool*);
/* Time (ms, HIP events on the pool stream) each kernel of the last ow_pool_render took:
 * [0] ops  [1] voices  [2] tremolo  [3] preamp  [4] post.  Enabled by ow_pool_set_profiling(pool,1). */
void ow_pool_set_profiling(ow_pool*, int on);
void ow_pool_last_kernel_ms(const ow_pool*, float ms[5]);

/* ---- engines: the WurliEngine API (engine.rs) -------------------------------------------- */
ow_engine* ow_engine_new(double sample_rate, int device, int preamp_kind);        /* WurliEngine::new        :194 */
ow_engine* ow_engine_new_with(double sample_rate, int device, int preamp_kind, int power_amp_kind);
ow_engine* ow_engine_new_kinds(double sample_rate, int device, int preamp_kind, int power_amp_kind, int tremolo_kind);   /* every cargo feature of the crate as a runtime kind */
void ow_engine_free(ow_engine*);                                                  /* Drop (pool-of-one only)      */
void ow_engine_set_sample_rate(ow_engine*, double sample_rate);                   /* set_sample_rate         :272 */
void ow_engine_reset(ow_engine*);                                                 /* reset                   :231 */
void ow_engine_warm_up(ow_engine*);                                               /* warm_up                 :261 */
void ow_engine_ensure_buffer_capacity(ow_engine*, size_t max_samples);            /* ensure_buffer_capacity  :288 */
void ow_engine_note_on(ow_engine*, uint8_t note, float velocity);                 /* note_on                 :299 */
void ow_engine_note_off(ow_engine*, uint8_t note);                                /* note_off                :340 */
void ow_engine_set_sustain(ow_engine*, int held);                                 /* set_sustain             :361 */
void ow_engine_set_volume(ow_engine*, double v);                                  /* set_volume              :378 */
void ow_engine_set_tremolo_depth(ow_engine*, double depth);                       /* set_tremolo_depth       :382 */
void ow_engine_set_speaker_character(ow_engine*, double c);                       /* set_speaker_character   :386 */
void ow_engine_set_mlp_enabled(ow_engine*, int on);                               /* set_mlp_enabled         :390 */
void ow_engine_set_noise_enabled(ow_engine*, int on);                             /* set_noise_enabled       :394 (melange preamp; no-op on legacy) */
void ow_engine_set_noise_gain(ow_engine*, double gain);                           /* set_noise_gain          :398 (-> set_thermal_gain; no-op on legacy) */
void ow_engine_set_rail_sag(ow_engine*, int on);                                  /* set_rail_sag            :406 (melange power amp; no-op otherwise) */
int ow_engine_rail_sag_enabled(const ow_engine*);                                 /* rail_sag_enabled        :410 */
/* power_amp_diag (engine.rs:418-420: clamp_count, nr_max_iter_count, peak_output_volts of the solver state) plus what the adapter
 * keeps besides: NaN resets of the solver, divergence-guard resets (power_amp.rs:410-421; the reference does not count them) and
 * the rail magnitudes (PowerAmp::rail_voltages, :359-365).  All zero / 22.5 V on the behavioural amp. */
typedef struct ow_power_amp_diag {
    uint64_t clamp_count, nr_max_iter_count;
    double peak_output_volts;
    uint64_t nan_resets, guard_resets;
    double rail_pos_volts, rail_neg_volts;
} ow_power_amp_diag;
void ow_engine_power_amp_diag(const ow_engine*, ow_power_amp_diag* out);
/* gen_preamp::CircuitState::set_seed (gen_preamp.rs:2094-2100) of this engine's main preamp state: restarts its 11 thermal-noise
 * streams from `seed` (0 = the process-wide clock entropy every engine starts from, like the reference) and clears the lag.  Not
 * reachable through WurliEngine in the reference (whose noise is therefore never reproducible); exported so parity can be tested.
 * Survives reset / set_sample_rate.  No-op on the legacy preamp. */
void ow_engine_set_noise_seed(ow_engine*, uint64_t seed);
void ow_engine_render(ow_engine*, float* out, size_t len);                        /* render                  :425 (pool-of-one only) */
void ow_engine_get_diag(const ow_engine*, ow_diag* out);
int ow_engine_slot_state(const ow_engine*, int slot);                             /* VoiceSlot.state              */
int ow_engine_slot_note(const ow_engine*, int slot);                              /* VoiceSlot.midi_note          */
int ow_engine_has_steal_voice_for(const ow_engine*, uint8_t note);                /* has_steal_voice_for     :627 */

/* ---- offline / batch ---------------------------------------------------------------------- */
/* Voice::render_note (voice.rs:191-221): one voice, no chain, f64.  Returns the number of samples
 * of the note ((dur_s*sr) as usize); writes min(n, cap).  Negative on device error. */
long long ow_render_note(uint8_t midi, double velocity, double dur_s, double sample_rate, int device, double* out, size_t cap);
/* Voice::render_note_with_scale(.., Some(displacement_scale)) (voice.rs:201-221): the same with the pickup's displacement scale overridden. */
long long ow_render_note_with_scale(uint8_t midi, double velocity, double dur_s, double sample_rate, double displacement_scale, int device,
                                    double* out, size_t cap);

/* `preamp-bench render` job (tools/preamp-bench/src/main.rs:371-549) as driven by ml/render_model_notes.py:49-116.  One field per flag of
 * the command that changes samples; zero-initialise and set the first seven for what the ML pipeline passes. */
typedef struct ow_job {
    uint8_t note;        /* --note, 33..96 */
    uint8_t velocity;    /* --velocity, 0..127 (vel_norm = velocity/127) */
    uint8_t mlp;         /* !--no-mlp */
    uint8_t poweramp;    /* !--no-poweramp */
    uint8_t no_preamp;               /* --no-preamp: the reed / pickup signal goes straight to the output stage (main.rs:425-427) */
    uint8_t no_attack_noise;         /* --no-attack-noise: Voice::disable_attack_noise (main.rs:409-411, voice.rs:150-152) */
    uint8_t has_displacement_scale;  /* --displacement-scale given (main.rs:388-392) */
    uint8_t reserved;
    double volume;       /* --volume (audio taper: x volume^2) */
    double speaker;      /* --speaker character */
    double r_ldr;        /* --ldr static resistance (used while tremolo_depth <= 0) */
    double tremolo_depth;        /* --tremolo-depth: > 0 puts Tremolo::new(depth, preamp rate) in front of the preamp instead of the static --ldr
                                  * (main.rs:430-441,447-463) */
    double displacement_scale;   /* Voice::set_displacement_scale when has_displacement_scale (main.rs:406-408) */
} ow_job;
typedef struct ow_batch_cfg {
    uint32_t struct_size;  /* = sizeof(ow_batch_cfg) of the caller's header */
    uint32_t job_size;     /* = sizeof(ow_job) of the caller's header (the stride of `jobs`) */
    double sample_rate;  /* --sample-rate (44100 in the reference, main.rs:27) */
    double duration_s;   /* --duration */
    int device;
    int preamp_kind;
    int power_amp_kind;  /* which PowerAmp the command was built with (cargo feature legacy-power-amp, main.rs:480): OW_POWER_AMP_BEHAVIORAL, or
                          * OW_POWER_AMP_MELANGE = PowerAmp::new() = the 7-BJT solver at 44.1 kHz whatever --sample-rate says (power_amp.rs:321-323) */
    int no_rail_sag;     /* --no-rail-sag (main.rs:381,481-483; melange power amp only) */
} ow_batch_cfg;
/* --normalize (main.rs:505-511): the factor write_wav_24bit applies to a finished render, 0.7 / peak when the peak exceeds 0.7, else 1.0;
 * pass it as `scale` to ow_wav24_write / ow_wav24_quantize.  (The samples ow_batch_render returns are never scaled, like final_output.) */
double ow_normalize_scale(const double* samples, size_t n);
/* Renders n_jobs independent jobs lane-parallel (lane = job).  out: f64 [n_jobs][stride], stride >= (duration*sr) as usize.
 * If out_is_device != 0, `out` is a device pointer and nothing is copied to the host.  Returns samples per job, <0 on error. */
long long ow_batch_render(const ow_job* jobs, size_t n_jobs, const ow_batch_cfg* cfg, double* out, size_t stride, int out_is_device);

/* ---- note-on MLP corrections given at run time (ml/: train -> model_weights.json -> render, without a rebuild) ---------------------
 * The reference bakes the network into mlp_weights.rs at compile time; here a weight set, or the corrections themselves, are data of a
 * batch render.  Nothing else of a job changes: every other ow_job field and ow_batch_cfg mean what they mean to ow_batch_render. */
#define OW_MLP_HIDDEN 16
#define OW_MLP_OUTPUTS 11
typedef struct ow_mlp_weights {            /* mlp_weights.rs, same shapes and order */
    double w1[16][2], b1[16], w2[16][16], b2[16], w3[11][16], b3[11], target_means[11], target_stds[11];
} ow_mlp_weights;
typedef struct ow_mlp_corrections {        /* MlpCorrections, mlp_correction.rs:38-45 */
    double freq_offsets_cents[5], decay_offsets[5], ds_correction;
} ow_mlp_corrections;
/* The built-in set (the one the library's note-ons use).  Host only, no device touched.  Returns 0, <0 on a null pointer. */
int ow_mlp_default_weights(ow_mlp_weights* out);
/* MlpCorrections::infer (mlp_correction.rs:61-140) of every (set, point) on the device: out[set * n_points + point]; raw_out (NULL or
 * [n_sets][n_points][11]) receives the denormalised network outputs before the fade outside MIDI 65..97 and the clamps.
 * sets == NULL with n_sets == 1 means the built-in set.  velocities are the normalised ones (clamped to 0..1 like the reference's).
 * Returns 0, <0 on error (a null pointer, a non-finite weight or velocity: refused on the host before the device is touched). */
int ow_mlp_infer(const ow_mlp_weights* sets, size_t n_sets, const uint8_t* notes, const double* velocities, size_t n_points,
                 int device, ow_mlp_corrections* out, double* raw_out);
/* ow_batch_render with job j's note-on taking corr[j] in place of what infer would return; jobs[j].mlp is ignored.  A non-finite
 * correction or a decay_offsets entry <= 0 (note-on divides by it) is refused on the host: <0, ow_last_error() names job and field. */
long long ow_batch_render_corrected(const ow_job* jobs, size_t n_jobs, const ow_batch_cfg* cfg, const ow_mlp_corrections* corr,
                                    double* out, size_t stride, int out_is_device);
/* ow_batch_render with the network's weights per job: a job with mlp != 0 takes the corrections of sets[set_of_job[j]] at
 * (note, velocity / 127), a job with mlp == 0 the identity.  ow_mlp_infer into a device table, then the render of
 * ow_batch_render_corrected; nothing passes through the host in between.  set_of_job[j] >= n_sets or a non-finite weight is refused. */
long long ow_batch_render_mlp(const ow_job* jobs, size_t n_jobs, const ow_batch_cfg* cfg, const ow_mlp_weights* sets, size_t n_sets,
                              const uint32_t* set_of_job, double* out, size_t stride, int out_is_device);

/* ---- training weight sets (ml/train_mlp.py's train(), many models per call) -----------------------------------------------------------
 * One wavefront trains one model, its whole run inside one launch (k_mlp_train): per epoch the forward and backward pass over the
 * model's train rows (masked Huber loss weighted per row, divided by the number of masked-in entries), torch.optim.Adam(lr,
 * betas (0.9, 0.999), eps 1e-8, weight_decay as L2 in the gradient), the validation loss with the updated weights,
 * ReduceLROnPlateau(min, sched_factor, sched_patience, threshold 1e-4 relative, min_lr, eps 1e-8) and early stopping after `patience`
 * epochs without a strictly lower validation loss.  All arithmetic is f64; the result is deterministic and does not depend on the
 * other models of the call. */
typedef struct ow_mlp_train_model {        /* one model's hyper-parameters; train_mlp.py's flags */
    double lr, min_lr, weight_decay, huber_delta, sched_factor;
    uint32_t epochs, patience, sched_patience;
    uint32_t target_mask;                  /* bit i set = target i is trained on (ANDed with the data's mask); --mask-decay-h3 clears bit 6 */
} ow_mlp_train_model;
typedef struct ow_mlp_train_cfg {
    uint32_t struct_size, model_size;      /* sizeof(ow_mlp_train_cfg), sizeof(ow_mlp_train_model) */
    int device;
    uint32_t n_rows;
    uint32_t history_epochs;               /* epochs per model in history_out; at least every model's `epochs` when history_out is given */
    uint32_t reserved;
    double* kernel_ms_out;                 /* NULL, or receives the time of k_mlp_train between two device events, in ms */
} ow_mlp_train_cfg;
typedef struct ow_mlp_train_result {
    double best_val_loss, last_train_loss, last_val_loss, last_lr;     /* last_lr: the rate after the last epoch's scheduler step */
    uint32_t best_epoch, epochs_run, lr_reductions;
    uint32_t status;                       /* 0 = ok, 1 = no epoch ever improved (best_out = init) */
} ow_mlp_train_result;
/* The most row-epochs (n_rows x epochs) of one model: a model is one serial wavefront, and the launch is on a machine others share.
 * Measured (tools/bench_mlp_train.py, one MI355X): 99 ns per row-epoch of a model running alone (2 000 epochs over 409 train and
 * 103 validation rows in 101.7 ms), so a model at the cap whose train and validation rows together are n_rows (a split
 * without overlap) holds its wavefront for about 6.7 s -- and for about 13 s where every row is in both parts (--no-split: an epoch
 * walks 2 x n_rows rows, the cap counts n_rows); the instruction-count estimate behind the cap (1 400 multiply-adds per row-epoch at
 * 32 per cycle) had said about one second. */
#define OW_MLP_TRAIN_MAX_ROW_EPOCHS 67108864u      /* 2^26 */
/* inputs [n_rows][2], targets [n_rows][11] (standardised), mask [n_rows][11] (non-zero = valid), row_weights [n_rows]: shared by all
 * models.  split [n_models][n_rows]: bit 0 = train row, bit 1 = validation row of that model (80/20, no split, k-fold, leave-one-out
 * are all rows of this table).  init [n_models]: the initial sets; their target_means / target_stds are copied into best_out unchanged,
 * so best_out[i] is a set ow_mlp_infer / ow_batch_render_mlp take as it stands: the parameters after the epoch with the lowest
 * validation loss.  history_out: NULL or [n_models][history_epochs][3] = train loss, validation loss, learning rate in force during
 * the epoch's step; rows from a model's epochs_run on are 0.  Returns 0, <0 on error: everything is validated on the host before the
 * device is touched (null pointers, n_rows == 0, non-finite data / weights / hyper-parameters, lr <= 0, huber_delta <= 0, sched_factor
 * outside (0, 1), min_lr < 0, weight_decay < 0, epochs == 0, a model without a masked-in train or validation entry, more than 65535
 * models, n_rows x epochs above OW_MLP_TRAIN_MAX_ROW_EPOCHS, history_epochs below a model's epochs, and two bounds on the call's
 * memory: n_models x n_rows above 2^27 (the models' row lists: up to 1 GiB), n_models x history_epochs above 2^27 with history_out
 * given (3 GiB)); ow_last_error() names model and field.  A masked-out entry and a lane past the end of a row list contribute exact
 * zeros as long as the prediction is finite; once a model's weights have diverged, 0 x inf is NaN there as it is in torch. */
int ow_mlp_train(const double* inputs, const double* targets, const uint8_t* mask, const double* row_weights, const uint8_t* split,
                 const ow_mlp_weights* init, const ow_mlp_train_model* models, size_t n_models, const ow_mlp_train_cfg* cfg,
                 ow_mlp_weights* best_out, ow_mlp_train_result* results, double* history_out);

/* Plain device buffers for chaining the offline entry points without a host round trip (out_is_device / audio_is_device). */
void* ow_device_alloc(size_t bytes, int device);   /* NULL on failure */
void ow_device_free(void* ptr, int device);
/* Page-locked host memory for `out_host` of ow_pool_render: the block copy of a big pool then runs at PCIe rate instead of through
 * the runtime's staging of pageable memory.  (A pool of one copies 2 KB per block; it does not need this.) */
void* ow_host_alloc(size_t bytes, int device);     /* NULL on failure */
void ow_host_free(void* ptr, int device);

/* ---- ML-pipeline stage after the batch render --------------------------------- */
/* 24-bit PCM quantisers of the reference's two WAV writers.  OW_WAV_ROUND: preamp-bench write_wav_24bit
 * (tools/preamp-bench/src/main.rs:941-957): (sample * scale * (2^23-1)).round() as i32, clamped to +-(2^23-1); Rust round() is
 * half-away-from-zero and the cast saturates (NaN -> 0).  OW_WAV_TRUNCATE: reed-renderer write_wav
 * (tools/reed-renderer/src/main.rs:110-126): (s.clamp(-1,1) * (2^23-1)) as i32, truncation toward zero (scale ignored). */
enum { OW_WAV_ROUND = 0, OW_WAV_TRUNCATE = 1 };
int ow_wav24_quantize(const double* samples, size_t n, double scale, int mode, int32_t* out);
/* Mono 24-bit PCM WAV file with that quantiser.  Container as hound 3.5.1 (Cargo.lock) writes it for 24-bit data:
 * RIFF/WAVE, 40-byte WAVE_FORMAT_EXTENSIBLE "fmt " chunk (PCM sub-format, 24 valid bits, channel mask 0x4), "data" chunk of
 * little-endian 3-byte samples.  Returns 0, <0 on I/O error. */
int ow_wav24_write(const char* path, const double* samples, size_t n, uint32_t sample_rate, double scale, int mode);

/* extract_harmonics_fft (ml/goertzel_utils.py:60-107) on many segments at once, as extract_model_features
 * (ml/render_model_notes.py:118-237) applies it to each rendered note: amplitude and frequency of the peak bin of the
 * Hann-windowed, 4x zero-padded spectrum inside +-search_pct of each harmonic h*f0, h = 1..n_harmonics (<= OW_MAX_HARMONICS);
 * harmonics at or above sr/2 - 100 Hz, or without a bin in the band, report amplitude 1e-20 at h*f0.  Also the RMS of every
 * segment (max(sqrt(mean(x^2)), 1e-20); n_harmonics = 0 asks for the RMS only). */
#define OW_MAX_HARMONICS 8
typedef struct ow_segment {
    uint32_t row;          /* audio row (job) */
    uint32_t start, end;   /* sample range [start, end) inside the row */
    uint32_t n_harmonics;  /* 0..OW_MAX_HARMONICS */
    double f0;             /* fundamental the harmonics are searched around */
} ow_segment;
/* audio: f64 [n_rows][stride] (device pointer if audio_is_device != 0, e.g. the output of ow_batch_render).
 * wav24_mode: OW_WAV_ROUND / OW_WAV_TRUNCATE analyse what a 24-bit WAV written with that quantiser and read back as float
 * (int / 2^23, libsndfile's PCM_24 normalisation used by the script's load_audio, goertzel_utils.py:11-17) would contain;
 * OW_WAV_NONE analyses the samples as they are.
 * amps, freqs: [n_segs][OW_MAX_HARMONICS] (entries past n_harmonics are 0); rms: [n_segs] or NULL.  Returns 0, <0 on error. */
#define OW_WAV_NONE (-1)
int ow_extract_harmonics(const double* audio, size_t n_rows, size_t stride, double sample_rate, const ow_segment* segs, size_t n_segs,
                         double search_pct, int wav24_mode, int device, int audio_is_device, double* amps, double* freqs, double* rms);

/* ---- the recording side of the ML loop: stage 3 (ml/extract_harmonics.py) and stage 5 (ml/compute_residuals.py) ---- */
/* What the two entry points below share.  audio is f64 [n_rows][stride], a device pointer if audio_is_device != 0; wav24_mode as for
 * ow_extract_harmonics. */
typedef struct ow_harmonics_cfg {
    uint32_t struct_size;   /* sizeof(ow_harmonics_cfg) */
    uint32_t segment_size;  /* sizeof(ow_segment) */
    double sample_rate;
    double search_pct;      /* ow_goertzel_harmonics: half-width of the offset search (the reference's 0.01); ow_interharmonic_noise ignores it */
    int wav24_mode;         /* OW_WAV_NONE / OW_WAV_ROUND / OW_WAV_TRUNCATE */
    int device;
    int audio_is_device;
    int reserved;           /* 0 */
} ow_harmonics_cfg;
/* extract_harmonics_goertzel (ml/goertzel_utils.py:34-57, 106-119) on many segments at once, the Goertzel counterpart of
 * ow_extract_harmonics.  Per harmonic h*f0 below sr/2 - 100 Hz: the OW_GOERTZEL_OFFSETS offsets of np.linspace(-search_pct, search_pct, 11)
 * (start + i*step, the last one search_pct itself), f = h*f0 * (1.0 + offset), k = nearbyint(f * N / sr) (half to even, as Python's round
 * of a float64), skipped if k <= 0 or k >= N / 2; coeff = 2.0 * cos(2.0 * pi * k / N); the recurrence s0 = (x + coeff*s1) - s2 over the N
 * samples of the segment, every operation a single rounded f64 operation on the device; magnitude sqrt(s1*s1 + s2*s2 - coeff*s1*s2) / N * 2.0;
 * the first maximum over the offsets (strict >, starting from 0.0), floored at 1e-20.  Harmonics at or above sr/2 - 100 Hz report 1e-20.
 * Offsets of one harmonic that round to the same k run once: the same k gives the same (s1, s2) and a strict > ignores repeats.
 * amps: [n_segs][OW_MAX_HARMONICS] (entries past n_harmonics are 0).
 * coeffs_out / bins_out: NULL, or [n_segs][OW_MAX_HARMONICS][OW_GOERTZEL_OFFSETS]: the coefficient and the bin k of every offset as
 * the library used them (k = -1 and coefficient 0 where the offset was skipped, the harmonic lies past the cut or past n_harmonics).
 * Refuses (<0, ow_last_error() says why): a null argument, sizes that do not match this header, an unknown wav24_mode, a sample rate or
 * search_pct that is not finite and positive / non-negative, a segment out of range, longer than 2^22 samples or with an f0 that is not
 * finite.  n_segs == 0 returns 0. */
#define OW_GOERTZEL_OFFSETS 11
int ow_goertzel_harmonics(const double* audio, size_t n_rows, size_t stride, const ow_segment* segs, size_t n_segs, const ow_harmonics_cfg* cfg,
                          double* amps, double* coeffs_out, int32_t* bins_out);
/* The noise floor of measure_interharmonic_snr (ml/compute_residuals.py:93-117) of many segments at once: for h = 0..n_harmonics-1 the
 * np.median of the Hann-windowed, 4x zero-padded spectrum (scaled 2 / N / 0.5) over the bins inside [0.99, 1.01] x (h + 1.5) x f0, floored
 * at 1e-20; 1e-20 where (h + 1.5) x f0 >= sr/2 - 100 Hz or no bin lies in the band.  noise: [n_segs][OW_MAX_HARMONICS] (entries past
 * n_harmonics are 0).  Refuses what ow_goertzel_harmonics refuses, and a segment one of whose bands holds more than OW_NOISE_MAX_BAND_BINS
 * bins (the band's magnitudes are held on chip; the reference's 0.15 s window reaches about 260).  n_segs == 0 returns 0. */
#define OW_NOISE_MAX_BAND_BINS 4096
int ow_interharmonic_noise(const double* audio, size_t n_rows, size_t stride, const ow_segment* segs, size_t n_segs, const ow_harmonics_cfg* cfg,
                           double* noise);

/* ---- recorded-note intake: stage 2 (ml/score_isolation.py) and the non-neural half of stage 1 (ml/extract_notes.py) ---- */
/* One note of score_notes' list.  window_start / window_end: the analysis window as score_notes (score_isolation.py:266-271) plans it,
 * computed by the caller.  id_key stands for the note's "id": equal strings, equal keys (an other is skipped by id equality, :43, not by
 * position).  score == 0: the reference does not score this note (obm_isolated, duration score 0); it still counts as an other. */
typedef struct ow_iso_note {
    double onset_s, offset_s, amplitude;
    double window_start, window_end;
    int64_t id_key;
    int32_t midi_note;      /* 0..127 */
    int32_t score;
} ow_iso_note;
typedef struct ow_iso_cfg {
    uint32_t struct_size;        /* sizeof(ow_iso_cfg) */
    uint32_t note_size;          /* sizeof(ow_iso_note) */
    int device;
    int reserved;                /* 0 */
    double collision_ratio;      /* 2.0 ** (50.0 / 1200.0), score_isolation.py:79 */
    const double* decay_rate;    /* [128]: 0.26 * exp(0.049 * midi), :31, in the caller's own libm */
    const double* midi_freq;     /* [128]: midi_to_freq (ml/goertzel_utils.py:129-131), in the caller's own libm */
    double* kernel_ms_out;       /* NULL, or where the kernel's device time goes (0 when no kernel ran) */
} ow_iso_cfg;
/* harmonic_collision_check (ml/score_isolation.py:69-102) of one target against one other, for all pairs of MIDI numbers:
 * table[target * 128 + other], bit h set while harmonic h + 1 of the target is clean.  Host arithmetic only (multiply, divide, max, min,
 * compare): no device needed.  Refuses a null argument and a non-finite frequency or ratio. */
int ow_isolation_collision_table(const double* midi_freq, double collision_ratio, uint8_t* table);
/* score_temporal, score_harmonic_collision and score_energy_dominance (ml/score_isolation.py:36-167) for all notes of all files in one
 * call.  notes[file_first[f] .. file_first[f + 1]) are the notes of file f in their order in the caller's list, which is the order the
 * sums run in (file_first has n_files + 1 entries, from 0 to n_notes).  Per scored note, unrounded: temporal (after the 0.05 floor),
 * collision (clean weight / 12), dominance, and mask (bit h: harmonic h + 1 clean; no energetic other: 0xFF and collision 1.0); zeros
 * for a note with score == 0.  remaining = pow(10.0, -(rate * t) / 20.0) is the device library's pow; everything else is the reference's
 * arithmetic operation for operation, every comparison strict as there.
 * Refuses (<0, ow_last_error() says why): a null argument, sizes that do not match this header, a midi_note outside 0..127, a
 * non-finite time, amplitude, window or table entry, file ranges that are not ascending or do not cover the notes.  n_notes == 0
 * returns 0. */
int ow_isolation_score(const ow_iso_note* notes, size_t n_notes, const uint64_t* file_first, size_t n_files, const ow_iso_cfg* cfg,
                       double* temporal, double* collision, double* dominance, uint8_t* mask);
/* detect_obm_onset / detect_obm_offset (ml/extract_notes.py:43-64) and the onset search of extract_sustain_window
 * (ml/goertzel_utils.py:139-153) on many clips at once.  clips: host f64 [n_clips][stride]; lengths[c] <= stride samples of row c are
 * audio, the rest of the row is not read.  Per clip: peak = max |x| (0 for an empty clip), first = the first index with
 * |x| > onset_frac * peak, last = the last index >= 1 with |x| > offset_frac * peak (the reference's backward loop stops before index 0);
 * -1: none.  Each threshold is the one product, each comparison strict.  Seconds and the fallbacks (peak < 1e-10, none found) are the
 * caller's.  Refuses a null argument, a non-finite fraction, a stride of 0 and a length above the stride.  n_clips == 0 returns 0. */
int ow_clip_bounds(const double* clips, size_t n_clips, size_t stride, const uint32_t* lengths, double onset_frac, double offset_frac, int device,
                   double* peak, int64_t* first, int64_t* last);

/* ---- click-band alias audit (crates/openwurli-dsp/src/alias_audit.rs) ----------- */
/* AliasAuditResult (alias_audit.rs:68-93), same fields in the same order. */
#define OW_AUDIT_HARMONICS 12
typedef struct ow_alias_audit_result {
    double f0_hz;                               /* peak of the +-5 Hz / 0.1 Hz search around the nominal pitch */
    double h1_dbfs;                             /* H1 magnitude, dB FS */
    double harmonic_db[OW_AUDIT_HARMONICS];     /* H(i+1), dB FS */
    double harmonic_dbc[OW_AUDIT_HARMONICS];    /* H(i+1) relative to H1, dB; [0] is 0.0 */
    double max_step_up_db;                      /* largest harmonic_dbc[n+1] - harmonic_dbc[n], n over H6..H10 */
    uint32_t max_step_up_from_harmonic;         /* 1-based harmonic the worst rise starts from */
    uint32_t reserved;
    double hf_band_dbc;                         /* RMS of the 5-18 kHz band relative to H1, dB */
} ow_alias_audit_result;
/* analyze (alias_audit.rs:163-211) of n_signals rows at once.  signals: f64 [n_signals][stride], the first `len` samples of a
 * row are the render (device pointer if signals_is_device != 0); the last floor(sample_rate * 0.5) of them are analysed.
 * nominal_f0: [n_signals].  Returns 0; <0 if len is shorter than the analysis window (the reference asserts) or on a device error. */
int ow_alias_audit_analyze(const double* signals, size_t n_signals, size_t stride, size_t len, double sample_rate,
                           const double* nominal_f0, int device, int signals_is_device, ow_alias_audit_result* out);
/* run_with_note for n (note, velocity 0..127) pairs at once (alias_audit.rs:104-108; run_sweep :123-133 is the three
 * STIMULUS_NOTES at velocity 120): one pool engine per pair renders the canonical stimulus (render_stimulus :135-160: 44.1 kHz,
 * volume 0.5, tremolo depth 0, speaker 0, MLP on, noise off, six settling blocks of 1024, note-on, 1.5 s in blocks of 1024), the
 * blocks stay in HBM and are analysed there.  signals_out: NULL or host f64 [n][signals_stride >= 66150] receiving the renders. */
int ow_alias_audit_run(const uint8_t* notes, const uint8_t* velocities, size_t n, int device, int preamp_kind,
                       ow_alias_audit_result* out, double* signals_out, size_t signals_stride);

/* ---- MIDI-file render (`preamp-bench render-midi`, tools/preamp-bench/src/main.rs:1603-1923) ---- */
/* One timed event of the command's internal list (main.rs:1639-1649). */
typedef struct ow_timed_event {
    double time_s;
    uint8_t type;        /* 0 NoteOn(note, value = velocity 1..127)  1 NoteOff(note)  2 Pedal(value != 0 = down) */
    uint8_t note;
    uint8_t value;
    uint8_t reserved[5];
} ow_timed_event;
/* The part of midly 0.5.3 (Cargo.lock) the command uses: Standard MIDI File -> events with absolute times in seconds, in file
 * order (main.rs:1627-1708): metrical timing only, tempo meta events applied per track (every track starts at 500 000 us per
 * beat), note-on with velocity 0 = note-off, controller 64 >= 64 = pedal down.  track_filter < 0: all tracks (`--track N`
 * otherwise).  Returns the event count (writes min(cap, count) events; out may be NULL with cap 0), <0 on malformed data. */
long long ow_smf_parse(const uint8_t* data, size_t len, int track_filter, ow_timed_event* out, size_t cap);
typedef struct ow_midi_render_cfg {
    uint32_t struct_size;  /* = sizeof(ow_midi_render_cfg) of the caller's header */
    uint32_t reserved0;
    double volume;       /* --volume, default 0.60 (applied squared)       */
    double speaker;      /* --speaker, default 1.0                         */
    double tail_s;       /* --tail, default 2.0                            */
    int no_poweramp;     /* --no-poweramp                                  */
    int device;
    int preamp_kind;     /* OW_PREAMP_LEGACY8 (`--model dk` of the default build) or OW_PREAMP_MELANGE12 (melange-preamp build) */
    int power_amp_kind;  /* the build's PowerAmp::new() (main.rs:1756): OW_POWER_AMP_BEHAVIORAL or OW_POWER_AMP_MELANGE (44.1 kHz, rail sag on) */
    int no_rail_sag;     /* PowerAmp::set_rail_sag(false) (not a flag of render-midi; for parity with `render`) */
    int reserved;
} ow_midi_render_cfg;
typedef struct ow_midi_render_stats { uint64_t n_samples, note_ons, peak_polyphony; } ow_midi_render_stats;
/* cmd_render_midi's render loop (main.rs:1711-1891) for n_jobs event lists at once, 44.1 kHz (BASE_SR, main.rs:27).
 * Job j owns events[job_offsets[j] .. job_offsets[j+1]); they are stably sorted by time like the command does.  Its output is
 * floor((last event time + tail_s) * 44100) samples (0 for an empty list, where the command prints and returns).
 * out: host f64 [n_jobs][stride], rows zero-padded behind their job's samples; NULL only fills stats (to size the buffer).
 * Returns the longest job's sample count, <0 on error (e.g. stride too small, NaN times). */
long long ow_render_midi(const ow_timed_event* events, const size_t* job_offsets, size_t n_jobs, const ow_midi_render_cfg* cfg,
                         double* out, size_t stride, ow_midi_render_stats* stats);

/* ---- calibration sweep (`preamp-bench calibrate` / `sensitivity`, tools/preamp-bench/src/main.rs:1069-1395) ---------------- */
/* One grid point: a (note, velocity byte) pair under its own CalibrationConfig (crates/openwurli-dsp/src/tables.rs:254-277), so a whole
 * `sensitivity` sweep -- several configs -- is one call.  CalibrationConfig::default() is ds_at_c4 0.85, ds_exponent 0.75, ds_clamp
 * (0.02, 0.95), target_db -35, voicing_slope -0.04, zero_trim 0; `calibrate` itself defaults to ds_at_c4 0.75 and ds_clamp_hi 0.82. */
typedef struct ow_calib_point {
    uint8_t note;          /* 33..96 (MIDI_LO..MIDI_HI, tables.rs:6-7: the tables are defined there; other notes are refused) */
    uint8_t velocity;      /* 0..127, a MIDI velocity byte (velocity = byte / 127, main.rs:1147); larger values are refused */
    uint8_t zero_trim;     /* CalibrationConfig.zero_trim */
    uint8_t reserved[5];
    double ds_at_c4, ds_exponent, ds_clamp_lo, ds_clamp_hi, target_db, voicing_slope;
} ow_calib_point;
typedef struct ow_calibrate_cfg {
    uint32_t struct_size;  /* = sizeof(ow_calibrate_cfg) of the caller's header */
    uint32_t point_size;   /* = sizeof(ow_calib_point) of the caller's header (the stride of `points`) */
    double volume;         /* --volume (default 0.40; applied squared in front of the power amp) */
    double speaker;        /* --speaker character (default 1.0) */
    int device;
    int preamp_kind;       /* --model dk of the default build / dk-legacy: OW_PREAMP_LEGACY8; dk of a melange-preamp build: OW_PREAMP_MELANGE12 */
    int power_amp_kind;    /* the build's PowerAmp::new() (main.rs:1212): OW_POWER_AMP_BEHAVIORAL or OW_POWER_AMP_MELANGE (44.1 kHz, rail sag on) */
    int reserved;
} ow_calibrate_cfg;
/* CalibrateRow (main.rs:1099-1121), same fields in the same order; dB values carry the reference's -120 floors. */
typedef struct ow_calibrate_row {
    uint8_t midi, velocity;
    uint8_t reserved[6];
    double ds_at_c4, ds_actual, y_peak;
    double t2_peak_db, t2_rms_db, t2_h2_h1_db;
    double t3_peak_db, t3_rms_db;
    double t4_peak_db, t4_rms_db, t4_h2_h1_db;
    double t5_peak_db, t5_rms_db, t5_h2_h1_db;
    double proxy_db, trim_db, proxy_error_db, tanh_compression_db;
} ow_calibrate_row;
#define OW_CALIB_SAMPLES 22050   /* 0.5 s at BASE_SR 44 100 Hz (main.rs:27,1137) */
/* run_calibrate (main.rs:1128-1262) for n points at once, lane = point, at 44.1 kHz: T1 ModalReed::new(.., onset 0, ..) without MLP or
 * attack noise, T2 Pickup::new_with_scale(ds_actual), T3 x output_scale_with_config, T4 a fresh preamp (new + set_ldr_resistance(1e6)) with
 * per-sample 2x oversampling, T5 x volume^2 -> PowerAmp::new() -> Speaker(character) -> x POST_SPEAKER_GAIN; metrics over samples
 * [4410, 17640).  Large grids run in chunks of a fixed device-memory budget (OW_CALIB_CHUNK=<points> caps a chunk; tests use it).
 * rows_out: [n].  taps_out: NULL or host f64 [n][5][taps_stride >= OW_CALIB_SAMPLES] receiving T1..T5.
 * Returns 0, <0 on error (ow_last_error says why: "ABI mismatch", a note outside 33..96, a velocity above 127, an invalid clamp, a
 * device error). */
int ow_calibrate(const ow_calib_point* points, size_t n, const ow_calibrate_cfg* cfg, ow_calibrate_row* rows_out, double* taps_out,
                 size_t taps_stride);

/* ---- preamp measurements (`preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep`, tools/preamp-bench/src/main.rs:150-369) ---- */
/* One measurement point: a sine of freq_hz / amplitude through a fresh Oversampler and the 2x-oversampled preamp, 22 050 samples at BASE_SR
 * (measure_gain_at :157-190, cmd_harmonics :256-323).  r_ldr is what set_ldr_resistance receives (:620-626: clamp to 1 kohm, 0.01 ohm
 * hysteresis).  r_reset is the LDR resistance the legacy preamp's DC solve runs at before that: reset() solves DC at the PREVIOUS
 * self.r_ldr (dk_preamp_legacy.rs:628-640), so point i of a `sweep` / `tremolo-sweep` -- one preamp object, reset per point (:217-254,
 * :325-368) -- starts from the DC state of point i-1's resistance; `gain`, `harmonics` and point 0 start from new(), i.e. 1e6.  The
 * melange preamp's reset() clones its settled state and ignores r_reset.  With r_reset explicit every point is independent. */
typedef struct ow_preamp_point { double freq_hz, amplitude, r_ldr, r_reset; } ow_preamp_point;
typedef struct ow_preamp_measure_cfg {
    uint32_t struct_size;  /* = sizeof(ow_preamp_measure_cfg) of the caller's header */
    uint32_t point_size;   /* = sizeof(ow_preamp_point) of the caller's header (the stride of `points`) */
    int device;
    int preamp_kind;       /* create_preamp (:132-148): `--model dk` of the default build / dk-legacy: OW_PREAMP_LEGACY8; dk of a melange-preamp build: OW_PREAMP_MELANGE12 */
    int reserved[4];
} ow_preamp_measure_cfg;
/* gain = peak |out| over [OW_PBENCH_GAIN_LO, OW_PBENCH_SAMPLES) / amplitude (measure_gain_at), gain_db = 20 log10(gain); h[k-1] =
 * dft_magnitude (:893-903) at k x freq_hz over [OW_PBENCH_HARM_LO, OW_PBENCH_SAMPLES), k = 1..5; thd_pct and h2_h3_db as cmd_harmonics forms
 * them (h2_h3_db = INFINITY when h3 <= 1e-15).  Both windows come from the same single run. */
typedef struct ow_preamp_measure_row {
    double freq_hz, amplitude, r_ldr;
    double gain, gain_db;
    double h[5];
    double thd_pct, h2_h3_db;
} ow_preamp_measure_row;
#define OW_PBENCH_SAMPLES 22050  /* (BASE_SR * 0.5) as usize (:266); = (BASE_SR * 0.3) + (BASE_SR * 0.2) settle + measure (:165-166) */
#define OW_PBENCH_GAIN_LO 13230  /* (BASE_SR * 0.3) as usize: the settle of measure_gain_at */
#define OW_PBENCH_HARM_LO 16537  /* output.len() * 3 / 4: cmd_harmonics' last quarter */
/* n points at once.  rows_out: [n].  trace_out: NULL or host f64 [n][trace_stride >= OW_PBENCH_SAMPLES] receiving the base-rate preamp
 * output (downsample_2x's); with a trace the grid runs in chunks of a fixed device-memory budget (OW_PBENCH_CHUNK=<points> caps them).
 * Returns 0, <0 on error (ow_last_error says why: "ABI mismatch", a non-finite or non-positive freq_hz / amplitude / r_ldr / r_reset,
 * a short trace_stride, a device error). */
int ow_preamp_measure(const ow_preamp_point* points, size_t n, const ow_preamp_measure_cfg* cfg, ow_preamp_measure_row* rows_out,
                      double* trace_out, size_t trace_stride);

/* ---- chord intermodulation (`preamp-bench render-poly`, tools/preamp-bench/src/main.rs:1397-1592) --------------------------- */
/* One chord.  Voice i is Voice::note_on(notes[i], velocities[i] / 127, 44100, notes[i] * 2654435761 + i (u32 wrapping), mlp = true)
 * (:1435-1440).  The voices' sum goes through ONE chain (`final`), every voice through a chain of its OWN, added in voice order
 * (`separate_sum`); residual = final - separate_sum is what the shared preamp, power amp and speaker intermodulate (:1460-1513).  A
 * chain is a fresh legacy DkPreamp at 88 200 Hz, set_ldr_resistance(r_ldr) (clamp to 1 kohm, 0.01 ohm hysteresis against new()'s
 * 1 Mohm) and THEN reset() -- so the DC solve runs at the chord's --ldr, the opposite order of `render` / ow_batch_render --, per-sample
 * 2x oversampling (:961-974), x volume^2, PowerAmp::new() at the base rate unless no_poweramp, Speaker(speaker), x POST_SPEAKER_GAIN. */
#define OW_POLY_MAX_NOTES 31        /* a chord's n + 1 chains fit one wavefront in either lane layout */
typedef struct ow_poly_chord {
    uint8_t n_notes;                       /* 1..OW_POLY_MAX_NOTES */
    uint8_t no_poweramp;                   /* --no-poweramp */
    uint8_t reserved[6];
    uint8_t notes[32], velocities[32];     /* --notes (33..96) / --velocities (0..127; velocity = byte / 127), already padded to n_notes (:1410-1420) */
    double volume, speaker, r_ldr;         /* --volume (applied squared), --speaker, --ldr */
} ow_poly_chord;
typedef struct ow_poly_cfg {
    uint32_t struct_size;  /* = sizeof(ow_poly_cfg) of the caller's header */
    uint32_t chord_size;   /* = sizeof(ow_poly_chord) of the caller's header (the stride of `chords`) */
    double duration_s;     /* --duration (default 3.0); every chord renders (duration_s * 44100.0) as usize samples */
    int device;
    int preamp_kind;       /* OW_PREAMP_LEGACY8 only (below) */
    int power_amp_kind;    /* OW_POWER_AMP_BEHAVIORAL only (below) */
    int reserved;
} ow_poly_cfg;
/* Index 0 / 1 / 2 of the arrays: the shared chain (poly), the separate chains' sum, the residual.  Window = samples
 * [8820, min(88200, n)) (:1516-1517). */
typedef struct ow_poly_row {
    double peak;                           /* peak_abs(final_output), whole render (:1530) */
    double residual_peak;                  /* peak_abs(residual), whole render (:1543) */
    double win_peak[3], win_mean_sq[3];    /* poly, separate, residual: linear values */
    double peak_db[3], rms_db[3];          /* peak_db / rms_db (:916-927) with their -120 floors */
    double intermod_ratio_db;              /* rms_db[0] - rms_db[2] (:1575) */
} ow_poly_row;
/* cmd_render_poly for n_chords chords at once, 44.1 kHz.  rows_out: [n_chords].  final_out / separate_sum_out / residual_out: each NULL
 * or a host f64 array [n_chords][stride >= samples per chord]; which of them are asked for changes no number.  Large grids run in chunks
 * of a fixed device-memory budget (a chord takes n_notes voice rows plus three result rows; OW_POLY_CHUNK=<chords> caps a chunk; tests
 * use it).  A chord's numbers do not depend on the other chords of the call.
 * Returns the samples per chord, <0 on error.  Refused before any device work (ow_last_error says why): "ABI mismatch", n_notes of 0 or
 * above OW_POLY_MAX_NOTES, a note outside 33..96, a velocity above 127, a non-finite or non-positive r_ldr, a non-finite volume or
 * speaker, a duration of 8820 samples or fewer (the reference's window slice panics there), a short stride, and two follow-ups:
 *   - OW_PREAMP_MELANGE12: the melange adapter's reset() re-clones the settled state AFTER set_ldr_resistance and so silently discards
 *     --ldr (melange_adapter.rs:83-93); what the command then measures needs a decision of its own;
 *   - OW_POWER_AMP_MELANGE: the 7-BJT solver runs as its own launch between the preamp and the speaker stage (as in ow_batch_render). */
long long ow_render_poly(const ow_poly_chord* chords, size_t n_chords, const ow_poly_cfg* cfg, ow_poly_row* rows_out,
                         double* final_out, double* separate_sum_out, double* residual_out, size_t stride);

/* ---- centroid tracking (`preamp-bench centroid-track`, tools/preamp-bench/src/main.rs:1925-2135) ------------------------------ */
/* One note: Voice::render_note_with_scale(note, velocity / 127, duration, 44100, displacement scale) -- MLP off, attack noise on, seed
 * note * 2654435761 -- through a fresh legacy DkPreamp at 88 200 Hz, set_ldr_resistance(r_ldr) and THEN reset() (:1989-1991: the DC
 * solve runs at the clamped --ldr, as in render-poly and unlike `render` / ow_batch_render), per-sample 2x oversampling, x volume^2,
 * PowerAmp::new() at the base rate unless no_poweramp, Speaker(speaker), x POST_SPEAKER_GAIN. */
typedef struct ow_centroid_job {
    uint8_t note;                    /* --note, 33..96 */
    uint8_t velocity;                /* --velocity, 0..127 (velocity / 127.0) */
    uint8_t no_preamp;               /* --no-preamp: the reed / pickup signal goes straight to the output stage */
    uint8_t no_poweramp;             /* --no-poweramp */
    uint8_t has_displacement_scale;  /* --displacement-scale given */
    uint8_t reserved[3];
    double displacement_scale;       /* Voice::set_displacement_scale when has_displacement_scale */
    double volume;                   /* --volume (default 0.60; applied squared) */
    double speaker;                  /* --speaker character (default 1.0) */
    double r_ldr;                    /* --ldr (default 1e6) */
} ow_centroid_job;
/* The frame grid is per call: every job of a call has the same frames.  window / hop / end in samples are (ms / 1000.0 * 44100.0) as
 * usize (5 ms -> 220); frame j starts at j * hop and exists while pos + window <= len && pos + window / 2 <= end (integer half);
 * its time is center_ms = (pos + window / 2.0) / 44100 * 1000 (float half).  Bins: freq_resolution = 44100 / window,
 * k_min = ceil(50 / freq_resolution), k_max = min(floor(11025 / freq_resolution), window / 2), all in f64. */
typedef struct ow_centroid_cfg {
    uint32_t struct_size;  /* = sizeof(ow_centroid_cfg) of the caller's header */
    uint32_t job_size;     /* = sizeof(ow_centroid_job) of the caller's header (the stride of `jobs`) */
    double duration_s;     /* --duration (default 1.0) */
    double window_ms;      /* --window-ms (default 5.0) */
    double hop_ms;         /* --hop-ms (default 2.5) */
    double end_ms;         /* --end-ms (default 500.0) */
    int device;
    int preamp_kind;       /* OW_PREAMP_LEGACY8 only (below) */
    int power_amp_kind;    /* OW_POWER_AMP_BEHAVIORAL only (below) */
    int reserved;
} ow_centroid_cfg;
#define OW_CENTROID_MAX_WINDOW 4096   /* samples (93 ms; the command's default is 5 ms): a frame then fits 32 KB of LDS */
enum { OW_CENTROID_NO_DATA = 0, OW_CENTROID_OK = 1, OW_CENTROID_MISS = 2 };
/* The command's summary (:2074-2129).  c10 / c300: the centroid of the FIRST frame whose center_ms >= 10.0 / >= 300.0 (frame10 /
 * frame300, -1 and has_* = 0 when no frame reaches that far) -- even when that frame's centroid is 0.0, which then reads MISS, not
 * "no data".  drift = c300 - c10 when both exist, else 0.  Targets by register: note <= 48, <= 72, else (:2079-2088). */
typedef struct ow_centroid_row {
    double c10, c300, drift;
    double attack_lo, attack_hi, sustain_lo, sustain_hi, drift_lo, drift_hi;
    int32_t frame10, frame300;
    uint8_t has_c10, has_c300;
    uint8_t attack_status, sustain_status, drift_status;   /* OW_CENTROID_OK / OW_CENTROID_MISS; OW_CENTROID_NO_DATA where the command prints no figure */
    uint8_t reserved[3];
} ow_centroid_row;
/* Host only: the number of frames the command's `while` loop visits for this configuration (to size buffers); <0 when the configuration
 * is refused (ow_last_error says why). */
long long ow_centroid_frame_count(const ow_centroid_cfg* cfg);
/* cmd_centroid_track for n_jobs notes at once.  frames_out: host f64 [n_jobs][frames_stride >= frames], the centroid in Hz per frame,
 * 0.0 where the reference's `power_sum > 0.0` fails.  rows_out: [n_jobs].  audio_out: NULL, or host f64 [n_jobs][audio_stride >=
 * (duration_s * 44100) as usize] receiving final_output; asking for it changes no number.  The audio stays in HBM for the analysis;
 * large grids run in chunks of a fixed device-memory budget (OW_CENTROID_CHUNK=<jobs> caps a chunk; tests use it).  A job's numbers do
 * not depend on the other jobs of the call.
 * Returns the frame count, <0 on error.  Refused before any device work (ow_last_error says why): "ABI mismatch", a note outside 33..96,
 * a velocity above 127, a non-finite volume, speaker or displacement_scale, a non-finite or non-positive r_ldr, a hop of 0 samples (the
 * reference would loop forever), a window with no bin in range (k_min > k_max), a window of more than OW_CENTROID_MAX_WINDOW samples, a
 * short stride, and, for the reasons given at ow_render_poly, OW_PREAMP_MELANGE12 (the melange adapter's reset() discards --ldr) and
 * OW_POWER_AMP_MELANGE (the 7-BJT solver needs its own launch). */
long long ow_centroid_track(const ow_centroid_job* jobs, size_t n_jobs, const ow_centroid_cfg* cfg, ow_centroid_row* rows_out,
                            double* frames_out, size_t frames_stride, double* audio_out, size_t audio_stride);
/* The analysis stage alone (spectral_centroid :1931-1958 over the periodic-Hann frames of :2021-2056) on n_rows given rows: signals f64
 * [n_rows][stride], the first `len` samples of a row are analysed (a device pointer if signals_is_device != 0, e.g. what
 * ow_batch_render left in HBM), at 44 100 Hz.  frames_out: host f64 [n_rows][frames_stride >= frames]; entries past the frame count are
 * left untouched.  Returns the frame count (0: nothing written), <0 on error; the same refusals for hop, window and strides. */
long long ow_centroid_analyze(const double* signals, size_t n_rows, size_t stride, size_t len, size_t window_samples, size_t hop_samples,
                              size_t end_sample, int device, int signals_is_device, double* frames_out, size_t frames_stride);

/* ---- note audits (`preamp-bench intermod-audit` and `overshoot`, tools/preamp-bench/src/main.rs:675-903, 2137-2247) ------------ */
/* Both commands audit Voice::render_note(note, velocity / 127, duration, 44100) alone: one voice (MLP off, attack noise on, seed
 * note * 2654435761, the note's own displacement scale; voice.rs:191-221), no preamp, no power amp, no speaker. */
typedef struct ow_note_job {
    uint8_t note;                    /* 33..96 */
    uint8_t velocity;                /* 0..127 (velocity / 127.0); `intermod-audit` itself renders at 1.0 = 127 */
    uint8_t reserved[6];
} ow_note_job;

/* tables::intermod_risk (tables.rs:675-801): how close the ratio of each mode 2..7 lies to an integer harmonic. */
typedef struct ow_intermod_product {
    uint32_t mode;                   /* 2..7 (1-indexed, as the command prints it) */
    uint32_t nearest_integer;        /* ratio.round() as u32 */
    double mode_ratio;
    double fractional_offset;        /* |ratio - nearest| */
    double beat_hz;                  /* fractional_offset * fundamental_hz */
    double effective_amplitude;      /* BASE_MODE_AMPLITUDES x spatial coupling x dwell attenuation at ff */
    double perceptual_weight;        /* perceptual_beat_weight(beat_hz) */
    double risk_score;               /* effective_amplitude * perceptual_weight */
} ow_intermod_product;
typedef struct ow_intermod_report {
    uint8_t midi;
    uint8_t reserved[7];
    double fundamental_hz, mu;
    ow_intermod_product products[6];
    double max_risk, total_risk;
} ow_intermod_report;
/* Host only (no device): the report of any MIDI byte, as the reference's function accepts any.  Returns 0, <0 on a null `out`. */
int ow_intermod_risk(uint8_t midi, ow_intermod_report* out);

/* dft_magnitude (:893-903) of the window [start, end) of every row: signals f64 [n_rows][stride] (a device pointer if signals_is_device
 * != 0), freqs host f64 [n_rows][n_probes], mags_out host f64 [n_rows][n_probes].  The phase index counts from the window start.  A NaN
 * entry of freqs means "no probe": its output is 0.0 and costs nothing.  Returns 0, <0 on error: end > stride, end <= start, a null
 * pointer, a sample rate that is not a finite positive number, a device error. */
int ow_dft_magnitudes(const double* signals, size_t n_rows, size_t stride, size_t start, size_t end, double sample_rate, const double* freqs,
                      size_t n_probes, int device, int signals_is_device, double* mags_out);

#define OW_INTERMOD_MAX_PROBES 75    /* 32 harmonics + 31 midpoints + 6 x (mode frequency, nearest harmonic) */
/* Host only: the probe frequencies of the render analysis for one note, in the order the analysis sums them: harmonics n * f0 for
 * n = 1..=H, H = min(floor(22050 / f0), 32), stopping at the first >= 22050; midpoints (n + 0.5) * f0 for n in 1..H with the same stop;
 * then, for each product with risk_score >= 0.001, mode_ratio * f0 and nearest_integer * f0.  freqs_out: [OW_INTERMOD_MAX_PROBES] (the
 * rest is left untouched).  Returns the probe count, <0 on error (a null pointer, a note outside 33..96). */
int ow_intermod_probes(uint8_t midi, double* freqs_out, uint32_t* n_harmonics_out, uint32_t* n_midpoints_out);

typedef struct ow_intermod_cfg {
    uint32_t struct_size;  /* = sizeof(ow_intermod_cfg) of the caller's header */
    uint32_t job_size;     /* = sizeof(ow_note_job) of the caller's header (the stride of `jobs`) */
    double duration_s;     /* --duration (default 3.0) */
    int device;
    int reserved;
} ow_intermod_cfg;
enum { OW_INTERMOD_DIRTY = 0, OW_INTERMOD_MARGINAL = 1, OW_INTERMOD_OK = 2, OW_INTERMOD_CLEAN = 3 };
typedef struct ow_intermod_detail {  /* one line of "Per-product detail" (:869-886) */
    uint32_t mode, nearest_integer;
    double intermod_freq, nearest_freq;       /* mode_ratio * f0, nearest_integer * f0 */
    double intermod_mag, nearest_mag;         /* dft_magnitude of the window at them */
    double ratio_db;                          /* 20 log10(intermod_mag / nearest_mag), 0.0 when nearest_mag <= 1e-15 */
    double risk_score;
    uint8_t listed;                           /* risk_score >= 0.001: the command lists it; the magnitudes are 0 otherwise */
    uint8_t reserved[7];
} ow_intermod_detail;
typedef struct ow_intermod_row {
    uint8_t midi, velocity;
    uint8_t too_short;                        /* end <= start: "(signal too short)", every figure below is 0 */
    uint8_t verdict;                          /* OW_INTERMOD_*: ratio_db > 40 CLEAN, > 30 OK, > 20 MARGINAL, else DIRTY */
    uint32_t n_harmonics, n_midpoints;        /* probes that entered the two energy sums */
    uint32_t window_start, window_end;        /* (0.5 * 44100) as usize, (2.0 * 44100).min(len) as usize */
    uint32_t reserved;
    double fundamental_hz;
    double harmonic_energy, midpoint_energy;  /* sums of mag^2 in probe order */
    double h_db, m_db, ratio_db;              /* 10 log10 of the energies (-120.0 when not > 0), h_db - m_db */
    ow_intermod_detail products[6];           /* always filled: only the command's text applies its `ratio_db <= 30.0` rule */
} ow_intermod_row;
/* The render analysis of cmd_intermod_audit (:822-888) for n_jobs (note, velocity) jobs at once.  rows_out: [n_jobs].  audio_out: NULL,
 * or host f64 [n_jobs][audio_stride >= (duration_s * 44100) as usize] receiving the voice rows; asking for it changes no number.  The
 * rows stay in HBM between render and analysis; large grids run in chunks of a fixed device-memory budget (OW_NOTE_AUDIT_CHUNK=<jobs>
 * caps a chunk; tests use it).  A job's numbers do not depend on the other jobs of the call or on the chunking.  When the window is
 * empty (duration <= 0.5 s) every row says too_short and, unless audio_out is given, no device is needed.  n_jobs == 0 returns the
 * sample count and touches nothing.
 * Returns the samples per job, <0 on error.  Refused before any device work (ow_last_error says why): "ABI mismatch", a note outside
 * 33..96, a velocity above 127, a duration giving 2^31 samples or more, a short audio_stride, null arguments. */
long long ow_intermod_audit(const ow_note_job* jobs, size_t n_jobs, const ow_intermod_cfg* cfg, ow_intermod_row* rows_out, double* audio_out,
                            size_t audio_stride);

typedef struct ow_overshoot_cfg {
    uint32_t struct_size;  /* = sizeof(ow_overshoot_cfg) of the caller's header */
    uint32_t job_size;     /* = sizeof(ow_note_job) of the caller's header (the stride of `jobs`) */
    double duration_s;     /* the command's constant 2.0 (:2151), a parameter here */
    int device;
    int reserved;
} ow_overshoot_cfg;
/* cmd_overshoot's figures (:2167-2221).  Window edges are (t * 44100.0) as usize, clamped to the length as the command's slices and
 * rms_window (:2231-2239) clamp them; an empty window gives peak 0.0 / RMS 0.0. */
typedef struct ow_overshoot_row {
    uint8_t note, velocity;
    uint8_t reserved[6];
    double peak_0_10, peak_0_50;              /* max |x| over 0-10 ms, 0-50 ms */
    double rms_100_200, rms_1000_1500;        /* sqrt(sum x^2 / (e - s)) */
    double overshoot_db;                      /* 20 log10(peak_0_10 / rms_100_200), NaN unless rms_100_200 > 1e-15 */
    double bark_decay_db;                     /* 20 log10(peak_0_50 / rms_1000_1500), NaN unless rms_1000_1500 > 1e-15 */
    double pk_dbfs, rms1_dbfs, rms2_dbfs;     /* to_dbfs (:2241-2247) of peak_0_10, rms_100_200, rms_1000_1500: -120.0 at <= 1e-15 */
} ow_overshoot_row;
/* cmd_overshoot for n_jobs (note, velocity) jobs at once; rows_out, audio_out, chunking, independence, the return value and the refusals
 * as for ow_intermod_audit.  A duration of 0 samples needs no device. */
long long ow_overshoot(const ow_note_job* jobs, size_t n_jobs, const ow_overshoot_cfg* cfg, ow_overshoot_row* rows_out, double* audio_out,
                       size_t audio_stride);

/* ---- bark audit (`preamp-bench bark-audit`, tools/preamp-bench/src/main.rs:551-664) --------------------------------------------------
 * Per (note, velocity): how much second harmonic the reed carries into the pickup and out of the preamp.  Stage 1: ModalReed::new with
 * onset 0 (no MLP, no attack noise, no onset ramp), seed note * 2654435761; stage 2: Pickup::new_with_scale(44100, the table's
 * displacement scale); stage 3: a fresh preamp of preamp_kind at a static 1 Mohm, per-sample 2x oversampling (process_oversampled).
 * The figures are taken over the samples [window_start, window_end) = [(measure_start_s * 44100) as usize, (duration_s * 44100) as usize). */
typedef struct ow_bark_cfg {
    uint32_t struct_size;  /* = sizeof(ow_bark_cfg) of the caller's header */
    uint32_t job_size;     /* = sizeof(ow_note_job) of the caller's header (the stride of `jobs`) */
    double duration_s;     /* the command's constant 0.5 (:565), a parameter here */
    double measure_start_s; /* the command's constant 0.25 (:566) */
    int device;
    int preamp_kind;       /* create_preamp: OW_PREAMP_LEGACY8 or OW_PREAMP_MELANGE12 */
} ow_bark_cfg;
typedef struct ow_bark_row {
    uint8_t note, velocity;
    uint8_t reserved[6];
    uint32_t window_start, window_end;
    double fundamental_hz;                    /* params.fundamental_hz (undetuned): H1 is analysed there, H2 at 2.0 * fundamental_hz */
    double displacement_scale;                /* tables::pickup_displacement_scale(note), the value the pickup ran with */
    double reed_peak, y_peak;                 /* max |reed| over the window; reed_peak * displacement_scale */
    double pu_peak;                           /* max |pickup| over the window (volts; the command prints mV) */
    double pu_h1, pu_h2, pu_h2_h1;            /* dft_magnitude (:893-903) of the pickup window, phase counted from window_start; h2 / h1, 0.0 unless h1 > 1e-15 */
    double pre_h1, pre_h2, pre_h2_h1;         /* the same of the preamp window */
} ow_bark_row;
/* cmd_bark_audit for n_jobs (note, velocity) jobs at once.  rows_out: [n_jobs].  taps_out: NULL, or host f64 [n_jobs][3][tap_stride >=
 * samples] receiving the reed, pickup and preamp rows; asking for them changes no number.  The rows stay in HBM between the stages;
 * large grids run in chunks of a fixed device-memory budget (OW_BARK_CHUNK=<jobs> caps a chunk; tests use it).  A job's numbers do not
 * depend on the other jobs of the call or on the chunking.  The legacy preamp runs as a row of sixteen lanes per solver state for
 * launches of up to 4 096 jobs and as a lane pair above (OW_BARK_ROW=0/1 forces the form; the two give the same bits).  n_jobs == 0
 * returns the sample count and touches nothing; a duration of 0 samples needs no device (every figure 0).
 * Returns the samples per job, <0 on error.  Refused before any device work (ow_last_error says why): "ABI mismatch", null arguments, a
 * note outside 33..96, a velocity above 127, an unknown preamp_kind, a duration or start that is negative or not finite, a duration giving
 * 2^31 samples or more, a start that leaves no sample to measure, a short tap_stride. */
long long ow_bark_audit(const ow_note_job* jobs, size_t n_jobs, const ow_bark_cfg* cfg, ow_bark_row* rows_out, double* taps_out,
                        size_t tap_stride);

/* ---- the pump measurements: `preamp-bench pump-sweep` / `pump-trace` / `pump-spike` / `pump-step` / `pump-sinusoid` (main.rs:2329-3063) ----
 * These commands drive gen_preamp::process_sample directly on a CircuitState::default() of the melange 12-node preamp: no adapter, no
 * settled state, no main - shadow difference, no thermal noise.  One point is one run of one such state. */
enum { OW_PUMP_STATIC = 0,      /* the resistance stays at r_settle */
       OW_PUMP_STEP = 1,        /* set_runtime_R_r_ldr(r_to) before capture sample 0 (pump-step) */
       OW_PUMP_RAMP = 2,        /* r_settle + (r_to - r_settle) * (k / (capture - 1)) before capture sample k (pump-spike's slew, :2779-2783) */
       OW_PUMP_LOGCOS = 3 };    /* exp(ln_mid + ln_amp * cos((2 pi sched_freq) * (k * (1 / sample_rate)))) before sample k (pump-sinusoid, :2964-2998) */
typedef struct ow_pump_point {
    double sample_rate;          /* set_sample_rate(sample_rate) when it differs from 48 000 by more than 0.5; the codegen tables otherwise */
    double r_settle;             /* set_runtime_R_r_ldr(r_settle) before the first sample (its clamp to 1 k..1 M and its 1e-12 hysteresis apply) */
    uint64_t settle, capture;    /* sample counts */
    double in_amp, in_freq;      /* input in_amp * sin((2 pi in_freq / sample_rate) * k), k counted from the first settle sample (the extra
                                  * sample is not counted); in_amp == 0: silence */
    uint32_t extra_sample;       /* 1: one more zero-input sample between settle and capture (pump-step's `settled`, the `prev` of the slew
                                  * and of pump-sinusoid); its value is ow_pump_row.extra */
    uint32_t schedule;           /* OW_PUMP_* */
    double r_to;                 /* STEP, RAMP */
    double ln_mid, ln_amp, sched_freq;   /* LOGCOS */
} ow_pump_point;
typedef struct ow_pump_cfg {
    uint32_t struct_size;  /* = sizeof(ow_pump_cfg) of the caller's header */
    uint32_t point_size;   /* = sizeof(ow_pump_point) of the caller's header (the stride of `points`) */
    int device;
    int reserved[5];
} ow_pump_cfg;
typedef struct ow_pump_row {
    double sum, sum_sq;                       /* over the capture, in sample order (pump-sweep, :2397-2411) */
    double mean, std, min, max;               /* sum / n, sqrt(max(sum_sq / n - mean^2, 0)), :2412-2414 */
    double pair_mean, pair_std, raw_std;      /* pump-spike's measure (:2601-2619); meaningful when capture is even */
    double extra;                             /* the extra sample's value (0 without one) */
    double max_step;                          /* max |y[k] - y[k-1]| over the capture, y[-1] = the extra sample (without one: from k = 1) */
    uint64_t nr_exhausted, be_fallbacks, voltage_damps, nan_resets;   /* the state's diag_* counters after the last sample */
} ow_pump_row;
/* Runs n points, every one on its own lane of the device, one launch per distinct sample rate (and per chunk of a fixed device-memory
 * budget; OW_PUMP_CHUNK=<points> caps a chunk; tests use it).  rows_out: [n], in the caller's order.  trace_out: NULL, or host f64
 * [n][trace_stride >= the largest capture] receiving every captured sample (a row's tail beyond its own capture is 0); asking for it
 * changes no number.  A point's numbers do not depend on the other points of the call or on the chunking.  n == 0 returns 0 and touches
 * nothing.
 * Returns 0, <0 on error.  Refused before any device work (ow_last_error says why): "ABI mismatch", a non-finite or non-positive
 * sample_rate / r_settle (and r_to, ln_amp's exp, sched_freq where the schedule uses them), a non-finite in_amp / in_freq, capture == 0,
 * capture < 2 with OW_PUMP_RAMP, an unknown schedule, an extra_sample other than 0 or 1, a run of 2^40 samples or more, a short trace_stride, null arguments. */
int ow_pump_measure(const ow_pump_point* points, size_t n, const ow_pump_cfg* cfg, ow_pump_row* rows_out, double* trace_out, size_t trace_stride);

/* ---- the pump-dynamics fitter (tools/analyze_pump_dynamics.py) ------------------------------------------------------------------ */
/* Six cheap predictors R(t) -> pump(t) over the static pump table of `pump-sweep`, fitted to slewed-R captures of `pump-sinusoid` by
 * Nelder-Mead.  Plain scalars and pointers only (no record).
 * Traces: r / target are host f64, concatenated; trace t is samples offsets[t] .. offsets[t + 1] (offsets: n_traces + 1 entries,
 * offsets[0] == 0) at sample_rates[t].  Table: lut_r strictly ascending and positive, lut_v, 2 <= n_lut <= 1024 points;
 * the lookup is numpy.interp on ln(clip(x, lut_r[0], lut_r[n_lut - 1])) over ln(lut_r): slope * offset + the left value, exact on a
 * knot, the ends held.
 * Models (parameters in rows of four doubles, the first 1 / 1 / 2 / 2 / 3 / 4 used), a = 1 - exp(-1 / (sr tau_ms 1e-3)):
 *   0 lpf_R      [tau_ms]            s[0] = R[0], s[n] = s[n-1] + a (R[n] - s[n-1]); pred = table(s);           tau_ms <= 0: invalid
 *   1 lpf_lnR    [tau_ms]            the same on ln R; pred = table(exp(s))
 *   2 iir1_dR    [a, b]              xi[0] = 0, xi[n] = a xi[n-1] + b (R[n] - R[n-1]); pred = table(R) + xi;    a outside [0, 1): invalid
 *   3 iir1_dlnR  [a, b]              the same driven by ln R[n] - ln R[n-1]
 *   4 iir1_asym  [a, b_up, b_dn]     the same with b_up where the drive is positive, b_dn elsewhere
 *   5 iir2_dlnR  [a1, a2, b0, b1]    xi[0] = xi[1] = 0, xi[n] = a1 xi[n-1] + a2 xi[n-2] + b0 u[n] + b1 u[n-1], u[n] = ln R[n] - ln R[n-1];
 *                                    invalid unless both roots of z^2 - a1 z - a2 are inside the unit circle (the reference's test)
 * Loss: 1e9 for an invalid vector or a prediction that is not finite at every sample; else 1000 sqrt(mean(d d)) over samples skip .. n
 * (mV; the reference's skip is 200), d d summed in sample order.  Every stated operation is one IEEE operation in the reference's
 * order; exp and log are the device library's.
 * Refused with <0 before any launch, the outputs untouched (ow_last_error says why): a trace of skip + 1 samples or fewer, a table that is
 * not strictly ascending or too small / large, a non-positive R, a model id above 5, a trace index out of range, a non-finite input
 * (samples, rates, table, used parameters), maxiter == 0, a short pred_stride, null arguments. */
/* Plain numbers, no new constants (the ABI version stands).  The table holds at most 1024 points.  A fit's status is
 *   0  converged: both of scipy's termination tests passed
 *   1  maxiter: nit reached maxiter
 *   2  start invalid: the whole start simplex was invalid and no valid point was ever found; fun is 1e9 (scipy reports success) */
/* loss_out: host f64 [n_evals]; pred_out: NULL or host f64 [n_evals][pred_stride >= the evaluation's trace]: the prediction rows (NaN
 * rows for an invalid vector; 0 beyond the trace).  An evaluation's numbers do not depend on the other evaluations of the call. */
int ow_pump_fit_eval(const double* r, const double* target, const uint64_t* offsets, const double* sample_rates, size_t n_traces, const double* lut_r,
                     const double* lut_v, size_t n_lut, const uint32_t* eval_trace, const uint32_t* eval_model, const double* eval_params, size_t n_evals,
                     uint32_t skip, int device, double* loss_out, double* pred_out, size_t pred_stride);
/* scipy.optimize.minimize(method="Nelder-Mead", options={xatol, fatol, maxiter}) per fit, from x0 [n_fits][4]: the start simplex scales
 * each coordinate by 1.05 (0.00025 where it is zero); rho 1, chi 2, psi = sigma 0.5; scipy's termination tests and acceptance
 * inequalities; a stable ordering; maxfun unbounded; vertex arithmetic in scipy's operation order.  Outputs by fit: x_out [n_fits][4]
 * (0 beyond the model's parameters), fun_out, nit_out, nfev_out (as scipy counts them), status_out (0 / 1 / 2, above).  A fit's result does
 * not depend on the other fits of the call or on their order. */
int ow_pump_fit(const double* r, const double* target, const uint64_t* offsets, const double* sample_rates, size_t n_traces, const double* lut_r,
                const double* lut_v, size_t n_lut, const uint32_t* fit_trace, const uint32_t* fit_model, const double* x0, size_t n_fits, uint32_t skip,
                double xatol, double fatol, uint32_t maxiter, int device, double* x_out, double* fun_out, uint32_t* nit_out, uint32_t* nfev_out,
                uint32_t* status_out);

/* ---- the pickup-law study (ml/h3_analysis_v2.py) --------------------------------------------------------------------------------- */
/* compute_harmonics (:58-94) and its two inline variants (:291-319, :346-375) for every (carrier, law) pair of a call.  Plain scalars and
 * pointers only (no record, no new constant).  A carrier is a row of three doubles: f0_hz, ds, vel_scale.  A law is a kind and one parameter p:
 *   0  power   nl = y / pow(1 - y, p)                                   (the alpha sweep)
 *   1  factor  nl = (y / (1 - y)) * (1 + p y)                           (the k list)
 *   2  blend   nl = ((1 - p) * (y / (1 - y))) + (p * (y / (1 - y y)))   (the blend list)
 * One job, i = 0 .. n_samples - 1: t = i / sample_rate; reed = vel_scale * sin((2 pi f0) t); y = min(max(reed * ds, -clip), clip);
 * v = nl * sensitivity; out[i] = ((hpf_b0 v[i]) - (hpf_b0 v[i-1])) + (hpf_a1 out[i-1]) from zeros.  y_peak = max |y[i]| over
 * i >= n_samples / 4.  With sig = out[n_samples / 2 :] of m samples and h = 1 .. n_harmonics (<= OW_MAX_HARMONICS):
 * phase = ((2 pi (h f0)) k) / sample_rate, re = sum(sig[k] cos(phase)) / m, im = -sum(sig[k] sin(phase)) / m, amp = 2 sqrt(re re + im im).
 * Every stated operation is one IEEE operation in that order; the sums run in ascending k (numpy's are pairwise); sin, cos and pow are the
 * device library's, except that pow(g, 1.0) is g itself (kind 0 with p == 1 equals kind 1 with p == 0 bit for bit).  hpf_b0 / hpf_a1 are the caller's (the reference: w = tan(pi 2312 / sr), b0 = 1 / (1 + w), a1 = (1 - w) / (1 + w)).
 * amps_out: host f64 [n_carriers][n_laws][n_harmonics]; y_peak_out: host f64 [n_carriers].  A job's numbers do not depend on the other
 * jobs of the call, on their order or on how the laws are cut into wavefronts (by kind, at most 64 per wavefront).
 * Returns 0, <0 on error.  Refused before any launch, the outputs untouched (ow_last_error says why): a null argument, n_samples < 4,
 * n_harmonics of 0 or above OW_MAX_HARMONICS, a kind outside 0..2, a clip that is not inside (0, 1), any non-finite input, a sample rate
 * that is not finite and positive.  n_carriers == 0 or n_laws == 0 returns 0 and touches nothing. */
int ow_pickup_law(const double* carriers, size_t n_carriers, const int32_t* law_kinds, const double* law_params, size_t n_laws, double sample_rate,
                  uint32_t n_samples, uint32_t n_harmonics, double sensitivity, double clip, double hpf_b0, double hpf_a1, int device,
                  double* amps_out, double* y_peak_out);

/* ---- recorded notes against renders (tools/wurli_compare.py) ------------------------------------------------------------------- */
/* compute_stft (:46-58) and what its two callers take from S (harmonic_profile :61-78, measure_spectral_centroid :122-127), for many
 * clips per call.  clips: f64 [n_clips][stride] (a device pointer if clips_is_device != 0, e.g. what ow_batch_render left in HBM);
 * lengths[c] <= stride valid samples; wav24_mode as for ow_extract_harmonics.  Per clip: n_frames = max(1, floor((len - n_fft) / hop) + 1)
 * (Python's floor: one frame when len < n_fft), frame i = samples [i * hop, i * hop + n_fft), zero-padded past len; the analysis reads
 * nothing at or beyond lengths[c].
 * mean_mag: host f64 [n_clips][n_fft / 2 + 1] or NULL: the mean over the frames of |rfft(frame * window)|, frames added in ascending order.
 * centroid: host f64 [n_clips] or NULL: the mean over the frames of sum_k f_k |X_k|^2 / (sum_k |X_k|^2 + 1e-10), f_k = k * (1 / (n_fft *
 * (1 / sample_rate))), numpy's rfftfreq.  At least one of the two is given.
 * window: host f64 [n_fft], the caller's: np.hanning(n_fft).astype(float32) widened, so its bits are the host libm's, as those of the
 * library's own Hann tables are.
 * Arithmetic: the reference holds float32, so a sample is rounded to float32 (after the 24-bit quantiser, if any) and frame * window is one
 * rounded float32 product; from there on f64: an n_fft / 2-point complex FFT in LDS with twiddles from exact integer phases, fixed
 * summation orders, no atomics.  A clip's numbers do not depend on the other clips of the call or on the chunking (1 GiB of device
 * memory per chunk for rows copied from the host and per-frame magnitudes).
 * Returns 0, <0 on error.  Refused (ow_last_error says why), never clamped: a null argument, an n_fft that is not a power of two in 64..8192,
 * hop == 0, an unknown wav24_mode, a sample rate that is not finite and positive, a length beyond the stride, a clip that alone exceeds the
 * chunk's memory.  n_clips == 0 returns 0. */
int ow_stft_profile(const double* clips, size_t n_clips, size_t stride, const uint32_t* lengths, const double* window, uint32_t n_fft, uint32_t hop,
                    double sample_rate, int wav24_mode, int device, int clips_is_device, double* mean_mag, double* centroid);
/* The RMS envelopes of measure_decay (:95-107; 2048 / 512) and measure_attack_time (:136-147; 1024 / 128) and the sum of measure_rms
 * (:130-133) on the same kind of rows, the same float32 rounding of a sample, squares and sums in f64: rms: host f64 [n_clips][frames_stride],
 * rms[c][i] = sqrt(sum of the squares of frame i (zero-padded past len) / frame_len) for i < n_frames[c] = max(1, floor((len - frame_len) /
 * hop) + 1), 0.0 beyond; n_frames: host [n_clips]; sum_sq: host f64 [n_clips] (the squares of the whole clip) or NULL.
 * Returns 0, <0 on error.  Refused: a null argument, frame_len == 0, hop == 0, an unknown wav24_mode, a length beyond the stride, a
 * frames_stride smaller than a clip's frame count.  n_clips == 0 returns 0. */
int ow_frame_rms(const double* clips, size_t n_clips, size_t stride, const uint32_t* lengths, uint32_t frame_len, uint32_t hop, int wav24_mode,
                 int device, int clips_is_device, double* rms, size_t frames_stride, uint32_t* n_frames, double* sum_sq);

#ifdef __cplusplus
}
#endif
#endif /* OPENWURLI_HIP_H */
