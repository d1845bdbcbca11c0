/* openwurli-hip: TEST AND DEBUG hooks of the library -- NOT part of the drop-in boundary.
 *
 * A facade binds what include/openwurli_hip.h declares; nothing in this header replaces an item of the reference's API.
 * These entry points exist so that tests can reach pieces that have no public surface: the host voice-pool state machine
 * without a device, the note-on MLP's raw outputs, the kernels' own division / exp / tanh routines next to the device
 * library's, and a fault injector for the "never fails, degrades to silence" contract.
 */
#ifndef OPENWURLI_HIP_TEST_H
#define OPENWURLI_HIP_TEST_H

#include "openwurli_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host-logic test hooks ------------------------------------------------------------------ */
/* A detached engine: the host voice-pool / MIDI state machine (engine.rs:299-374,569-602) without a pool or a device.
 * note_on / note_off / set_sustain / get_diag / slot_* work on it; the slot ops it would send to the GPU can be taken
 * out, and the post-render bookkeeping can be driven with an explicit "silent" mask.  Used by the CPU-only tests. */
ow_engine* ow_test_engine_new(double sample_rate);
void ow_test_engine_free(ow_engine*);
/* Copies up to cap pending ops (type 1 = note-on, 2 = damper, 3 = move-to-steal; seed = fade length for type 3), clears the queue,
 * returns the number that were pending. */
size_t ow_test_engine_take_ops(ow_engine*, uint8_t* type, uint8_t* slot, uint8_t* note, uint32_t* seed, double* velocity, size_t cap);
void ow_test_engine_after_render(ow_engine*, size_t len, uint64_t silent_mask);
uint64_t ow_test_engine_masks(const ow_engine*, int which /* 0 = slot voices, 1 = steal voices */);

/* ---- diagnostics ------------------------------------------------------------------------- */
/* Raw (pre-fade, pre-clamp) outputs of the note-on MLP (mlp_correction.rs:86-116) for n (note, velocity) pairs:
 * out[n][11].  use_mfma = 1 runs the wavefront-batched v_mfma_f64_16x16x4_f64 path that k_apply_ops uses,
 * 0 the scalar lane path (batch jobs).  Returns 0, <0 on device error. */
int ow_debug_mlp_raw(const uint8_t* notes, const double* velocities, size_t n, double* out, int use_mfma, int device);
/* The kernels' division routine (ow_voice_dev.h, ow_div: the compiler's IEEE f64 division sequence without the operand
 * pre-scaling that only extreme exponents need) next to the compiler's own `a / b`, element-wise on the device:
 * fast[i], ieee[i] for n operand pairs.  Returns 0, <0 on device error. */
int ow_debug_div(const double* a, const double* b, size_t n, double* fast, double* ieee, int device);
/* The same for the constant-divisor form (OW_DIV_C): which = 0 jitter draw 2147483647.5, 1 Twin-T V_T, 2 LED span 10.25,
 * 3 preamp V_T 0.026, 4 power-amp 0.013^2, 5 power-amp headroom 22, 6 attack-noise draw 2147483647, 7 pickup soft-limit range 0.04.  a == NULL (which = 0 or 6) runs
 * every numerator of that draw (all 2^31 integers / every int32) on the device and stores the number of quotients that differ from
 * `a / B` in *mismatches. */
int ow_debug_div_const(int which, const double* a, size_t n, double* fast, double* ieee, uint64_t* mismatches, int device);
/* The other short division forms of the kernels next to the compiler's `a / b`, element-wise: mode 0 = divisor with a host-computed
 * reciprocal y[i] = 1.0 / b[i] (ow_div_const: the power amp's per-device constants), 1 = refined reciprocal shared among the quotients over
 * one pivot (ow_rcp_refined + ow_div_y), 2 = the same without the final v_div_fixup (finite operands, pivots checked: the melange column
 * kernel). */
int ow_debug_div_forms(int mode, const double* a, const double* b, const double* y, size_t n, double* fast, double* ieee, int device);
/* Element-wise, the kernels' own elementary functions next to the device library's: which = 0 the preamp's junction exponential
 * (exp without the overflow / underflow selects, for arguments inside the junction clamp) and exp(); 1 the power amp's / speaker's
 * tanh (expm1-based, <= 2 ulp) and tanh(); 2 / 3 / 4 the reed's onset gain (reed.rs:251-264: (0.5 (1 - cos x))^p as exp(p ln .)) at phase x
 * with p = 1.25 / 1.5 / 1.9 and the same expression with the library's pow(). */
int ow_debug_unary(int which, const double* x, size_t n, double* fast, double* lib, int device);
/* ONE step of the legacy DK preamp (DkPreamp::dk_step, dk_preamp_legacy.rs:447-554) on n independent cases at chain rate `rate`, through
 * one of the kernels' four forms of it: form 0 = dk_step, one state per lane (k_preamp); 1 = dk_step_pair, one lane holds case 2k as its
 * main and case 2k + 1 as its shadow state and uses case 2k's g_ldr / g_ldr_prev for both (k_preamp_pair); 2 = dk_step_wide, four lanes
 * per state (k_preamp_wide, k_chain_fused); 3 = dk_step_row, sixteen lanes per state (k_chain_row).  The production device functions with
 * the production constants of that rate; the state is prepared as at a block start (the fourteen fields, then the junctions'
 * transconductances at v_nl).  states_in / states_out: [n][14] = j_cin, cin_rhs_prev, v[8], i_nl[2], v_nl[2]; input, g_ldr, g_ldr_prev,
 * out: [n] (out = the step's return value, v[OUT]).  Cases fill the wavefronts in order (64 / 128 / 16 / 4 cases per wavefront); n need
 * not fill the last one.  Returns 0, <0 on error. */
int ow_debug_dk_step(int form, double rate, const double* states_in, const double* input, const double* g_ldr, const double* g_ldr_prev, size_t n,
                     double* states_out, double* out, int device);
/* ONE step of the Twin-T tremolo oscillator (TremCircuit::process_sample(0.0), gen_tremolo.rs:2353-3116) on n independent cases at chain
 * rate `rate`, through one of the kernels' three forms of it: form 0 = trem_osc_step, one system per lane, TremPark / TremMats in LDS as
 * k_tremolo sets them up (64 cases per wavefront); 1 = trem_osc_step_wide, four lanes per system (k_tremolo_wide, k_trem_traj_extend: 16
 * cases per wavefront); 2 = trem_osc_step_row, sixteen lanes per system with its generic-sweep and backward-Euler wrappers
 * (k_trem_settle_row, k_trem_traj_extend_row: one case per wavefront).  The production device functions with the production constants of
 * that rate; the CdS cell (env, r_ldr) is not stepped.  states_in / states_out: [n][15] = v_prev[7], i_nl_prev[4], i_nl_prev_prev[4] (the
 * first fifteen of ow_debug_trem_trajectory's state rows); out: [n] = the step's return value, v[OUT]; info: [n] = the step's increment of
 * the backward-Euler fallback counter.  Cases fill the wavefronts in order; n need not fill the last one.  Returns 0, <0 on error. */
int ow_debug_trem_step(int form, double rate, const double* states_in, size_t n, double* states_out, double* out, unsigned long long* info, int device);
/* ONE step of the melange 12-node preamp solver (set_runtime_R; process_sample, gen_preamp.rs:1973-1984, 3399-3663) on n independent
 * cases at chain rate `rate`, through one of its device forms: 0 = mel_process, the rank-one form with MelMats in LDS (k_preamp_mel,
 * k_mel_settle); 1 / 2 = mel_process_lit after the fast leading-block / the generic rebuild (k_preamp_mel_lit); 3 / 4 = mel_process_col,
 * fast / generic (k_preamp_mel_col); 5 / 6 = mel_eng_sample, fast / generic (k_preamp_mel_eng).  The production device functions with
 * the production constants of that rate; no noise; mel_set_r(r_ldr) runs before the step.  states_in / states_out: [n][21] = v[12],
 * i_nl_prev[3], i_nl_prev_prev[3], input_prev, pot, be_cooldown (as a double); input, r_ldr, out: [n]; info: [n][2] = the step's
 * increments of the backward-Euler fallback and NaN-reset counters.  Forms 1-6 take case 2k as an engine's main state and case 2k+1 as
 * its shadow and build the matrices for the main's pot; forms 5 / 6 also give the shadow the main's resistance and input 0, so a shadow
 * case is expected to carry those.  n need not fill the last wavefront or pair.  Returns 0, <0 on error. */
int ow_debug_mel_step(int form, double rate, const double* states_in, const double* input, const double* r_ldr, size_t n, double* states_out, double* out,
                      unsigned* info, int device);

/* ---- tremolo phase groups -------------------------------------------------------------------- */
/* Engines whose tremolo oscillators are bit-identical share one oscillator (a fresh pool is one group).  This hook cuts the pool into
 * n_groups groups {g, g + n_groups, ...} and runs group g ahead by g * (one oscillator period / n_groups) samples: decorrelated
 * tremolo phases, as instances that were reset at different times would have -- what the bench uses to price the per-engine path.
 * Returns 0, <0 on error. */
int ow_test_pool_stagger_tremolo(ow_pool*, size_t n_groups);
/* Number of tremolo phase groups of the pool (1 for a fresh pool, +1 for every engine reset / warmed up on its own). */
size_t ow_test_pool_tremolo_groups(const ow_pool*);

/* The melange power amp ALONE (melange_adapter::PowerAmp::new_at_sample_rate(sample_rate) + process, power_amp.rs:335-431) on n_rows
 * independent input rows of n samples each (f64 [n_rows][n]), one solver per row.  poke_at / poke_node / poke_val (each [n_rows], or all
 * NULL): before sample poke_at[r] of row r, node voltage poke_node[r] of the solver state is overwritten with poke_val[r] (forced
 * divergence).  out: [n_rows][n] normalised amp output; taps (or NULL): [n_rows][n][3] = outer Newton iterations of the sample (70 =
 * exhausted), divergence-guard resets so far, positive rail voltage after the sample.  Returns 0, <0 on error. */
int ow_debug_power_amp(double sample_rate, const double* in, size_t n_rows, size_t n, int rail_sag, const long long* poke_at, const int* poke_node,
                       const double* poke_val, double* out, double* taps, int device);

/* ---- melange power amp: solver taps ------------------------------------------------------------ */
/* Keep the amp's output of every chain-rate sample of the last block (before the half-band down-sampler): f64 [n_engines][n_os] through
 * ow_test_pool_read_power_amp_out.  Costs 16 B per engine and chain-rate sample of the block capacity; off until enabled. */
int ow_test_pool_enable_power_amp_tap(ow_pool*);
/* Melange power amp: Newton passes (main sweep) engine k spent on its LAST rendered block -- the figure the demand-ordered dispatch of
 * k_post_mpa sorts by (0 = not rendered yet).  out: one uint32 per engine of the pool; n must equal the pool size.  -1 without the amp. */
int ow_test_pool_power_amp_passes(ow_pool*, uint32_t* out, size_t n);
int ow_test_pool_read_power_amp_out(ow_pool*, double* out_host, size_t out_stride, size_t n_os);
/* Overwrite one node voltage of the amp's solver state (v_prev[node], node < 20) before the next block: the way to force the
 * divergence guard (power_amp.rs:410-421: |node| > 100 V -> reset + hold last good) at a known sample. */
int ow_test_engine_poke_power_amp_node(ow_engine*, int node, double volts);

/* ---- host constant builders ------------------------------------------------------------------ */
/* The library's own set_sample_rate / rebuild_matrices of the three generated solvers (ow_consts_host.hpp; gen_tremolo.rs:2111-2342,
 * gen_preamp.rs:1930-2219, gen_power_amp.rs:8588-8831) at chain rate `rate`, on the host, no device needed.  solver: 0 Twin-T tremolo
 * (N 7, M 4), 1 melange preamp at the nominal pot (N 12, M 3), 2 melange power amp (N 20, M 16).  Outputs are row-major s[N][N] k[M][M]
 * sni[N][M] aneg[N][N] and the backward-Euler set (any pointer may be NULL).  force_rebuild != 0 rebuilds even at the solver's codegen
 * rate, where the reference copies its baked tables -- the tests compare that rebuild with the baked tables.  Returns N * 100 + M. */
int ow_test_host_matrices(int solver, double rate, int force_rebuild, double* s, double* k, double* sni, double* aneg,
                          double* s_be, double* k_be, double* sni_be, double* aneg_be);

/* ---- settled-state caches --------------------------------------------------------------------- */
/* The library keeps the settled Twin-T oscillator state per (device, chain rate) and the settled melange preamp / power-amp states per
 * device for the life of the process (the reference's OnceLock caches: melange_adapter.rs:12-29, power_amp.rs:283-299; the Twin-T one is
 * this library's own, tremolo.rs:92-102 pays 2 s of solver steps per Tremolo::new).  This drops them, so that the next pool runs the
 * settle kernels again -- the test compares a cached engine with a freshly settled one bit for bit.  Returns the number of cached
 * Twin-T states dropped. */
int ow_test_clear_settle_caches(void);

/* ---- the trajectory's oscillator kernels on their own --------------------------------------------- */
/* CircuitState at DC_OP, n_settle oscillator steps without the cell, then n steps of the shared trajectory (r_ldr[0 .. n)) in launches of
 * `chunk` steps, with the quad-lane kernels (row = 0: ow_trem_wide.h) or the one-system-per-wavefront kernels (row = 1: ow_trem_row.h).
 * No store and no pool are touched.  r_out[n]; state_out[18] = the oscillator rows after the last step; ckpt_out[(n / 4096 + 2) * 16] and
 * be_out[1024] may be NULL; *ms_out = device time of the trajectory launches; cold_out[2] (or NULL, row kernels only) = Newton sweeps the row
 * step handed to the generic sweep / steps that took the backward-Euler retry during those launches; kick18 (or NULL): added to the
 * DC_OP state rows (v[7], i_prev[4], i_pp[4]) before anything runs -- a circuit pushed off its operating point.  The two must agree bit for bit
 * (tests/test_gpu_trajectory.py); the time per step is the figure every small pool waits for.  Returns 0, <0 on error. */
int ow_debug_trem_trajectory(double sample_rate, long long n_settle, long long n, long long chunk, int row, double* r_out, double* state_out,
                             double* ckpt_out, unsigned long long* be_out, double* ms_out, int device, unsigned long long* cold_out, const double* kick18);

/* ---- voice-sum NaN guard ----------------------------------------------------------------------- */
/* Overwrite one double of a voice record on the device before the next block (slot 0..63; steal != 0 selects the slot's steal voice;
 * field = a VF_* index of openwurli_amd/csrc/ow_types.h: OW_TEST_VF_Q is the pickup charge, OW_TEST_VF_S0 mode 0's sine state).  A
 * voice cannot turn non-finite through the API, so this is how the guard of engine.rs:496-521 (zero the block, render every voice
 * again, free the culprits; the survivors advance twice) is provoked.  Returns 0, <0 on error. */
#define OW_TEST_VF_S0 0
#define OW_TEST_VF_Q 81
int ow_test_engine_poke_voice(ow_engine*, int slot, int steal, int field, double value);

/* The same for the legacy preamp: overwrite node voltage `node` (0..7) of engine e's main (shadow = 0) or shadow solver state before the next
 * block.  A non-finite value provokes the preamp's own NaN reset (dk_preamp_legacy.rs:610-615).  Returns 0, <0 on error. */
int ow_test_engine_poke_preamp_node(ow_engine*, int shadow, int node, double volts);
/* ... and read that state back after the blocks rendered so far: out14 = j_cin, cin_rhs_prev, v[8], i_nl[2], v_nl[2] (DkState,
 * dk_preamp_legacy.rs:231-239).  Returns 0, <0 on error. */
int ow_test_engine_read_preamp_state(ow_engine*, int shadow, double* out14);

/* ---- chain-state rows ---------------------------------------------------------------------------- */
/* Rows [first_row, first_row + n_rows) of engine e's chain state (CS_* of openwurli_amd/csrc/ow_types.h, one double each; u64 rows as
 * their bits) copied out to / in from n_rows doubles.  The output stage -- power amp, half-band decimator, speaker, the two smoothers,
 * f32 cast and NaN guard -- keeps all it carries from block to block in the rows named here, so "rows before + the stage's input
 * (ow_pool_read_preamp_out / ow_test_pool_read_power_amp_out) + setters -> rows after + f32 block" is a pure function that
 * tests/test_gpu_post_stage.py compares with the oracle's (owo_output_stage_block).  The write forgets a block rendered ahead and waits
 * for the stream first; the host's own mirror of a smoother's target is not touched, so write the target it holds.  Both refuse rows
 * outside [0, OW_TEST_CS_COUNT).  Return 0, <0 on error. */
#define OW_TEST_CS_SM_SPK 22   /* [4] speaker-character smoother: current, target, step, remaining (u64) */
#define OW_TEST_CS_SM_VOL 26   /* [4] volume smoother */
#define OW_TEST_CS_OS_DA 67    /* [3] half-band decimator, branch A */
#define OW_TEST_CS_OS_DB 70    /* [3] branch B */
#define OW_TEST_CS_OS_DD 73    /* down_delay */
#define OW_TEST_CS_SPK_HPF 74  /* [7] b0 b1 b2 a1 a2 s1 s2 */
#define OW_TEST_CS_SPK_LPF 81  /* [7] */
#define OW_TEST_CS_SPK_CHAR 88
#define OW_TEST_CS_SPK_A2 89
#define OW_TEST_CS_SPK_A3 90
#define OW_TEST_CS_SPK_TC 91
#define OW_TEST_CS_SPK_TS 92
#define OW_TEST_CS_FLAGS 93    /* u64, bit 0: the output guard fired, preamp and upsampler reset pending */
#define OW_TEST_CS_COUNT 137
int ow_test_engine_read_chain_rows(ow_engine*, int first_row, int n_rows, double* out);
int ow_test_engine_write_chain_rows(ow_engine*, int first_row, int n_rows, const double* in);

/* ---- voice records -------------------------------------------------------------------------------- */
/* One voice record (VF_* of openwurli_amd/csrc/ow_types.h) copied out to / in from OW_TEST_VF_COUNT doubles, field-major: out[f] is field
 * f of the voice in `slot` (steal != 0: the slot's steal voice); on the device the fields lie 64 doubles apart.  u64 fields travel as
 * their bits: SAMPLE and ONSET_N whole; RNG = jitter_state | noise rng << 32; NCNT = noise remaining | fade-in remaining << 32; FLAGS =
 * (bit 0 damper active, bit 1 ramp done) | midi note << 32; STEAL (steal records only) = steal_fade | steal_fade_len << 32.  The mode
 * fields are seven wide (a name ending in 0 is mode 0's).  A voice block -- k_voice, k_voice_steady and its skewed, attack, steal and release variants
 * -- is a pure function (record, L) -> (record, L samples at the voice-sum tap, status bits), which tests/test_gpu_voice_block.py compares
 * with the oracle's (owo_voice_block).  The read waits for the stream and shows the records as the last render left them (ops queued
 * since are applied by the next render).  The write forgets a block rendered ahead, has the voice lists packed again and re-derives the
 * engine's transient flag -- which voice kernel its slot voices get -- from the records of its sounding slot voices as they then stand
 * (damper bit, sample < onset_n, noise remaining); which slots are occupied, releasing or stolen stays what the API calls made it.
 * Return 0, <0 on error. */
#define OW_TEST_VF_C0 7
#define OW_TEST_VF_ENV0 14
#define OW_TEST_VF_DRIFT0 21
#define OW_TEST_VF_COS_INC0 28
#define OW_TEST_VF_SIN_INC0 35
#define OW_TEST_VF_PHASE_INC0 42
#define OW_TEST_VF_AMP0 49
#define OW_TEST_VF_DECAY0 56
#define OW_TEST_VF_DRATE0 63
#define OW_TEST_VF_DMULT0 70
#define OW_TEST_VF_ONSET_INC 77
#define OW_TEST_VF_ONSET_EXP 78
#define OW_TEST_VF_DRAMP 79
#define OW_TEST_VF_DCOUNT 80
#define OW_TEST_VF_DS 82
#define OW_TEST_VF_GAIN 83
#define OW_TEST_VF_NAMP 84
#define OW_TEST_VF_NB0 85      /* [5] attack-noise band-pass b0 b1 b2 a1 a2 */
#define OW_TEST_VF_NS1 90
#define OW_TEST_VF_NS2 91
#define OW_TEST_VF_SAMPLE 92
#define OW_TEST_VF_ONSET_N 93
#define OW_TEST_VF_RNG 94
#define OW_TEST_VF_NCNT 95
#define OW_TEST_VF_FLAGS 96
#define OW_TEST_VF_STEAL 97
#define OW_TEST_VF_BETA 98
#define OW_TEST_VF_JREV 99
#define OW_TEST_VF_JDIFF 100
#define OW_TEST_VF_NDECAY 101
#define OW_TEST_VF_VSR 102
#define OW_TEST_VF_COUNT 103
int ow_test_engine_read_voice_record(ow_engine*, int slot, int steal, double* out);
int ow_test_engine_write_voice_record(ow_engine*, int slot, int steal, const double* in);

/* Plain device-to-host copy, for reading a block that ow_pool_render(pool, NULL, ...) left in HBM (ow_pool_device_output). */
int ow_test_device_read(void* dst_host, const void* src_device, size_t bytes, int device);
/* Plain host-to-device copy into a buffer of ow_device_alloc, for handing given audio to an entry point's audio_is_device path. */
int ow_test_device_write(void* dst_device, const void* src_host, size_t bytes, int device);

/* k_window_stats (the analysis kernel of ow_overshoot) on given host rows: signals f64 [n_rows][stride]; up to four windows [starts[k],
 * ends[k]) with ends[k] <= stride, kinds[k] 0 = max |x| (NaN samples ignored, an empty window gives 0), 1 = sum of squares; out host f64
 * [n_rows][n_windows].  Returns 0, <0 on error. */
int ow_debug_window_stats(const double* signals, size_t n_rows, size_t stride, const uint32_t* starts, const uint32_t* ends, const uint32_t* kinds,
                          size_t n_windows, int device, double* out);
/* The voices' per-note table as the device builds it (tables.rs:804-830 and the note-only scalars of Voice::note_on): out host f64
 * [OW_TEST_NOTE_TABLE_FIELDS][64], field-major, note index = midi - 33.  Fields: 0 detuned f0, 1..7 mode ratios, 8..14 base amplitude x
 * spatial coupling, 15..21 decay rates, 22..28 amplitude offsets, 29 displacement scale, 30 velocity exponent, 31 f0, 32 register trim,
 * 33 voicing.  Returns 0, <0 on error. */
#define OW_TEST_NOTE_TABLE_FIELDS 34
int ow_debug_note_table(double* out, int device);

/* Fast paths of the melange preamp's literal rebuild the host found usable at chain rate `rate` (host only): bit 0 = leading block
 * replayed once per rate, bit 1 = the LU factors have the compiled-in sparsity pattern of the column-streamed kernel.  <0 on error. */
int ow_test_host_melange_paths(double rate);

/* ---- latched switches ------------------------------------------------------------------------- */
/* The OW_* environment switches ("Environment switches") are read once, when a pool is created, and kept in the pool: the
 * render path never calls getenv.  These change / read one on a live pool, by its name in the library's one table of switches
 * (host_base.inc: the variable's name in lower case without "OW_"; -1 = by size for the tri-state ones, "pa_sort" 0..2).  set returns 0,
 * <0 for an unknown switch or one that is environment-only ("trem_traj", "trem_cache", the offline entry points' switches); get returns
 * the value, -2 for an unknown name, and also answers "trem_traj" (the pool reads the shared trajectory), "voice_skew_active",
 * "blocks_steady" / "_general" / "_attack" / "_steal" and "midi_device_bursts". */
int ow_test_pool_set_switch(ow_pool*, const char* name, int value);
int ow_test_pool_get_switch(const ow_pool*, const char* name);
/* The chain and output-stage kernels one block of a pool gets (host only, no pool): preamp / power-amp kind of openwurli_hip.h, whether
 * the chain is oversampled, whether the melange factors have the compiled-in sparsity pattern, engines and samples of the block,
 * whether its rows go to a pinned block of ow_host_alloc.  switches: overrides of the DEFAULT switches (the environment is not read)
 * as "name=value,name=value", or NULL.  Writes the kernels' names as a kernel trace shows them, e.g. "k_preamp_pair + k_post<false,true>"
 * or "k_chain_stream" alone.  Returns 0; -1 for an unknown switch name, a refused value or a buffer that is too short. */
int ow_test_block_plan(int preamp_kind, int power_amp_kind, int oversample, int ml_sparse_ok, int n_engines, int block_len, int to_pinned_block,
                       const char* switches, char* out, size_t cap);
/* out[0] = engines of the pool reading the shared tremolo trajectory, out[1] = samples its store holds (produced or enqueued),
 * out[2] = the store's capacity in samples. */
int ow_test_pool_trajectory_info(const ow_pool*, uint64_t out[3]);
/* The store behind the pool, in samples: [0] produced or enqueued, [1] known complete, [2] held by its buffers now, [3] configured capacity,
 * [4] t of the pool's oldest engine on it. */
int ow_test_pool_trajectory_state(const ow_pool*, uint64_t out[5]);

/* ---- fault injection ------------------------------------------------------------------------ */
/* The next n_renders calls of ow_pool_render / ow_engine_render on this pool fail before their first launch, exactly as a HIP
 * error would (exception inside the guarded region): the caller's block must come back as silence in every row, ow_last_error
 * must name the failure, and the renders after them must work again. */
void ow_test_inject_render_faults(ow_pool*, int n_renders);
/* The k-th acquisition (0-based) of a device buffer, pinned buffer, event or stream that the calling thread makes from now on throws
 * a std::runtime_error naming this hook INSTEAD of calling HIP (a host exception: no device state is touched), then the hook disarms
 * itself.  k < 0 disarms it.  Whatever entry point was running reports the error the way it reports a failed hipMalloc; nothing it
 * had acquired up to there may stay behind, and the object it worked on must remain usable. */
void ow_test_fail_acquire_after(int k);
/* Device buffers, pinned buffers, events and streams the library owns right now, process-wide (pools, trajectory stores, running calls). */
uint64_t ow_test_live_resources(void);

#ifdef __cplusplus
}
#endif
#endif /* OPENWURLI_HIP_TEST_H */
