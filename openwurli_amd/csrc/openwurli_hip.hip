// openwurli-hip: host side of the C-ABI (include/openwurli_hip.h) -- pool/engine objects,
// the voice-pool / MIDI state machine of WurliEngine (engine.rs:299-374,569-602) and the
// kernel launch sequence of one render (host_pool.inc: render_range, a sequence of named
// phases; which chain / output-stage kernel a block gets is decided by the pure functions
// choose_chain / choose_post there).  The state machine is integer/branchy host work;
// everything that touches audio samples runs in the gfx950 kernels of ow_kernels.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <emmintrin.h>
#include <string>
#include <thread>
#include <vector>

#include "../../include/openwurli_hip.h"
#include "../../include/openwurli_hip_test.h"
#include "ow_consts_host.hpp"
#include "ow_vm.h"
#include "ow_kernels.h"
#include "ow_job_kernels.h"
#include "ow_mlp_mfma.h"
#include "ow_mlp_train.h"
#include "ow_melange_dev.h"
#include "ow_melange_lit.h"
#include "ow_melange_col.h"
#include "ow_melange_eng.h"
#include "ow_power_amp_dev.h"
#include "ow_features.h"
#include "ow_goertzel_kernels.h"
#include "ow_isolation_kernels.h"
#include "ow_trem_wide.h"
#include "ow_trem_row.h"
#include "ow_chain_row.h"
#include "ow_dk_step_debug.h"
#include "ow_trem_step_debug.h"
#include "ow_mel_step_debug.h"
#include "ow_audit.h"
#include "ow_calib_kernels.h"
#include "ow_pbench_kernels.h"
#include "ow_poly_kernels.h"
#include "ow_centroid_kernels.h"
#include "ow_stft_kernels.h"
#include "ow_note_audit_kernels.h"
#include "ow_bark_kernels.h"
#include "ow_pump_kernels.h"
#include "ow_pump_fit_kernels.h"
#include "ow_pickup_law_kernels.h"
#include "ow_midi_kernels.h"
#include "ow_chain_wide.h"
#include "ow_chain_stream.h"
#include "ow_vm_kernels.h"
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>

using owdev::OwEngineOut;

// The host side is ONE translation unit cut along its seams (round 6: 4 200 lines in one file before); every piece is included here, in
// dependency order, and nowhere else.
#include "host/host_base.inc"           // errors, device buffers, persistent host workers, latched switches and their one table
#include "host/host_types.inc"          // ow_engine / ow_pool: the host side of one engine and of a pool
#include "host/host_settle.inc"         // voice-pool mirror synchronisation, process-wide settled states (melange preamp / power amp, Twin-T)
#include "host/host_trajectory.inc"     // the shared Twin-T / CdS trajectory store (TremTraj), its helper thread, traj_acquire
#include "host/host_offline.inc"        // what the offline entry points share: refusals, row geometry and chunking, OfflineCall, the melange power amp stage
#include "host/host_jobs_chain.inc"     // kernel choice for the job paths and the job chain (batch render, render-midi)
#include "host/host_pool.inc"           // tremolo phase groups, chain (re)initialisation, kernel choice of a block, voice lists, render_range and its phases, post-render bookkeeping, pool life cycle
#include "host/api_pool.inc"            // C-ABI: library / pool entry points, host blocks, taps, trajectory control and persistence, MIDI bursts
#include "host/api_engines.inc"         // C-ABI: the WurliEngine API (engine.rs)
#include "host/api_test_hooks.inc"      // C-ABI of include/openwurli_hip_test.h: host-logic hooks, diagnostics, switches
#include "host/api_offline.inc"         // C-ABI: render_note, batch render, WAV writers, feature stage
#include "host/api_mlp.inc"             // C-ABI: note-on MLP corrections given at run time (weight sets per job, explicit corrections)
#include "host/api_mlp_train.inc"       // C-ABI: training note-on MLP weight sets on the device (ml/train_mlp.py's train(), many models per call)
#include "host/api_alias_audit.inc"     // C-ABI: the click-band alias audit (alias_audit.rs)
#include "host/api_midi_render.inc"     // C-ABI: `preamp-bench render-midi` (SMF reader, voice manager, chain)
#include "host/api_calibrate.inc"       // C-ABI: `preamp-bench calibrate` / `sensitivity` (the calibration sweep)
#include "host/api_preamp_measure.inc"  // C-ABI: `preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep` (the preamp measurements)
#include "host/api_render_poly.inc"     // C-ABI: `preamp-bench render-poly` (chord intermodulation, many chords per call)
#include "host/api_centroid.inc"        // C-ABI: `preamp-bench centroid-track` (spectral centroid over time, many notes per call)
#include "host/api_note_audit.inc"      // C-ABI: `preamp-bench intermod-audit` / `overshoot` (the note audits, many notes per call)
#include "host/api_bark_audit.inc"      // C-ABI: `preamp-bench bark-audit` (H2 / H1 per chain stage, many notes per call)
#include "host/api_pump.inc"            // C-ABI: `preamp-bench pump-sweep` / `pump-trace` / `pump-spike` / `pump-step` / `pump-sinusoid` (the pump measurements)
#include "host/api_pump_fit.inc"        // C-ABI: tools/analyze_pump_dynamics.py (six IIR predictors of the pump, their RMSE, Nelder-Mead; many fits per call)
#include "host/api_pickup_law.inc"     // C-ABI: ml/h3_analysis_v2.py (the pickup-law study: every law point of every carrier per call)
#include "host/api_harmonics.inc"       // C-ABI: the recording side of the ML loop (Goertzel harmonics, inter-harmonic noise floor; many segments per call)
#include "host/api_compare.inc"         // C-ABI: the analysis of tools/wurli_compare.py (LDS FFT: mean spectrum and centroid of many clips per call; RMS envelopes)
#include "host/api_isolation.inc"       // C-ABI: recorded-note intake (isolation sub-scores of all notes of all files per call, clip bounds of many clips per call)
