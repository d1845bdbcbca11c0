"""ctypes wrapper of the CPU ORACLE (oracle/_build/libow_oracle.so).

Test infrastructure only: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg -- never by the product package.
"""
import ctypes as C
import subprocess

import numpy as np

import native


def build():
    """All three libraries at once (build.sh); lib*() below ask make for their own."""
    subprocess.check_call(["make", "-s", "-C", native.ORACLE_DIR])


def lib():
    return native.load("ow_oracle")


def lib_perturbed():
    """Sensitivity variant of the oracle (BJT exp() off by one ulp, oracle/ow_chain.hpp)."""
    return native.load("ow_oracle", "perturbed")


def lib_voice_perturbed():
    """Second sensitivity variant: the voice path's rotation / decay library calls off by one ulp (oracle/ow_voice.hpp)."""
    return native.load("ow_oracle", "voice_perturbed")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OracleEngine:
    """CPU restatement of WurliEngine with the reference's method names."""

    def __init__(self, sr, perturbed=False, preamp_kind=0, power_amp_kind=0, tremolo_kind=0):
        self.L = lib_voice_perturbed() if perturbed == "voice" else (lib_perturbed() if perturbed else lib())
        self.h = C.c_void_p(self.L.owo_engine_new_kinds3(sr, int(preamp_kind), int(power_amp_kind), int(tremolo_kind)))

    def close(self):
        if self.h:
            self.L.owo_engine_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_sample_rate(self, sr): self.L.owo_engine_set_sample_rate(self.h, sr)
    def reset(self): self.L.owo_engine_reset(self.h)
    def warm_up(self): self.L.owo_engine_warm_up(self.h)
    def note_on(self, n, v): self.L.owo_engine_note_on(self.h, int(n), v)
    def note_off(self, n): self.L.owo_engine_note_off(self.h, int(n))
    def set_sustain(self, h): self.L.owo_engine_set_sustain(self.h, 1 if h else 0)
    def set_volume(self, v): self.L.owo_engine_set_volume(self.h, v)
    def set_tremolo_depth(self, v): self.L.owo_engine_set_tremolo_depth(self.h, v)
    def set_speaker_character(self, v): self.L.owo_engine_set_speaker_character(self.h, v)
    def set_mlp_enabled(self, on): self.L.owo_engine_set_mlp_enabled(self.h, 1 if on else 0)
    def set_noise_enabled(self, on): self.L.owo_engine_set_noise_enabled(self.h, 1 if on else 0)
    def set_noise_gain(self, g): self.L.owo_engine_set_noise_gain(self.h, g)
    def set_noise_seed(self, seed): self.L.owo_engine_set_noise_seed(self.h, int(seed))

    def render(self, n):
        out = np.zeros(int(n), dtype=np.float32)
        self.L.owo_engine_render(self.h, _p(out), int(n))
        return out

    def render_tap(self, n):
        out = np.zeros(int(n), dtype=np.float32)
        vs = np.zeros(int(n), dtype=np.float64)
        self.L.owo_engine_render_tap(self.h, _p(out), _p(vs), int(n))
        return out, vs

    def render_taps(self, n, osr=2):
        out = np.zeros(int(n), dtype=np.float32)
        vs = np.zeros(int(n), dtype=np.float64)
        pre = np.zeros(int(n) * osr, dtype=np.float64)
        r = np.zeros(int(n) * osr, dtype=np.float64)
        self.L.owo_engine_render_taps(self.h, _p(out), _p(vs), _p(pre), _p(r), int(n))
        return out, vs, pre, r

    def set_rail_sag(self, on): self.L.owo_engine_set_rail_sag(self.h, 1 if on else 0)
    def rail_sag_enabled(self): return bool(self.L.owo_engine_rail_sag_enabled(self.h))

    def power_amp_diag(self):
        """(clamp_count, nr_max_iter_count, peak_output_volts, guard_resets)"""
        a, b, g = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        pk = C.c_double()
        self.L.owo_engine_power_amp_diag(self.h, C.byref(a), C.byref(b), C.byref(pk), C.byref(g))
        return a.value, b.value, pk.value, g.value

    def render_pa_tap(self, n, osr=2):
        out = np.zeros(int(n), dtype=np.float32)
        pa = np.zeros(int(n) * osr, dtype=np.float64)
        self.L.owo_engine_render_pa_tap(self.h, _p(out), _p(pa), int(n))
        return out, pa

    def advance_tremolo(self, n): self.L.owo_engine_advance_tremolo(self.h, int(n))

    def poke_voice(self, slot, steal, field, value):
        """test poke: field 81 = pickup charge q, 0 = mode 0's sine state (the product's ow_test_engine_poke_voice)"""
        return self.L.owo_engine_poke_voice(self.h, int(slot), 1 if steal else 0, int(field), value)

    def poke_preamp_node(self, node, volts, shadow=False):
        """test poke: a node voltage of the legacy preamp's solver state (the product's ow_test_engine_poke_preamp_node)"""
        self.L.owo_engine_poke_preamp_node(self.h, 1 if shadow else 0, int(node), volts)

    def preamp_state(self, shadow=False):
        """the legacy preamp's solver state as stored (j_cin, cin_rhs_prev, v[8], i_nl[2], v_nl[2]) + bjt_ic(v_nl[0..1]) evaluated now"""
        out = np.zeros(16, dtype=np.float64)
        self.L.owo_engine_preamp_state(self.h, 1 if shadow else 0, out.ctypes.data_as(C.c_void_p))
        return out

    def preamp_ldr(self):
        """(r_ldr, g_ldr, g_ldr_prev) of the legacy preamp as they stand now"""
        out = np.zeros(3, dtype=np.float64)
        self.L.owo_engine_preamp_ldr(self.h, out.ctypes.data_as(C.c_void_p))
        return out

    def set_r_ulp(self, ulps):
        """test instrumentation: the tremolo's r_ldr moved by `ulps` doubles from now on (another libm's pow / exp / sin)"""
        self.L.owo_engine_set_r_ulp(self.h, int(ulps))

    def poke_power_amp_node(self, node, volts): self.L.owo_engine_poke_pa_node(self.h, int(node), volts)

    def stage_rows(self):
        """the output stage's state as the product's chain-state rows (float64 [STAGE_ROW_COUNT], CS_* indices; the rest 0)"""
        rows = np.zeros(STAGE_ROW_COUNT)
        self.L.owo_engine_stage_rows(self.h, _p(rows))
        return rows

    def set_stage_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.shape == (STAGE_ROW_COUNT,)
        self.L.owo_engine_set_stage_rows(self.h, _p(rows))

    def voice_record(self, slot, steal=False):
        """the voice of `slot` (its steal voice) with the slot's steal counters as the product's voice record (float64 [VOICE_RECORD_FIELDS],
        VF_* indices, u64 fields as their bits); None if the slot has no such voice"""
        rec = np.zeros(VOICE_RECORD_FIELDS)
        return rec if self.L.owo_engine_voice_record(self.h, int(slot), 1 if steal else 0, _p(rec)) == 0 else None

    def set_voice_record(self, slot, record, steal=False):
        record = np.ascontiguousarray(record, dtype=np.float64)
        assert record.shape == (VOICE_RECORD_FIELDS,)
        assert self.L.owo_engine_set_voice_record(self.h, int(slot), 1 if steal else 0, _p(record)) == 0, (slot, steal)

    def count_voices_in_state(self, st): return self.L.owo_engine_count_state(self.h, int(st))
    def active_voice_count(self): return self.L.owo_engine_active_voice_count(self.h)
    def steal_voice_count(self): return self.L.owo_engine_steal_voice_count(self.h)
    def nan_guard_fires(self): return self.L.owo_engine_nan_guard_fires(self.h)
    def slot_state(self, s): return self.L.owo_engine_slot_state(self.h, int(s))
    def slot_note(self, s): return self.L.owo_engine_slot_note(self.h, int(s))


DK_EXIT_CONVERGED, DK_EXIT_SINGULAR, DK_EXIT_SIX_UPDATES = 0, 1, 2

# ---- the output stage as a function of its state rows (owo_output_stage_block; tests/post_stage_cases.py)
STAGE_ROW_COUNT = 137            # CS_COUNT of openwurli_amd/csrc/ow_types.h: rows are indexed as the product's chain state is
STAGE_AMP_BEHAVIORAL, STAGE_AMP_IDENTITY = 0, 1
STAGE_MUTANTS = {"none": 0, "no_down_delay": 1, "thermal_after_gain": 2, "bypass_on_smoother": 3, "thermal_alpha_chain_rate": 4,
                 "guard_keeps_ts": 5, "guard_on_f64": 6, "newton_7": 7}
STAGE_PATTERNS = {"up": 1, "down": 2, "alternate": 3, "random": 4}
# How far a library result of the stage is moved, in doubles: the device function's documented bound plus glibc's.
#   exp    1 + 1   exp_any is the device library's f64 exp operation for operation (ow_chain_dev.h; within 1 ulp of the true value on the
#                  yardstick of tests/test_gpu_division.py); glibc's exp 1
#   tanh   2 + 2   tanh_fast <= 2 ulp (DESIGN section 2 deviation 14, test_gpu_division.py); glibc's tanh 2
#   pow    2 + 2   the device library's pow and glibc's, "a 2-ulp function on each side" (the isolation score's rows)
#   cos    2 + 2   "a sin / cos good to 2 ulp on both sides" (DESIGN, the note audits' bars)
#   sin    2 + 2
# Division and sqrt are IEEE on both sides (ow_div is tested bit-equal to the division) and are left alone.
STAGE_PERTURB_ULPS = (2, 4, 4, 4, 4)


def output_stage_block(host_rate, rows_in, tap, n, set_flags=0, spk_target=0.0, vol_target=0.0, amp_kind=STAGE_AMP_BEHAVIORAL, pattern=None,
                       seed=0, mutant="none", ulps=STAGE_PERTURB_ULPS):
    """One block of n host samples of the oracle's output stage from the state rows `rows_in` [STAGE_ROW_COUNT] and the stage's input
    `tap` [n * osr] (osr = 2 below 88.2 kHz): the preamp tap with the behavioural amp, the amp's output with STAGE_AMP_IDENTITY.
    set_flags bit 1 / 2: set_speaker_character(spk_target) / set_volume(vol_target) in front of the block.  pattern: None or a key of
    STAGE_PATTERNS -- every exp / tanh / pow / cos / sin result `ulps` doubles away, that way.  Returns (rows_out, out float32 [n], info)
    with info = dict(sweeps [n * osr], converged [n * osr], redesigned [n], fired [n], out64 [n]: the sample in front of the f32 cast)."""
    n = int(n)
    osr = 2 if host_rate < 88200.0 else 1
    rows_in = np.ascontiguousarray(rows_in, dtype=np.float64)
    tap = np.ascontiguousarray(tap, dtype=np.float64)
    assert rows_in.shape == (STAGE_ROW_COUNT,) and tap.shape == (n * osr,), (rows_in.shape, tap.shape, n, osr)
    rows_out = np.zeros(STAGE_ROW_COUNT); out = np.zeros(n, dtype=np.float32); info = np.zeros(2 * n * osr + 2 * n, dtype=np.int32)
    out64 = np.zeros(n)
    pert = None
    if pattern is not None:
        pert = np.array(list(ulps) + [STAGE_PATTERNS[pattern], int(seed)], dtype=np.int32)
    rc = lib().owo_output_stage_block(host_rate, osr, int(amp_kind), _p(rows_in), int(set_flags), spk_target,
                                      vol_target, _p(tap), n, _p(rows_out), _p(out), _p(info),
                                      None if pert is None else _p(pert), int(STAGE_MUTANTS[mutant]), _p(out64))
    assert rc == 0, rc
    m = n * osr
    return rows_out, out, dict(sweeps=info[:m], converged=info[m:2 * m], redesigned=info[2 * m:2 * m + n], fired=info[2 * m + n:], out64=out64)


VOICE_RECORD_FIELDS = 103        # VF_COUNT of openwurli_amd/csrc/ow_types.h


def voice_block(record, steal, length):
    """One block of `length` samples of one voice from its record (owo_voice_block: Voice::render, and for a steal voice the crossfade of
    engine.rs:483-490).  Returns (record_out, y float64 [length], dict(silent, transient, finite))."""
    record = np.ascontiguousarray(record, dtype=np.float64)
    assert record.shape == (VOICE_RECORD_FIELDS,)
    out = np.zeros(VOICE_RECORD_FIELDS); y = np.zeros(int(length)); info = np.zeros(3, dtype=np.int32)
    rc = lib().owo_voice_block(_p(record), 1 if steal else 0, int(length), _p(out), _p(y), _p(info))
    assert rc == 0, rc
    return out, y, dict(silent=bool(info[0]), transient=bool(info[1]), finite=bool(info[2]))


def dk_step_cases(rate, states, inputs, g_ldr, g_ldr_prev, perturbed=False):
    """ONE DkPreamp::dk_step (dk_preamp_legacy.rs:447-554) on each of n independent cases at chain rate `rate`: states [n][14] in the
    preamp_state order.  Returns (states_out [n][14], out [n], info [n][4] = Newton updates, exit (DK_EXIT_*), evaluations clamped at
    -1 V, at 0.85 V).  perturbed=True: the one-ulp-exp build."""
    L = lib_perturbed() if perturbed else lib()
    st = np.ascontiguousarray(states, dtype=np.float64)
    n = st.shape[0]
    assert st.shape == (n, 14)
    x = np.ascontiguousarray(inputs, dtype=np.float64); g = np.ascontiguousarray(g_ldr, dtype=np.float64)
    gp = np.ascontiguousarray(g_ldr_prev, dtype=np.float64)
    assert x.shape == (n,) and g.shape == (n,) and gp.shape == (n,)
    so = np.zeros((n, 14)); out = np.zeros(n); info = np.zeros((n, 4), dtype=np.int32)
    L.owo_dk_step_cases(rate, _p(st), _p(x), _p(g), _p(gp), n, _p(so), _p(out), _p(info))
    return so, out, info


TREM_INFO = ("trap_iter", "be_taken", "be_iter", "converged", "nan_reset", "pivot_sweeps", "singular_sweeps", "log_sweeps", "cap_sweeps", "thr_sweeps")


def trem_step_cases(rate, states, log_ulp=0):
    """ONE TremCircuit::process_sample(0.0) (gen_tremolo.rs:2353-3116) on each of n independent cases at chain rate `rate`: states [n][15] =
    v_prev[7], i_nl_prev[4], i_nl_prev_prev[4].  Returns (states_out [n][15], out [n], info [n][10] in the order of TREM_INFO: iteration
    index at which the trapezoidal solve converged (50 = exhausted), retry taken, its iteration index, the kept solve converged, NaN
    reset, sweeps with a row exchange / a singular Jacobian / a pnjlim logarithm / the 3.5 V cap / a port step above the limiter's 1e-4 V threshold).  log_ulp: pnjlim's logarithm moved by
    that many doubles (what another libm does to it)."""
    st = np.ascontiguousarray(states, dtype=np.float64)
    n = st.shape[0]
    assert st.shape == (n, 15)
    so = np.zeros((n, 15)); out = np.zeros(n); info = np.zeros((n, 10), dtype=np.int32)
    lib().owo_trem_step_cases(rate, _p(st), n, int(log_ulp), _p(so), _p(out), _p(info))
    return so, out, info


def trem_harvest(rate, n, every, state=None):
    """States [ceil(n / every)][15] in front of every `every`-th of n consecutive oscillator steps at chain rate `rate`, from `state` or (None)
    from the circuit as init_default(); set_sample_rate(rate) leaves it (DC_OP after the warm-up: where Tremolo::new's settle starts)."""
    m = (int(n) + int(every) - 1) // int(every)
    out = np.zeros((m, 15))
    st = None if state is None else _p(np.ascontiguousarray(state, dtype=np.float64))
    lib().owo_trem_harvest(rate, st, int(n), int(every), _p(out))
    return out


MEL_INFO = ("trap_sweeps", "be_taken", "be_sweeps", "nr_failed", "ringing", "forced", "lim_sweeps", "cap_sweeps", "singular_sweeps", "damped", "nan_reset",
            "rebuilt", "thr_sweeps", "be_failed")


def melange_step_cases(rate, states, inputs, r_ldr, log_ulp=0, r_ulp=0, rebuilt=False):
    """ONE MelState::process_sample (gen_preamp.rs:3399-3663) on each of n independent cases at chain rate `rate`: states [n][21] =
    v_prev[12], i_nl_prev[3], i_nl_prev_prev[3], input_prev, pot, be_cooldown; matrices in sync with the row's pot; then
    set_runtime_r_ldr(r_ldr[k]) and process_sample(inputs[k]).  Returns (states_out [n][21], out [n], info [n][14] in the order of
    MEL_INFO).  log_ulp: pnjlim's logarithm moved by that many doubles; r_ulp: the resistance every rebuild sees moved by that many.
    rebuilt: the state's resistance has moved before, so that at the codegen rate and the nominal pot it runs on rebuild_matrices'
    tables, not the baked ones (the reference never returns to those; the state row does not carry that history)."""
    st = np.ascontiguousarray(states, dtype=np.float64)
    n = st.shape[0]
    assert st.shape == (n, 21)
    x = np.ascontiguousarray(inputs, dtype=np.float64); r = np.ascontiguousarray(r_ldr, dtype=np.float64)
    assert x.shape == (n,) and r.shape == (n,)
    so = np.zeros((n, 21)); out = np.zeros(n); info = np.zeros((n, 14), dtype=np.int32)
    if rebuilt:
        assert log_ulp == 0 and r_ulp == 0
        lib().owo_melange_step_cases_rebuilt(rate, _p(st), _p(x), _p(r), n, _p(so), _p(out), _p(info))
        return so, out, info
    lib().owo_melange_step_cases(rate, _p(st), _p(x), _p(r), n, int(log_ulp), int(r_ulp), _p(so), _p(out), _p(info))
    return so, out, info


def melange_harvest(rate, n, every, x=None, r=None):
    """(states [ceil(n / every)][21] in front of every `every`-th of n consecutive steps of one melange solver state from init_state(rate),
    y [n] = every step's return value); per step set_runtime_r_ldr(r[k]) (None: untouched) and process_sample(x[k]) (None: 0)."""
    n = int(n); every = int(every)
    out = np.zeros(((n + every - 1) // every, 21)); y = np.zeros(n)
    xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    rr = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
    assert (xx is None or xx.shape == (n,)) and (rr is None or rr.shape == (n,))
    lib().owo_melange_harvest(rate, None if xx is None else _p(xx), None if rr is None else _p(rr), n, every, _p(out), _p(y))
    return out, y


def preamp_dc_nodes(rate, r_ldr):
    """The eight node voltages of the legacy preamp after set_ldr_resistance(r_ldr); reset() at chain rate `rate` (full_dc_solve at that R)."""
    v = np.zeros(8)
    lib().owo_preamp_step(rate, r_ldr, 0, r_ldr, None, None, 0, _p(v))
    return v


def render_note(midi, vel, dur, sr):
    n = int(dur * sr)
    out = np.zeros(max(n, 1))
    got = lib().owo_render_note(int(midi), vel, dur, sr, _p(out), out.size)
    return out[:got]


def batch_render_job(note, vel_u8, dur, sr, volume=1.0, speaker=0.0, r_ldr=1e6, mlp=False, poweramp=False, perturbed=False, preamp_kind=0):
    n = int(dur * sr)
    out = np.zeros(max(n, 1))
    got = (lib_perturbed() if perturbed else lib()).owo_batch_render_job_kind(
        int(note), int(vel_u8), dur, sr, volume, speaker, r_ldr,
        1 if mlp else 0, 1 if poweramp else 0, int(preamp_kind), _p(out), out.size)
    return out[:got]


def batch_render_job_ex(note, vel_u8, dur, sr, volume=0.60, speaker=1.0, r_ldr=1e6, tremolo_depth=0.0, displacement_scale=None, mlp=True,
                        poweramp=True, no_preamp=False, no_attack_noise=False, no_rail_sag=False, preamp_kind=0, power_amp_kind=0):
    """`preamp-bench render` with every sample-changing flag (tools/preamp-bench/src/main.rs:371-549); defaults = the command's."""
    L = lib()
    n = int(dur * sr)
    out = np.zeros(max(n, 1))
    opts = np.array([volume, speaker, r_ldr, tremolo_depth, float("nan") if displacement_scale is None else displacement_scale])
    flags = (1 if mlp else 0) | (2 if poweramp else 0) | (4 if no_preamp else 0) | (8 if no_attack_noise else 0) | (16 if no_rail_sag else 0)
    got = L.owo_batch_render_job_ex(int(note), int(vel_u8), dur, sr, _p(opts), flags, int(preamp_kind),
                                    int(power_amp_kind), _p(out), out.size)
    return out[:got]


def render_note_scaled(midi, vel, dur, sr, scale):
    L = lib()
    n = int(dur * sr)
    out = np.zeros(max(n, 1))
    got = L.owo_render_note_scaled(int(midi), vel, dur, sr, scale, _p(out), out.size)
    return out[:got]


def render_midi_ex(time_s, types, notes, values, volume=0.6, speaker=1.0, no_poweramp=False, tail=2.0, preamp_kind=0, power_amp_kind=0, no_rail_sag=False):
    L = lib()
    t = np.ascontiguousarray(time_s, dtype=np.float64); ty = np.ascontiguousarray(types, dtype=np.uint8)
    no = np.ascontiguousarray(notes, dtype=np.uint8); va = np.ascontiguousarray(values, dtype=np.uint8)
    cap = int((float(t.max()) + tail) * 44100.0) + 16 if t.size else 1
    out = np.zeros(cap)
    got = L.owo_render_midi_ex(_p(t), _p(ty), _p(no), _p(va), t.size, volume, speaker, 1 if no_poweramp else 0,
                               tail, int(preamp_kind), int(power_amp_kind), 1 if no_rail_sag else 0, _p(out), cap)
    return out[:got]


def normalize_scale(x):
    L = lib()
    x = np.ascontiguousarray(x, dtype=np.float64)
    return L.owo_batch_normalize_scale(_p(x), x.size)


class AliasAuditResult(C.Structure):
    """alias_audit.rs:68-93 (same field order as include/openwurli_hip.h ow_alias_audit_result)."""
    _fields_ = [("f0_hz", C.c_double), ("h1_dbfs", C.c_double), ("harmonic_db", C.c_double * 12), ("harmonic_dbc", C.c_double * 12),
                ("max_step_up_db", C.c_double), ("max_step_up_from_harmonic", C.c_uint32), ("pad", C.c_uint32), ("hf_band_dbc", C.c_double)]


def alias_audit_render_stimulus(note, velocity, preamp_kind=0, perturbed=False):
    out = np.zeros(int(44100.0 * 1.5))
    got = (lib_perturbed() if perturbed else lib()).owo_alias_audit_render_stimulus(int(note), int(velocity), int(preamp_kind), _p(out), out.size)
    assert got == out.size
    return out


def alias_audit_analyze(signal, sr, nominal_f0):
    assert lib().owo_alias_audit_result_size() == C.sizeof(AliasAuditResult)
    signal = np.ascontiguousarray(signal, dtype=np.float64)
    r = AliasAuditResult()
    rc = lib().owo_alias_audit_analyze(_p(signal), signal.size, sr, nominal_f0, C.byref(r))
    if rc != 0:
        raise ValueError("alias_audit signal too short")
    return r


def alias_audit_run(note, velocity, preamp_kind=0):
    r = AliasAuditResult()
    assert lib().owo_alias_audit_run(int(note), int(velocity), int(preamp_kind), C.byref(r)) == 0
    return r


# Absolute indeterminacy of the REFERENCE ALGORITHM itself at the f32 output: the legacy preamp's Newton loop
# stops at |f| < 1e-9 V (dk_preamp_legacy.rs:500), so a libm whose exp() differs in the last bit moves the preamp
# node by ~5e-10 V and the output by ~5e-10 (tests/test_oracle_sensitivity.py measures it on the CPU oracle alone).
ABS_FLOOR_OUTPUT = 2e-9
ABS_FLOOR_PREAMP = 2e-9
# batch jobs (`preamp-bench render`): output = preamp x volume^2 x 7.5 with a static LDR, so the same indeterminacy
# shows up ~10x larger: 8.9e-9 on short bass / mid jobs, 2.6e-8 on the 5 s render of note 96 at velocity 50 -- the job on which the GPU's own
# worst batch error (2.5e-8) falls (test_oracle_sensitivity.py::test_batch_job_floor)
ABS_FLOOR_BATCH = 3e-8
# alias-audit stimulus (tremolo depth 0, i.e. the LDR dark and the preamp at its lowest loop gain): the same one-ulp experiment
# moves quiet samples by up to 2.5e-9 (tests/test_oracle_sensitivity.py::test_alias_audit_stimulus_floor)
ABS_FLOOR_AUDIT = 4e-9
# dense play (up to 64 voices, volume 0.65, tremolo depth up to 1): the Newton stop is an absolute threshold at the preamp node and what
# reaches the output scales with volume^2 and the tremolo's gain swing; the one-ulp experiment on such a script moves quiet samples by
# up to 3.1e-9 (tests/test_oracle_sensitivity.py::test_dense_play_floor, tools/soak_parity.py)
ABS_FLOOR_DENSE = 5e-9
# long dense soaks (tools/soak_parity.py: 120 s x 6 engines per seed, tests/test_gpu_soak.py): over minutes of random play the reference
# algorithm passes through states -- an engine at tremolo depth 0 under a dense chord, mostly -- in which the SAME one-ulp experiment moves a
# quiet sample by up to 3.4e-8 (seed 5, block 691, engine 0; seeds 3 and 4: 9e-9 and 1.4e-8), at the very blocks and engines where the GPU's
# own worst samples sit (1.5e-8 / 1.0e-8 / 9.5e-9: profiles/r06_soak.md has the eight seeds side by side).  The dense-play floor above
# stays what the suites' short scenarios use; a soak is held to 2e-8 = 0.6 x the reference's own movement on the worst seed.
ABS_FLOOR_SOAK = 2e-8
# ... and with the `legacy-tremolo` LFO in place of the Twin-T (tremolo_kind 1; first soaked in round 6): the same script passes through the
# same state (seed 5, block 691, engine 0), where the reference is four times touchier to its tremolo's R than to its preamp's exp(): the
# oracle against itself with every r_ldr moved to the NEIGHBOURING double (what another libm's sin / pow / exp behind the CdS law does)
# moves that sample by 1.06e-7 (4.3e-8 with the Twin-T; tests/test_oracle_sensitivity.py::test_soak_floor_legacy_tremolo_governing_measurement).
# The GPU, whose device library is such a libm, sits at 1.2e-7 there and below 1e-8 everywhere else (profiles/r06_soak.md).
ABS_FLOOR_SOAK_LFO = 1.5e-7
# melange 12-node solver.  The reference (and the oracle) re-invert the 12x12 MNA matrix by LU for every sample whose R_ldr
# moved; the GPU applies the mathematically identical rank-one (Sherman-Morrison) update of the inverse at the nominal pot.
# While R_ldr is steady the two agree to 4-7e-10 at the preamp node.  While R_ldr moves fast (depth-knob ramp, tremolo trough)
# the audible signal contains the DIFFERENCE of successive inverses, and the LU result carries rounding noise of
# eps * cond(A) that the rank-one form does not have: measured deviation up to 1.8e-7 V at the preamp node (2.5e-6 of peak),
# i.e. inside the 1e-5 bar relative to peak but not sample-by-sample relative to small samples.  The melange tests
# therefore use an absolute floor of 5e-7 V (preamp) / 1.5e-6 (output) AND assert max error < 1e-5 of peak.
ABS_FLOOR_MELANGE_PREAMP = 5e-7
ABS_FLOOR_MELANGE_OUTPUT = 1.5e-6
# The default melange kernel (ow_melange_lit.h) re-factors the system per sample, operation for operation like the reference: what is left
# is the reference's own indeterminacy -- the LU's rounding noise is a chaotic function of R_ldr's last bits, and R_ldr comes out of
# exp / powf, where the device library and glibc differ in the last place (tests/test_oracle_sensitivity.py measures 1.4e-8 V at the
# preamp node for R off by one ulp).  3.4e-8 = 2.5 x that at the node (5e-8 until round 6); the same at the f32 output (chain gain ~1 at volume 0.5, plus f32 rounding).
ABS_FLOOR_MELANGE_LIT_PREAMP = 3.4e-8
ABS_FLOOR_MELANGE_LIT_OUTPUT = 3.4e-8

# single steps of the Twin-T oscillator (tests/trem_step_cases.py, tests/test_gpu_trem_step.py): state rows are held to 1e-5 relative plus
# these.  The only operation of the step that is not IEEE arithmetic is pnjlim's logarithm; with its result moved to the neighbouring
# double either way, the oracle's step -- on the finite cases that keep their exits (retry taken or not, converged or exhausted, reset) --
# leaves the relative term alone on no volt row at all and on junction-current rows by at most 2.64e-11 A (a backward-Euler retry that
# converges one sweep later: 96 kHz, a 6e-7 A base current; tests/test_oracle_sensitivity.py::test_trem_step_floors).  So volts get no
# floor, and amps get 2.5 x that.
ABS_FLOOR_TREM_STEP_V = 0.0
ABS_FLOOR_TREM_STEP_I = 6.5e-11

# single steps of the melange preamp solver (tests/mel_step_cases.py, tests/test_gpu_mel_step.py): the twelve v rows and the six junction
# currents are held to 1e-5 relative plus these.  Measured as the Twin-T's: the oracle's step against itself with pnjlim's logarithm one
# double away and with the resistance every rebuild sees one double away, either way, on the finite cases that keep their fallback, reset
# and cooldown decisions (all of them do) -- no row of any of the 40 872 finite cases moves by more than 1.9e-7 of its value (the worst:
# a limited sweep count that changes by one at 88.2 kHz), so no row's tolerance is ever governed by a floor and 2.5 x 0 is 0
# (tests/test_oracle_sensitivity.py::test_melange_step_floors).  The resistance knob moves nothing at all: 1/R enters
# g_eff[6][6] = G[6][6] + (1/R - 1/R_nom), where one double of R (<= 1.1e-19 S at 1 kOhm) is below half an ulp of the sum.
ABS_FLOOR_MELANGE_STEP_V = 0.0
ABS_FLOOR_MELANGE_STEP_I = 0.0

# Every absolute floor above with the one-ulp measurement that governs it (DESIGN.md section 2 carries the numbers).  The rule of the
# table, asserted by tests/test_oracle_sensitivity.py on the CPU: floor <= 2.5 x (what the reference algorithm itself moves by, on the
# samples where the floor -- not the relative bar -- is the tolerance, when exp() is off by one ulp on the scenario family the floor is
# used for).  No floor changes without its row.
FLOORS = {
    "ABS_FLOOR_OUTPUT": ABS_FLOOR_OUTPUT, "ABS_FLOOR_PREAMP": ABS_FLOOR_PREAMP, "ABS_FLOOR_BATCH": ABS_FLOOR_BATCH,
    "ABS_FLOOR_AUDIT": ABS_FLOOR_AUDIT, "ABS_FLOOR_DENSE": ABS_FLOOR_DENSE, "ABS_FLOOR_SOAK": ABS_FLOOR_SOAK,
    "ABS_FLOOR_SOAK_LFO": ABS_FLOOR_SOAK_LFO,
    "ABS_FLOOR_MELANGE_LIT_PREAMP": ABS_FLOOR_MELANGE_LIT_PREAMP, "ABS_FLOOR_MELANGE_LIT_OUTPUT": ABS_FLOOR_MELANGE_LIT_OUTPUT,
    "ABS_FLOOR_TREM_STEP_V": ABS_FLOOR_TREM_STEP_V, "ABS_FLOOR_TREM_STEP_I": ABS_FLOOR_TREM_STEP_I,
    "ABS_FLOOR_MELANGE_STEP_V": ABS_FLOOR_MELANGE_STEP_V, "ABS_FLOOR_MELANGE_STEP_I": ABS_FLOOR_MELANGE_STEP_I,
}
FLOOR_RULE = 2.5


def floor_governed_delta(x, y, floor, rel=1e-5, floor_frac=1e-3):
    """max |x - y| over the samples of x whose tolerance in parity_report is the absolute floor (not the relative bar): what a floor has to
    cover.  NaN when the floor governs no sample."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    peak = float(np.max(np.abs(x))) if x.size else 0.0
    m = rel * np.maximum(np.abs(x), floor_frac * peak) < floor
    return float(np.max(np.abs(x - y)[m])) if m.any() else float("nan")


def parity_report(gpu, cpu, rel=1e-5, floor_frac=1e-3, abs_floor=0.0):
    """SURVEY.md 8d parity metric: |gpu-cpu| <= max(rel * max(|cpu|, floor_frac * peak|cpu|), abs_floor)."""
    gpu = np.asarray(gpu, dtype=np.float64)
    cpu = np.asarray(cpu, dtype=np.float64)
    peak = float(np.max(np.abs(cpu))) if cpu.size else 0.0
    tol = np.maximum(rel * np.maximum(np.abs(cpu), floor_frac * peak), abs_floor)
    err = np.abs(gpu - cpu)
    bad = np.nonzero(err > tol)[0]
    wi = int(np.argmax(err / np.maximum(tol, 1e-300))) if err.size else -1
    # which of the three terms of the bar was the tolerance of the worst sample: 1e-5 * |cpu| / 1e-5 * 1e-3 * peak / the absolute floor
    branch = "" if wi < 0 else ("floor" if tol[wi] == abs_floor and abs_floor > 0.0 else ("relative" if abs(cpu[wi]) >= floor_frac * peak else "peak_fraction"))
    return {
        "worst_index": wi, "worst_branch": branch,
        "peak": peak,
        "max_abs_err": float(err.max()) if err.size else 0.0,
        "max_err_rel_peak": float(err.max() / peak) if peak > 0 else 0.0,
        "worst_ratio": float(np.max(err / np.maximum(tol, 1e-300))) if err.size else 0.0,
        "n_bad": int(bad.size),
        "first_bad": int(bad[0]) if bad.size else -1,
    }
