"""The output stage one block at a time, in f64: corpus and comparison behind tests/test_oracle_post_stage_cases.py (CPU) and
tests/test_gpu_post_stage.py (the eleven chain kernels that carry a copy of the stage).

The stage -- behavioural power amp, half-band decimator, speaker-character smoother, Hammerstein speaker, volume smoother, f32 cast and
NaN guard -- keeps all it carries from block to block in chain-state rows, so "rows before + the tap it reads + setter calls -> rows
after + f32 block" is a pure function.  The oracle evaluates it (oracle_binding.output_stage_block); a kernel has to reproduce it from
the same rows (written through ow_test_engine_write_chain_rows) and the tap it actually read.

A RECIPE is one engine's part in a block: (the state the block starts from, setter calls in front of it, what drives the tap).  The
start rows are built on the CPU from the oracle alone, so every form and both sides start from the same bits; the drive only has to put
the tap where the stage's branches are -- the reference is computed from the tap actually read.

Drives.  A kick of the legacy preamp's OUT node (main state) leaves the tap at -kick, +kick, -kick ... for the rest of the block (the
node has no capacitor to ground in the trapezoidal step; it decays by 1e-11 per sample), so a kick IS the tap level, on both signs.  The
oracle's `info` places the power amp's sweep counts (48 kHz, 200 000-point grids on each sign and 200 000 log-uniform taps 1e-9 .. 8 V):
one sweep up to 1.8e-6 V and wherever the estimate is already inside the tolerance, two to four from 1.3e-5 V up, and FIVE TO EIGHT ONLY
for |tap| in 1.0512 .. 1.2864 V, where the closed-loop estimate 68.9 x tap / 4 meets the +-22 V rail: six in 1.1906 .. 1.2833, seven in
1.2499 .. 1.2802, eight in 1.27472 .. 1.27707 V.  Every finite tap converged within the eight sweeps.  Hence KICKS.
"""
import numpy as np

import oracle_binding as ob

# chain-state rows of the stage (OW_TEST_CS_* of include/openwurli_hip_test.h, guarded there by static_asserts)
SM_SPK, SM_VOL, OS_DA, OS_DB, OS_DD, HPF, LPF, CHAR, A2, A3, TC, TS, FLAGS = 22, 26, 67, 70, 73, 74, 81, 88, 89, 90, 91, 92, 93
WRITE_SPANS = ((SM_SPK, SM_VOL + 4), (OS_DA, TS + 1))       # what a case writes: not the preamp's rows between them, not the flags word
READ_SPAN = (SM_SPK, FLAGS + 1)

RATES = (44100.0, 48000.0, 96000.0)
LENGTHS = (1, 2, 37, 64, 65, 129)        # the read-ahead's min(base + n + 1, L - 1) and the 64-sample tile edge
POOLS = (1, 33, 65, 130)                 # partly filled wavefronts in the 32-, 64- and 8-engines-per-wavefront layouts
NOTES = list(range(33, 97))


def osr_of(rate):
    return 2 if rate < 88200.0 else 1


def ramp_of(rate):
    return max(int(rate * 0.005), 1)


def u64(x):
    return float(np.array([int(x)], dtype=np.uint64).view(np.float64)[0])


_BASE = {}


def base_rows(rate):
    """The stage rows of a fresh oracle engine (character 0, volume 0.5, all states 0)."""
    if rate not in _BASE:
        e = ob.OracleEngine(rate)
        _BASE[rate] = e.stage_rows()
        e.close()
    return _BASE[rate].copy()


_HELD = {}


def held_rows(rate, character, volume):
    """Rows of a stage at rest with the speaker held at `character`: the coefficient rows are the oracle's own design at that value, bit for
    bit (one silent sample from a far-away held character redesigns there), so a block without a redesign filters with the same
    coefficients on both sides."""
    key = (rate, character, volume)
    if key not in _HELD:
        rows = base_rows(rate)
        rows[SM_SPK:SM_SPK + 4] = (character, character, 0.0, u64(0))
        rows[SM_VOL:SM_VOL + 4] = (volume, volume, 0.0, u64(0))
        rows[CHAR] = 1.0 if character < 0.5 else 0.0
        out, _, info = ob.output_stage_block(rate, rows, np.zeros(osr_of(rate)), 1)
        assert info["redesigned"][0] == 1 and out[CHAR] == min(max(character, 0.0), 1.0)
        _HELD[key] = out
    return _HELD[key].copy()


def ramp_fields(current, target, remaining):
    """Smoother fields in the middle of a ramp towards `target`: `remaining` samples to go."""
    step = (target - current) / remaining if remaining else 0.0
    return (current, target, step, u64(remaining))


# ---- recipes ------------------------------------------------------------------------------------------------------------------------------
# drive: ("silent",) | ("chord", n_keys, velocity) struck at set-up | ("strike", n_keys, velocity) struck right before every block |
#        ("kick", volts) | ("nan_out",): the OUT node written with a NaN (the preamp's own reset answers it: the tap reads 0 there)
# c0 / v0: the targets the engine's setters were last called with (the host keeps its own copy of a smoother's target)
# rows: f(rows, rate) -> None, edits the held rows in place;  set: (speaker target | None, volume target | None) in front of the block
KICKS_MANY = (1.10, 1.17, 1.22, 1.245, 1.262, 1.268, 1.2755, 1.2760, 1.2765)      # inside the many-sweep band (module docstring)
KICKS_OTHER = (2.0e-6, 1.5e-5, 4.0e-5, 1.0e-3, 0.3, 1.0, 1.2868, 1.30, 2.5, 9.0)   # below it, between, beyond the rail


def _r(name, family, drive, c0=0.0, v0=0.5, rows=None, set=(None, None), fires=None):
    return dict(name=name, family=family, drive=drive, c0=c0, v0=v0, rows=rows, set=set, fires=fires)


def _states(vals):
    def f(rows, rate):
        rows[HPF + 5], rows[HPF + 6], rows[LPF + 5], rows[LPF + 6] = vals[0:4]
        rows[OS_DA:OS_DA + 3] = vals[4:7]; rows[OS_DB:OS_DB + 3] = vals[7:10]; rows[OS_DD] = vals[10]
    return f


def _set(idx, value):
    def f(rows, rate):
        rows[idx] = value
    return f


def _spk_ramp(current, target, remaining=None, per_sample=None):
    def f(rows, rate):
        rem = ramp_of(rate) if remaining is None else remaining
        cur = target - per_sample * rem if per_sample is not None else current
        rows[SM_SPK:SM_SPK + 4] = ramp_fields(cur, target, rem)
    return f


def _vol_ramp(current, target, remaining):
    def f(rows, rate):
        rows[SM_VOL:SM_VOL + 4] = ramp_fields(current, target, remaining)
    return f


def _both(*fs):
    def f(rows, rate):
        for g in fs:
            g(rows, rate)
    return f


_BELOW, _ABOVE = float(np.nextafter(1e-3, 0.0)), float(np.nextafter(1e-3, 1.0))
RECIPES = [
    # levels
    _r("silent", "levels", ("silent",), rows=_set(TS, 0.02), c0=1.0),
    _r("one_pp_key", "levels", ("chord", 1, 0.05)),
    _r("four_mf", "levels", ("chord", 4, 0.5), c0=0.5),
    _r("sixteen_ff", "levels", ("chord", 16, 1.0), c0=1.0),
    _r("sixty_four_ff", "levels", ("chord", 64, 1.0), c0=1.0, v0=1.0),
    _r("struck_three_ff", "levels", ("strike", 3, 1.0)),
    _r("struck_one_pp", "levels", ("strike", 1, 0.05), c0=1.0),
] + [
    _r(f"kick_{k:g}", "levels", ("kick", k), c0=(0.0, 1.0, 0.5)[i % 3]) for i, k in enumerate(KICKS_MANY + KICKS_OTHER)
] + [
    # speaker character
    _r("held_below_bypass", "character", ("chord", 16, 1.0), c0=_BELOW),
    _r("held_above_bypass", "character", ("chord", 16, 1.0), c0=_ABOVE),
    _r("ramp_across_bypass", "character", ("kick", 0.3), c0=0.01, rows=_both(_spk_ramp(0.0, 0.01), _set(CHAR, 0.0))),
    _r("ramp_redesign_every_few", "character", ("chord", 12, 0.8), c0=0.5, rows=_spk_ramp(None, 0.5, per_sample=0.0007)),
    _r("ramp_ends_at_1", "character", ("chord", 8, 0.9), c0=0.6, rows=_spk_ramp(0.6 - 1 * 0.0011, 0.6, 1)),
    _r("ramp_ends_at_63", "character", ("chord", 8, 0.9), c0=0.6, rows=_spk_ramp(0.6 - 63 * 0.0011, 0.6, 63)),
    _r("ramp_ends_at_64", "character", ("kick", 0.4), c0=0.6, rows=_spk_ramp(0.6 - 64 * 0.0011, 0.6, 64)),
    _r("retarget_held", "character", ("chord", 24, 1.0), c0=0.2, set=(0.8, None)),
    _r("retarget_mid_ramp", "character", ("kick", 0.2), c0=0.9, rows=_spk_ramp(0.5, 0.9, 100), set=(0.0, 0.9)),
    # state
    _r("thermal_large", "state", ("chord", 32, 1.0), c0=1.0, rows=_set(TS, 0.9)),
    _r("states_mixed", "state", ("chord", 6, 0.7), c0=0.5,
       rows=_states((0.7, -0.31, -1.9, 1.2, 1e-3, -0.8, 0.05, -2.0, 0.6, -4e-4, 0.9))),
    _r("states_mixed_kick", "state", ("kick", 1.255), c0=1.0,
       rows=_both(_states((-2e-3, 5e-4, 0.3, -0.29, -1.0, 1.0, -1.0, 1e-6, -1e-5, 1e-4, -0.5)), _set(TS, 0.3))),
    _r("states_subnormal_silent", "state", ("silent",), c0=0.5,
       rows=_both(_states((5e-324, -1e-310, 3e-315, -2e-308, 1e-310, -5e-324, 2e-312, -1e-309, 1.5e-308, 1e-320, -1e-311)), _set(TS, 1e-310))),
    _r("states_subnormal_pp", "state", ("chord", 1, 0.05), c0=1.0,
       rows=_both(_states((1e-310, 1e-310, -1e-310, 5e-324, -5e-324, 1e-315, 1e-320, 0.0, -0.0, 1e-309, -1e-309)), _set(TS, 5e-324))),
    _r("volume_ramp_through_zero", "state", ("chord", 16, 1.0), c0=0.5, v0=-0.1, rows=_vol_ramp(0.1, -0.1, 40)),
    # guard
    _r("guard_lpf_1e39", "guard", ("silent",), rows=_set(LPF + 5, 1e39), fires=True),
    _r("guard_lpf_1e37", "guard", ("silent",), rows=_set(LPF + 5, 1e37), fires=False),
    _r("guard_hpf_1e41_loud", "guard", ("chord", 16, 1.0), c0=1.0, rows=_both(_set(HPF + 5, -1e41), _set(TS, 0.4)), fires=True),
    _r("guard_nan_da0", "guard", ("chord", 4, 0.5), c0=0.5, rows=_set(OS_DA, float("nan")), fires="oversampled"),     # no decimator at 96 kHz: its rows are carried along
    _r("guard_nan_out_node", "guard", ("nan_out",), c0=0.5),
]
R = len(RECIPES)
NAMES = [r["name"] for r in RECIPES]


def chord_notes(n_keys, salt):
    return sorted({NOTES[(5 * salt + 7 * i) % 64] for i in range(n_keys)})


def start_rows(recipe, rate):
    rows = held_rows(rate, recipe["c0"], recipe["v0"])
    if recipe["rows"] is not None:
        recipe["rows"](rows, rate)
    return rows


def expect_fired(recipe, rate):
    """None: not a guard case; else whether the guard has to fire in the block."""
    f = recipe["fires"]
    return (osr_of(rate) == 2) if f == "oversampled" else f


def set_args(recipe):
    """(set_flags, speaker target, volume target) of the block under test, as the kernels' arguments carry them."""
    s, v = recipe["set"]
    return ((2 if s is not None else 0) | (4 if v is not None else 0), 0.0 if s is None else s, 0.0 if v is None else v)


def recipe_of(k, n_engines):
    """Engine k of a pool of n_engines plays RECIPES[...]: all of them from 65 engines up, the first 33, and for the pool of one the
    eight-sweep kick."""
    return (NAMES.index("kick_1.276") if n_engines == 1 else k) % R


# Both OracleEngine and the product's engine handle offer note_on / set_* / poke_preamp_node; reading the OUT nodes differs.
def engine_setup(e, recipe, salt):
    """Once per engine: the setters' targets, the chord."""
    e.set_volume(recipe["v0"]); e.set_speaker_character(recipe["c0"]); e.set_tremolo_depth(0.5)
    if recipe["drive"][0] == "chord":
        for note in chord_notes(recipe["drive"][1], salt):
            e.note_on(note, recipe["drive"][2])


def engine_before_block(e, recipe, salt, out_nodes):
    """In front of every block under test.  out_nodes() -> (main, shadow) voltage of the preamp's OUT node."""
    d = recipe["drive"]
    if d[0] == "strike":
        for note in chord_notes(d[1], salt):
            e.note_on(note, d[2])
    elif d[0] == "kick":
        e.poke_preamp_node(6, out_nodes()[1] + d[1])         # main = shadow + kick: the tap is their difference
    elif d[0] == "nan_out":
        e.poke_preamp_node(6, float("nan"))
    # the host's copy of a target follows the last accepted call, the rows were written with c0 / v0: call both in that order
    s, v = recipe["set"]
    if s is not None:
        e.set_speaker_character(recipe["c0"]); e.set_speaker_character(s)
    if v is not None:
        e.set_volume(recipe["v0"]); e.set_volume(v)


def reference(rate, recipe, rows_in, tap, n, amp_kind=ob.STAGE_AMP_BEHAVIORAL, **kw):
    flags, s, v = set_args(recipe)
    return ob.output_stage_block(rate, rows_in, tap, n, flags, s, v, amp_kind, **kw)


# ---- the CPU corpus: the same recipes on oracle engines ---------------------------------------------------------------------------------
_CORPUS = {}


def cpu_corpus(rate):
    """[(recipe, n, rows_in, tap)] for every recipe and block length at this rate: one oracle engine per recipe, warmed, then the block
    lengths in turn.  Only its preamp tap is used -- the stage runs as the function, from the recipe's start rows."""
    if rate in _CORPUS:
        return _CORPUS[rate]
    cases = []
    for k, recipe in enumerate(RECIPES):
        e = ob.OracleEngine(rate)
        engine_setup(e, recipe, k)
        e.render(768)
        rows = start_rows(recipe, rate)
        for n in LENGTHS:
            engine_before_block(e, recipe, k, lambda: (e.preamp_state(False)[8], e.preamp_state(True)[8]))
            tap = e.render_taps(n, osr_of(rate))[2]
            cases.append((recipe, n, rows, tap))
        e.close()
    _CORPUS[rate] = cases
    return cases


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------
# Rows that are IEEE arithmetic on both sides are bit-equal: both smoothers' four fields, character, a2, a3, thermal coefficient, the flags
# bit, the coefficient rows of a block without a redesign (copies), and with them the redesign and guard decisions.  The rest by class,
# |got - ref| <= BARS[class] x the class's scale in the case: the largest magnitude among the class's rows before and after the block, for
# the f32 block of the oracle's f64 block, for a coefficient its own magnitude.  A block in which the speaker was redesigned has classes
# of its own for what lies behind the biquads: a cos 4 doubles away moves 1 - cos(w0) of the 20 .. 30 Hz high-pass by 6e-11 of itself, the
# filter's corner with it, and so its state and output; a block that keeps its coefficients is not given that room.
# Where a class's scale is itself subnormal (< SUBNORMAL_SCALE) a relative measure means nothing: there the bar is a count of steps of the
# smallest subnormal -- the only absolute term, because the measurement shows one only there.
EXACT_ROWS = tuple(range(SM_SPK, SM_VOL + 4)) + (CHAR, A2, A3, TC)
COEF_ROWS = tuple(range(HPF, HPF + 5)) + tuple(range(LPF, LPF + 5))
CLASS_ROWS = {
    "half_band": tuple(range(OS_DA, OS_DD + 1)),
    "biquad_state": (HPF + 5, HPF + 6, LPF + 5, LPF + 6),
    "thermal": (TS,),
    "coefficients": COEF_ROWS,
}
CLASSES = ("half_band", "biquad_state", "thermal", "coefficients", "f32_block")
BAR_KEYS = ("half_band", "thermal", "biquad_state", "biquad_state_redesigned", "coefficients", "f32_block", "f32_block_redesigned", "subnormal_steps")
SUBNORMAL_SCALE = 1e-290
FLOOR_RULE = ob.FLOOR_RULE          # bar <= 2.5 x its measurement
SUBNORMAL_STEP = 4.9406564584124654e-324
# MEASURED[key]: the largest movement of the perturbed oracle from the plain one over the CPU corpus (every recipe x block length x rate) and
# the perturbation patterns (up, down, alternating, two random seeds); BARS = at most 2.5 x that, zero where it is zero.
# Both are asserted by tests/test_oracle_post_stage_cases.py::test_bars_are_measured.
MEASURED = {
    "half_band": 1.00e-15,                 # 44.1 kHz, a 2.5 V kick, 37 samples, random signs
    "thermal": 3.39e-15,                   # 44.1 kHz, a 1.3 V kick, 129 samples, all down
    "biquad_state": 7.19e-12,              # 44.1 kHz, a 1.262 V kick (six and seven sweeps), 129 samples: the 30 Hz high-pass integrates the amp's 5e-16
    "biquad_state_redesigned": 4.72e-11,   # 48 kHz, retarget in the middle of a ramp, 129 samples, alternating
    "coefficients": 2.42e-14,              # same recipe, 37 samples: (1 - cos w0) of the high-pass
    "f32_block": 1.12e-12,                 # 96 kHz, a 1.17 V kick, 129 samples
    "f32_block_redesigned": 2.46e-12,      # 96 kHz, a character ramp ending at sample 63
    "subnormal_steps": 1871.0,             # 44.1 kHz, silent engine with subnormal states at character 0.5: tanh of a subnormal, 4 steps, integrated
}
BARS = {k: 2.5 * m for k, m in MEASURED.items()}
# share of f32 samples at which the perturbed oracle rounds to the neighbouring float (largest over the patterns, same corpus)
MEASURED_NEIGHBOUR_SHARE = 2.43e-5     # one sample of the corpus' 41 124


def _same(a, b):
    """bit-equal, or both NaN"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def bar_key(cls, redesigned):
    return cls + "_redesigned" if redesigned and cls in ("biquad_state", "f32_block") else cls


def class_scale(cls, rows_in, ref_rows, ref_info):
    if cls == "f32_block":
        v = ref_info["out64"]
    else:
        idx = list(CLASS_ROWS[cls])
        v = np.concatenate([rows_in[idx], ref_rows[idx]])
    v = np.abs(v[np.isfinite(v)])
    return float(v.max()) if v.size else 0.0


def class_errors(rows_in, ref, got_rows, got_f64=None):
    """{bar key: error} of one case: per class the largest |got - ref| over the finite reference values, relative to the class's scale
    (inf where they differ at a zero scale), or under `subnormal_steps` in steps of the smallest subnormal where that scale is subnormal.
    The f32 block is measured on the f64 sample in front of the cast when got_f64 is given (oracle against oracle)."""
    ref_rows, ref_f32, info = ref
    redesigned = bool(info["redesigned"].any())
    err = {"subnormal_steps": 0.0}
    for cls in CLASSES:
        if cls == "f32_block":
            if got_f64 is None:
                continue
            a, b = np.asarray(got_f64), info["out64"]
        else:
            idx = list(CLASS_ROWS[cls])
            a, b = got_rows[idx], ref_rows[idx]
        ok = np.isfinite(b)
        d = np.where(_same(a, b), 0.0, np.abs(a - b))
        d = np.where(np.isnan(d), np.inf, d)[ok]               # a NaN against a finite reference
        if cls == "coefficients":
            s = np.abs(b[ok])
        else:
            scale = class_scale(cls, rows_in, ref_rows, info)
            if 0.0 < scale < SUBNORMAL_SCALE:
                err["subnormal_steps"] = max(err["subnormal_steps"], float(d.max() / SUBNORMAL_STEP) if d.size else 0.0)
                err[bar_key(cls, redesigned)] = 0.0
                continue
            s = np.full(d.shape, scale)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(d == 0.0, 0.0, d / s)
        err[bar_key(cls, redesigned)] = float(q.max()) if q.size else 0.0
    return err


def neighbour_samples(ref_f32, got_f32):
    """indices where got is the float next to the reference's (not equal)"""
    a = ref_f32.view(np.int32).astype(np.int64); b = got_f32.view(np.int32).astype(np.int64)
    fin = np.isfinite(ref_f32) & np.isfinite(got_f32)
    return np.nonzero(fin & (np.abs(a - b) == 1) & ((a < 0) == (b < 0)))[0]


def compare(rows_in, ref, got_rows, got_f32, bars=None, where=""):
    """-> (failures [str], {bar key: error / bar}, n_neighbour).  `ref` = reference(...)'s result, got_* what a kernel (or a mutant of the
    oracle) left.  n_neighbour: samples accepted as the neighbouring float (the oracle's f64 value within the bar of the midpoint)."""
    bars = BARS if bars is None else bars
    ref_rows, ref_f32, info = ref
    fails = []
    ctx = lambda: (f"[{where}; sweep counts 1..8 of the block {np.bincount(info['sweeps'], minlength=9)[1:].tolist()}, redesigns "
                   f"{int(info['redesigned'].sum())}, guard fired {int(info['fired'].sum())}]")
    for r in EXACT_ROWS:
        if not _same(got_rows[r], ref_rows[r]):
            fails.append(f"row {r}: {got_rows[r]!r} != oracle {ref_rows[r]!r} (bit-equal row) {ctx()}")
    got_flag = int(np.array([got_rows[FLAGS]]).view(np.uint64)[0]) & 1
    ref_flag = int(np.array([ref_rows[FLAGS]]).view(np.uint64)[0]) & 1
    if got_flag != ref_flag:
        fails.append(f"row {FLAGS} bit 0: {got_flag} != oracle {ref_flag} {ctx()}")
    redesigned = bool(info["redesigned"].any())
    if not redesigned:
        for r in COEF_ROWS:
            if not _same(got_rows[r], rows_in[r]):
                fails.append(f"coefficient row {r} changed without a redesign: {got_rows[r]!r} from {rows_in[r]!r} {ctx()}")
    err = class_errors(rows_in, ref, got_rows)
    ratios = {}

    def ratio(key):
        e = err.get(key, 0.0)
        return e / bars[key] if bars[key] > 0.0 else (0.0 if e == 0.0 else float("inf"))

    for cls in ("half_band", "biquad_state", "thermal", "coefficients"):
        if cls == "coefficients" and not redesigned:
            continue
        key = bar_key(cls, redesigned)
        ratios[key] = ratio(key)
        idx = list(CLASS_ROWS[cls])
        nonfinite_ok = all(bool(_same(got_rows[r], ref_rows[r])) for r in idx if not np.isfinite(ref_rows[r]))
        if ratios[key] > 1.0 or not nonfinite_ok:
            w = idx[int(np.argmax(np.where(_same(got_rows[idx], ref_rows[idx]), 0.0, np.nan_to_num(np.abs(got_rows[idx] - ref_rows[idx]), nan=np.inf))))]
            fails.append(f"{cls} row {w}: {got_rows[w]!r} against oracle {ref_rows[w]!r}: error {err[key]:.3e} of the class's scale, bar {bars[key]:.3e} {ctx()}")
    ratios["subnormal_steps"] = ratio("subnormal_steps")
    if ratios["subnormal_steps"] > 1.0:
        fails.append(f"a class of subnormal scale is {err['subnormal_steps']:.0f} steps from the oracle, bar {bars['subnormal_steps']:.0f} {ctx()}")
    # the f32 block: float32(oracle f64), or its neighbour where the f64 value lies within the bar of the rounding midpoint
    o64 = info["out64"]
    osr = len(info["sweeps"]) // len(ref_f32)
    around = lambda i: info["sweeps"][max(0, osr * (i - 1)):osr * (i + 2)].tolist()
    key = bar_key("f32_block", redesigned)
    scale = class_scale("f32_block", rows_in, ref_rows, info)
    room = bars[key] * scale if scale >= SUBNORMAL_SCALE else bars["subnormal_steps"] * SUBNORMAL_STEP
    differ = np.nonzero(ref_f32.view(np.uint32) != got_f32.view(np.uint32))[0]
    near = set(neighbour_samples(ref_f32, got_f32).tolist())
    n_neighbour = 0
    worst = 0.0
    for i in differ.tolist():
        if i in near:
            mid = 0.5 * (float(ref_f32[i]) + float(got_f32[i]))
            dist = abs(float(o64[i]) - mid)
            if dist <= room:
                n_neighbour += 1
                worst = max(worst, dist / room)
                continue
            fails.append(f"sample {i}: {got_f32[i]!r} is the float next to float32(oracle {o64[i]!r}) = {ref_f32[i]!r}, but the oracle lies "
                         f"{dist:.3e} from the midpoint, bar {room:.3e} (sweeps around it {around(i)}) {ctx()}")
        else:
            fails.append(f"sample {i}: {got_f32[i]!r} != float32(oracle {o64[i]!r}) = {ref_f32[i]!r} "
                         f"(sweeps around it {around(i)}, guard fired {int(info['fired'][i])}) {ctx()}")
    ratios[key] = worst
    return fails, ratios, n_neighbour


def measure_bars(rates=RATES):
    """The measurement behind MEASURED: -> ({bar key: largest error}, {bar key: where}, neighbour share, samples)."""
    meas = {k: 0.0 for k in BAR_KEYS}
    where = {}
    runs = [(p, s) for p in ob.STAGE_PATTERNS for s in ((1, 2) if p == "random" else (0,))]
    flips = {r: 0 for r in runs}
    samples = 0
    for rate in rates:
        for recipe, n, rows, tap in cpu_corpus(rate):
            ref = reference(rate, recipe, rows, tap, n)
            samples += n
            for pat, seed in runs:
                got = reference(rate, recipe, rows, tap, n, pattern=pat, seed=seed)
                for r in EXACT_ROWS + (FLAGS,):
                    assert _same(got[0][r], ref[0][r]), (recipe["name"], r)
                assert (got[2]["fired"] == ref[2]["fired"]).all() and (got[2]["redesigned"] == ref[2]["redesigned"]).all(), recipe["name"]
                if not ref[2]["redesigned"].any():
                    assert _same(got[0][list(COEF_ROWS)], rows[list(COEF_ROWS)]).all()
                for k, v in class_errors(rows, ref, got[0], got[2]["out64"]).items():
                    if k == "coefficients" and not ref[2]["redesigned"].any():
                        continue
                    if v > meas[k]:
                        meas[k] = v; where[k] = (rate, recipe["name"], n, pat, seed)
                flips[(pat, seed)] += int(np.sum(got[1].view(np.uint32) != ref[1].view(np.uint32)))
    return meas, where, max(flips.values()) / samples, samples
