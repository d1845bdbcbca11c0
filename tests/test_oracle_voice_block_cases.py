"""What tests/test_gpu_voice_block.py rests on, on the CPU: the oracle's voice block function IS the engine; the numpy restatement of it
agrees at float64; the bars of the comparison are measured on the reference alone (its f64 error against the long-double run of the same
block, its own movement under a one-ulp change of the record); the reference's decisions do not depend on its precision; nothing is left
out but what two stated conditions leave out; and the comparison sees each of eight deliberate slips on a named case."""
import numpy as np
import pytest

import oracle_binding as ob
import voice_block_cases as vc
from voice_block_cases import vp

HAVE_LD = np.finfo(np.longdouble).nmant >= 63
_RUNS = {}


def corpus(rate):
    """[(recipe, L, record, steal)] of every recipe and block length at `rate`"""
    return [(r, L, vc.record(r, L), r["setup"] == "steal") for r in vc.recipes(rate) + vc.steal_recipes(rate) for L in vc.lengths_of(r)]


def runs(rate):
    """the corpus through the oracle, the numpy block at float64 and at long double: once per session"""
    if rate not in _RUNS:
        cases = corpus(rate)
        _RUNS[rate] = (cases, [ob.voice_block(rec, steal, L) for _, L, rec, steal in cases],
                       [vp.voice_block(rec, steal, L) for _, L, rec, steal in cases],
                       [vp.voice_block(rec, steal, L, T=np.longdouble) for _, L, rec, steal in cases] if HAVE_LD else None)
    return _RUNS[rate]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- the function is the engine -----------------------------------------------------------------------------------------------------------
def _script(rate):
    """(calls before the block, block length)*: onset, hold, release, re-strike, pedal, and a full engine that steals"""
    yield [("note_on", 60, 0.8)], 64
    yield [], 129
    yield [("note_on", 33, 0.3), ("note_on", 96, 1.0)], 200
    yield [], 1030
    yield [("note_off", 60)], 37
    yield [("set_sustain", True), ("note_off", 33), ("note_on", 60, 0.5)], 512
    yield [("note_on", 33, 0.9)], 48                       # re-strike of a sustained key: it starts to damp
    yield [("set_sustain", False)], 300
    yield [("note_on", 40 + k, 0.2 + 0.01 * k) for k in range(52)] + [("note_on", 41, 1.0)] * 12, 100      # every slot taken ...
    yield [("note_on", 70, 0.6), ("note_on", 71, 0.6)], 24          # ... two steals
    yield [], 129
    yield [], int(rate * 0.005)                            # the crossfades run out inside this block
    yield [("note_off", 41)], 1024
    yield [], 2000


@pytest.mark.parametrize("rate", vc.RATES)
def test_block_function_is_the_engine(rate):
    """Records harvested from an engine in the middle of a played script; owo_voice_block of each reproduces the engine's next block bit for
    bit: every record after it, and the voice-sum tap as the slot-order sum of the voices' samples (engine.rs:469-493)."""
    e = ob.OracleEngine(rate)
    seen = dict(steal=0, damp=0, attack=0, steady=0, blocks=0, single=0)
    for calls, L in _script(rate):
        for c in calls:
            getattr(e, c[0])(*c[1:])
        before = {(s, st): e.voice_record(s, st) for s in range(64) for st in (False, True)}
        before = {k: v for k, v in before.items() if v is not None}
        _, tap = e.render_tap(L)
        acc = np.zeros(L)
        for (s, st), rec in sorted(before.items()):
            out, y, info = ob.voice_block(rec, st, L)
            acc = acc + y
            seen["steal" if st else vc.state_of(rec)] += 1
            after = e.voice_record(s, st)
            if after is None:                              # freed: silent, or a crossfade that ran out
                assert info["silent"] if not st else vc.lo32(out, vc.STEAL) == 0, (s, st, L)
                continue
            if not st:
                out[vc.STEAL] = after[vc.STEAL]            # a slot voice's record carries the slot's counters, which its steal voice moves
            assert _bits_equal(out, after), (s, st, L, np.nonzero(out.view(np.uint64) != after.view(np.uint64))[0])
        assert _bits_equal(acc, tap), (L, float(np.max(np.abs(acc - tap))))
        seen["blocks"] += 1
        seen["single"] += len(before) == 1
    e.close()
    assert seen["steal"] >= 4 and seen["damp"] >= 3 and seen["attack"] >= 3 and seen["steady"] >= 64 and seen["single"] >= 2, seen


def test_set_voice_record_round_trips():
    e = ob.OracleEngine(48000.0)
    e.note_on(60, 0.7)
    rec = vc.record(vc.recipes(48000.0)[3], 33)
    e.set_voice_record(0, rec)
    assert _bits_equal(e.voice_record(0), rec)
    _, tap = e.render_tap(33)
    assert _bits_equal(tap, ob.voice_block(rec, False, 33)[1])
    assert e.voice_record(5) is None
    e.close()


# ---- the numpy restatement at float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", vc.RATES)
def test_numpy_block_agrees_at_float64(rate):
    """The second restatement, started from the record: integer state, constants and status bits equal, everything else within 1e-13 of
    its class's scale (tests/test_oracle_voice_path_numpy.py's bar for the two; measured: bit-identical)."""
    cases, orc, npy, _ = runs(rate)
    bars = {k: 1e-13 for k in vc.CLASSES}
    bars["subnormal_steps"] = 0.0
    worst = 0.0
    for (recipe, L, rec, steal), a, b in zip(cases, orc, npy):
        fails, ratios = vc.compare(rec, a, b[0], b[1], steal=False, bars=bars, where=f"{recipe['name']}, {L} samples")
        assert not fails, fails[:4]
        assert {k: b[2][k] for k in ("silent", "transient", "finite")} == a[2], (recipe["name"], L)
        worst = max(worst, max(v for k, v in ratios.items() if k != "subnormal_steps"))
    print(f"{len(cases)} blocks at {rate:g} Hz, worst difference {worst * 1e-13:.3e} of its scale")


# ---- bars -----------------------------------------------------------------------------------------------------------------------------------
CONTINUOUS = tuple(range(vc.S, vc.DRIFT + 7)) + (vc.Q, vc.NAMP, vc.NS1, vc.NS2)


def _one_ulp(rec, seed):
    rng = np.random.default_rng(seed)
    r = rec.copy()
    for f in CONTINUOUS:
        if r[f] != 0.0 and np.isfinite(r[f]):
            r[f] = np.nextafter(r[f], np.inf if rng.integers(2) else -np.inf)
    r[vc.ENV:vc.ENV + 7] = np.minimum(r[vc.ENV:vc.ENV + 7], 1.0)
    return r


def measure():
    meas = {k: 0.0 for k in vc.CLASSES}
    where = {}
    for rate in vc.RATES:
        cases, orc, _, ld = runs(rate)
        for i, (recipe, L, rec, steal) in enumerate(cases):
            ref = ld[i]
            moved = ob.voice_block(_one_ulp(rec, i), steal, L)
            for kind, r_, got in (("long double", ref, orc[i]), ("one ulp", orc[i], moved)):
                if steal and not vc.steal_record_compared(r_[0]):
                    errs = {"samples": vc.class_errors(rec, r_[0], r_[1], got[0], got[1])["samples"]}
                else:
                    errs = vc.class_errors(rec, r_[0], r_[1], got[0], got[1])
                for k, (e, at) in errs.items():
                    if e > meas[k]:
                        meas[k] = e; where[k] = (rate, recipe["name"], L, kind, at)
            # the carried quantity of the damper variants, stepped by the reference itself
            carried, modes = vc.carried_record(rec)
            if modes and vc.bits(rec, vc.FLAGS) & 1:
                a = ob.voice_block(carried, steal, L)[0]
                for kind, b in (("long double", vp.voice_block(carried, steal, L, T=np.longdouble)[0]), ("one ulp", ob.voice_block(_one_ulp(carried, i), steal, L)[0])):
                    for m in modes:
                        e = abs(a[vc.ENV + m] - b[vc.ENV + m]) / vc.SUBNORMAL_STEP
                        if e > meas["subnormal_steps_carried"]:
                            meas["subnormal_steps_carried"] = e; where["subnormal_steps_carried"] = (rate, recipe["name"], L, kind, f"mode {m}")
    return meas, where


@pytest.mark.skipif(not HAVE_LD, reason="no extended precision on this platform")
def test_bars_are_measured():
    """Every bar is at most 2.5 x what the reference itself shows on the corpus -- its f64 error against the long-double run of the same
    block, or its movement when the record's continuous fields go to a neighbouring double, whichever is larger -- and zero where that is
    zero; the recorded measurement is what this machine measures within the same factor."""
    meas, where = measure()
    for k in vc.CLASSES:
        print(f"{k:16s} measured {meas[k]:.3e} at {where.get(k)}  recorded {vc.MEASURED[k]:.3e}  bar {vc.BARS[k]:.3e}")
    for k in vc.CLASSES:
        assert vc.BARS[k] <= vc.FLOOR_RULE * meas[k], (k, vc.BARS[k], meas[k])
        assert vc.BARS[k] <= vc.FLOOR_RULE * vc.MEASURED[k]
        assert (vc.BARS[k] == 0.0) == (meas[k] == 0.0), k
        assert meas[k] <= vc.FLOOR_RULE * vc.MEASURED[k], (k, meas[k])
    assert max(vc.BARS[k] for k in vc.CLASSES if not k.startswith("subnormal_steps")) < 1e-9        # the renormalisation cases' 1e-9 stays visible


# ---- decisions and exclusions -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_LD, reason="no extended precision on this platform")
@pytest.mark.parametrize("rate", vc.RATES)
def test_decisions_are_the_references_alone(rate):
    """The f64 oracle and the long-double run agree on the silent bit, the transient bit, ramp-done and the saturated side of every
    sample, in every case: no decision of the corpus hangs on a rounding."""
    cases, orc, npy, ld = runs(rate)
    sat = dict(pos=0, neg=0, none=0)
    silent = 0
    for (recipe, L, rec, steal), a, b, c in zip(cases, orc, npy, ld):
        for k in ("silent", "transient", "finite"):
            assert a[2][k] == c[2][k], (recipe["name"], L, k)
        assert b[2]["ramp_done"] == c[2]["ramp_done"] == bool(vc.bits(a[0], vc.FLAGS) & 2), (recipe["name"], L)
        assert np.array_equal(b[2]["sat"], c[2]["sat"]), (recipe["name"], L)
        assert _bits_equal(a[0][list(vc.EXACT)], c[0][list(vc.EXACT)]), (recipe["name"], L)
        sat["pos"] += int((b[2]["sat"] > 0).sum()); sat["neg"] += int((b[2]["sat"] < 0).sum()); sat["none"] += int((b[2]["sat"] == 0).sum())
        silent += a[2]["silent"]
    assert sat["pos"] > 100 and sat["neg"] > 100 and sat["none"] > 10000 and 0 < silent < len(cases) // 4, (sat, silent)
    # the recipes that are a decision say what they decide
    by = {(r["name"], L): o for (r, L, _, _), o in zip(cases, orc)}
    for L in vc.LENGTHS:
        assert by[("minus_80_db_all_below", L)][2]["silent"] and not by[("minus_80_db_mode_0_above", L)][2]["silent"]
        assert by[("ten_seconds_over", L)][2]["silent"] and not by[("ten_seconds_not_yet", L)][2]["silent"]
        assert not by[("released_no_damper", L)][2]["transient"] and by[("damper_60_ramp_done", L)][2]["transient"]
        for note in (33, 60, 84):
            assert vc.bits(by[(f"damper_{note}_ends_at_L-1", L)][0], vc.FLAGS) & 2 and not vc.bits(by[(f"damper_{note}_ends_at_beyond", L)][0], vc.FLAGS) & 2
            if L > 1:
                assert not vc.bits(ob.voice_block(vc.record([r for r in vc.recipes(rate) if r["name"] == f"damper_{note}_ends_at_L-1"][0], L), False, L - 1)[0], vc.FLAGS) & 2


# share of compared quantities (7 pairs + 1 record per block) the two exclusion rules leave out on the corpus
MAX_EXCLUDED_PAIRS = 0.148        # 4566 of 30940: four upper modes of note 96 are below 1e-290 three thousand samples after the strike
MAX_EXCLUDED_STEAL_RECORDS = 0.059  # 276 of 4696 blocks


def test_exclusions_are_conditions():
    """Left out of the comparison: the (s, c) pair of a mode whose reference envelope after the block is below 1e-290 (its envelope is still
    compared, in steps of the smallest subnormal where it is subnormal) and the record of a steal voice whose fade has run out (its
    samples are still compared).  Nothing else; the share is what those two rules give here."""
    pairs = excluded = records = dropped = 0
    for rate in vc.RATES:
        cases, orc, _, _ = runs(rate)
        for (recipe, L, rec, steal), o in zip(cases, orc):
            records += 1
            if steal and not vc.steal_record_compared(o[0]):
                dropped += 1
                continue
            pairs += 7
            ex = vc.pair_excluded(o[0])
            assert all(o[0][vc.ENV + m] < vc.SUBNORMAL_SCALE for m in ex)
            excluded += len(ex)
    print(f"pairs excluded: {excluded} of {pairs} ({excluded / pairs:.4f}); steal records not compared: {dropped} of {records} ({dropped / records:.4f})")
    assert 0 < excluded / pairs <= MAX_EXCLUDED_PAIRS and 0 < dropped / records <= MAX_EXCLUDED_STEAL_RECORDS


def test_corpus_reaches_what_it_claims():
    for rate in vc.RATES:
        cases, orc, _, _ = runs(rate)
        forms = {}
        for (recipe, L, rec, steal), o in zip(cases, orc):
            for f in (("steal",) if steal else vc.forms_of(recipe["setup"], rec)):
                forms.setdefault(f, set()).add(recipe["family"])
            assert o[2]["finite"], (recipe["name"], L)
        assert forms["steady"] >= {"counter", "envelope", "pickup", "damper"} and forms["attack"] >= {"counter", "attack"}, forms
        assert forms["release"] == {"damper"} and forms["declined"] == {"damper"} and forms["k_voice"] >= {"counter", "envelope", "pickup", "attack", "damper"}
        residues = {vc.bits(rec, vc.SAMPLE) & 15 for r, L, rec, _ in cases if r["family"] == "counter"}
        assert residues == set(range(16))
        shapes = {("cos" if rec[vc.ONSET_EXP] <= 1.001 else "square" if rec[vc.ONSET_EXP] >= 1.999 else "pow")
                  for r, L, rec, _ in cases if vc.bits(rec, vc.SAMPLE) < vc.bits(rec, vc.ONSET_N) and rec[vc.AMP] != 0.0}
        assert shapes == {"cos", "square", "pow"}
        # the pickup's charge at rest, below and above it on each side of the knee
        for side in (lambda p: p < 0.94, lambda p: p >= 0.94):
            qs = {float(rec[vc.Q]) for r, L, rec, _ in cases if r["family"] == "pickup" and r["name"].count("_") == 2 and side(float(r["name"].split("_")[1]))}
            assert qs == {1.0, 0.3, 3.0}, qs
        # modes without amplitude under the damper, inside the ramp and behind it, in the release and the steal variant's hands
        for fam, form in (("damper", "release"), ("steal", "steal")):
            zero = [(rec, o) for (r, L, rec, st), o in zip(cases, orc) if r["family"] == fam and (rec[vc.AMP:vc.AMP + 7] == 0.0).any()
                    and vc.bits(rec, vc.FLAGS) & 1 and not vc.declines(rec)]
            assert any(not vc.bits(o[0], vc.FLAGS) & 2 for _, o in zero) and any(vc.bits(rec, vc.FLAGS) & 2 for rec, _ in zero), (fam, len(zero))
            assert any(not vc.bits(rec, vc.FLAGS) & 2 and vc.bits(o[0], vc.FLAGS) & 2 for rec, o in zero), fam       # the ramp ends inside the block
            assert any(0.0 < (rec[vc.AMP:vc.AMP + 7] == 0.0).sum() < 7 for rec, _ in zero), fam                         # one mode of a sounding voice
        # every mode alone above the -80 dB test where its amplitude allows it (mode 0 always; upper modes of the loud low notes)
        above = {int(r["name"].split("_")[4]) for r, L, rec, _ in cases if r["name"].startswith("minus_80_db_mode_")}
        assert 0 in above and len(above) >= 2, above
        for (r, L, rec, _), o in zip(cases, orc):
            if r["name"].startswith("minus_80_db_mode_"):
                assert not o[2]["silent"], r["name"]
        ramps = {float(rec[vc.DRAMP]) for r, L, rec, _ in cases if r["family"] == "damper" and vc.bits(rec, vc.FLAGS) & 1}
        assert ramps >= ({352.8, 1102.5, 2205.0} if rate == 44100.0 else {384.0, 1200.0, 2400.0}), ramps


# ---- teeth ----------------------------------------------------------------------------------------------------------------------------------
TEETH = {      # mutant -> (recipe, block length) on which the comparison has to see it
    "renorm_late": ("renorm_last", 33),
    "jitter_on_1": ("residue_5", 16),
    "env_write_back": ("sample_1025", 24),
    "onset_index": ("onset_left_24", 25),
    "crossfade_remaining": ("steal_ramp_ending_left_23", 24),
    "damper_final_mult": ("damper_84_ends_at_23", 25),
    "fade_table": ("noise_left_24", 17),
    "knee_095": ("pickup_0.945_pos", 48),
}


@pytest.mark.parametrize("mutant", vp.MUTANTS)
def test_the_comparison_sees_each_slip(mutant):
    """Each deliberate slip of the numpy block fails the comparison against the oracle, with the recorded bars, on its named case; the
    block without a slip passes there."""
    name, L = TEETH[mutant]
    for rate in vc.RATES:
        recipe = [r for r in vc.recipes(rate) + vc.steal_recipes(rate) if r["name"] == name][0]
        steal = recipe["setup"] == "steal"
        rec = vc.record(recipe, L)
        ref = ob.voice_block(rec, steal, L)
        good = vp.voice_block(rec, steal, L)
        assert not vc.compare(rec, ref, good[0], good[1], steal=steal)[0]
        bad = vp.voice_block(rec, steal, L, mutant=mutant)
        fails, _ = vc.compare(rec, ref, bad[0], bad[1], steal=steal)
        assert fails, (mutant, name, L, rate)
        print(f"{mutant} at {rate:g} Hz: {fails[0]}")


def test_record_indices_are_the_headers():
    """The VF_* indices are restated for the oracle (VR_* of ow_oracle_capi.cpp), the numpy block (voice_path_numpy.VF) and the corpus; the
    product guards include/openwurli_hip_test.h's OW_TEST_VF_* with static_asserts, and this holds the three copies to that header."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = dict(re.findall(r"#define OW_TEST_VF_(\w+) (\d+)", open(os.path.join(root, "include", "openwurli_hip_test.h")).read()))
    header = {k[:-1] if k.endswith("0") and k != "NB0" else k: int(v) for k, v in header.items()}
    assert len(header) == 34 and header["COUNT"] == ob.VOICE_RECORD_FIELDS
    assert vp.VF == header
    assert {k: getattr(vc, k) for k in header} == header
    capi = open(os.path.join(root, "oracle", "ow_oracle_capi.cpp")).read()
    assert {k: int(v) for k, v in re.findall(r"VR_(\w+) = (\d+)", capi)} == header
