"""GPU: openwurli_amd.wurli_compare (the reference's tools/wurli_compare.py) end to end.

The golden's clip pairs through compare_many give the reference's report; every unrounded figure lies within 2.5 x its class's stored
float32 -> float64 movement of the float32 form (the project's floor rule: the device may differ from the reference by what the
reference's own number format moves it) and within 1e-3 x that movement of the float64 form: the device must BE the float64 statement of
tests/wurli_compare_ref.py, not something in between (the two formats' epsilons are 5e8 apart, so 1e-3 is loose).  A class whose stored
movement is 0 (the attack time: an index times a constant) must agree exactly.
Rendered pairs: the jobs give bit for bit what a direct batch_render with the reference's flags gives, and the analysis of the device
buffer meets the float64 bar against the restatement on the fetched audio."""
import json

import numpy as np
import pytest

import wurli_compare_ref as ref
from openwurli_amd import wurli_compare as wc

pytestmark = pytest.mark.gpu
NOTES = (40, 60, 77, 96)


def _check_figures(got, f32, f64, movement, where):
    """got / f32 / f64: one side's figures each.  f32 = None: the float64 bar alone (the movement was measured on the fixtures; a render
    has its own, so the floor rule against the float32 form is stated for the fixtures only)."""
    assert got["bins"] == f64["bins"] and got["attack_frame"] == f64["attack_frame"], where
    vg, v64 = ref.class_values(got), ref.class_values(f64)
    v32 = v64 if f32 is None else ref.class_values(f32)
    for c in ref.CLASSES:
        assert len(vg[c]) == len(v64[c]) == len(v32[c]) and (len(vg[c]) > 0 or c in ("decay", "attack")), (where, c)
        for x, a, b in zip(vg[c], v32[c], v64[c]):
            print(where, c, "dev - f32", None if f32 is None else x - a, "dev - f64", x - b, "movement", movement[c])
            assert abs(x - a) <= 2.5 * movement[c], (where, c, x, a)
            assert abs(x - b) <= 1e-3 * movement[c], (where, c, x, b)


def test_golden_pairs_give_the_reference_report(hiplib):
    g, pairs = ref.load_golden()
    figures = []
    comps = wc.compare_many([p[0] for p in pairs], [p[2] for p in pairs], synths=[p[1] for p in pairs], figures=figures)
    for got, e in zip(comps, g["comparisons"]):
        assert json.loads(json.dumps(got)) == e["comparison"], e["note_name"]
    assert wc.format_comparison_report([dict(e, comparison=c) for e, c in zip(g["comparisons"], comps)], "OUT") == g["report_text"]
    for i, ((dr, ds), (ar, as_), (br, bs)) in enumerate(zip(figures, ref.golden_figures(np.float32), ref.golden_figures(np.float64))):
        _check_figures(dr, ar, br, g["movement"], f"pair {i} recorded")
        _check_figures(ds, as_, bs, g["movement"], f"pair {i} render")
    # the reference's functions one clip at a time give the report's figures
    y, f0 = pairs[1][0], pairs[1][2]
    c = g["comparisons"][1]["comparison"]
    sus = ref.slices(y, pairs[1][1])[0]
    assert wc.harmonic_profile(sus, 44100, f0) == c["harmonics_real"] and wc.measure_spectral_centroid(sus, 44100) == c["centroid_real_hz"]
    assert (wc.measure_decay(y, 44100), wc.measure_attack_time(y, 44100), wc.measure_rms(y)) == (c["decay_real_db_s"], c["attack_real_ms"], c["rms_real_db"])
    assert wc.harmonic_profile(np.zeros(9000), 44100, f0) is None and wc.measure_attack_time(np.zeros(9000), 44100) is None
    assert wc.measure_decay(np.ones(4000), 44100) is None                     # fewer than 5 frames after the attack


def _wav24(v):
    q = np.sign(v) * np.floor(np.abs(v) * 8388607.0 + 0.5)
    return np.clip(q, -8388607.0, 8388607.0) / 8388608.0


def test_rendered_pairs(hiplib):
    """Tier 2 and tier 3 of four notes, two durations: the renders are the reference's command lines, the analysis is the restatement's."""
    import openwurli_amd as ow
    g, pairs = ref.load_golden()
    jobs, durs, reals, f0s = [], [], [], []
    for tier3 in (False, True):
        for k, m in enumerate(NOTES):
            jobs.append(wc.render_job(m, 100, tier3)); durs.append(0.5 if (k == 1 and tier3) else 0.6)      # one job of another duration
            reals.append(pairs[k][0]); f0s.append(pairs[k][2])
    figures, audio = [], []
    comps = wc.compare_rendered(reals, f0s, jobs, durs, figures=figures, audio_out=audio)
    rows, lengths = audio
    assert lengths.tolist() == [26460] * 5 + [22050] + [26460] * 2
    # the stated flags, spelled out: tier 2 = --no-poweramp --speaker 0.0 --volume 1.0, tier 3 = --volume 0.40 --speaker 1.0, MLP on
    direct = ow.batch_render([{"note": m, "velocity": 100, "mlp": True, "poweramp": False, "volume": 1.0, "speaker": 0.0} for m in NOTES] +
                             [{"note": m, "velocity": 100, "mlp": True, "poweramp": True, "volume": 0.40, "speaker": 1.0} for m in NOTES if m != 60],
                             44100.0, 0.6)
    short = ow.batch_render([{"note": 60, "velocity": 100, "mlp": True, "poweramp": True, "volume": 0.40, "speaker": 1.0}], 44100.0, 0.5)
    want = [direct[0], direct[1], direct[2], direct[3], direct[4], short[0], direct[5], direct[6]]
    for i, w in enumerate(want):
        assert rows[i, :lengths[i]].tobytes() == np.ascontiguousarray(w).tobytes() and np.abs(w).max() > 1e-4, i
    for i, (comp, (dr, ds)) in enumerate(zip(comps, figures)):
        synth = _wav24(rows[i, :lengths[i]])                                   # the 24-bit file `preamp-bench render` writes, read back
        a64 = ref.pair_figures(reals[i], synth, f0s[i], np.float64)
        _check_figures(ds, None, a64[1], g["movement"], f"job {i} render")
        _check_figures(dr, None, a64[0], g["movement"], f"job {i} recorded")
        assert json.loads(json.dumps(comp)) == json.loads(json.dumps(wc.comparison_from_figures(a64[0], a64[1], f0s[i]))), i
        assert comp["harmonics_synth"] is not None and comp["harmonic_distance_db"] > 0.0


def test_rank_equals_separate_runs(hiplib):
    from openwurli_amd import mlp
    _, pairs = ref.load_golden()
    notes, reals, f0s = [77, 96], [pairs[2][0], pairs[3][0]], [pairs[2][2], pairs[3][2]]
    sets = [mlp.MlpWeights.builtin(), mlp.MlpWeights.builtin().perturbed(0.05, 3)]
    rows = wc.rank(reals, f0s, notes, [90, 60], [0.6, 0.6], sets, ["builtin", "sweep"], tiers=(2, 3))
    assert [(r["weights"], r["tier"]) for r in rows] == [("builtin", 2), ("builtin", 3), ("sweep", 2), ("sweep", 3)]
    separate = []
    for s in sets:
        for tier in (2, 3):
            comps = wc.compare_rendered(reals, f0s, [wc.render_job(m, v, tier == 3) for m, v in zip(notes, [90, 60])], [0.6, 0.6], [s], [0, 0])
            separate.append(comps)
    assert rows == wc.rank_rows(["builtin", "sweep"], [2, 3], separate)
    assert rows[0] != rows[2] and rows[0] != rows[1] and all(r["n_notes"] == 2 and r["harm_dist_mean_db"] is not None for r in rows)
