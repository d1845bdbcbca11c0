"""The oracle's output stage as a function of its state rows (owo_output_stage_block) and the corpus of tests/post_stage_cases.py, on the
CPU: the function IS the oracle engine's stage (bit for bit), the comparison's bars are measured and obey floor <= 2.5 x measurement, the
comparison sees each of seven deliberately wrong stages on the family named for it, and the corpus reaches what it claims to reach.

Measured here (glibc 2.x, x86-64): see MEASURED in post_stage_cases.py; printed by test_bars_are_measured with -s."""
import numpy as np
import pytest

import oracle_binding as ob
import post_stage_cases as ps


def _engine_blocks(rate, e, lengths, setters=None):
    """Render `lengths` on oracle engine e; before each block read the stage rows, then call setters(e, block) -> (flags, spk, vol) if given;
    the function must reproduce every block and the rows behind it bit for bit.  Returns the number of guard fires seen."""
    osr = ps.osr_of(rate)
    fired = 0
    for b, n in enumerate(lengths):
        rows = e.stage_rows()
        flags, s, v = setters(e, b) if setters else (0, 0.0, 0.0)
        out, _, pre, _ = e.render_taps(n, osr)
        rows_out, f32, info = ob.output_stage_block(rate, rows, pre, n, flags, s, v)
        after = e.stage_rows()
        assert f32.tobytes() == out.tobytes(), (rate, b, n)
        stage = list(range(ps.SM_SPK, ps.SM_VOL + 4)) + list(range(ps.OS_DA, ps.TS + 1))
        assert ps._same(rows_out[stage], after[stage]).all(), (rate, b, np.nonzero(~ps._same(rows_out[stage], after[stage]))[0])
        fired += int(info["fired"].sum())
    return fired


def test_function_is_the_engines_stage_fresh_engine_and_speaker_ramp():
    """tests/test_gpu_parity.py::test_engine_fresh_without_warmup_and_speaker_ramp's scenario: WurliEngine::new without a warm-up, the
    speaker character ramping through the 0.002 hysteresis, a ragged block length; the second half's setters go in as set_flags."""
    e = ob.OracleEngine(48000.0)
    e.set_volume(0.8); e.set_tremolo_depth(1.0); e.set_speaker_character(0.7)
    for n in (45, 60, 64, 79):
        e.note_on(n, 0.8)
    assert _engine_blocks(48000.0, e, [256] * 8) == 0

    def setters(e, b):
        if b:
            return 0, 0.0, 0.0
        e.set_speaker_character(1.0); e.set_volume(0.3); e.set_tremolo_depth(0.2)
        return 6, 1.0, 0.3
    assert _engine_blocks(48000.0, e, [333] * 30, setters) == 0
    e.close()


@pytest.mark.parametrize("rate", [44100.0, 96000.0])
def test_function_is_the_engines_stage_guard_event(rate):
    """A speaker state too large for f32 but not for f64: the engine's guard fires, resets speaker and oversampler (and the preamp, which
    the next block's tap shows); rows and blocks stay those of the function."""
    e = ob.OracleEngine(rate)
    e.set_speaker_character(1.0)
    for n in (40, 52, 64):
        e.note_on(n, 1.0)
    e.render(512)
    rows = e.stage_rows()
    rows[ps.LPF + 5] = 1e39
    e.set_stage_rows(rows)
    assert _engine_blocks(rate, e, [65, 37]) == 1
    e.close()


def test_bars_are_measured():
    """Every bar of the comparison is at most 2.5 x the largest movement of the perturbed oracle (every exp / tanh / pow / cos / sin result
    of the stage STAGE_PERTURB_ULPS doubles away: all up, all down, alternating, two seeded random sign sequences) from the plain one over
    the whole corpus, and zero where that is zero; the recorded measurement is what this machine measures within a factor of 2.5 too.  The
    perturbation changes no bit-equal row, no redesign and no guard decision (asserted inside measure_bars)."""
    meas, where, share, samples = ps.measure_bars()
    for k in ps.BAR_KEYS:
        print(f"{k:26s} measured {meas[k]:.3e} at {where.get(k)}  recorded {ps.MEASURED[k]:.3e}  bar {ps.BARS[k]:.3e}")
        assert ps.BARS[k] <= ps.FLOOR_RULE * meas[k], (k, ps.BARS[k], meas[k])
        assert ps.BARS[k] <= ps.FLOOR_RULE * ps.MEASURED[k]
        assert (ps.BARS[k] == 0.0) == (meas[k] == 0.0), k
        assert meas[k] <= ps.FLOOR_RULE * ps.MEASURED[k], (k, meas[k])
    print(f"neighbouring float32 at {share:.3e} of {samples} samples (recorded {ps.MEASURED_NEIGHBOUR_SHARE:.3e})")
    assert ps.MEASURED_NEIGHBOUR_SHARE <= share
    # the reference pins the stage far below the f32 bar of the parity tests: nothing here is looser than 1e-10 of its scale
    assert max(ps.BARS[k] for k in ps.BAR_KEYS if k != "subnormal_steps") < 1.2e-10


def test_corpus_reaches_what_it_claims():
    """Every sweep count 1 .. 8 of the power amp's Newton loop in at least 64 chain samples of the corpus at every rate, on both
    signs of the tap for five sweeps and more; the loop converged on every finite tap (so no finite case is left out: the allowed share is
    zero); every guard recipe fires or not as it says; every family and every way the speaker can go through a block occurs."""
    for rate in ps.RATES:
        hist = {1: np.zeros(9, dtype=np.int64), -1: np.zeros(9, dtype=np.int64)}
        redesign_blocks = 0
        ends = set()
        for recipe, n, rows, tap in ps.cpu_corpus(rate):
            _, f32, info = ps.reference(rate, recipe, rows, tap, n)
            fin = np.isfinite(tap)
            assert info["converged"][fin].all(), (rate, recipe["name"], n)
            for sgn in (1, -1):
                hist[sgn] += np.bincount(info["sweeps"][fin & (np.sign(tap) == sgn)], minlength=9)
            want = ps.expect_fired(recipe, rate)
            if want is not None:
                assert bool(info["fired"].any()) == want, (rate, recipe["name"], n)
            elif recipe["name"] != "guard_nan_out_node":
                assert not info["fired"].any(), (rate, recipe["name"], n)
            redesign_blocks += bool(info["redesigned"].any())
            if recipe["name"] == "ramp_redesign_every_few" and n >= 37:
                gaps = np.diff(np.nonzero(info["redesigned"])[0])
                assert gaps.size and gaps.min() >= 2 and gaps.max() <= 4, gaps         # 0.0007 per sample against the 0.002 hysteresis
            if recipe["name"].startswith("ramp_ends_at_") and n >= 65:
                ends.add(int(recipe["name"].rsplit("_", 1)[1]))
            if recipe["name"] == "silent":
                after = ps.reference(rate, recipe, rows, tap, n)[0]
                assert not tap.any() and not f32.any() and 0.0 < after[ps.TS] < rows[ps.TS]      # exact zeros, the thermal state decaying
        print(rate, "sweeps on positive taps", hist[1][1:].tolist(), "negative", hist[-1][1:].tolist())
        for k in range(1, 9):
            assert hist[1][k] + hist[-1][k] >= 64, (rate, k)
            if k >= 5:
                assert hist[1][k] >= 64 and hist[-1][k] >= 64, (rate, k, hist[1][k], hist[-1][k])
        assert ends == {1, 63, 64} and redesign_blocks >= 20
    assert {r["family"] for r in ps.RECIPES} == {"levels", "character", "state", "guard"}
    assert len(set(ps.NAMES)) == ps.R <= 65               # a pool of 65 engines plays every recipe


# mutant -> (recipes of the family named for it, rates at which the variant differs at all)
MUTANT_FAMILY = {
    "no_down_delay": (("four_mf", "sixteen_ff", "kick_0.3"), (44100.0, 48000.0)),
    "thermal_after_gain": (("thermal_large", "sixteen_ff", "states_mixed_kick"), ps.RATES),
    "bypass_on_smoother": (("ramp_across_bypass",), ps.RATES),
    "thermal_alpha_chain_rate": (("thermal_large", "sixty_four_ff"), (44100.0, 48000.0)),
    "guard_keeps_ts": (("guard_hpf_1e41_loud",), ps.RATES),
    "guard_on_f64": (("guard_lpf_1e39",), ps.RATES),
    "newton_7": (("kick_1.2755", "kick_1.276", "kick_1.2765"), ps.RATES),
}


@pytest.mark.parametrize("mutant", list(MUTANT_FAMILY))
def test_comparison_flags_the_mutant(mutant):
    """With the measured bars the comparison fails each wrong stage on every recipe named for it, at every rate and block length at which
    the variant is reached (a block of one or two samples cannot show a ramp's 25th sample, nor an eighth sweep that no sample takes).
    The seven-sweep Newton cap is resolved too: leaving out the eighth correction of the samples that take eight sweeps moves the
    decimator's rows by 1e-12 .. 3e-12 (test_eighth_newton_correction_size prints it), the half-band bar is 2.5e-15 of a state near 1."""
    names, rates = MUTANT_FAMILY[mutant]
    flagged = reached = 0
    for rate in rates:
        for recipe, n, rows, tap in ps.cpu_corpus(rate):
            if recipe["name"] not in names:
                continue
            ref = ps.reference(rate, recipe, rows, tap, n)
            got = ps.reference(rate, recipe, rows, tap, n, mutant=mutant)
            if mutant == "newton_7":
                if not (ref[2]["sweeps"] == 8).any():
                    continue
            elif mutant == "bypass_on_smoother":
                if n <= ps.ramp_of(rate) // 10 + 1:
                    continue                             # the smoother passes 0.001 a tenth into the ramp: sample 22, 24, 48
            fails, ratios, _ = ps.compare(rows, ref, got[0], got[1], where=f"{mutant} {recipe['name']} {rate} n={n}")
            reached += 1
            assert fails, (mutant, recipe["name"], rate, n, ratios)
            flagged += 1
            same = ps.compare(rows, ref, ref[0], ref[1])
            assert not same[0] and same[2] == 0
    print(mutant, "flagged on", flagged, "of", reached, "cases")
    assert flagged == reached and reached >= 6


def test_eighth_newton_correction_size():
    """What the seven-sweep cap leaves out, seen in the decimator's state after a block that ends on eight-sweep samples."""
    rate = 48000.0
    sizes = []
    for recipe, n, rows, tap in ps.cpu_corpus(rate):
        if recipe["family"] != "levels" or n != 129:
            continue
        ref = ps.reference(rate, recipe, rows, tap, n)
        m = ref[2]["sweeps"] == 8
        if not m.any():
            continue
        got = ps.reference(rate, recipe, rows, tap, n, mutant="newton_7")      # the half-band rows carry the amp's last outputs
        d = np.abs(got[0][list(ps.CLASS_ROWS["half_band"])] - ref[0][list(ps.CLASS_ROWS["half_band"])]).max()
        sizes.append(d)
    print("half-band rows moved by the seven-sweep cap:", sizes)
    assert sizes and min(sizes) > 100 * ps.BARS["half_band"]
