"""`preamp-bench render-poly` (tools/preamp-bench/src/main.rs:1397-1592), host side: no GPU needed.

The CPU restatement (tests/c/render_poly_ref.cpp) against the existing oracle's batch job where the two commands coincide, and where they
must not (the reset order); the sample floor of the GPU test under the project's floor rule, measured here; the condition that keeps the
GPU test's intermod_ratio_db assertion honest; the Python report, padding, verdict and WAV logic against main.rs; the restatement's row
against the binding's (the structs' layouts: tests/test_abi_layout.py); and ow_render_poly's refusals, which come before any device work.
"""
import ctypes as C
import math

import numpy as np
import pytest

import render_poly_ref as ref


@pytest.fixture(scope="module")
def chord_refs():
    """{name: (restatement, one-ulp-exp restatement)} of the GPU test's chords."""
    names = list(ref.CHORDS)
    a = ref.render_many([ref.CHORDS[k] for k in names])
    b = ref.render_many([ref.CHORDS[k] for k in names], perturbed=True)
    return {k: (x, y) for k, x, y in zip(names, a, b)}


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poweramp", [True, False])
def test_one_note_chord_equals_the_oracles_batch_job_bit_for_bit(oracle, poweramp):
    """One note, seed + 0, r_ldr = 1 Mohm (where set_ldr_resistance moves nothing and the order of reset() is immaterial): the chain of
    render-poly is the chain of `render`."""
    note, vel, dur = 57, 90, 0.5
    r = ref.render([note], [vel], dur, 0.60, 1.0, 1e6, no_poweramp=not poweramp)
    job = oracle.batch_render_job_ex(note, vel, dur, 44100.0, 0.60, 1.0, 1e6, mlp=True, poweramp=poweramp)
    assert r.final.size == job.size == 22050
    assert r.final.tobytes() == job.tobytes()
    assert r.separate_sum.tobytes() == r.final.tobytes() and r.voices[0].tobytes() == r.final.tobytes()
    assert not r.residual.any() and r.row["rms_db"][2] == -120.0 and r.row["peak_db"][2] == -120.0 and r.row["residual_peak"] == 0.0


def test_reset_order_matters_at_19k(oracle):
    """set_ldr_resistance BEFORE reset(): the DC solve runs at the chord's --ldr.  `render` resets first (DC at 1 Mohm, then the step to
    19 kohm rings through the coupling network): more than the parity bar apart."""
    note, vel, dur = 57, 90, 0.5
    r = ref.render([note], [vel], dur, 0.60, 1.0, 19_000.0)
    job = oracle.batch_render_job_ex(note, vel, dur, 44100.0, 0.60, 1.0, 19_000.0, mlp=True, poweramp=True)
    rep = oracle.parity_report(r.final, job, abs_floor=oracle.ABS_FLOOR_BATCH)
    assert rep["n_bad"] > 1000 and rep["max_err_rel_peak"] > 1e-2, rep


def test_second_voice_of_a_note_gets_its_own_seed():
    """note * 2654435761 + i: the same note twice gives two different voices (attack noise and frequency jitter are seeded), so a unison
    is not 2 x one voice."""
    r = ref.render([60, 60], [90, 90], 0.25, 0.60, 1.0, 1e6)
    assert not np.array_equal(r.voices[0], r.voices[1])
    assert r.row["residual_peak"] > 0.0


def test_window_and_row_figures_of_the_restatement():
    r = ref.render_chord(ref.CHORDS["ldr_19k"])
    n = r.final.size
    assert n == 44100 and ref.window(n) == slice(8820, 44100) and ref.window(200000) == slice(8820, 88200)
    w = ref.window(n)
    assert r.row["peak"] == np.abs(r.final).max() and r.row["residual_peak"] == np.abs(r.residual).max()
    assert np.array_equal(r.residual, r.final - r.separate_sum)
    for k, x in enumerate((r.final, r.separate_sum, r.residual)):
        assert r.row["win_peak"][k] == np.abs(x[w]).max()
        assert abs(r.row["win_mean_sq"][k] / np.mean(np.square(x[w])) - 1.0) < 1e-12        # sequential against pairwise summation
        assert r.row["peak_db"][k] == 20.0 * math.log10(r.row["win_peak"][k]) and r.row["rms_db"][k] == 10.0 * math.log10(r.row["win_mean_sq"][k])
    assert r.row["intermod_ratio_db"] == r.row["rms_db"][0] - r.row["rms_db"][2]
    with pytest.raises(ValueError):
        ref.render([60], [90], 0.2)                                                          # n = 8820: the reference's slice panics


# ---- the floor of the GPU test's sample bars ---------------------------------------------------------------------------------------
def test_sample_floor_follows_the_floor_rule(oracle, chord_refs):
    """The project's rule (oracle_binding.FLOORS): F <= 2.5 x what the reference algorithm itself moves by, on the samples the floor
    governs, when exp() is off by one ulp.  Measured on the chords the GPU test uses: 9.3e-9 (the loud low dyad).  ABS_FLOOR_BATCH would be
    too wide here (3e-8 > 2.5 x 9.3e-9), hence ABS_FLOOR_POLY."""
    worst = {}
    for k, (a, b) in chord_refs.items():
        d = oracle.floor_governed_delta(a.final, b.final, ref.ABS_FLOOR_POLY)
        assert d == d, k                                                                   # the floor governs samples of every chord
        worst[k] = d
        assert np.abs(a.final - b.final).max() / np.abs(a.final).max() < 1e-5 * 0.2, k     # far inside the relative bar
    w = max(worst.values())
    print(f"\n[floor table] ABS_FLOOR_POLY {ref.ABS_FLOOR_POLY:.1e}: one-ulp {w:.2e} ({worst}), ratio {ref.ABS_FLOOR_POLY / w:.2f}")
    assert 1e-10 < w < ref.ABS_FLOOR_POLY
    assert ref.ABS_FLOOR_POLY <= oracle.FLOOR_RULE * w, worst
    assert oracle.ABS_FLOOR_BATCH > oracle.FLOOR_RULE * w                                   # why the batch floor is not used


def test_residual_stands_clear_of_its_bar_on_every_chord_whose_ratio_is_asserted(chord_refs):
    """For every chord the GPU test asserts intermod_ratio_db on (all of CHORDS), the restatement's residual RMS over the window is at
    least 10 x the RMS of the residual's sample bar: the ratio then measures intermodulation, not tolerance."""
    for k, (a, _) in chord_refs.items():
        assert ref.ratio_is_assertable(a, ref.ABS_FLOOR_POLY), k
    # ... which is a real condition: a loud chord through a linear speaker leaves a residual inside the bar
    quiet = ref.render([36, 40, 43], [120, 110, 110], 1.0, 0.9, 0.0, 120_000.0)
    assert not ref.ratio_is_assertable(quiet, ref.ABS_FLOOR_POLY)


def test_bars_add_over_the_voices(chord_refs):
    a, _ = chord_refs["ldr_19k"]
    F = ref.ABS_FLOOR_POLY
    sb = ref.separate_bar(a.voices, F)
    assert sb.shape == a.final.shape and (sb >= 3 * F).all()
    assert np.array_equal(ref.residual_bar(a, F), ref.final_bar(a.final, F) + sb)
    i = int(np.argmax(np.abs(a.voices[0])))
    assert sb[i] >= 1e-5 * np.abs(a.voices[0][i])


# ---- the Python mirror ------------------------------------------------------------------------------------------------------------
def _row(peak=0.5, residual_peak=1e-3, peak_db=(-38.36, -38.37, -96.64), rms_db=(-51.24, -51.25, -106.06)):
    from openwurli_amd import render_poly as rp
    r = np.zeros(1, dtype=rp.ROW_DTYPE)[0]
    r["peak"], r["residual_peak"], r["peak_db"], r["rms_db"] = peak, residual_peak, peak_db, rms_db
    r["intermod_ratio_db"] = rms_db[0] - rms_db[2]
    return r


def test_report_text_byte_for_byte():
    from openwurli_amd import render_poly as rp
    text = rp.format_report((38, 59, 62, 66), (45, 40), 3.0, 0.60, 1.0, _row(), "/tmp/x.wav")
    assert text == ("Polyphonic render complete\n"
                    '  Notes:     ["D2 (38)", "B3 (59)", "D4 (62)", "F#4 (66)"]\n'
                    "  Velocities: [45, 40, 40, 40]\n"
                    "  Duration:  3.0s\n"
                    "  Volume:    0.600 (audio taper: 0.360)\n"
                    "  Speaker:   1.0\n"
                    "  Peak:      -6.0 dBFS\n"
                    "\n"
                    "  === INTERMOD ANALYSIS (0.2-2.0s window) ===\n"
                    "  Shared chain (poly):  peak=-38.4 dBFS  rms=-51.2 dBFS\n"
                    "  Separate chains (sum): peak=-38.4 dBFS  rms=-51.2 dBFS\n"
                    "  Residual (intermod):  peak=-96.6 dBFS  rms=-106.1 dBFS\n"
                    "  Intermod ratio:       54.8 dB below signal\n"
                    "\n"
                    "  Verdict: OK — intermod present but likely inaudible\n"
                    "\n"
                    "  Output:    /tmp/x.wav\n"
                    "  Residual:  /tmp/x_residual.wav (normalized for listening)\n")
    one = rp.format_report([60], [], 0.25, 1.0, 0.0, _row(peak=0.0, peak_db=(-20.0, -20.0, -120.0), rms_db=(-30.0, -30.0, -120.0)), "out.wav").splitlines()
    assert one[1] == '  Notes:     ["C4 (60)"]' and one[2] == "  Velocities: [80]" and one[3] == "  Duration:  0.2s"      # 0.25 -> half to even
    assert one[6] == "  Peak:      -120.0 dBFS" and one[12] == "  Intermod ratio:       90.0 dB below signal" and one[14].startswith("  Verdict: CLEAN")


def test_velocity_padding_note_names_and_list_parsing():
    from openwurli_amd import render_poly as rp
    assert rp.pad_velocities([1, 2, 3, 4], [45, 40]) == [45, 40, 40, 40]
    assert rp.pad_velocities([1, 2], [9, 8, 7]) == [9, 8] and rp.pad_velocities([1, 2], []) == [80, 80]
    assert [rp.midi_note_name(n) for n in (0, 21, 33, 60, 61, 96, 127)] == ["C-1", "A0", "A1", "C4", "C#4", "C7", "G9"]
    assert rp.parse_csv_u8("38, 59,x,300,-1,+7,,62") == [38, 59, 7, 62]
    c = rp.make_chord((38, 59, 62), (45,), 0.5, 0.25, 19_000.0, True)[0]
    assert c["n_notes"] == 3 and c["no_poweramp"] == 1 and list(c["notes"][:4]) == [38, 59, 62, 0] and list(c["velocities"][:4]) == [45, 45, 45, 0]
    assert (c["volume"], c["speaker"], c["r_ldr"]) == (0.5, 0.25, 19_000.0)
    g = rp.dyad_grid(33, 96)
    assert g.size == 2016 and (g["n_notes"] == 2).all() and list(g["notes"][0, :2]) == [33, 34] and list(g["notes"][-1, :2]) == [95, 96]
    rows = np.zeros(2, dtype=rp.ROW_DTYPE)
    rows["intermod_ratio_db"] = [54.825, -0.004]
    assert rp.format_grid_csv(g[:2], rows) == "note_a,note_b,vel_a,vel_b,intermod_ratio_db\n33,34,80,80,54.83\n33,35,80,80,-0.00\n"
    assert rp.samples(3.0) == 132300 and rp.samples(0.2) == 8820 and rp.samples(-1.0) == 0


def test_verdict_boundaries():
    from openwurli_amd import render_poly as rp
    up = lambda x: math.nextafter(x, math.inf)
    assert rp.verdict(up(60.0)).startswith("CLEAN") and rp.verdict(60.0).startswith("OK") and rp.verdict(up(40.0)).startswith("OK")
    assert rp.verdict(40.0).startswith("MARGINAL") and rp.verdict(up(20.0)).startswith("MARGINAL")
    assert rp.verdict(20.0).startswith("DIRTY") and rp.verdict(-5.0).startswith("DIRTY") and rp.verdict(math.nan).startswith("DIRTY")
    assert rp.verdict(61.0) == "CLEAN — intermod negligible" and rp.verdict(0.0) == "DIRTY — intermod clearly audible"


def test_wav_scales_and_files(hiplib_host, tmp_path):
    from openwurli_amd import render_poly as rp
    assert rp.wav_scales(1.4, 0.25, True) == (0.5, 2.0) and rp.wav_scales(1.4, 0.25, False) == (1.0, 2.0)
    assert rp.wav_scales(0.7, 1e-10, True) == (1.0, 1.0) and rp.wav_scales(0.5, 2e-10, True)[1] == 0.5 / 2e-10
    assert rp.residual_path("a.wav") == "a_residual.wav" and rp.residual_path("d.wav/a.wav") == "d_residual.wav/a_residual.wav"
    assert rp.residual_path("noext") == "noext"
    final = np.array([0.0, 1.4, -0.7, 0.35]); residual = np.array([0.0, 0.25, -0.125, 0.0625])
    out = str(tmp_path / "x.wav")
    assert rp.write_wavs(out, final, residual, 1.4, 0.25, True) == (0.5, 2.0)

    def pcm(path):
        b = open(path, "rb").read()
        d = b[b.index(b"data") + 8:]
        return [int.from_bytes(d[i:i + 3], "little", signed=True) for i in range(0, 12, 3)]
    mx = (1 << 23) - 1
    assert pcm(out) == [0, round(0.7 * mx), -round(0.35 * mx), round(0.175 * mx)]
    assert pcm(str(tmp_path / "x_residual.wav")) == [0, round(0.5 * mx), -round(0.25 * mx), round(0.125 * mx)]


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------
def test_restatement_row_is_the_bindings_row():
    from openwurli_amd import binding
    assert list(ref.ROW) == [f[0] for f in binding.OwPolyRow._fields_]      # which tests/test_abi_layout.py holds to the header's declarators


def _call(lib, chords, cfg, final=None, stride=0):
    from openwurli_amd import render_poly as rp
    rows = np.zeros(max(chords.size, 1), dtype=rp.ROW_DTYPE)
    return lib.ow_render_poly(chords.ctypes.data_as(C.c_void_p), chords.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p),
                              final.ctypes.data_as(C.c_void_p) if final is not None else None, None, None, stride)


def _refused(lib, chords, cfg, *needles, **kw):
    from openwurli_amd import binding
    lib.ow_clear_error()
    assert _call(lib, chords, cfg, **kw) < 0
    msg = binding.take_error(lib)
    assert msg.startswith("ow_render_poly: ") and all(s in msg for s in needles), msg


def test_struct_size_guards_refuse_before_device_work(hiplib):
    from openwurli_amd import binding, render_poly as rp
    ch = rp.make_chord(rp.DEFAULT_NOTES, rp.DEFAULT_VELOCITIES)
    for field, bad in (("struct_size", C.sizeof(binding.OwPolyCfg) - 4), ("chord_size", C.sizeof(binding.OwPolyChord) + 8)):
        cfg = binding.OwPolyCfg()
        setattr(cfg, field, bad)
        _refused(hiplib, ch, cfg, "ABI mismatch")


def test_bad_chords_are_refused(hiplib):
    from openwurli_amd import binding, render_poly as rp
    good = rp.make_chords([((60, 64), (90, 90)), (rp.DEFAULT_NOTES, rp.DEFAULT_VELOCITIES)])
    cfg = binding.OwPolyCfg()

    def bad(field, value, index=None):
        ch = good.copy()
        if index is None:
            ch[field][1] = value
        else:
            ch[field][1, index] = value
        return ch
    _refused(hiplib, bad("n_notes", 0), cfg, "chord 1", "n_notes 0")
    _refused(hiplib, bad("n_notes", 32), cfg, "chord 1", "n_notes 32", "1..31")
    _refused(hiplib, bad("notes", 32, 2), cfg, "chord 1", "note 32", "33..96")
    _refused(hiplib, bad("notes", 97, 0), cfg, "chord 1", "note 97")
    _refused(hiplib, bad("velocities", 128, 3), cfg, "chord 1", "velocity 128", "127")
    for v in (0.0, -1.0, math.nan, math.inf):
        _refused(hiplib, bad("r_ldr", v), cfg, "chord 1", "r_ldr", "finite positive")
    for f in ("volume", "speaker"):
        for v in (math.nan, math.inf, -math.inf):
            _refused(hiplib, bad(f, v), cfg, "chord 1", f, "finite")
    ch = good.copy()
    ch["notes"][1, 4] = 200                        # behind n_notes: not a note of the chord, not looked at
    ch["n_notes"][0] = 0
    _refused(hiplib, ch, cfg, "chord 0", "n_notes 0")


def test_bad_configurations_are_refused(hiplib):
    from openwurli_amd import binding, render_poly as rp
    ch = rp.make_chord(rp.DEFAULT_NOTES, rp.DEFAULT_VELOCITIES)
    for d in (0.2, 0.0, -1.0, math.nan, 1e9):      # 0.2 s = 8820 samples: the window [8820, 8820) is where the reference panics
        _refused(hiplib, ch, binding.OwPolyCfg(duration_s=d), "duration_s", "8820")
    buf = np.zeros(1000)
    _refused(hiplib, ch, binding.OwPolyCfg(duration_s=0.25), "stride", "11025", final=buf, stride=1000)
    _refused(hiplib, ch, binding.OwPolyCfg(preamp_kind=1), "OW_PREAMP_MELANGE12", "--ldr")
    _refused(hiplib, ch, binding.OwPolyCfg(power_amp_kind=1), "OW_POWER_AMP_MELANGE")
    _refused(hiplib, ch, binding.OwPolyCfg(preamp_kind=7), "preamp_kind")
    _refused(hiplib, ch, binding.OwPolyCfg(power_amp_kind=7), "power_amp_kind")
    with pytest.raises(binding.OwError, match="n_notes 0"):
        bad = ch.copy()
        bad["n_notes"] = 0
        rp.run_chords(bad, 0.25)
    with pytest.raises(ValueError):
        rp.make_chord(range(33, 65))


def test_empty_call_returns_the_sample_count(hiplib):
    from openwurli_amd import binding, render_poly as rp
    assert _call(hiplib, np.zeros(0, dtype=rp.CHORD_DTYPE), binding.OwPolyCfg(duration_s=0.25)) == 11025
    assert rp.run_chords(np.zeros(0, dtype=rp.CHORD_DTYPE), 3.0).size == 0
