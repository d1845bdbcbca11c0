"""Host side of openwurli_amd.wurli_compare (the reference's tools/wurli_compare.py): the float32 restatement reproduces what the
reference itself returned on the committed fixtures (tests/golden/make_wurli_compare_golden.py), the float64 restatement (the device's
contract) rounds to the same report, and the script's bookkeeping -- selection, velocity mapping, render flags, file names, truthiness
quirks, report texts -- is checked without a device.

The fixtures' float32 -> float64 movement, per class of figure, is stored in the golden as `movement` (has the
table); the GPU test bounds the device by it."""
import json
import os

import numpy as np
import pytest

import wurli_compare_ref as ref
from openwurli_amd import wurli_compare as wc


def _entries(g, comps):
    return [dict(e, comparison=c) for e, c in zip(g["comparisons"], comps)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_rounds_to_the_reference_report(dtype):
    """Every rounded figure of the reference's compare_note, and its report text, from both forms of the restatement."""
    g, _ = ref.load_golden()
    comps = [wc.comparison_from_figures(a, b, e["f0_hz"]) for (a, b), e in zip(ref.golden_figures(dtype), g["comparisons"])]
    for got, e in zip(comps, g["comparisons"]):
        assert json.loads(json.dumps(got)) == e["comparison"], e["note_name"]
    assert wc.format_comparison_report(_entries(g, comps), "OUT") == g["report_text"]


def test_both_forms_pick_the_same_bins_and_attack_frame():
    for (a32, b32), (a64, b64) in zip(ref.golden_figures(np.float32), ref.golden_figures(np.float64)):
        for x, y in ((a32, a64), (b32, b64)):
            assert x["bins"] == y["bins"] and x["attack_frame"] == y["attack_frame"] and x["attack_frame"] is not None


def test_stored_movement_is_the_restatements():
    g, _ = ref.load_golden()
    f32, f64 = ref.golden_figures(np.float32), ref.golden_figures(np.float64)
    m = ref.movement([s for p in f32 for s in p], [s for p in f64 for s in p])
    assert set(m) == set(ref.CLASSES) == set(g["movement"])
    for c in ref.CLASSES:
        assert m[c] == g["movement"][c], c
    # float32 carries 2^-24: the movement stays near that, far above float64's own rounding and far below a report digit
    assert 0.0 < m["ratio"] < 1e-5 and 0.0 < m["db"] < 1e-4 and 0.0 < m["centroid"] < 0.5 and m["attack"] == 0.0 and 0.0 < m["rms"] < 1e-4


def test_selection_and_summary(tmp_path, capsys):
    g, _ = ref.load_golden()
    dirs = []
    for d, notes in g["meta"].items():
        os.makedirs(tmp_path / d)
        dirs.append(str(tmp_path / d))
        with open(tmp_path / d / "extraction_metadata.json", "w") as f:
            json.dump({"notes": [{"note_name": n, "midi_note": m, "isolation_score": iso, "velocity_norm": v, "duration": du,
                                  "f0_hz": 440.0 * 2.0 ** ((m - 69) / 12.0), "filename": f"{d}_{n}_{k}.wav"}
                                 for k, (n, m, iso, v, du) in enumerate(notes)]}, f)
    for key, (top, names) in {"top1": (1, None), "top2": (2, None), "named": (3, ["C4", "F5"])}.items():
        sel = wc.select_best_notes(wc.load_extractions(dirs), top, names)
        assert [[midi, [n["filename"] for n in notes]] for midi, notes in sel.items()] == g["selections"][key], key
    all_notes = wc.load_extractions(dirs + [str(tmp_path / "missing")])
    assert "WARNING: No metadata in" in capsys.readouterr().err
    assert all_notes[0]["_wav_path"] == os.path.join(dirs[0], all_notes[0]["filename"])
    wc.print_summary(all_notes)
    assert capsys.readouterr().out == g["summary_text"]


def test_velocity_flags_and_names():
    assert [wc.velocity_midi({"velocity_norm": v}) for v in (0.0, 0.004, 0.5, 0.999, 1.0, 7.0)] == [1, 1, 63, 126, 127, 127]
    assert wc.velocity_midi({"velocity_norm": 0.5}, 90) == 90 and wc.velocity_midi({"velocity_norm": 0.5}, 0) == 63     # --velocity 0 is falsy
    assert wc.render_job(60, 100) == {"note": 60, "velocity": 100, "mlp": True, "poweramp": False, "volume": 1.0, "speaker": 0.0}
    assert wc.render_job(60, 100, tier3=True) == {"note": 60, "velocity": 100, "mlp": True, "poweramp": True, "volume": 0.40, "speaker": 1.0}
    assert wc.wav_names("C#4", 0, 1) == ("Cs4_real.wav", "Cs4_synth.wav") and wc.wav_names("B♭3", 2, 3) == ("Bb3_2_real.wav", "Bb3_2_synth.wav")
    assert wc.wav_names("F♯2", 1, 2)[1] == "Fs2_1_synth.wav"


def test_plan_follows_the_scripts_loop(tmp_path):
    notes = [{"note_name": "C4", "midi_note": 60, "isolation_score": 0.9, "velocity_norm": 0.5, "duration": 0.2, "f0_hz": 261.6, "filename": "a.wav"},
             {"note_name": "C4", "midi_note": 60, "isolation_score": 0.8, "velocity_norm": 0.7, "duration": 1.25, "f0_hz": 261.6, "filename": "b.wav"},
             {"note_name": "C8", "midi_note": 108, "isolation_score": 0.7, "velocity_norm": 0.7, "duration": 0.7, "f0_hz": 4186.0, "filename": "c.wav"},
             {"note_name": "D4", "midi_note": 62, "isolation_score": 0.6, "velocity_norm": 0.7, "duration": 0.7, "f0_hz": 293.7, "filename": "gone.wav"}]
    for n in notes:
        n["_source_dir"] = str(tmp_path); n["_wav_path"] = str(tmp_path / n["filename"])
        if n["filename"] != "gone.wav":
            wc.write_wav16(n["_wav_path"], np.zeros(8), 44100)
    plan = wc.plan_run(wc.select_best_notes(notes, 2), 2, "out")
    assert [p["head"] for p in plan] == ["  [1/4] C4 (MIDI 60, iso=0.90)...", "  [2/4] C4 (MIDI 60, iso=0.80)...", "  [3/4] D4 (MIDI 62, iso=0.60)...",
                                         "  [4/4] C8 (MIDI 108, iso=0.70)..."]
    assert [p["missing"] for p in plan] == [False, False, True, False]         # D4: the script's SKIP (wav missing)
    plan = [p for p in plan if not p["missing"]]
    assert [p["duration"] for p in plan] == [0.5, 1.25, 0.7]                   # max(0.5, duration)
    assert [os.path.basename(p["synth_wav"]) for p in plan] == ["C4_0_synth.wav", "C4_1_synth.wav", "C8_0_synth.wav"]
    assert plan[0]["job"]["velocity"] == 63 and plan[2]["job"] is None         # MIDI 108: the reference's RENDER FAILED
    e = wc.result_entry(plan[1], {"harmonic_distance_db": None})
    assert list(e) == ["note_name", "midi_note", "f0_hz", "isolation", "velocity_norm", "velocity_midi", "duration", "source", "real_wav", "synth_wav",
                       "comparison"] and e["source"] == tmp_path.name and e["velocity_midi"] == 88


def _fig(decay=-10.0, centroid=900.0, amps=(1.0, 0.5)):
    return {"amps": list(amps), "bins": [10, 20], "decay": decay, "centroid": centroid, "attack_frame": 3, "attack_ms": 3 * 128 / 44100 * 1000, "rms_db": -20.04}


def test_truthiness_quirks():
    c = wc.comparison_from_figures(_fig(decay=0.04), _fig(decay=-12.0), 100.0)          # rounds to exactly 0.0: falsy, no difference
    assert c["decay_real_db_s"] == 0.0 and c["decay_diff_db_s"] is None
    c = wc.comparison_from_figures(_fig(centroid=0.0), _fig(), 100.0)
    assert c["centroid_diff_hz"] is None
    c = wc.comparison_from_figures(_fig(), _fig(decay=None), 100.0)
    assert c["decay_synth_db_s"] is None and c["decay_diff_db_s"] is None
    c = wc.comparison_from_figures(_fig(amps=(1e-11, 0.5)), _fig(), 100.0)              # H1 below 1e-10: no profile, no distance
    assert c["harmonics_real"] is None and c["harmonic_distance_db"] is None and c["harmonic_diffs_db"] is None
    c = wc.comparison_from_figures(_fig(), _fig(), 100.0)
    assert c["harmonic_distance_db"] == 0.0 and c["harmonic_diffs_db"] == [0.0] and c["attack_real_ms"] == 8.7 and c["rms_real_db"] == -20.0
    progress_tail = wc.progress_tail
    assert progress_tail(0.0) == "n/a" and progress_tail(None) == "n/a" and progress_tail(3.25) == "dist=3.2dB"


def test_pcm16_rule_and_wav_round_trip(tmp_path):
    y = np.array([0.0, 1.0, -1.0, 0.5, 1.5, -2.0, 1.5 / 32767.0, 2.5 / 32767.0, 0.25 + 1e-9])
    q = wc.pcm16_roundtrip(y) * 32768.0
    assert q.tolist() == [0.0, 32767.0, -32767.0, 16384.0, 32767.0, -32768.0, 2.0, 2.0, 8192.0]      # lrint: half to even; clipped
    wc.write_wav16(tmp_path / "a.wav", y, 44100)
    assert wc.read_wav(tmp_path / "a.wav").tolist() == wc.pcm16_roundtrip(y).tolist()
    assert wc.load_real(tmp_path / "a.wav").tolist() == wc.pcm16_roundtrip(wc.pcm16_roundtrip(y)).tolist()


def test_sustain_slices():
    assert wc.sustain_slices(26460, 26460) == ((3528, 22932), (3528, 22932))
    assert wc.sustain_slices(100000, 60000) == ((3528, 44100), (3528, 44100))
    assert wc.sustain_slices(3528, 50000) == ((0, 3528), (3528, 3528))            # a clip of 80 ms or less is taken whole
    assert wc.sustain_slices(4000, 3000) == ((3528, 472), (0, 3000))
    for n_r, n_s in ((26460, 26460), (3528, 50000), (4000, 3000), (0, 10)):
        a, b = np.arange(n_r), np.arange(n_s)
        sa, sb = ref.slices(a, b)
        (r0, rn), (s0, sn) = wc.sustain_slices(n_r, n_s)
        assert a[r0:r0 + rn].tolist() == sa.tolist() and b[s0:s0 + sn].tolist() == sb.tolist()


def test_rank_rows():
    comps = [[{"harmonic_distance_db": 3.0, "decay_diff_db_s": 1.0, "centroid_diff_hz": -10.0},
              {"harmonic_distance_db": 9.0, "decay_diff_db_s": None, "centroid_diff_hz": 30.0},
              {"harmonic_distance_db": None, "decay_diff_db_s": 2.0, "centroid_diff_hz": None}], []]
    rows = wc.rank_rows(["a"], [2, 3], comps)
    assert rows[0] == {"weights": "a", "tier": 2, "n_notes": 3, "harm_dist_mean_db": 6.0, "harm_dist_median_db": 6.0, "harm_dist_worst_db": 9.0,
                       "decay_diff_mean_db_s": 1.5, "centroid_diff_mean_hz": 10.0}
    assert rows[1]["tier"] == 3 and rows[1]["harm_dist_mean_db"] is None and rows[1]["n_notes"] == 0
