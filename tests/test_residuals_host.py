"""Stage 5's bookkeeping without a device: bucket_velocity, detect_anomalous_harmonics, compute_note_residual and assemble_dataset of
openwurli_amd/residuals.py -- and their restatement in tests/harmonics_ref.py -- against the outputs of the reference's own Python stored
in tests/golden/residuals_golden.npz.  This is pure bookkeeping on given dictionaries, so equality is the bar.  Also the SNR window, the
report's text against hand-written lines, the npz the trainer reads, and the tool's flags."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import harmonics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "residuals_golden.npz"))


def _json(g, key):
    return json.loads(str(g[key]))


def test_bucket_velocity_and_anomalies():
    from openwurli_amd import residuals
    want = {1: 20, 27: 20, 28: 35, 42: 35, 43: 50, 57: 50, 58: 65, 72: 65, 73: 80, 87: 80, 88: 95, 102: 95, 103: 110, 118: 110, 119: 127, 127: 127}
    for v, b in want.items():
        assert residuals.bucket_velocity(v) == b == ref.bucket_velocity(v), v
    db = [0.0, -10.0, -8.0, -20.0, None, -5.0, -30.0, -29.0]
    assert residuals.detect_anomalous_harmonics(db) == {1, 6} == ref.anomalous(db)         # H3 > H2, H8 > H7; a None hides its neighbours
    assert residuals.detect_anomalous_harmonics([0.0, -3.0]) == set() == residuals.detect_anomalous_harmonics([])
    assert residuals.detect_anomalous_harmonics([0.0, -3.0, -3.0]) == set()                 # a tie is not an anomaly


def test_note_residuals_equal_reference(golden):
    from openwurli_amd import residuals
    model = _json(golden, "model_json")
    seen_masks = set()
    for i in range(int(golden["n_clips"][0])):
        midi, vel = int(golden[f"meta{i}"][1]), int(golden[f"meta{i}"][3])
        m = model[f"{midi}_{residuals.bucket_velocity(vel)}"]
        for k, key in enumerate(("gold_json", "fft_json")):
            real = _json(golden, f"{key}{i}")
            for fn in (residuals.compute_note_residual, ref.note_residual):
                t, mask = fn(real, m, golden[f"snr{i}"])
                assert np.array_equal(mask, golden[f"res_m{i}"][k]) and np.array_equal(t, golden[f"res_t{i}"][k], equal_nan=True), (i, key, fn)
            seen_masks.add(tuple(golden[f"res_m{i}"][k]))
    # the branches the clips reach: everything valid, the anomalous H3 taken out, the SNR taking H3 out, no window at all
    assert len(seen_masks) >= 4 and tuple([False] * 11) in seen_masks
    anomalous = _json(golden, "gold_json2")["windows"]["early_sustain"]["amps_dB_rel_H1"]
    assert anomalous[2] > anomalous[1] and not golden["res_m2"][0][1] and golden["res_m2"][0][0]
    assert golden["snr6"][2] < 10.0 and not golden["res_m6"][0][1]
    # without SNR data nothing is masked for SNR; a threshold of its own moves the mask
    real6 = _json(golden, "gold_json6")
    m6 = model[f"55_{residuals.bucket_velocity(90)}"]
    assert residuals.compute_note_residual(real6, m6, None)[1][1] and residuals.compute_note_residual(real6, m6, golden["snr6"], snr_threshold=5.0)[1][1]
    assert not residuals.compute_note_residual(real6, m6, golden["snr6"], snr_threshold=20.0)[1][0]


def test_assemble_dataset_equals_reference(golden, tmp_path):
    from openwurli_amd import residuals, mlp_train
    feats, model = _json(golden, "features_json"), _json(golden, "model_json")
    cache = {f"clip_{i}": golden[f"snr{i}"] for i in range(7)}
    for tag, snr_cache in (("snr", cache), ("nosnr", None)):
        inputs, targets, mask, weights, ids, stats = residuals.assemble_dataset(feats, model, snr_cache)
        for got, key in ((inputs, "inputs"), (targets, "targets"), (mask, "mask"), (weights, "weights")):
            assert got.dtype == golden[f"ds_{tag}_{key}"].dtype and np.array_equal(got, golden[f"ds_{tag}_{key}"]), (tag, key)
        assert ids == _json(golden, f"ds_{tag}_ids") and stats == _json(golden, f"ds_{tag}_stats")
        r = ref.assemble(feats, model, snr_cache)
        assert all(np.array_equal(a, b) for a, b in zip(r[:4], (inputs, targets, mask, weights))) and r[4] == ids
    assert inputs.dtype == np.float32 and mask.dtype == bool and "clip_5" not in ids          # the attack-only note has no target
    # unmatched notes are counted and left out; an empty result keeps the reference's shapes
    inputs, targets, mask, weights, ids, stats = residuals.assemble_dataset(feats, {}, None)
    assert stats["total_notes"] == 7 and stats["matched"] == 0 and inputs.shape == (0,) and ids == []
    path = residuals.save_npz(str(tmp_path / "out" / "ml_data"), *residuals.assemble_dataset(feats, model, cache)[:4])
    assert path.endswith(os.path.join("ml_data", "training_data.npz"))
    data = mlp_train.load_data(path)
    assert data.inputs.shape == (6, 2) and np.array_equal(data.mask, golden["ds_snr_mask"])


def test_snr_window_and_empty_calls():
    from openwurli_amd import residuals
    assert residuals.snr_window(44100, 44100.0, 0.0) == (2205, 8820) == ref.snr_window(44100, 44100.0)
    assert residuals.snr_window(5292, 44100.0, 0.0) == (2205, 5292)
    assert residuals.snr_window(2205 + 127, 44100.0, 0.0) is None and residuals.snr_window(44100, 44100.0, -1.0) is None
    assert residuals.snr_window(44100, 44100.0, -0.1) == (0, 4410)                            # a window that starts before the audio
    assert residuals.measure_interharmonic_snr_many([]).shape == (0, 8)
    short = residuals.measure_interharmonic_snr(np.zeros(2300), 44100.0, 440.0, 0.0)            # all-NaN without a device call
    assert short.shape == (8,) and np.all(np.isnan(short))
    assert residuals.load_audio_for_snr([{"id": "a", "source_file": "missing.wav", "f0": 440.0}], {}) == {}


def test_report_text_by_hand():
    from openwurli_amd import residuals
    inputs = np.array([[(40 - 21) / 87, 100 / 127.0], [(72 - 21) / 87, 64 / 127.0]], dtype=np.float32)
    targets = np.zeros((2, 11), dtype=np.float32)
    mask = np.zeros((2, 11), dtype=bool)
    targets[:, 0], mask[:, 0] = [1.5, -2.5], True
    targets[0, 5], mask[0, 5] = 0.98, True
    targets[1, 10], mask[1, 10] = 1.25, True
    weights = np.array([1.0, 0.6], dtype=np.float32)
    stats = {"total_notes": 3, "matched": 2, "h2_freq_valid": 2, "h3_freq_valid": 0, "h2_decay_valid": 1, "ds_valid": 1}
    text = residuals.format_dataset_summary(inputs, targets, mask, weights, ["obm_c2", "clip_1"], stats)
    want = ["", "Dataset: 2 observations", "", "  SNR Filtering Summary:", "    Total notes examined:  3", "    Model-matched:         2",
            "    H2 freq valid:         2/2", "    H3 freq valid:         0/2", "    H2 decay valid:        1/2", "    ds_correction valid:   1/2",
            "    H4-H6 targets:         masked (below OBM noise floor)", "", "  MIDI range: 40 - 72", "  Velocity range: 64 - 100",
            "  gold: 1", "  silver: 1", "  bronze: 0", "", "  Target coverage:",
            "         freq_H2:     2/2 valid  mean=  -0.50  std=  2.00  range=[  -2.50,   +1.50]",
            "         freq_H3:     0/2 valid  (fully masked)"]
    lines = text.splitlines()
    assert lines[:len(want)] == want
    assert lines[24] == "        decay_H2:     1/2 valid  mean=  +0.98  std=  0.00  range=[  +0.98,   +0.98]"
    assert lines[29] == "         ds_corr:     1/2 valid  mean=  +1.25  std=  0.00  range=[  +1.25,   +1.25]"
    assert lines[30:] == ["", "  Per-note OBM residuals (valid targets only):",
                          "          obm_c2 (MIDI 40): freq_H2=    +1.5 ¢  decay_H2=    0.98  ds=  MASKED"]
    assert "Per-note OBM" not in residuals.format_dataset_summary(inputs, targets, mask, weights, ["a", "b"], stats)
    table = residuals.format_snr_table([{"id": "clip_4"}, {"id": "none"}], {"clip_4": np.array([np.nan, 49.84, 51.87, 9.96, 1.0])})
    assert table == "\n  Per-harmonic SNR (dB):\n          Note      H1      H2      H3      H4\n        clip_4     nan    49.8    51.9    10.0\n"


def test_tool_flags_and_text(golden, monkeypatch, tmp_path):
    from openwurli_amd import residuals
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compute_residuals as tool
    feats, model = _json(golden, "features_json"), _json(golden, "model_json")
    (tmp_path / "h.json").write_text(json.dumps(feats))
    (tmp_path / "m.json").write_text(json.dumps(model))
    seen = {}

    def fake(feats_, audio, device=0):
        seen["snr"] = (len(feats_), sorted(audio), device)
        return {f"clip_{i}": golden[f"snr{i}"] for i in range(7)}
    monkeypatch.setattr(residuals, "load_audio_for_snr", fake)
    buf = io.StringIO()
    with redirect_stdout(buf):
        path = tool.main(["--real", str(tmp_path / "h.json"), "--model", str(tmp_path / "m.json"), "--output-dir", str(tmp_path / "d"), "--snr-threshold", "12",
                          "--device", "3"])
    assert seen["snr"] == (7, [], 3)                                                           # the clips' files do not exist here
    text = buf.getvalue()
    assert text.startswith("Real observations: 7\nModel note/vel combos: 7\n\nComputing inter-harmonic SNR (threshold: 12 dB)...\n  SNR computed for 7 notes\n")
    assert "        clip_4     nan    49.8    51.9    49.2\n" in text and "\nDataset: 6 observations\n" in text
    assert text.endswith(f"\nSaved to {path}\n  inputs:  (6, 2)\n  targets: (6, 11)\n  mask:    (6, 11)\n  weights: (6,)\n")
    d = np.load(path)
    assert np.array_equal(d["mask"], golden["ds_snr_mask"]) and np.array_equal(d["targets"], golden["ds_snr_targets"])   # the flag moves the text only
    seen.clear()
    with redirect_stdout(io.StringIO()) as out:
        path = tool.main(["--real", str(tmp_path / "h.json"), "--model", str(tmp_path / "m.json"), "--output-dir", str(tmp_path / "e"), "--no-snr-filter"])
    assert not seen and "\nSNR filtering DISABLED (--no-snr-filter)\n" in out.getvalue()
    assert np.array_equal(np.load(path)["mask"], golden["ds_nosnr_mask"])
