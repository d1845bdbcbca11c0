"""GPU parity of the inter-harmonic noise floor (ow_interharmonic_noise, k_feat_band_median) and of stages 3 and 5 end to end
(openwurli_amd/harmonics.py, openwurli_amd/residuals.py) on the fixture clips of tests/golden/residuals_golden.npz.

Noise medians: the bar of tests/test_gpu_features.py -- 1e-10 relative, with a floor of 1e-13 of the strongest harmonic of the segment
(a magnitude that far below the fundamental is mostly its leakage: the device's direct summation and numpy's FFT both carry an error
proportional to the whole signal) -- against the reference's own medians and against the numpy restatement."""
import json
import ctypes as C
import os
import sys

import numpy as np
import pytest

import harmonics_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import features_oracle as fo  # noqa: E402

SR = 44100.0
AMP_REL = 1e-10


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "residuals_golden.npz"))


@pytest.fixture(scope="module")
def rows(golden):
    n = int(golden["n_clips"][0])
    out = np.zeros((n, max(len(golden[f"pcm{i}"]) for i in range(n))))
    for i in range(n):
        out[i, :len(golden[f"pcm{i}"])] = golden[f"pcm{i}"] / 32768.0
    return out


@pytest.fixture
def dev_rows(hiplib, rows):
    """The same matrix in a device buffer."""
    dev = hiplib.ow_device_alloc(rows.nbytes, 0)
    assert dev and hiplib.ow_test_device_write(C.c_void_p(dev), rows.ctypes.data_as(C.c_void_p), rows.nbytes, 0) == 0
    yield dev
    hiplib.ow_device_free(dev, 0)


def amp_tol(values, peak):
    return np.maximum(AMP_REL * np.abs(values), 1e-13 * peak)


def close_noise(got, want, peak):
    skipped = want == 1e-20
    assert np.array_equal(got[skipped], want[skipped])
    assert np.all(np.abs(got[~skipped] - want[~skipped]) <= amp_tol(want[~skipped], peak)), (got, want, peak)


def test_noise_medians(hiplib, golden, rows, dev_rows):
    from openwurli_amd import features
    # the reference's own windows, then windows of other lengths and harmonic counts: bands of one bin and of hundreds, odd and even counts,
    # bands past the cut and bands without a bin
    segs = [(i, 2205, min(8820, len(golden[f"pcm{i}"])), 8, golden[f"meta{i}"][2]) for i in range(7)]
    segs += [(0, 8820, 35280, 8, golden["meta0"][2]), (5, 100, 229, 8, golden["meta5"][2]), (3, 0, 2205, 3, golden["meta3"][2]), (2, 7, 4418, 8, 4186.0),
             (4, 0, 11466, 1, golden["meta4"][2]), (6, 0, 2205, 0, golden["meta6"][2]), (2, 2205, 8820, 8, 2793.8), (0, 8820, 35280, 8, 2093.0)]
    noise = features.noise_segments(rows, SR, segs)
    counts = set()
    for k, (r, a, b, nh, f0) in enumerate(segs):
        x = rows[r, a:b]
        peak = np.max(fo.extract_harmonics(x, SR, f0, max(nh, 1))[0])
        close_noise(noise[k, :nh], ref.noise_medians(x, SR, f0, nh), peak)
        assert np.all(noise[k, nh:] == 0.0)
        if k < 7:
            close_noise(noise[k], golden[f"snr_noise{k}"], peak)
        counts |= {None if band is None else band[1] - band[0] + 1 for band in ref.noise_bands(b - a, SR, f0, nh)}
    sizes = {c for c in counts if c is not None}
    assert None in counts and 1 in sizes and max(sizes) > 256 and {c % 2 for c in sizes} == {0, 1}
    assert golden["snr_noise4"][0] == 1e-20 and noise[4, 0] == 1e-20          # MIDI 33: no bin in the band at 82.5 Hz
    # audio that is already on the device, and the 24-bit quantisers: the same medians as the host path / as the restatement on quantised audio
    assert np.array_equal(features.noise_segments(None, SR, segs, device_audio=(dev_rows, rows.shape[0], rows.shape[1])), noise)
    q = features.noise_segments(rows, SR, segs[:7], wav24="round")
    for k, (r, a, b, nh, f0) in enumerate(segs[:7]):
        x = fo.quantize_round(rows[r, a:b]) / 8388608.0
        close_noise(q[k], ref.noise_medians(x, SR, f0, nh), np.max(fo.extract_harmonics(x, SR, f0, nh)[0]))


def test_snr_and_its_masks(hiplib, golden, rows):
    """measure_interharmonic_snr of the seven clips in one batch: the NaN pattern and the side of the 10 dB threshold as in the reference
    (the fixture keeps every value 1e-6 dB away from it).  Values: an amplitude within rel of its reference moves 20 log10 by
    20 / ln 10 * rel, so the bar per entry is 8.686 * (rel_h + rel_n), rel = max(1e-10, 1e-13 * peak / value), with 1 % of slack for the
    linearisation."""
    from openwurli_amd import residuals
    items = [(golden[f"pcm{i}"] / 32768.0, SR, golden[f"meta{i}"][2], 0.0) for i in range(7)]
    snr = residuals.measure_interharmonic_snr_many(items)
    for i in range(7):
        want = golden[f"snr{i}"]
        assert np.array_equal(np.isnan(snr[i]), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(snr[i][ok] < residuals.SNR_THRESHOLD_DB, want[ok] < residuals.SNR_THRESHOLD_DB)
        h, n = golden[f"snr_hamp{i}"], golden[f"snr_noise{i}"]
        peak = np.max(h)
        bar = 1.01 * 20.0 / np.log(10.0) * (amp_tol(h, peak) / h + amp_tol(n, peak) / n)
        print(i, "snr error / bar:", np.nanmax(np.abs(snr[i][ok] - want[ok]) / bar[ok]))
        assert np.all(np.abs(snr[i][ok] - want[ok]) <= bar[ok]), (i, snr[i], want, bar)
    one = residuals.measure_interharmonic_snr(items[6][0], SR, items[6][2], 0.0)
    assert np.array_equal(one, snr[6], equal_nan=True)
    assert np.all(np.isnan(residuals.measure_interharmonic_snr(items[0][0][:2300], SR, items[0][2], 0.0)))      # fewer than 128 samples in the window


def half_step_equal(a, b, step):
    assert [x is None for x in a] == [x is None for x in b]
    assert np.allclose([x for x in a if x is not None], [x for x in b if x is not None], rtol=0, atol=1.01 * step), (a, b)


def test_stages_3_and_5_end_to_end(hiplib, golden, tmp_path):
    """extract_all_harmonics on the seven clips (gold notes by Goertzel, the others by FFT) against the reference's own list: the
    pattern of None identical, frequencies equal (peak bins, or the nominal h * f0), the rounded numbers within half a rounding step
    more than their own step, as tests/test_gpu_features.py compares them.  From those features, assemble_dataset against the stored
    model features: masks, inputs and weights equal; targets within what one rounding flip of an input can do:
      * frequency offsets 1200 log2(rf / mf): rf and mf are compared for equality above, so these are equal;
      * decay ratios t = (rs / re) / (ms / me): the recording's re and rs may each sit one step of 1e-8 off, which moves t by at most
        t * (1e-8 / re + 1e-8 / rs) to first order (1 % of slack for the higher orders);
      * the displacement-scale correction t = 2^((r2 - m2) / 6): r2 may sit one step of 0.01 dB off: t * (2^(0.01 / 6) - 1);
      * and the float32 the targets are stored as: one float32 ulp, 2^-23 |t|, where the flip crosses a float32 rounding boundary."""
    from openwurli_amd import harmonics, residuals, mlp_train
    notes = json.loads(str(golden["notes_json"]))
    want = json.loads(str(golden["features_json"]))
    audio = {n["source_file"]: (golden[f"pcm{i}"] / 32768.0, 44100) for i, n in enumerate(notes)}
    got = harmonics.extract_all_harmonics(notes, audio, min_tier="bronze", use_goertzel_for_gold=True)
    assert len(got) == len(want) == 7
    for f, r, note in zip(got, want, notes):
        assert list(f) == list(r)
        for key in ("id", "midi_note", "f0", "duration_s", "isolation_tier", "isolation_score", "velocity_midi", "source_file"):
            assert f[key] == r[key], key
        for name in ("attack", "early_sustain", "sustain"):
            a, b = f["windows"][name], r["windows"][name]
            assert (a is None) == (b is None)
            if a is not None:
                assert a["freqs_hz"] == b["freqs_hz"]
                half_step_equal(a["amps_linear"], b["amps_linear"], 1e-8)
                half_step_equal(a["amps_dB_rel_H1"], b["amps_dB_rel_H1"], 0.01)
        assert f["decay"]["times_s"] == r["decay"]["times_s"]
        half_step_equal(f["decay"]["h1_amps"], r["decay"]["h1_amps"], 1e-8)
        half_step_equal([f["decay"]["decay_rate_dB_s"]], [r["decay"]["decay_rate_dB_s"]], 0.01)
        half_step_equal([f["overshoot_dB"]], [r["overshoot_dB"]], 0.01)
        for name in ("attack", "sustain"):
            half_step_equal([f[f"centroid_{name}"]], [r[f"centroid_{name}"]], 0.1)
    assert got[1]["windows"]["attack"]["amps_linear"][4] is None                 # the harmonic_mask of clip 1
    gold_fft = harmonics.extract_note_features(audio["clip_0.wav"][0], 44100, notes[0], use_goertzel=False)
    assert gold_fft["windows"]["attack"]["amps_linear"][0] == 0.0 != got[0]["windows"]["attack"]["amps_linear"][0]   # FFT: no bin in H1's band, 1e-20

    model = json.loads(str(golden["model_json"]))
    feats = json.loads(json.dumps(got))                                          # through the file format, as the tools pass them on
    cache = residuals.load_audio_for_snr(feats, audio)
    assert sorted(cache) == [f"clip_{i}" for i in range(7)]
    for tag, snr_cache in (("snr", cache), ("nosnr", None)):
        inputs, targets, mask, weights, ids, stats = residuals.assemble_dataset(feats, model, snr_cache)
        assert inputs.dtype == targets.dtype == weights.dtype == np.float32 and mask.dtype == bool
        assert np.array_equal(mask, golden[f"ds_{tag}_mask"]) and np.array_equal(inputs, golden[f"ds_{tag}_inputs"])
        assert np.array_equal(weights, golden[f"ds_{tag}_weights"])
        assert ids == json.loads(str(golden[f"ds_{tag}_ids"])) and stats == json.loads(str(golden[f"ds_{tag}_stats"]))
        t_want = golden[f"ds_{tag}_targets"]
        by_id = {f["id"]: f for f in want}
        for row, nid in enumerate(ids):
            assert np.array_equal(targets[row, :residuals.N_FREQ], t_want[row, :residuals.N_FREQ])
            early, sus = by_id[nid]["windows"]["early_sustain"], by_id[nid]["windows"]["sustain"]
            for h in range(2):
                t = float(t_want[row, residuals.N_FREQ + h])
                if mask[row, residuals.N_FREQ + h]:
                    slack = 1.01 * abs(t) * (1e-8 / early["amps_linear"][h + 1] + 1e-8 / sus["amps_linear"][h + 1]) + 2.0 ** -23 * abs(t)
                    assert abs(float(targets[row, residuals.N_FREQ + h]) - t) <= slack, (tag, nid, h)
                else:
                    assert targets[row, residuals.N_FREQ + h] == 0.0
            t = float(t_want[row, residuals.DS_IDX])
            assert abs(float(targets[row, residuals.DS_IDX]) - t) <= abs(t) * (2.0 ** (0.01 / 6.0) - 1.0) + 2.0 ** -23 * abs(t), (tag, nid)
            assert np.all(targets[row, residuals.N_FREQ + 2:residuals.DS_IDX] == 0.0)
    assert not np.array_equal(golden["ds_snr_mask"], golden["ds_nosnr_mask"])    # the SNR mask takes something away
    path = residuals.save_npz(str(tmp_path / "ml_data"), inputs, targets, mask, weights)
    data = mlp_train.load_data(path)
    assert data.inputs.shape == (6, 2) and data.mask.shape == (6, 11) and np.array_equal(data.mask, mask)
