#!/usr/bin/env python3
"""Generate tests/golden/residuals_golden.npz by running the REFERENCE's own ml/goertzel_utils.py, ml/extract_harmonics.py and
ml/compute_residuals.py, whose directory is the script's one argument (the reference tree is not part of this repository and is not
where the tests run, so its outputs travel as a fixture).  `soundfile` is
not installed; the modules only need it for load_audio, so an empty stub is registered before the import.

Inputs are seven seeded synthetic notes (decaying harmonic series + Gaussian noise) stored as int16 PCM; the tests divide by 32768,
which is exact in f64.  Stored per clip i:
  pcm{i}, meta{i} = [sr, midi, f0, velocity, length_s]
  gseg{i} [n, 3] (start, end, n_harmonics), gamp{i} [n, 8], gulp{i} [n, 8]    every extract_harmonics_goertzel call of the gold
        extraction in call order, its amplitudes, and their largest relative movement when the coefficient 2 cos(w) moves one ulp up or
        down (the reference's own loop, run with numpy's cos shifted by one ulp)
  fseg{i}, famp{i}, ffreq{i}                                                 the same for extract_harmonics_fft of the FFT extraction
  snr{i} [8], snr_hamp{i} [8], snr_noise{i} [8]                              measure_interharmonic_snr, its harmonic amplitudes and
        noise medians (1e-20 where the reference skips the band)
  gold_json{i}, fft_json{i}                                                  both feature dictionaries
  res_t{i}, res_m{i} [2, 11]                                                 compute_note_residual(gold | fft dictionary, model, snr)
and for the whole set: notes_json (the scored notes, tiers mixed), features_json (extract_all_harmonics' list), model_json, the
assembled dataset with and without the SNR cache, filter_stats_json.
The script asserts that no stored SNR lies within 1e-6 dB of the threshold, that no pair of dB values the anomaly test compares lies
within 1e-6 of a tie and that none of them lies within 1e-6 of a rounding boundary of the two printed decimals: device rounding cannot
flip a mask."""
import json
import os
import sys
import types

import numpy as np

sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
if len(sys.argv) < 2:
    sys.exit("usage: make_residuals_golden.py <the reference's ml/ directory>")
sys.path.insert(0, sys.argv[1])
import goertzel_utils as gu  # noqa: E402
import extract_harmonics as eh  # noqa: E402
import compute_residuals as cr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 44100

# (seed, midi, length_s, noise, velocity, tier, boost, level): boost = (harmonic, factor) or None; level scales the harmonic series
CLIPS = [(11, 40, 1.70, 1e-4, 100, "gold", None, 0.3),
         (12, 60, 0.90, 2e-3, 64, "silver", None, 0.3),
         (13, 72, 0.45, 1e-4, 127, "gold", (3, 6.0), 0.3),
         (14, 91, 0.30, 5e-4, 30, "bronze", None, 0.3),
         (15, 33, 0.26, 1e-4, 80, "gold", None, 0.3),
         (16, 96, 0.12, 1e-4, 110, "silver", None, 0.3),
         (17, 55, 0.60, 6e-2, 90, "gold", (3, 0.35), 0.05)]    # a quiet note with a weak H3, noise raised until H3's SNR falls below 10 dB


def synth(seed, midi, length_s, noise, boost, level, detune_cents=2.0):
    rng = np.random.default_rng(seed)
    n = int(round(length_s * SR))
    t = np.arange(n) / SR
    f0 = gu.midi_to_freq(midi) * 2.0 ** (detune_cents / 1200.0)
    x = np.zeros(n)
    for h in range(1, 11):
        if f0 * h >= SR / 2:
            break
        a = 0.6 / h ** 1.6 * rng.uniform(0.7, 1.0)
        if boost is not None and h == boost[0]:
            a *= boost[1]
        x += a * np.exp(-t * (1.5 + 0.8 * h)) * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28))
    x = level * x + noise * rng.standard_normal(n)
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


class Recorder:
    """Stands in for one of the reference's extraction functions inside a module that imported it by name."""

    def __init__(self, fn, audio):
        self.fn, self.audio, self.calls = fn, audio, []

    def __call__(self, segment, sr, f0, n_harmonics=8, *a, **k):
        out = self.fn(segment, sr, f0, n_harmonics, *a, **k)
        start = (segment.ctypes.data - self.audio.ctypes.data) // 8
        self.calls.append((int(start), int(start) + len(segment), int(n_harmonics), out))
        return out


class ShiftedCos:
    """numpy, but cos is one ulp off: what the module sees as `np`."""

    def __init__(self, up):
        self.to = np.inf if up else -np.inf

    def __getattr__(self, name):
        return getattr(np, name)

    def cos(self, w):
        return np.nextafter(np.cos(w), self.to)


class MedianLog:
    def __init__(self):
        self.values = []

    def __getattr__(self, name):
        return getattr(np, name)

    def median(self, a):
        self.values.append(float(np.median(a)))
        return np.median(a)


def pad8(v):
    out = np.zeros(8)
    out[:len(v)] = v
    return out


def clear_of_flips(feat, what):
    for name, w in feat["windows"].items():
        if w is None:
            continue
        db = w["amps_dB_rel_H1"]
        for h in range(1, 7):
            if db[h] is not None and db[h + 1] is not None:
                assert abs(db[h + 1] - db[h]) > 1e-6, (what, name, h, db)


def clear_of_rounding(calls, what, fft):
    """No dB value of a window call (8 harmonics) within 1e-6 dB of where round(x, 2) changes its answer."""
    for a, b, nh, res in calls:
        if nh != 8:
            continue
        x = gu.amps_to_dB(res[0] if fft else res) * 100.0
        assert np.all(np.abs(np.abs(x - np.floor(x)) - 0.5) > 1e-4), (what, a, b, x)


def main():
    out = {"n_clips": np.array([len(CLIPS)])}
    notes, snr_cache = [], {}
    for i, (seed, midi, length_s, noise, vel, tier, boost, level) in enumerate(CLIPS):
        pcm = synth(seed, midi, length_s, noise, boost, level)
        audio = pcm.astype(np.float64) / 32768.0
        f0 = float(gu.midi_to_freq(midi))
        note = {"id": f"clip_{i}", "onset_s": 0.0, "offset_s": len(pcm) / SR, "midi_note": midi, "isolation_tier": tier,
                "isolation_score": {"gold": 1.0, "silver": 0.6, "bronze": 0.3}[tier], "velocity_midi": vel, "source_file": f"clip_{i}.wav"}
        if i == 1:
            note["harmonic_mask"] = [True, True, True, True, False, True, True, False]
        notes.append(note)
        out[f"pcm{i}"] = pcm
        out[f"meta{i}"] = np.array([SR, midi, f0, vel, length_s], dtype=np.float64)

        # gold extraction, every Goertzel call recorded; then again with the coefficient one ulp up and down
        rec = Recorder(gu.extract_harmonics_goertzel, audio)
        eh.extract_harmonics_goertzel = rec
        gold = eh.extract_note_features(audio, SR, note, use_goertzel=True)
        eh.extract_harmonics_goertzel = gu.extract_harmonics_goertzel
        moved = np.zeros((len(rec.calls), 8))
        for up in (True, False):
            gu.np = ShiftedCos(up)
            for c, (a, b, nh, amps) in enumerate(rec.calls):
                shifted = gu.extract_harmonics_goertzel(audio[a:b], SR, f0, nh)
                moved[c] = np.maximum(moved[c], pad8(np.abs(shifted - amps) / amps))
            gu.np = np
        clear_of_rounding(rec.calls, (i, "gold"), False)
        out[f"gseg{i}"] = np.array([c[:3] for c in rec.calls], dtype=np.int64).reshape(-1, 3)
        out[f"gamp{i}"] = np.array([pad8(c[3]) for c in rec.calls]).reshape(-1, 8)
        out[f"gulp{i}"] = moved

        rec = Recorder(gu.extract_harmonics_fft, audio)
        eh.extract_harmonics_fft = rec
        fft = eh.extract_note_features(audio, SR, note, use_goertzel=False)
        eh.extract_harmonics_fft = gu.extract_harmonics_fft
        clear_of_rounding(rec.calls, (i, "fft"), True)
        out[f"fseg{i}"] = np.array([c[:3] for c in rec.calls], dtype=np.int64).reshape(-1, 3)
        out[f"famp{i}"] = np.array([pad8(c[3][0]) for c in rec.calls]).reshape(-1, 8)
        out[f"ffreq{i}"] = np.array([pad8(c[3][1]) for c in rec.calls]).reshape(-1, 8)
        out[f"gold_json{i}"] = np.array(json.dumps(gold))
        out[f"fft_json{i}"] = np.array(json.dumps(fft))
        for feat, what in ((gold, "gold"), (fft, "fft")):
            clear_of_flips(feat, (i, what))

        # SNR, its harmonic amplitudes and noise medians
        rec = Recorder(gu.extract_harmonics_fft, audio)
        log = MedianLog()
        cr.extract_harmonics_fft, cr.np = rec, log
        snr = cr.measure_interharmonic_snr(audio, SR, f0, 0.0, n_harmonics=8)
        cr.extract_harmonics_fft, cr.np = gu.extract_harmonics_fft, np
        hamp, noise_med = np.zeros(8), np.zeros(8)
        if rec.calls:
            a, b, _, (hamp, _) = rec.calls[0]
            axis = np.fft.rfftfreq(4 * (b - a), d=1.0 / SR)
            vals = iter(log.values)
            for h in range(8):
                nf = (h + 1.5) * f0
                skipped = nf >= SR / 2 - 100 or not np.any((axis >= nf * 0.99) & (axis <= nf * 1.01))
                noise_med[h] = 1e-20 if skipped else max(next(vals), 1e-20)
            assert next(vals, None) is None
            for h in range(8):
                want = 20.0 * np.log10(hamp[h] / noise_med[h]) if hamp[h] > 1e-20 and noise_med[h] > 1e-20 else np.nan
                assert (np.isnan(want) and np.isnan(snr[h])) or want == snr[h], (i, h, want, snr[h])
        assert not np.any(np.abs(snr[~np.isnan(snr)] - cr.SNR_THRESHOLD_DB) < 1e-6), (i, snr)
        out[f"snr{i}"], out[f"snr_hamp{i}"], out[f"snr_noise{i}"] = snr, hamp, noise_med
        snr_cache[note["id"]] = snr
        print(i, "midi", midi, "goertzel calls", len(out[f"gseg{i}"]), "snr", np.round(snr, 2), "ulp move %.1e..%.1e" % (
            moved[moved > 0].min() if np.any(moved > 0) else 0.0, moved.max() if moved.size else 0.0))

    # the model side: the reference's FFT features of a second, slightly different rendition of every note
    model = {}
    for i, (seed, midi, length_s, noise, vel, tier, boost, level) in enumerate(CLIPS):
        m_audio = synth(seed + 100, midi, max(length_s, 1.0), 1e-5, None, 0.3, detune_cents=0.0).astype(np.float64) / 32768.0
        feat = eh.extract_note_features(m_audio, SR, {"id": f"model_{i}", "onset_s": 0.0, "offset_s": len(m_audio) / SR, "midi_note": midi})
        model[f"{midi}_{cr.bucket_velocity(vel)}"] = feat
    out["model_json"] = np.array(json.dumps(model))
    for i in range(len(CLIPS)):
        pair = [cr.compute_note_residual(json.loads(str(out[f"{k}_json{i}"])), model[f"{CLIPS[i][1]}_{cr.bucket_velocity(CLIPS[i][4])}"], snr_cache[f"clip_{i}"])
                for k in ("gold", "fft")]
        out[f"res_t{i}"] = np.array([p[0] for p in pair])
        out[f"res_m{i}"] = np.array([p[1] for p in pair])

    # extract_all_harmonics' own list (gold by Goertzel, the rest by FFT) and the assembled dataset
    audio_of = {n["source_file"]: out[f"pcm{i}"].astype(np.float64) / 32768.0 for i, n in enumerate(notes)}
    eh.load_audio = lambda path: (audio_of[path], SR)
    features = eh.extract_all_harmonics(notes, min_tier="bronze", use_goertzel_for_gold=True)
    features = json.loads(json.dumps(features))                                # what compute_residuals.py reads back from harmonics.json
    out["notes_json"] = np.array(json.dumps(notes))
    out["features_json"] = np.array(json.dumps(features))
    for tag, cache in (("snr", snr_cache), ("nosnr", None)):
        inputs, targets, mask, weights, ids, stats = cr.assemble_dataset(features, model, cache)
        out[f"ds_{tag}_inputs"], out[f"ds_{tag}_targets"], out[f"ds_{tag}_mask"], out[f"ds_{tag}_weights"] = inputs, targets, mask, weights
        out[f"ds_{tag}_ids"] = np.array(json.dumps(ids))
        out[f"ds_{tag}_stats"] = np.array(json.dumps(stats))
        print(tag, "rows", len(ids), stats)
    h3 = out["snr6"][2]
    assert h3 < cr.SNR_THRESHOLD_DB, h3                                        # the clip that exercises the SNR mask
    path = os.path.join(HERE, "residuals_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
