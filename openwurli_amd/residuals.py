"""Host mirror of stage 5 of the ML loop, `ml/compute_residuals.py`: residuals (recording - model) and the training set.

The measuring part, `measure_interharmonic_snr`, runs on the GPU for all notes at once: the harmonic amplitudes through
`ow_extract_harmonics`, the noise floor between the harmonics through `ow_interharmonic_noise`.  The rest is the script's bookkeeping,
kept as it is there: the v2 target layout (5 frequency offsets in cents, 5 decay ratios, 1 displacement-scale correction), the SNR and
anomaly masks, the arrays as float32 / bool.  No CPU fallback.
"""
import math
import os

import numpy as np

from . import features

N_HARMONICS = 8
N_FREQ, N_DECAY = 5, 5
N_TARGETS = N_FREQ + N_DECAY + 1
DS_IDX = N_FREQ + N_DECAY
TIER_WEIGHTS = {"gold": 1.0, "silver": 0.6, "bronze": 0.3}
SNR_THRESHOLD_DB = 10.0
MAX_RELIABLE_HARMONIC = 2                       # only the H2 and H3 targets are ever valid
VELOCITY_BUCKETS = [20, 35, 50, 65, 80, 95, 110, 127]      # render_model_notes.py:26


def bucket_velocity(velocity_midi):
    """render_model_notes.py:34-36: the nearest bucket, the lower one on a tie."""
    return min(VELOCITY_BUCKETS, key=lambda b: abs(b - velocity_midi))


def snr_window(n_audio, sr, onset_s, window_start=0.05, window_end=0.20):
    """Sample range measure_interharmonic_snr analyses, or None where it answers all-NaN (fewer than 128 samples)."""
    a, b = max(int((onset_s + window_start) * sr), 0), min(int((onset_s + window_end) * sr), n_audio)
    return (a, b) if b - a >= 128 else None


def measure_interharmonic_snr_many(items, n_harmonics=N_HARMONICS, window_start=0.05, window_end=0.20, device=0):
    """measure_interharmonic_snr (compute_residuals.py:59-127) of many notes in two GPU calls.  items: (audio, sr, f0, onset_s), one
    sample rate per call.  Returns snr_db [len(items), n_harmonics]; NaN where the harmonic or its noise floor is not above 1e-20."""
    items = list(items)
    snr = np.full((len(items), n_harmonics), np.nan)
    if not items:
        return snr
    sr = items[0][1]
    if any(it[1] != sr for it in items):
        raise ValueError("measure_interharmonic_snr_many: one sample rate per call")
    spans = [snr_window(len(it[0]), sr, it[3], window_start, window_end) for it in items]
    live = [j for j, w in enumerate(spans) if w is not None]
    if not live:
        return snr
    rows = np.zeros((len(live), max(spans[j][1] - spans[j][0] for j in live)))
    segs = []
    for r, j in enumerate(live):
        a, b = spans[j]
        rows[r, :b - a] = np.asarray(items[j][0][a:b], dtype=np.float64)
        segs.append((r, 0, b - a, n_harmonics, items[j][2]))
    h_amps, _, _ = features.extract_segments(rows, sr, segs, 0.01, device)
    noise = features.noise_segments(rows, sr, segs, device)
    for r, j in enumerate(live):
        for h in range(n_harmonics):
            if h_amps[r, h] > 1e-20 and noise[r, h] > 1e-20:
                snr[j, h] = 20.0 * np.log10(h_amps[r, h] / noise[r, h])
    return snr


def measure_interharmonic_snr(audio, sr, f0, onset_s, n_harmonics=N_HARMONICS, window_start=0.05, window_end=0.20, device=0):
    """Drop-in for compute_residuals.measure_interharmonic_snr."""
    return measure_interharmonic_snr_many([(audio, sr, f0, onset_s)], n_harmonics, window_start, window_end, device)[0]


def load_audio_for_snr(feats, audio_by_file, device=0):
    """load_audio_for_snr (compute_residuals.py:251-285) on audio in memory: note id -> snr_db, for every note whose source file is in
    audio_by_file[source_file] = (audio, sr).  The onset is 0.0 as there: the isolated-note files start at the note."""
    known = [f for f in feats if f.get("source_file", "") in audio_by_file]
    cache = {}
    for sr in sorted({audio_by_file[f["source_file"]][1] for f in known}):
        group = [f for f in known if audio_by_file[f["source_file"]][1] == sr]
        snr = measure_interharmonic_snr_many([(audio_by_file[f["source_file"]][0], sr, f["f0"], 0.0) for f in group], device=device)
        for f, row in zip(group, snr):
            cache[f.get("id", "")] = row
    return cache


def detect_anomalous_harmonics(real_dB):
    """compute_residuals.py:130-147: targets (0 = H2 ... ) whose harmonic is stronger than the one below it."""
    found = set()
    for h in range(1, min(len(real_dB) - 1, 7)):
        upper, lower = real_dB[h + 1], real_dB[h]
        if upper is not None and lower is not None and upper > lower:
            found.add(h)
    return found


def _below_threshold(snr_db, h_idx, threshold):
    return snr_db is not None and h_idx < len(snr_db) and (np.isnan(snr_db[h_idx]) or snr_db[h_idx] < threshold)


def compute_note_residual(real_feat, model_feat, snr_db=None, snr_threshold=SNR_THRESHOLD_DB):
    """compute_residuals.py:150-248: (targets [11] with NaN where invalid, mask [11])."""
    targets = np.full(N_TARGETS, np.nan)
    mask = np.zeros(N_TARGETS, dtype=bool)
    real_win, model_win = real_feat["windows"].get("early_sustain"), model_feat["windows"].get("early_sustain")
    if real_win is None or model_win is None:
        real_win, model_win = real_feat["windows"].get("sustain"), model_feat["windows"].get("sustain")
    if real_win is None or model_win is None:
        return targets, mask
    real_dB, model_dB = real_win["amps_dB_rel_H1"], model_win["amps_dB_rel_H1"]
    anomalous = detect_anomalous_harmonics(real_dB)

    for h in range(N_FREQ):                                  # frequency offsets of H2..H6, cents
        rf, mf = real_win["freqs_hz"][h + 1], model_win["freqs_hz"][h + 1]
        if rf is None or mf is None or rf <= 0 or mf <= 0:
            continue
        if h >= MAX_RELIABLE_HARMONIC or _below_threshold(snr_db, h + 1, snr_threshold) or h in anomalous:
            continue
        targets[h] = 1200.0 * math.log2(rf / mf)
        mask[h] = True

    wins = [f["windows"].get(w) for f in (real_feat, model_feat) for w in ("early_sustain", "sustain")]
    if all(w is not None for w in wins):                     # decay proxy: sustain / early-sustain amplitude, recording over model
        for h in range(min(MAX_RELIABLE_HARMONIC, N_DECAY)):
            re, rs, me, ms = (w["amps_linear"][h + 1] for w in wins)
            if re is None or rs is None or me is None or ms is None or not (re > 1e-12 and rs > 1e-12 and me > 1e-12 and ms > 1e-12):
                continue
            if _below_threshold(snr_db, h + 1, snr_threshold) or h in anomalous:
                continue
            targets[N_FREQ + h] = (rs / re) / (ms / me)
            mask[N_FREQ + h] = True

    if real_dB[1] is not None and model_dB[1] is not None:   # displacement scale from the H2 / H1 discrepancy: 2^(delta / 6)
        if 0 not in anomalous and not _below_threshold(snr_db, 1, snr_threshold):
            targets[DS_IDX] = 2.0 ** ((real_dB[1] - model_dB[1]) / 6.0)
            mask[DS_IDX] = True
    return targets, mask


def assemble_dataset(real_features, model_features, snr_cache=None):
    """compute_residuals.py:288-363: (inputs [n, 2] f32, targets [n, 11] f32, mask [n, 11] bool, weights [n] f32, note_ids, filter_stats)."""
    inputs, targets, masks, weights, note_ids = [], [], [], [], []
    stats = {"total_notes": 0, "matched": 0, "h2_freq_valid": 0, "h3_freq_valid": 0, "h2_decay_valid": 0, "ds_valid": 0}
    for real in real_features:
        midi, vel = real["midi_note"], real.get("velocity_midi", 80)
        stats["total_notes"] += 1
        model = model_features.get(f"{midi}_{bucket_velocity(vel)}")
        if model is None:
            continue
        stats["matched"] += 1
        note_id = real.get("id", "")
        t, m = compute_note_residual(real, model, snr_cache.get(note_id) if snr_cache else None)
        for key, i in (("h2_freq_valid", 0), ("h3_freq_valid", 1), ("h2_decay_valid", N_FREQ), ("ds_valid", DS_IDX)):
            stats[key] += int(m[i])
        if not np.any(m):
            continue
        inputs.append([(midi - 21) / (108 - 21), vel / 127.0])
        targets.append(t)
        masks.append(m)
        weights.append(TIER_WEIGHTS.get(real.get("isolation_tier", "bronze"), 0.3))
        note_ids.append(note_id)
    return (np.array(inputs, dtype=np.float32), np.nan_to_num(np.array(targets, dtype=np.float32), nan=0.0), np.array(masks, dtype=bool),
            np.array(weights, dtype=np.float32), note_ids, stats)


TARGET_NAMES = [f"freq_H{h + 2}" for h in range(N_FREQ)] + [f"decay_H{h + 2}" for h in range(N_DECAY)] + ["ds_corr"]


def format_dataset_summary(inputs, targets, mask, weights, note_ids, filter_stats):
    """The text of print_dataset_summary (compute_residuals.py:366-426)."""
    n = len(inputs)
    s = filter_stats
    out = ["", f"Dataset: {n} observations", "", "  SNR Filtering Summary:",
           f"    Total notes examined:  {s['total_notes']}", f"    Model-matched:         {s['matched']}",
           f"    H2 freq valid:         {s['h2_freq_valid']}/{s['matched']}", f"    H3 freq valid:         {s['h3_freq_valid']}/{s['matched']}",
           f"    H2 decay valid:        {s['h2_decay_valid']}/{s['matched']}", f"    ds_correction valid:   {s['ds_valid']}/{s['matched']}",
           "    H4-H6 targets:         masked (below OBM noise floor)"]
    midi_vals = inputs[:, 0] * (108 - 21) + 21
    vel_vals = inputs[:, 1] * 127
    out += ["", f"  MIDI range: {midi_vals.min():.0f} - {midi_vals.max():.0f}", f"  Velocity range: {vel_vals.min():.0f} - {vel_vals.max():.0f}"]
    counts = {}
    for w in weights:
        for tier, tw in TIER_WEIGHTS.items():
            if abs(w - tw) < 0.01:
                counts[tier] = counts.get(tier, 0) + 1
                break
    out += [f"  {tier}: {counts.get(tier, 0)}" for tier in ("gold", "silver", "bronze")]
    out += ["", "  Target coverage:"]
    for i, name in enumerate(TARGET_NAMES):
        valid = mask[:, i].sum()
        if valid > 0:
            v = targets[mask[:, i], i]
            out.append(f"    {name:>12}: {valid:>5}/{n} valid  mean={v.mean():+7.2f}  std={v.std():6.2f}  range=[{v.min():+7.2f}, {v.max():+7.2f}]")
        else:
            out.append(f"    {name:>12}:     0/{n} valid  (fully masked)")
    if any("obm_" in nid for nid in note_ids):
        out += ["", "  Per-note OBM residuals (valid targets only):"]
        for i, nid in enumerate(note_ids):
            if "obm_" not in nid:
                continue
            midi = int(inputs[i, 0] * (108 - 21) + 21)
            freq = f"{targets[i, 0]:+.1f} ¢" if mask[i, 0] else "MASKED"
            decay = f"{targets[i, N_FREQ]:.2f}" if mask[i, N_FREQ] else "MASKED"
            ds = f"{targets[i, DS_IDX]:.3f}" if mask[i, DS_IDX] else "MASKED"
            out.append(f"    {nid:>12} (MIDI {midi:>2}): freq_H2={freq:>10}  decay_H2={decay:>8}  ds={ds:>8}")
    return "\n".join(out) + "\n"


def print_dataset_summary(inputs, targets, mask, weights, note_ids, filter_stats):
    print(format_dataset_summary(inputs, targets, mask, weights, note_ids, filter_stats), end="")


def format_snr_table(feats, snr_cache):
    """The per-note SNR lines compute_residuals.py:463-470 prints."""
    out = ["", "  Per-harmonic SNR (dB):", f"  {'Note':>12} {'H1':>7} {'H2':>7} {'H3':>7} {'H4':>7}"]
    for f in feats:
        nid = f.get("id", "")
        snr = snr_cache.get(nid)
        if snr is not None:
            v = [f"{x:>7.1f}" if not np.isnan(x) else "    nan" for x in snr[:4]]
            out.append(f"  {nid:>12} {v[0]} {v[1]} {v[2]} {v[3]}")
    return "\n".join(out) + "\n"


def save_npz(output_dir, inputs, targets, mask, weights):
    """training_data.npz as the script writes it; returns its path."""
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, "training_data.npz")
    np.savez(path, inputs=inputs, targets=targets, mask=mask, weights=weights)
    return path
