"""Host mirror of stage 3 of the ML loop, `ml/extract_harmonics.py`: harmonic features of scored, recorded notes.

The reference walks the notes one by one and calls `extract_harmonics_fft` or, for gold-tier notes, the interpreted Goertzel loop on
every window.  Here all segments of all notes are planned first, the clips are gathered as rows (at most 1.6 s after the onset is ever
read), and two GPU calls do the measuring: `ow_extract_harmonics` for the FFT notes and every RMS span, `ow_goertzel_harmonics` for
the Goertzel notes.  What stays on the host is the script's bookkeeping: the clipping of windows by the note's length, `harmonic_mask`,
the rounding of the reported numbers, the decay fit, overshoot and centroids.  No CPU fallback.
"""
import math
import os

import numpy as np

from . import features
from .features import WINDOWS, DECAY_TIMES, N_HARMONICS, amps_to_dB, midi_to_freq

MIN_DURATION = {"attack": 0.100, "early_sustain": 0.250, "sustain": 0.500}      # extract_harmonics.py:27-31, third column
TIER_ORDER = {"gold": 3, "silver": 2, "bronze": 1, "reject": 0, "pending": -1}


def load_audio(path, sr_target=44100):
    """goertzel_utils.load_audio (:12-31) without soundfile: a PCM WAV of 16, 24 or 32 bits through the standard library's `wave`, as
    float64 (integer / 2^(bits - 1), the normalisation soundfile applies), channels averaged, resampled with scipy's resample_poly only
    when the file's rate is not sr_target.  Returns (data, sample_rate)."""
    import io
    import wave
    with open(path, "rb") as f:
        raw = bytearray(f.read())
    at = raw.find(b"fmt ")
    # WAVE_FORMAT_EXTENSIBLE with the PCM sub-format (what ow_wav24_write and hound write for 24 bits): `wave` knows plain PCM only
    if at >= 0 and raw[at + 8:at + 10] == b"\xfe\xff" and raw[at + 32:at + 34] == b"\x01\x00":
        raw[at + 8:at + 10] = b"\x01\x00"
    try:
        with wave.open(io.BytesIO(bytes(raw)), "rb") as w:
            channels, width, sr, frames = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            payload = w.readframes(frames)
    except wave.Error as e:
        raise ValueError(f"{path}: not a PCM WAV file this reader understands ({e}); convert it to 16-, 24- or 32-bit PCM WAV") from None
    if width == 2:
        ints = np.frombuffer(payload, dtype="<i2").astype(np.int64)
    elif width == 3:
        b = np.frombuffer(payload, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        ints = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        ints = ints - ((ints & 0x800000) << 1)
    elif width == 4:
        ints = np.frombuffer(payload, dtype="<i4").astype(np.int64)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples; this reader takes 16-, 24- or 32-bit PCM")
    data = ints.astype(np.float64) / float(1 << (8 * width - 1))
    data = data.reshape(-1, channels)
    data = data.mean(axis=1) if channels > 1 else data[:, 0]
    if sr != sr_target:
        try:
            from scipy.signal import resample_poly
        except ImportError:
            raise RuntimeError(f"{path} is at {sr} Hz, not {sr_target} Hz: resampling needs scipy (scipy.signal.resample_poly), which is not installed; "
                               f"resample the file to {sr_target} Hz first") from None
        g = math.gcd(sr_target, sr)
        data = resample_poly(data, sr_target // g, sr // g)
        sr = sr_target
    return data, sr


def plan_note(n_audio, sr, note):
    """Where extract_note_features (extract_harmonics.py:46-201) looks: None if the note lies outside the audio, else
    (onset_sample, [11 entries]): 3 windows, 6 decay points, 2 RMS spans, each (start, end, n_harmonics) relative to the onset, or None
    where the script skips it."""
    duration_s = note["offset_s"] - note["onset_s"]
    onset = int(note["onset_s"] * sr)
    offset = min(int(note["offset_s"] * sr), n_audio)
    if onset >= n_audio or onset >= offset:
        return None
    length = offset - onset
    segs = []
    for name, w0, w1 in WINDOWS:
        end = min(w1, duration_s)
        a, b = min(int(w0 * sr), length), min(int(end * sr), length)          # a slice of note_audio stops at its end
        segs.append((a, b, N_HARMONICS) if duration_s >= MIN_DURATION[name] and w0 < end and b - a >= 128 else None)
    for t in DECAY_TIMES:
        a, b = int(t * sr), min(int((t + 0.100) * sr), length)
        segs.append((a, b, 1) if t < duration_s - 0.05 and b - a >= 64 else None)
    pe, ss, se = min(int(0.010 * sr), length), int(0.100 * sr), min(int(0.200 * sr), length)
    ok = duration_s >= 0.250 and pe > 0 and se > ss
    segs.append((0, pe, 0) if ok else None)
    segs.append((ss, se, 0) if ok else None)
    return onset, segs


def _masked(values, mask, digits):
    return [round(float(v), digits) if keep else None for v, keep in zip(values, mask)]


def _note_dict(note, f0, duration_s, idx, amps, freqs, rms):
    """The script's bookkeeping for one note; idx: its 11 result rows (None where skipped)."""
    mask = note.get("harmonic_mask", [True] * N_HARMONICS)
    feat = {"id": note["id"], "midi_note": note["midi_note"], "f0": f0, "duration_s": round(duration_s, 4), "windows": {}}
    for w, (name, _, _) in enumerate(WINDOWS):
        if idx[w] is None:
            feat["windows"][name] = None
            continue
        am, fr = amps[idx[w]], freqs[idx[w]]
        feat["windows"][name] = {"amps_linear": _masked(am, mask, 8), "amps_dB_rel_H1": _masked(amps_to_dB(am), mask, 2), "freqs_hz": _masked(fr, mask, 2)}
    decay = [None if idx[3 + i] is None else round(float(amps[idx[3 + i]][0]), 8) for i in range(len(DECAY_TIMES))]
    pts = [(t, a) for t, a in zip(DECAY_TIMES, decay) if a is not None and a > 1e-15]
    rate = None
    if len(pts) >= 3:
        ts = np.array([p[0] for p in pts]); la = np.log10(np.array([p[1] for p in pts]))
        if np.std(ts) > 0:
            rate = round(float(-20.0 * np.polyfit(ts, la, 1)[0]), 2)
    feat["decay"] = {"times_s": list(DECAY_TIMES), "h1_amps": decay, "decay_rate_dB_s": rate}
    feat["overshoot_dB"] = (round(float(20.0 * np.log10(rms[idx[9]] / rms[idx[10]])), 2) if idx[9] is not None and idx[10] is not None else None)
    for name in ("attack", "sustain"):
        w = feat["windows"].get(name)
        valid = [] if w is None else [(f, a) for f, a in zip(w["freqs_hz"], w["amps_linear"]) if f is not None and a is not None and a > 1e-15]
        if valid:
            fv = np.array([v[0] for v in valid]); av = np.array([v[1] for v in valid])
            feat[f"centroid_{name}"] = round(float(np.sum(fv * av) / np.sum(av)), 1)
        else:
            feat[f"centroid_{name}"] = None
    return feat


def extract_many(items, device=0):
    """extract_note_features for many notes at once.  items: (audio, sr, note, use_goertzel); one sample rate per call.
    Returns a list with the features dictionary, or None, of every item."""
    items = list(items)
    out = [None] * len(items)
    if not items:
        return out
    sr = items[0][1]
    if any(it[1] != sr for it in items):
        raise ValueError("extract_many: one sample rate per call")
    plans = [plan_note(len(it[0]), sr, it[2]) for it in items]
    live = [j for j, p in enumerate(plans) if p is not None]
    width = max([max([s[1] for s in plans[j][1] if s is not None], default=0) for j in live], default=0)
    rows = np.zeros((max(len(live), 1), max(width, 1)))
    fft_segs, g_segs, where = [], [], {}
    for r, j in enumerate(live):
        audio, _, note, use_goertzel = items[j]
        onset, segs = plans[j]
        need = max([s[1] for s in segs if s is not None], default=0)
        rows[r, :need] = np.asarray(audio[onset:onset + need], dtype=np.float64)
        f0 = note.get("measured_f0", midi_to_freq(note["midi_note"]))
        for i, s in enumerate(segs):
            if s is None:
                continue
            to = g_segs if use_goertzel and s[2] > 0 else fft_segs
            where[(j, i)] = (to is g_segs, len(to))
            to.append((r, s[0], s[1], s[2], f0))
    f_amps, f_freqs, f_rms = features.extract_segments(rows, sr, fft_segs, 0.01, device)
    g_amps, g_freqs, _ = features.extract_segments(rows, sr, g_segs, 0.01, device, method="goertzel")
    n_f = len(fft_segs)
    amps, freqs = np.concatenate([f_amps, g_amps]), np.concatenate([f_freqs, g_freqs])
    rms = np.concatenate([f_rms, np.zeros(len(g_segs))])
    for j in live:
        note = items[j][2]
        idx = [None if (j, i) not in where else where[(j, i)][1] + (n_f if where[(j, i)][0] else 0) for i in range(11)]
        out[j] = _note_dict(note, note.get("measured_f0", midi_to_freq(note["midi_note"])), note["offset_s"] - note["onset_s"], idx, amps, freqs, rms)
    return out


def extract_note_features(audio, sr, note, use_goertzel=False, device=0):
    """Drop-in for extract_harmonics.extract_note_features."""
    return extract_many([(audio, sr, note, use_goertzel)], device)[0]


def extract_all_harmonics(notes, audio_by_file, min_tier="bronze", use_goertzel_for_gold=True, device=0, goertzel_all=False):
    """extract_all_harmonics (extract_harmonics.py:204-254) on audio that is already in memory: audio_by_file[source_file] = (audio, sr).
    goertzel_all: Goertzel for every note, whatever its tier (what the script's --goertzel-all stands for).
    A note whose file is missing from audio_by_file is reported and skipped, as a file that fails to load is there."""
    floor = TIER_ORDER.get(min_tier, 1)
    eligible = [n for n in notes if TIER_ORDER.get(n.get("isolation_tier", "reject"), 0) >= floor]
    print(f"Extracting harmonics for {len(eligible)} notes (>= {min_tier})...")
    by_file = {}
    for note in eligible:
        by_file.setdefault(note["source_file"], []).append(note)
    items, report = [], []                  # the per-file lines are printed in the script's order once the one batch is done
    for source_file, file_notes in sorted(by_file.items()):
        report.append(f"  Loading {os.path.basename(source_file)}...")
        if source_file not in audio_by_file:
            report.append(f"    ERROR loading: no audio given for {source_file}")
            continue
        audio, sr = audio_by_file[source_file]
        for note in file_notes:
            items.append((audio, sr, note, goertzel_all or (use_goertzel_for_gold and note.get("isolation_tier") == "gold")))
        report.append(f"    Extracted {len(file_notes)} notes")
    results = [None] * len(items)
    for sr in sorted({it[1] for it in items}):
        group = [j for j, it in enumerate(items) if it[1] == sr]
        for j, feat in zip(group, extract_many([items[j] for j in group], device)):
            results[j] = feat
    for line in report:
        print(line)
    all_features = []
    for (_, _, note, _), feat in zip(items, results):
        if feat is not None:
            feat["isolation_tier"] = note.get("isolation_tier", "unknown")
            feat["isolation_score"] = note.get("isolation_score", 0.0)
            feat["velocity_midi"] = note.get("velocity_midi", 80)
            feat["source_file"] = note["source_file"]
            all_features.append(feat)
    return all_features


def format_summary(feats):
    """The text of print_summary (extract_harmonics.py:257-281)."""
    n = len(feats)
    lines = ["", f"Extracted features for {n} notes"]
    tiers = {}
    for f in feats:
        t = f.get("isolation_tier", "unknown")
        tiers[t] = tiers.get(t, 0) + 1
    lines += [f"  {t}: {tiers.get(t, 0)}" for t in ("gold", "silver", "bronze")]
    for name, _, _ in WINDOWS:
        lines.append(f"  {name} window: {sum(1 for f in feats if f['windows'].get(name) is not None)}/{n} notes")
    lines.append(f"  Decay rate: {sum(1 for f in feats if f['decay']['decay_rate_dB_s'] is not None)}/{n} notes")
    lines.append(f"  Overshoot: {sum(1 for f in feats if f['overshoot_dB'] is not None)}/{n} notes")
    return "\n".join(lines) + "\n"


def print_summary(feats):
    print(format_summary(feats), end="")
