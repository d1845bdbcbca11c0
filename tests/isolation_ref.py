"""CPU restatement (plain Python / numpy) of recorded-note intake.  TEST INFRASTRUCTURE ONLY.

Restates (reference file:line):
  * decay_remaining_amplitude, score_temporal, harmonic_collision_check, score_harmonic_collision, score_energy_dominance,
    score_notes                                   ml/score_isolation.py:23-167, 224-291
  * detect_obm_onset / detect_obm_offset          ml/extract_notes.py:43-64
  * correct_octave_errors                         ml/extract_notes.py:94-171
Pinned: tests/test_isolation_host.py holds it bit for bit to tests/golden/isolation_golden.json and tests/golden/intake_golden.npz, the
outputs of the reference's own Python (tests/golden/make_isolation_golden.py).

The reference makes three passes over a target's others; here one pass feeds the three sub-scores, each sum still in list order, so the
bits are the same.  `pow10` stands for `10.0 ** x`: the tests pass a shifted one to see what a device pow that is a few ulp away may move.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import features_oracle as fo  # noqa: E402

WEIGHTS = (2.0, 2.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0)


def midi_to_freq(m):
    return 440.0 * 2.0 ** ((m - 69) / 12.0)


def decay_rate(m):
    return 0.26 * math.exp(0.049 * m)


def pow10(x):
    return 10.0 ** x


def remaining_after(m, t, p10=pow10):
    return 1.0 if t <= 0 else p10(-(decay_rate(m) * t) / 20.0)


def pair_mask(target_midi, other_midi):
    """8 bools: harmonic h + 1 of the target clean of every harmonic of the other (ratio of the two frequencies at or above 50 cents)."""
    limit = 2.0 ** (50.0 / 1200.0)
    ft, fo_ = midi_to_freq(target_midi), midi_to_freq(other_midi)
    out = []
    for a in range(1, 9):
        fa = ft * a
        out.append(all(max(fa, fo_ * b) / max(min(fa, fo_ * b), 1e-6) >= limit for b in range(1, 9)))
    return out


def collision_table():
    """uint8 [128 target, 128 other]: bit h set while harmonic h + 1 is clean."""
    t = np.zeros((128, 128), dtype=np.uint8)
    for a in range(128):
        for b in range(128):
            t[a, b] = sum(1 << h for h, clean in enumerate(pair_mask(a, b)) if clean)
    return t


def window_of(note):
    ws, we = note["onset_s"] + 0.050, min(note["onset_s"] + 0.800, note["offset_s"])
    return (note["onset_s"], note["offset_s"]) if ws >= we else (ws, we)


def sub_scores(target, file_notes, p10=pow10, table=None):
    """(temporal, collision, dominance, mask as 8 bools) of one target among the notes of its file, unrounded."""
    ws, we = window_of(target)
    mid = (ws + we) / 2.0
    floor = max(target["amplitude"], 1e-6)
    score, total, mask, any_energy = 1.0, target["amplitude"], [True] * 8, False
    for o in file_notes:
        if o["id"] == target["id"]:
            continue
        if o["onset_s"] < we and o["offset_s"] > ws:
            level, energetic, at_mid = o["amplitude"], True, o["amplitude"]
        elif o["offset_s"] < ws:
            level = remaining_after(o["midi_note"], ws - o["offset_s"], p10) * o["amplitude"]
            energetic = level > 0.05
            at_mid = remaining_after(o["midi_note"], mid - o["offset_s"], p10) * o["amplitude"]
        else:
            continue
        rel = level / floor
        if rel > 0.1:
            score -= 0.10 * min(rel, 1.0)
        total += at_mid
        if energetic:
            any_energy = True
            pm = pair_mask(target["midi_note"], o["midi_note"]) if table is None else [bool(table[target["midi_note"], o["midi_note"]] >> h & 1) for h in range(8)]
            mask = [a and b for a, b in zip(mask, pm)]
    collision = sum(w for w, clean in zip(WEIGHTS, mask) if clean) / 12.0 if any_energy else 1.0
    return max(0.05, score), collision, (1.0 if total < 1e-10 else target["amplitude"] / total), mask


def duration_score(d):
    return 0.0 if d < 0.150 else 0.3 if d < 0.300 else 0.7 if d < 0.600 else 1.0


def composite(temporal, collision, dominance, duration):
    if collision <= 0.0 or duration <= 0.0:
        return 0.0
    return math.exp(0.35 * math.log(collision) + 0.20 * math.log(max(temporal, 0.05)) + 0.20 * math.log(max(dominance, 0.05)) + 0.25 * math.log(duration))


def tier(score):
    return "gold" if score >= 0.85 else "silver" if score >= 0.55 else "bronze" if score >= 0.15 else "reject"


def score_notes(notes, p10=pow10, table=None):
    """In place, as the reference's score_notes; returns the unrounded (temporal, collision, dominance) per note (None: not scored)."""
    by_file = {}
    for n in notes:
        by_file.setdefault(n["source_file"], []).append(n)
    raw = []
    for n in notes:
        d = duration_score(n["offset_s"] - n["onset_s"])
        if n.get("source_type") == "obm_isolated" or d == 0.0:
            v = 1.0 if n.get("source_type") == "obm_isolated" else 0.0
            n["isolation_score"] = v
            n["isolation_tier"] = "gold" if v else "reject"
            n["sub_scores"] = {"temporal": v, "collision": v, "dominance": v, "duration": v}
            n["harmonic_mask"] = [bool(v)] * 8
            raw.append(None)
            continue
        t, c, dom, mask = sub_scores(n, by_file[n["source_file"]], p10, table)
        comp = composite(t, c, dom, d)
        n["isolation_score"] = round(comp, 4)
        n["isolation_tier"] = tier(comp)
        n["sub_scores"] = {"temporal": round(t, 4), "collision": round(c, 4), "dominance": round(dom, 4), "duration": round(d, 4)}
        n["harmonic_mask"] = mask
        raw.append((t, c, dom))
    return raw


# ---- extract_notes.py -------------------------------------------------------------------------------------------------------------------
def clip_bounds(x, onset_frac=0.10, offset_frac=0.01):
    """(peak, first, last): first index with |x| > onset_frac * peak, last index >= 1 with |x| > offset_frac * peak; -1: none."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    peak = float(a.max()) if a.size else 0.0
    on = np.flatnonzero(a > onset_frac * peak)
    off = np.flatnonzero(a[1:] > offset_frac * peak) + 1
    return peak, (int(on[0]) if on.size else -1), (int(off[-1]) if off.size else -1)


def obm_seconds(x, sr):
    """(onset_s, offset_s) as detect_obm_onset / detect_obm_offset give them."""
    peak, first, last = clip_bounds(x)
    if peak < 1e-10:
        return 0.0, len(x) / sr
    return (first / sr if first >= 0 else 0.0), (last / sr if last >= 0 else len(x) / sr)


def sustain_window(x, sr, onset_offset_ms=150, sustain_end_ms=800):
    """(start, end, onset_idx) of goertzel_utils.extract_sustain_window (:139-159); a silent clip: the whole clip, onset 0."""
    peak, first, _ = clip_bounds(x)
    if peak < 1e-10:
        return 0, len(x), 0
    onset = max(first, 0)
    start, end = onset + int(onset_offset_ms * sr / 1000), min(onset + int(sustain_end_ms * sr / 1000), len(x))
    return (max(0, end - int(0.2 * sr)) if start >= end else start), end, onset


def probe_window(note, n_audio, sr):
    on = int(note["onset_s"] * sr)
    for a, b in ((on + int(0.050 * sr), min(on + int(0.200 * sr), n_audio)), (on, min(on + int(0.150 * sr), n_audio))):
        if b - a >= 128:
            return a, b
    return None


def probes(note, audio, sr):
    """(amp_f0, amp_noise, amp_up, amp_down), or None where the note has no window of 128 samples."""
    win = probe_window(note, len(audio), sr)
    if win is None:
        return None
    seg = audio[win[0]:win[1]]
    f0 = midi_to_freq(note["midi_note"])
    h1 = lambda f: float(fo.extract_harmonics(seg, sr, f, 1)[0][0])
    noise = max(h1(f0 * 1.37), 1e-20) if f0 * 1.37 < sr / 2 - 200 else 1e-20
    return h1(f0), noise, (h1(f0 * 2) if f0 * 2 < sr / 2 - 200 else 0.0), (h1(f0 / 2) if f0 / 2 > 30 else 0.0)


def decide(midi, a_f0, a_noise, a_up, a_down):
    """The MIDI note to keep, None to drop."""
    best, keep = a_f0, midi
    if a_up > a_f0 * 2.0 and a_up > a_noise * 5:
        best, keep = a_up, midi + 12
    elif a_down > a_f0 * 2.0 and a_down > a_noise * 5:
        best, keep = a_down, midi - 12
    return None if best / max(a_noise, 1e-20) < 3.0 else keep


def correct_octave_errors(notes, audio, sr):
    """In place; returns (corrected, removed, [probe amplitudes or None per input note])."""
    all_probes = [probes(n, audio, sr) for n in notes]
    corrected, drop = 0, []
    for i, (n, pr) in enumerate(zip(notes, all_probes)):
        keep = None if pr is None else decide(n["midi_note"], *pr)
        if keep is None:
            drop.append(i)
        elif keep != n["midi_note"]:
            n["octave_corrected"] = n["midi_note"]
            n["midi_note"] = keep
            n["measured_f0"] = round(midi_to_freq(keep), 2)
            corrected += 1
    for i in reversed(drop):
        notes.pop(i)
    return corrected, len(drop), all_probes
