"""Host mirror of stage 2 of the ML loop, `ml/score_isolation.py`: isolation scores of extracted notes.

The reference walks, for every note, every other note of the same recording three times in interpreted Python.  Here the windows are
planned on the host, all notes of all files go to the device in ONE `ow_isolation_score` call (k_isolation_score: one lane per target,
the others in list order), and what comes back are the three unrounded pairwise sub-scores and the clean-harmonic mask.  What stays on
the host is the script's bookkeeping: the duration score, the composite, the tier, the rounding of the reported numbers, the OBM and
too-short short cuts, the report.  No CPU fallback.
"""
import ctypes as C
import math
import os

import numpy as np

from . import binding
from .binding import OwError
from .features import midi_to_freq

N_HARMONICS = 8
COLLISION_RATIO = 2.0 ** (50.0 / 1200.0)            # score_isolation.py:79


def decay_rate_table():
    """0.26 * exp(0.049 * midi) for midi 0..127 (decay_remaining_amplitude, score_isolation.py:31), with math.exp as there."""
    return np.array([0.26 * math.exp(0.049 * m) for m in range(128)], dtype=np.float64)


def midi_freq_table():
    """midi_to_freq for midi 0..127 (goertzel_utils.py:129-131)."""
    return np.array([midi_to_freq(m) for m in range(128)], dtype=np.float64)


def collision_table():
    """harmonic_collision_check for every pair of MIDI numbers: uint8 [128 target, 128 other], bit h set while harmonic h + 1 of the
    target is clean (ow_isolation_collision_table; host arithmetic, no device)."""
    lib = binding.load_library()
    freq = midi_freq_table()
    table = np.zeros((128, 128), dtype=np.uint8)
    if lib.ow_isolation_collision_table(freq.ctypes.data_as(C.c_void_p), COLLISION_RATIO, table.ctypes.data_as(C.c_void_p)) != 0:
        raise OwError(binding.take_error(lib))
    return table


def score_duration(duration_s):
    """score_isolation.py:170-185."""
    if duration_s < 0.150:
        return 0.0
    elif duration_s < 0.300:
        return 0.3
    elif duration_s < 0.600:
        return 0.7
    else:
        return 1.0


def compute_composite_score(temporal, collision, dominance, duration):
    """score_isolation.py:188-209: the weighted geometric mean, collision or duration of 0 vetoes."""
    if collision <= 0.0 or duration <= 0.0:
        return 0.0
    temporal = max(temporal, 0.05)
    dominance = max(dominance, 0.05)
    log_score = (0.35 * math.log(collision) +
                 0.20 * math.log(temporal) +
                 0.20 * math.log(dominance) +
                 0.25 * math.log(duration))
    return math.exp(log_score)


def tier_from_score(score):
    """score_isolation.py:212-221."""
    if score >= 0.85:
        return "gold"
    elif score >= 0.55:
        return "silver"
    elif score >= 0.15:
        return "bronze"
    else:
        return "reject"


def plan_window(note):
    """The analysis window of score_notes (:266-271), fallback included."""
    window_start = note["onset_s"] + 0.050
    window_end = min(note["onset_s"] + 0.800, note["offset_s"])
    if window_start >= window_end:
        window_start = note["onset_s"]
        window_end = note["offset_s"]
    return window_start, window_end


def is_scored(note):
    """False for the notes score_notes settles without looking at the others (:239, :254)."""
    return note.get("source_type") != "obm_isolated" and score_duration(note["offset_s"] - note["onset_s"]) != 0.0


def plan_notes(notes):
    """(records, file_first, order): the ow_iso_note records grouped by source_file in order of first appearance, inside a file in list
    order (by_file of score_notes: the accumulation order); file_first [n_files + 1]; order[k] = index in `notes` of record k."""
    by_file, keys = {}, {}
    for i, note in enumerate(notes):
        by_file.setdefault(note["source_file"], []).append(i)
    order = [i for idx in by_file.values() for i in idx]
    file_first = np.zeros(len(by_file) + 1, dtype=np.uint64)
    file_first[1:] = np.cumsum([len(idx) for idx in by_file.values()])
    rec = np.zeros(len(order), dtype=np.dtype(binding.ISO_NOTE_DTYPE))
    for k, i in enumerate(order):
        note = notes[i]
        ws, we = plan_window(note)
        rec[k] = (note["onset_s"], note["offset_s"], note["amplitude"], ws, we, keys.setdefault(note["id"], len(keys)), note["midi_note"],
                  1 if is_scored(note) else 0)
    return rec, file_first, order


def isolation_scores(records, file_first, device=0, kernel_ms=False):
    """ow_isolation_score on planned records: (temporal, collision, dominance, mask) per record, unrounded; zeros where score == 0.
    kernel_ms=True appends the kernel's device time in milliseconds."""
    lib = binding.load_library()
    rec = np.ascontiguousarray(records, dtype=np.dtype(binding.ISO_NOTE_DTYPE))
    ff = np.ascontiguousarray(file_first, dtype=np.uint64)
    n = rec.size
    temporal, collision, dominance = np.zeros(n), np.zeros(n), np.zeros(n)
    mask = np.zeros(n, dtype=np.uint8)
    rate, freq = decay_rate_table(), midi_freq_table()
    ms = C.c_double(0.0)
    cfg = binding.OwIsoCfg(COLLISION_RATIO, rate.ctypes.data_as(C.POINTER(C.c_double)), freq.ctypes.data_as(C.POINTER(C.c_double)), int(device),
                           C.pointer(ms) if kernel_ms else None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    if lib.ow_isolation_score(p(rec), n, p(ff), max(ff.size - 1, 0), C.byref(cfg), p(temporal), p(collision), p(dominance), p(mask)) != 0:
        raise OwError(binding.take_error(lib))
    return (temporal, collision, dominance, mask) + ((ms.value,) if kernel_ms else ())


def score_notes(notes, device=0):
    """Drop-in for score_isolation.score_notes: modifies the dictionaries in place."""
    rec, file_first, order = plan_notes(notes)
    temporal, collision, dominance, mask = isolation_scores(rec, file_first, device)
    at = {i: k for k, i in enumerate(order)}
    for i, note in enumerate(notes):
        if note.get("source_type") == "obm_isolated":
            note["isolation_score"] = 1.0
            note["isolation_tier"] = "gold"
            note["sub_scores"] = {"temporal": 1.0, "collision": 1.0, "dominance": 1.0, "duration": 1.0}
            note["harmonic_mask"] = [True] * N_HARMONICS
            continue
        dur_score = score_duration(note["offset_s"] - note["onset_s"])
        if dur_score == 0.0:
            note["isolation_score"] = 0.0
            note["isolation_tier"] = "reject"
            note["sub_scores"] = {"temporal": 0.0, "collision": 0.0, "dominance": 0.0, "duration": 0.0}
            note["harmonic_mask"] = [False] * N_HARMONICS
            continue
        k = at[i]
        temp_score, collision_score, dom_score = float(temporal[k]), float(collision[k]), float(dominance[k])
        composite = compute_composite_score(temp_score, collision_score, dom_score, dur_score)
        note["isolation_score"] = round(composite, 4)
        note["isolation_tier"] = tier_from_score(composite)
        note["sub_scores"] = {"temporal": round(temp_score, 4), "collision": round(collision_score, 4), "dominance": round(dom_score, 4),
                              "duration": round(dur_score, 4)}
        note["harmonic_mask"] = [bool(int(mask[k]) >> h & 1) for h in range(N_HARMONICS)]


def format_summary(notes):
    """The text of print_summary (score_isolation.py:294-330)."""
    tiers = {"gold": 0, "silver": 0, "bronze": 0, "reject": 0}
    for note in notes:
        tier = note.get("isolation_tier", "reject")
        tiers[tier] = tiers.get(tier, 0) + 1
    total = len(notes)
    lines = [f"\nIsolation scoring summary ({total} notes):"]
    for tier in ["gold", "silver", "bronze", "reject"]:
        count = tiers[tier]
        pct = 100.0 * count / max(total, 1)
        lines.append(f"  {tier:>7}: {count:>5} ({pct:>5.1f}%)")
    usable = tiers["gold"] + tiers["silver"] + tiers["bronze"]
    lines.append(f"  usable: {usable:>5} (bronze+)")
    usable_midis = [n["midi_note"] for n in notes if n.get("isolation_tier") != "reject"]
    if usable_midis:
        lines.append(f"  MIDI range (usable): {min(usable_midis)}-{max(usable_midis)}")
    lines.append("\nPer-source breakdown:")
    by_source = {}
    for n in notes:
        src = os.path.basename(n["source_file"])
        if src not in by_source:
            by_source[src] = {"gold": 0, "silver": 0, "bronze": 0, "reject": 0}
        by_source[src][n.get("isolation_tier", "reject")] += 1
    for src in sorted(by_source.keys()):
        counts = by_source[src]
        total_src = sum(counts.values())
        usable_src = counts["gold"] + counts["silver"] + counts["bronze"]
        lines.append(f"  {src}: {total_src} total, {usable_src} usable (G:{counts['gold']} S:{counts['silver']} B:{counts['bronze']})")
    return "\n".join(lines) + "\n"


def print_summary(notes):
    print(format_summary(notes), end="")
