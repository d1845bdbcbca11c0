#!/usr/bin/env python3
"""Generate tests/golden/isolation_golden.json and tests/golden/intake_golden.npz by running the REFERENCE's own ml/score_isolation.py and
ml/extract_notes.py, whose directory is the script's one argument (the reference tree is not part of this repository and is not where
the tests run, so its outputs travel as fixtures).  `soundfile` is not installed; the modules only need it for load_audio, so an empty
stub is registered before the import.

isolation_golden.json
  notes_in      three files of 1, 3 and 70 notes and two obm_isolated notes, shuffled: seeded random notes (times and amplitudes rounded to
                four places, as basic_pitch notes are) and the hand-placed cases listed at HAND below
  scored_text   json.dumps(notes, indent=2) after the reference's score_notes; report: what its print_summary printed
  raw           per note, [temporal, collision, dominance] from calling the three reference functions directly, unrounded (null: not scored)
  no_released   per note, true where no other of the note's file is released before its window (no pow: the device must be exact)
  nudge_ulp, nudge   the largest movement of temporal / dominance over the set when every `10 ** x` result of the reference moves by
                nudge_ulp ulp, all up or all down (np.nextafter applied nudge_ulp times)
The script asserts that no decision can flip under such a movement: no unrounded sub-score or composite within 1e-9 of a four-decimal
rounding edge or of a tier edge, no rel_energy or remaining * amplitude within 1e-9 relative of 0.1 or 0.05 other than the hand-placed
exact case, which involves no pow.  If a seed violates this, change the seed, not the margin.

intake_golden.npz
  pcm, sr, events [n, 4]       one synthetic recording as int16 PCM (the tests divide by 32768) and its note events
  probes [n, 4]                the reference's amplitudes at f0, f0 * 1.37, f0 * 2, f0 / 2 per event (NaN: probe not taken or note dropped
                               before probing), from extract_harmonics_fft as correct_octave_errors called it
  notes_in_json, notes_out_json, corrected, removed      the dictionaries before and after the reference's correct_octave_errors
  clip{i}, clip_sec{i} [2], clip_idx{i} [2], n_clips     clip-bounds clips, the reference's onset / offset seconds at sr and the indices
The script asserts that every amplitude comparison of the decision logic has at least a 1 % margin."""
import contextlib
import copy
import io
import json
import os
import sys
import types

import numpy as np

sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
if len(sys.argv) < 2:
    sys.exit("usage: make_isolation_golden.py <the reference's ml/ directory>")
sys.path.insert(0, sys.argv[1])
import score_isolation as si  # noqa: E402
import extract_notes as en  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 44100
SEED = 20
NUDGE_ULP = 4
FILE_A, FILE_B, FILE_C = "/recordings/solo.wav", "/recordings/trio.wav", "/recordings/take_07.wav"


def note(ident, onset, offset, midi, amp, source, kind="basic_pitch"):
    return {"id": ident, "onset_s": round(float(onset), 4), "offset_s": round(float(offset), 4), "midi_note": int(midi),
            "measured_f0": round(440.0 * 2.0 ** ((midi - 69) / 12.0), 2), "amplitude": round(float(amp), 4),
            "velocity_midi": max(1, min(127, int(round(amp * 127)))), "source_file": source, "source_type": kind, "isolation_tier": "pending"}


def hand_placed():
    """The 32 hand-placed notes of the 70-note file, each group in a time region of its own."""
    c = []
    # two notes with the same id, concurrent, and a third beside them: each of the two skips both
    c += [note("dup", 100.0, 101.0, 50, 0.6, FILE_C), note("dup", 100.2, 101.2, 57, 0.5, FILE_C), note("dup_third", 100.1, 101.1, 64, 0.4, FILE_C)]
    # an other whose offset EQUALS the target's window_start: neither held nor released
    onset = next(o for o in (110.0, 110.5, 111.0, 111.25, 112.0) if round(o + 0.050, 4) == o + 0.050)
    c += [note("ws_target", onset, onset + 1.0, 62, 0.5, FILE_C), note("ws_other", onset - 1.0, onset + 0.050, 69, 0.9, FILE_C)]
    assert c[-1]["offset_s"] == c[-2]["onset_s"] + 0.050
    # an other starting exactly at window_end (= the target's offset): not held
    c += [note("we_target", 120.0, 120.5, 55, 0.5, FILE_C), note("we_other", 120.5, 121.5, 67, 0.9, FILE_C)]
    # a target of amplitude 0 beside a sounding note
    c += [note("zero_target", 130.0, 131.0, 60, 0.0, FILE_C), note("zero_other", 130.1, 131.1, 71, 0.3, FILE_C)]
    # a same-pitch concurrent pair: collision 0, composite 0
    c += [note("same_a", 140.0, 141.0, 65, 0.5, FILE_C), note("same_b", 140.1, 141.1, 65, 0.6, FILE_C)]
    # a target under eleven loud held notes: the temporal floor
    c += [note("floor_target", 150.0, 151.0, 40, 0.5, FILE_C)] + [note(f"floor_{k}", 149.5 + 0.01 * k, 151.5, 41 + 3 * k, 0.9, FILE_C) for k in range(11)]
    # a note shorter than 150 ms between scored ones: not scored, still an other
    c += [note("short_l", 160.0, 161.0, 52, 0.5, FILE_C), note("short", 160.3, 160.4, 59, 0.8, FILE_C), note("short_r", 160.2, 161.2, 66, 0.5, FILE_C)]
    # an amplitude ratio of exactly 0.1 (0.05 / 0.5), held: not counted
    c += [note("tenth_target", 170.0, 171.0, 48, 0.5, FILE_C), note("tenth_other", 170.1, 171.1, 61, 0.05, FILE_C)]
    assert 0.05 / 0.5 == 0.1
    # released notes 0.01 s, 1 s and 30 s before a window (window_start = 230.05)
    c += [note("rel_target", 230.0, 231.0, 58, 0.5, FILE_C), note("rel_10ms", 229.0, 230.04, 63, 0.7, FILE_C),
          note("rel_1s", 228.0, 229.05, 70, 0.8, FILE_C), note("rel_30s", 199.0, 200.05, 45, 0.9, FILE_C)]
    assert len(c) == 32
    return c


def isolation_notes(rng):
    notes = [note("solo_0000", 1.0, 2.0, 60, 0.0, FILE_A)]                       # a lone target of amplitude 0: total_energy < 1e-10
    notes += [note("trio_0000", 0.5, 2.0, 60, 0.6, FILE_B), note("trio_0001", 0.6, 2.1, 72, 0.5, FILE_B),    # an octave and a fifth
              note("trio_0002", 0.7, 2.2, 67, 0.4, FILE_B)]
    c = hand_placed()
    for k in range(70 - len(c)):
        onset = rng.uniform(0.0, 60.0)
        c.append(note(f"take_07_{k:04d}", onset, onset + float(np.exp(rng.uniform(np.log(0.1), np.log(3.0)))), rng.integers(36, 97),
                      rng.uniform(0.05, 1.0), FILE_C))
    notes += c
    notes += [note("obm_50", 0.01, 3.0, 50, 0.63, "/obm/d3.wav", "obm_isolated"), note("obm_62", 0.02, 2.5, 62, 0.63, FILE_C, "obm_isolated")]
    for n in notes[-2:]:
        n["isolation_tier"] = "gold"
    order = rng.permutation(len(notes))
    return [notes[i] for i in order]


def windows(n):
    ws, we = n["onset_s"] + 0.050, min(n["onset_s"] + 0.800, n["offset_s"])
    return (n["onset_s"], n["offset_s"]) if ws >= we else (ws, we)


def scored(n):
    return n.get("source_type") != "obm_isolated" and si.score_duration(n["offset_s"] - n["onset_s"]) != 0.0


def raw_scores(notes):
    by_file = {}
    for n in notes:
        by_file.setdefault(n["source_file"], []).append(n)
    out = []
    for n in notes:
        if not scored(n):
            out.append(None)
            continue
        ws, we = windows(n)
        fn = by_file[n["source_file"]]
        out.append([si.score_temporal(n, fn, ws, we), si.score_harmonic_collision(n, fn, ws, we)[0], si.score_energy_dominance(n, fn, ws, we)])
    return out


def nudged(direction):
    """The reference's decay_remaining_amplitude with its `10 ** x` moved NUDGE_ULP ulp."""
    plain = si.decay_remaining_amplitude

    def moved(midi_note, t):
        v = plain(midi_note, t)
        if t <= 0:
            return v
        for _ in range(NUDGE_ULP):
            v = float(np.nextafter(v, direction))
        return v
    return plain, moved


def off_edge(x, what):
    f = x * 1e4 - np.floor(x * 1e4)
    assert abs(f - 0.5) > 1e-5, ("rounding edge", what, x)
    for edge in (0.85, 0.55, 0.15) if what[1] == "composite" else ():
        assert abs(x - edge) > 1e-9, ("tier edge", what, x)


def make_isolation():
    rng = np.random.default_rng(SEED)
    notes_in = isolation_notes(rng)
    assert sorted(sum(1 for n in notes_in if n["source_file"] == f and n["source_type"] != "obm_isolated") for f in (FILE_A, FILE_B, FILE_C)) == [1, 3, 70]
    raw = raw_scores(notes_in)
    by_file = {}
    for n in notes_in:
        by_file.setdefault(n["source_file"], []).append(n)
    # no decision near a flip
    no_released = []
    for n, r in zip(notes_in, raw):
        if r is None:
            no_released.append(False)
            continue
        ws, we = windows(n)
        mid = (ws + we) / 2.0
        released = False
        for o in by_file[n["source_file"]]:
            if o["id"] == n["id"]:
                continue
            floor = max(n["amplitude"], 1e-6)
            if o["onset_s"] < we and o["offset_s"] > ws:
                rel = o["amplitude"] / floor
                exact = o["id"] == "tenth_other" and n["id"] == "tenth_target"
                assert exact == (rel == 0.1), (n["id"], o["id"], rel)
                assert exact or abs(rel / 0.1 - 1.0) > 1e-9
            elif o["offset_s"] < ws:
                released = True
                e = si.decay_remaining_amplitude(o["midi_note"], ws - o["offset_s"]) * o["amplitude"]
                assert abs(e / floor / 0.1 - 1.0) > 1e-9 and abs(e / 0.05 - 1.0) > 1e-9, (n["id"], o["id"], e)
                assert mid - o["offset_s"] > 0
        no_released.append(not released)
        comp = si.compute_composite_score(r[0], r[1], r[2], si.score_duration(n["offset_s"] - n["onset_s"]))
        for x, what in ((r[0], "temporal"), (r[1], "collision"), (r[2], "dominance"), (comp, "composite")):
            off_edge(x, (n["id"], what))
    # the reference's own run
    out = copy.deepcopy(notes_in)
    si.score_notes(out)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        si.print_summary(out)
    for n, r in zip(out, raw):
        if r is not None:
            assert n["sub_scores"]["temporal"] == round(r[0], 4) and n["sub_scores"]["collision"] == round(r[1], 4) and n["sub_scores"]["dominance"] == round(r[2], 4)
    # the hand-placed cases do what they are there for
    by_id = {n["id"]: (n, r) for n, r in zip(out, raw) if n["id"] != "dup"}
    assert by_id["solo_0000"][1][2] == 1.0 and by_id["floor_target"][1][0] == 0.05 and by_id["same_a"][1][1] == 0.0 and by_id["same_a"][0]["isolation_score"] == 0.0
    assert by_id["short"][1] is None and by_id["short"][0]["isolation_tier"] == "reject"
    assert 0.0 < by_id["trio_0000"][1][1] < 1.0 and 0.0 < by_id["trio_0002"][1][1] < 1.0
    tiers = {n["isolation_tier"] for n in out}
    assert tiers == {"gold", "silver", "bronze", "reject"}, tiers
    # the nudge
    move = {"temporal": 0.0, "dominance": 0.0}
    for direction in (np.inf, -np.inf):
        plain, moved = nudged(direction)
        si.decay_remaining_amplitude = moved
        try:
            shifted = raw_scores(notes_in)
            again = copy.deepcopy(notes_in)
            si.score_notes(again)
        finally:
            si.decay_remaining_amplitude = plain
        assert again == out, "a rounded output moved under the nudge"
        for r, s in zip(raw, shifted):
            if r is not None:
                assert r[1] == s[1]
                move["temporal"] = max(move["temporal"], abs(r[0] - s[0]))
                move["dominance"] = max(move["dominance"], abs(r[2] - s[2]))
    assert move["temporal"] > 0.0 and move["dominance"] > 0.0
    doc = {"notes_in": notes_in, "scored_text": json.dumps(out, indent=2), "report": buf.getvalue(), "raw": raw, "no_released": no_released,
           "nudge_ulp": NUDGE_ULP, "nudge": move}
    path = os.path.join(HERE, "isolation_golden.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes; tiers", sorted((t, sum(1 for n in out if n["isolation_tier"] == t)) for t in tiers),
          "collision values", len({r[1] for r in raw if r is not None}), "nudge", move, "exact targets", sum(no_released))


# ---- intake -----------------------------------------------------------------------------------------------------------------------------
SLOT = 0.25


def tone(t, f0, rng, level=0.3):
    x = np.zeros_like(t)
    for h in range(1, 5):
        if f0 * h < SR / 2 - 500:
            x += level / h ** 1.6 * np.exp(-t * (2.0 + h)) * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28))
    return x


def make_intake(out):
    rng = np.random.default_rng(SEED + 1)
    f = en.midi_to_freq
    # (event midi, the pitch that sounds or None for noise only)
    slots = [(60, 60), (48, 60), (72, 60), (65, None), (33, 33), (108, 108), (126, 126), (57, 57)]
    n_total = int(len(slots) * SLOT * SR)
    audio = 1e-4 * rng.standard_normal(n_total)
    events = []
    for i, (ev_midi, real) in enumerate(slots):
        a = int(i * SLOT * SR)
        n = int(0.24 * SR)
        if real is None:
            audio[a:a + n] += 5e-3 * rng.standard_normal(n)
        else:
            audio[a:a + n] += tone(np.arange(n) / SR, f(real), rng)
        events.append((i * SLOT, i * SLOT + 0.24, float(ev_midi), 0.2 + 0.09 * i))
    # the last slot's note again: once where only the 0-150 ms fallback has 128 samples, once 100 samples before the end (too short)
    events.append(((n_total - 2300) / SR, n_total / SR, 57.0, 0.5))
    events.append(((n_total - 100) / SR, n_total / SR, 57.0, 0.5))
    pcm = np.clip(np.round(audio * 32768.0), -32768, 32767).astype(np.int16)
    audio = pcm.astype(np.float64) / 32768.0
    notes = []
    for i, (s, e, m, a) in enumerate(events):                    # extract_polyphonic_notes' dictionaries, built here as data
        notes.append(note(f"intake_{i:04d}", s, e, int(round(m)), a, "/recordings/intake.wav"))
    notes_in = copy.deepcopy(notes)
    probes = np.full((len(notes), 4), np.nan)
    real_fft = en.extract_harmonics_fft
    for i, n in enumerate(notes_in):
        calls = []

        def rec(segment, sr, f0, n_harmonics=8, *a, **k):
            res = real_fft(segment, sr, f0, n_harmonics, *a, **k)
            calls.append((f0, float(res[0][0])))
            return res
        en.extract_harmonics_fft = rec
        try:
            en.correct_octave_errors([copy.deepcopy(n)], audio, SR)
        finally:
            en.extract_harmonics_fft = real_fft
        f0 = f(n["midi_note"])
        for fq, amp in calls:
            col = [f0, f0 * 1.37, f0 * 2, f0 / 2].index(fq)
            probes[i, col] = amp
        if calls:                                                # every comparison of the decision at least 1 % from a tie
            a_f0 = probes[i, 0]
            a_n = 1e-20 if np.isnan(probes[i, 1]) else max(probes[i, 1], 1e-20)
            a_up = 0.0 if np.isnan(probes[i, 2]) else probes[i, 2]
            a_dn = 0.0 if np.isnan(probes[i, 3]) else probes[i, 3]
            best = a_up if (a_up > a_f0 * 2.0 and a_up > a_n * 5) else a_dn if (a_dn > a_f0 * 2.0 and a_dn > a_n * 5) else a_f0
            for x, y in ((a_up, a_f0 * 2.0), (a_up, a_n * 5), (a_dn, a_f0 * 2.0), (a_dn, a_n * 5), (best / a_n, 3.0)):
                assert abs(x / y - 1.0) > 0.01, (i, x, y)
    corrected, removed = en.correct_octave_errors(notes, audio, SR)
    kept = {n["id"]: n for n in notes}
    assert "octave_corrected" not in kept["intake_0000"] and kept["intake_0001"]["midi_note"] == 60 and kept["intake_0002"]["midi_note"] == 60
    assert "intake_0003" not in kept and "intake_0009" not in kept and "intake_0008" in kept
    assert np.isnan(probes[4, 3]) and not np.isnan(probes[5, 2]) and np.isnan(probes[6, 2]) and np.all(np.isnan(probes[9]))
    assert {"intake_0004", "intake_0005", "intake_0006", "intake_0007"} <= set(kept)
    out.update(pcm=pcm, sr=np.array([SR]), events=np.array(events), probes=probes, notes_in_json=np.array(json.dumps(notes_in)),
               notes_out_json=np.array(json.dumps(notes)), corrected=np.array([corrected]), removed=np.array([removed]))
    print("intake:", len(notes_in), "events,", corrected, "corrected,", removed, "removed")


def make_clips(out):
    rng = np.random.default_rng(SEED + 2)
    two_peaks = 0.2 * rng.standard_normal(300)
    two_peaks[[40, 200]] = [1.5, -1.5]
    junk_a, junk_b = 0.3 * rng.standard_normal(90), 0.3 * rng.standard_normal(33)
    clips = [np.zeros(100),                                                   # silent
             np.array([0.5]),                                                 # length 1
             np.array([1.0] + [0.0] * 63),                                    # peak at index 0 only: the backward loop never looks there
             rng.standard_normal(257) * np.exp(-np.arange(257) / 40.0),       # length 257
             np.array([0.0, 0.1, 0.5, 1.0, 0.3, 0.01, 0.0]),                  # samples exactly equal to both thresholds
             two_peaks,                                                       # two equal peaks
             junk_a, junk_b]                                                  # rows of unequal length (the tests put junk behind them)
    for i, x in enumerate(clips):
        on = en.detect_obm_onset(x, SR)
        off = en.detect_obm_offset(x, SR, on)
        a = np.abs(x)
        first = np.flatnonzero(a > 0.10 * a.max())
        last = np.flatnonzero(a[1:] > 0.01 * a.max()) + 1
        idx = [int(first[0]) if first.size and a.max() > 0 else -1, int(last[-1]) if last.size and a.max() > 0 else -1]
        if a.max() >= 1e-10:
            assert on == (idx[0] / SR if idx[0] >= 0 else 0.0) and off == (idx[1] / SR if idx[1] >= 0 else len(x) / SR), (i, on, off, idx)
        out[f"clip{i}"], out[f"clip_sec{i}"], out[f"clip_idx{i}"] = x, np.array([on, off]), np.array(idx, dtype=np.int64)
    assert list(out["clip_idx4"]) == [2, 4] and list(out["clip_idx2"]) == [0, -1]
    out["n_clips"] = np.array([len(clips)])


def main():
    make_isolation()
    out = {}
    make_intake(out)
    make_clips(out)
    path = os.path.join(HERE, "intake_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
