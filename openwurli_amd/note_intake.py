"""Host mirror of the non-neural half of stage 1 of the ML loop, `ml/extract_notes.py`: note observations from recordings.

The `basic_pitch` transcriber is not part of this project: its note events come in as rows of (start_s, end_s, pitch_midi, amplitude).
What the script does with them runs here: the dictionaries (`notes_from_events`), the pitch check (`correct_octave_errors`: all probes
of all notes in ONE `ow_extract_harmonics` call, the keep / shift / drop decision on the host) and the bounds of the isolated OBM notes
(`extract_obm_notes`: `ow_clip_bounds`, many clips per call).  No CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import binding, features
from .binding import OwError
from .features import midi_to_freq
from .harmonics import load_audio  # noqa: F401  (the loader of this stage, re-exported)

# extract_notes.py:26-40 as data: file name, MIDI note, measured f0 in Hz
OBM_FILES = (("87994__oldbassman__d3.wav", 50, 147.7), ("87998__oldbassman__f3.wav", 54, 186.2), ("87988__oldbassman__a3.wav", 58, 233.8),
             ("87995__oldbassman__d4.wav", 62, 293.8), ("87999__oldbassman__f4.wav", 66, 370.8), ("87989__oldbassman__a4.wav", 70, 466.2),
             ("87992__oldbassman__d5.wav", 74, 587.7), ("87993__oldbassman__f5.wav", 78, 738.5), ("87990__oldbassman__a5.wav", 82, 932.3),
             ("87996__oldbassman__d6.wav", 86, 1175.4), ("88000__oldbassman__f6.wav", 90, 1481.5), ("87991__oldbassman__a6.wav", 94, 1863.1),
             ("87997__oldbassman__d7.wav", 98, 2363.1))
OBM_SUBDIR = "5726__oldbassman__wurlitzer-200a"


def clip_bounds(clips, lengths=None, onset_frac=0.10, offset_frac=0.01, device=0):
    """ow_clip_bounds: (peak, first, last) per clip.  clips: a float64 matrix, or a list of 1-D arrays of any lengths (packed into rows
    here); lengths: samples of each row that are audio (default: the whole row / each array's own length).  first: the first index with
    |x| > onset_frac * peak; last: the last index >= 1 with |x| > offset_frac * peak; -1: none."""
    if isinstance(clips, np.ndarray) and clips.ndim == 2:
        rows = np.ascontiguousarray(clips, dtype=np.float64)
        lens = np.full(rows.shape[0], rows.shape[1], dtype=np.uint32) if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint32)
    else:
        arrs = [np.asarray(c, dtype=np.float64).ravel() for c in clips]
        lens = np.array([a.size for a in arrs], dtype=np.uint32)
        rows = np.zeros((len(arrs), max([a.size for a in arrs] + [1])))
        for r, a in enumerate(arrs):
            rows[r, :a.size] = a
    n = rows.shape[0]
    if lens.size != n:
        raise ValueError("clip_bounds: one length per clip")
    peak, first, last = np.zeros(n), np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    lib = binding.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    if lib.ow_clip_bounds(p(rows), n, rows.shape[1], p(lens), float(onset_frac), float(offset_frac), int(device), p(peak), p(first), p(last)) != 0:
        raise OwError(binding.take_error(lib))
    return peak, first, last


def bounds_to_seconds(peak, first, last, length, sr):
    """(onset_s, offset_s) of detect_obm_onset / detect_obm_offset (extract_notes.py:43-64) from one clip's bounds, fallbacks included."""
    if peak < 1e-10:
        return 0.0, length / sr
    return (first / sr if first >= 0 else 0.0), (last / sr if last >= 0 else length / sr)


def detect_obm_bounds(clips, sr, device=0):
    """[(onset_s, offset_s)] of many clips (a list of 1-D arrays) in one device call."""
    peak, first, last = clip_bounds(clips, device=device)
    return [bounds_to_seconds(float(peak[i]), int(first[i]), int(last[i]), len(clips[i]), sr) for i in range(len(clips))]


def sustain_windows(clips, sr, onset_offset_ms=150, sustain_end_ms=800, device=0):
    """extract_sustain_window (goertzel_utils.py:139-159) of many clips in one device call: [(start, end, onset_idx)], the window being
    clip[start:end]; a silent clip (peak < 1e-10) gives the whole clip and onset 0, as there."""
    peak, first, _ = clip_bounds(clips, device=device)
    out = []
    for i, clip in enumerate(clips):
        n = len(clip)
        if peak[i] < 1e-10:
            out.append((0, n, 0))
            continue
        onset_idx = max(int(first[i]), 0)
        start = onset_idx + int(onset_offset_ms * sr / 1000)
        end = min(onset_idx + int(sustain_end_ms * sr / 1000), n)
        if start >= end:
            start = max(0, end - int(0.2 * sr))
        out.append((start, end, onset_idx))
    return out


def extract_obm_notes(audio_by_name, obm_dir="", device=0):
    """extract_obm_notes (extract_notes.py:67-91) on audio that is already in memory: audio_by_name[file name] = (data, sr).  A name of
    the OBM table that is missing is reported and skipped, as a missing file is there."""
    todo = []
    for fname, midi, f0 in sorted(OBM_FILES, key=lambda x: x[1]):
        path = os.path.join(obm_dir, fname)
        if fname not in audio_by_name:
            print(f"  WARNING: missing {path}")
            continue
        todo.append((fname, midi, f0, path))
    notes = []
    if not todo:
        return notes
    clips = [np.asarray(audio_by_name[t[0]][0], dtype=np.float64) for t in todo]
    peak, first, last = clip_bounds(clips, device=device)
    for i, (fname, midi, f0, path) in enumerate(todo):
        sr = audio_by_name[fname][1]
        onset_s, offset_s = bounds_to_seconds(float(peak[i]), int(first[i]), int(last[i]), len(clips[i]), sr)
        notes.append({
            "id": f"obm_{midi}",
            "onset_s": round(onset_s, 4),
            "offset_s": round(offset_s, 4),
            "midi_note": midi,
            "measured_f0": f0,
            "amplitude": 0.63,
            "velocity_midi": 80,
            "source_file": os.path.abspath(path),
            "source_type": "obm_isolated",
            "isolation_tier": "gold",
        })
        print(f"  OBM {midi:>3} ({fname}): onset={onset_s:.3f}s  dur={offset_s - onset_s:.2f}s")
    return notes


def notes_from_events(events, audio_path):
    """The dictionaries extract_polyphonic_notes (extract_notes.py:192-209) builds from basic_pitch's note events; events: rows of
    (start_s, end_s, pitch_midi, amplitude) (a fifth entry, the pitch bends, is ignored as there)."""
    notes = []
    basename = os.path.splitext(os.path.basename(audio_path))[0]
    for i, ev in enumerate(events):
        start_s, end_s, pitch_midi, amplitude = ev[0], ev[1], ev[2], ev[3]
        pitch_midi = int(round(pitch_midi))
        velocity_midi = max(1, min(127, int(round(amplitude * 127))))
        notes.append({
            "id": f"{basename}_{i:04d}",
            "onset_s": round(float(start_s), 4),
            "offset_s": round(float(end_s), 4),
            "midi_note": pitch_midi,
            "measured_f0": round(440.0 * 2.0 ** ((pitch_midi - 69) / 12.0), 2),
            "amplitude": round(float(amplitude), 4),
            "velocity_midi": velocity_midi,
            "source_file": os.path.abspath(audio_path),
            "source_type": "basic_pitch",
            "isolation_tier": "pending",
        })
    return notes


def plan_probe_window(note, n_audio, sr):
    """Where correct_octave_errors (:109-120) looks: (start, end), 50-200 ms after the onset, else 0-150 ms; None where the script drops
    the note for having fewer than 128 samples."""
    onset_sample = int(note["onset_s"] * sr)
    start = onset_sample + int(0.050 * sr)
    end = min(onset_sample + int(0.200 * sr), n_audio)
    if end - start < 128:
        start = onset_sample
        end = min(onset_sample + int(0.150 * sr), n_audio)
        if end - start < 128:
            return None
    return start, end


def plan_probes(midi, sr):
    """The four probe frequencies of :124-141, None where the script does not measure: (f0, f0 * 1.37, f0 * 2, f0 / 2)."""
    f0 = midi_to_freq(midi)
    f_noise = f0 * 1.37
    return (f0, f_noise if f_noise < sr / 2 - 200 else None, f0 * 2 if f0 * 2 < sr / 2 - 200 else None, f0 / 2 if f0 / 2 > 30 else None)


def decide(midi, amp_f0, amp_noise, amp_up, amp_down):
    """The decision of :143-158 on the four amplitudes (amp_noise already floored at 1e-20; 0.0 for a probe not taken): the MIDI note to
    keep, or None to drop the note."""
    best_amp, best_midi = amp_f0, midi
    if amp_up > amp_f0 * 2.0 and amp_up > amp_noise * 5:
        best_amp, best_midi = amp_up, midi + 12
    elif amp_down > amp_f0 * 2.0 and amp_down > amp_noise * 5:
        best_amp, best_midi = amp_down, midi - 12
    if best_amp / max(amp_noise, 1e-20) < 3.0:
        return None
    return best_midi


def probe_amplitudes(notes, audio, sr, device=0):
    """[(amp_f0, amp_noise, amp_up, amp_down) or None] per note: every probe of every note in one features.extract_segments call."""
    audio = np.ascontiguousarray(audio, dtype=np.float64)
    segs, where = [], []
    for note in notes:
        win = plan_probe_window(note, len(audio), sr)
        if win is None or win[0] < 0 or win[0] >= len(audio):      # a slice of the audio that holds fewer than 128 samples
            where.append(None)
            continue
        idx = []
        for f in plan_probes(note["midi_note"], sr):
            idx.append(None if f is None else len(segs))
            if f is not None:
                segs.append((0, win[0], win[1], 1, f))
        where.append(idx)
    amps, _, _ = features.extract_segments(audio[None, :], sr, segs, 0.01, device)
    out = []
    for idx in where:
        if idx is None:
            out.append(None)
            continue
        a = [None if k is None else float(amps[k, 0]) for k in idx]
        out.append((a[0], 1e-20 if a[1] is None else max(a[1], 1e-20), 0.0 if a[2] is None else a[2], 0.0 if a[3] is None else a[3]))
    return out


def correct_octave_errors(notes, audio, sr, device=0):
    """Drop-in for extract_notes.correct_octave_errors: modifies `notes` in place, returns (corrected_count, removed_count)."""
    probes = probe_amplitudes(notes, audio, sr, device)
    corrected, to_remove = 0, []
    for i, (note, amps) in enumerate(zip(notes, probes)):
        midi = note["midi_note"]
        best_midi = None if amps is None else decide(midi, *amps)
        if best_midi is None:
            to_remove.append(i)
            continue
        if best_midi != midi:
            note["midi_note"] = best_midi
            note["measured_f0"] = round(midi_to_freq(best_midi), 2)
            note["octave_corrected"] = midi
            corrected += 1
    for i in reversed(to_remove):
        notes.pop(i)
    return corrected, len(to_remove)


def extract_polyphonic_notes(audio_path, events, device=0):
    """extract_polyphonic_notes (:174-220) with the transcriber's note events given: dictionaries, pitch check, the script's lines."""
    notes = notes_from_events(events, audio_path)
    print(f"    -> {len(notes)} notes detected, verifying pitches...")
    audio, sr = load_audio(audio_path)
    corrected, removed = correct_octave_errors(notes, audio, sr, device)
    print(f"    -> {corrected} octave-corrected, {removed} weak-removed, {len(notes)} kept")
    return notes
