#!/usr/bin/env python3
"""The non-neural half of ml/extract_notes.py on the GPU: the same flags and lines, notes.json as the result.  The bounds of the isolated
OBM notes and the pitch check of transcribed notes run on the device, see openwurli_amd/note_intake.py.

  python tools/extract_notes.py --input-dir input --output notes.json [--events DIR] [--obm-only] [--device 0]

Against the reference: the basic_pitch transcriber is not run here.  Its note events are read from
<--events DIR>/<recording basename>.events.json, a list of [start_s, end_s, pitch_midi, amplitude] (what basic_pitch's note_events hold,
produced elsewhere); a recording without such a file is reported and skipped, as a recording that raises is there.  Paths are taken as
given (not relative to the script); the OBM notes are looked for in <input-dir>/5726__oldbassman__wurlitzer-200a; recordings are PCM WAV
(FLAC is not read).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def find_recordings(input_dir, obm_subdir):
    """The WAV recordings of input_dir and of its sub-directories, one level deep, without the OBM notes, renders and test outputs."""
    found = []
    for entry in sorted(os.listdir(input_dir)):
        path = os.path.join(input_dir, entry)
        if os.path.isdir(path):
            if obm_subdir in entry:
                continue
            found += [os.path.join(path, sub) for sub in sorted(os.listdir(path))
                      if sub.lower().endswith(".wav") and os.path.isfile(os.path.join(path, sub))]
        elif entry.lower().endswith(".wav") and os.path.isfile(path):
            if not any(skip in entry.lower() for skip in ("vurli", "model", "output", "test")):
                found.append(path)
    return found


def main(argv=None):
    from openwurli_amd import note_intake
    ap = argparse.ArgumentParser(description="Extract note events from Wurlitzer recordings")
    ap.add_argument("--input-dir", default="input", help="Directory containing recordings")
    ap.add_argument("--output", default="notes.json", help="Output JSON file")
    ap.add_argument("--obm-only", action="store_true", help="Only extract OBM isolated notes")
    ap.add_argument("--events", default=None, metavar="DIR", help="Directory with <recording basename>.events.json (default: --input-dir)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    events_dir = a.events if a.events is not None else a.input_dir
    all_notes = []

    print("Extracting OBM isolated notes...")
    obm_dir = os.path.join(a.input_dir, note_intake.OBM_SUBDIR)
    obm_audio = {}
    for fname, _, _ in note_intake.OBM_FILES:
        path = os.path.join(obm_dir, fname)
        if os.path.exists(path):
            obm_audio[fname] = note_intake.load_audio(path)
    obm_notes = note_intake.extract_obm_notes(obm_audio, obm_dir, device=a.device)
    all_notes.extend(obm_notes)
    print(f"  {len(obm_notes)} OBM notes extracted")

    if not a.obm_only:
        recordings = find_recordings(a.input_dir, note_intake.OBM_SUBDIR)
        print(f"\nFound {len(recordings)} polyphonic recordings:")
        for r in recordings:
            print(f"  {os.path.basename(r)}")
        for rec_path in recordings:
            try:
                ev_path = os.path.join(events_dir, os.path.splitext(os.path.basename(rec_path))[0] + ".events.json")
                with open(ev_path) as f:
                    events = json.load(f)
                print(f"  Note events of {os.path.basename(rec_path)} from {ev_path}...")
                all_notes.extend(note_intake.extract_polyphonic_notes(rec_path, events, device=a.device))
            except Exception as e:
                print(f"  ERROR processing {rec_path}: {e}")

    print(f"\nTotal: {len(all_notes)} notes")
    by_type = {}
    for n in all_notes:
        by_type[n["source_type"]] = by_type.get(n["source_type"], 0) + 1
    for t, c in sorted(by_type.items()):
        print(f"  {t}: {c}")
    if all_notes:
        midis = [n["midi_note"] for n in all_notes]
        print(f"  MIDI range: {min(midis)}-{max(midis)}")
    with open(a.output, "w") as f:
        json.dump(all_notes, f, indent=2)
    print(f"\nSaved to {a.output}")
    return all_notes


if __name__ == "__main__":
    main()
