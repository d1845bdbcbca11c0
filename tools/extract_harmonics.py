#!/usr/bin/env python3
"""ml/extract_harmonics.py on the GPU: the same flags and report, harmonics.json as the result.  Every segment of every note is
measured in two calls (FFT notes and Goertzel notes), see openwurli_amd/harmonics.py.

  python tools/extract_harmonics.py --input scored_notes.json --output harmonics.json [--min-tier bronze] [--goertzel-all]

Against the reference: paths are taken as given (not relative to the script); source files are PCM WAV (16 / 24 / 32 bit), read with the
standard library and resampled to 44.1 kHz through scipy when their rate differs; --goertzel-all does what its help says (the reference
passes the flag on inverted, so that there it turns Goertzel off).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TIERS = {"gold": 3, "silver": 2, "bronze": 1, "reject": 0, "pending": -1}


def load_files(notes, min_tier, load_audio):
    """The audio of every source file an eligible note names; a file that cannot be read is left out (the extraction reports it)."""
    audio = {}
    for n in notes:
        path = n["source_file"]
        if TIERS.get(n.get("isolation_tier", "reject"), 0) < TIERS.get(min_tier, 1) or path in audio:
            continue
        try:
            audio[path] = load_audio(path)
        except Exception as e:
            print(f"  could not read {path}: {e}")
    return audio


def main(argv=None):
    from openwurli_amd import harmonics
    ap = argparse.ArgumentParser(description="Extract harmonic features from scored notes")
    ap.add_argument("--input", default="scored_notes.json", help="Input JSON from score_isolation.py")
    ap.add_argument("--output", default="harmonics.json", help="Output JSON with harmonic features")
    ap.add_argument("--min-tier", default="bronze", choices=["gold", "silver", "bronze"], help="Minimum isolation tier to extract")
    ap.add_argument("--goertzel-all", action="store_true", help="Use Goertzel for all notes (slow but precise)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    with open(a.input) as f:
        notes = json.load(f)
    audio = load_files(notes, a.min_tier, harmonics.load_audio)
    feats = harmonics.extract_all_harmonics(notes, audio, min_tier=a.min_tier, use_goertzel_for_gold=True, device=a.device, goertzel_all=a.goertzel_all)
    harmonics.print_summary(feats)
    with open(a.output, "w") as f:
        json.dump(feats, f, indent=2)
    print(f"\nSaved to {a.output}")
    return feats


if __name__ == "__main__":
    main()
