#!/usr/bin/env python3
"""ml/score_isolation.py on the GPU: the same flags, report and scored_notes.json.  All notes of all recordings are scored in one call,
see openwurli_amd/isolation.py.

  python tools/score_isolation.py --input notes.json --output scored_notes.json [--device 0]

Against the reference: paths are taken as given (not relative to the script).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from openwurli_amd import isolation
    ap = argparse.ArgumentParser(description="Score isolation quality for extracted notes")
    ap.add_argument("--input", default="notes.json", help="Input JSON from extract_notes.py")
    ap.add_argument("--output", default="scored_notes.json", help="Output JSON with isolation scores")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    with open(a.input) as f:
        notes = json.load(f)
    print(f"Scoring isolation for {len(notes)} notes...")
    isolation.score_notes(notes, device=a.device)
    isolation.print_summary(notes)
    with open(a.output, "w") as f:
        json.dump(notes, f, indent=2)
    print(f"\nSaved to {a.output}")
    return notes


if __name__ == "__main__":
    main()
