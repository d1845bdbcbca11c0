"""`preamp-bench intermod-audit` on the device (tools/preamp-bench/src/main.rs:675-903): the reference's flags and defaults, its stdout.

  python tools/intermod_audit.py [--threshold 0.07] [--render] [--duration 3.0] [--notes 36,48,...]
  python tools/intermod_audit.py grid --csv FILE [--notes 33..96] [--velocities 20,35,50,65,80,95,110,127] [--duration 3.0]
      (this project's addition, not a command of the reference: notes x velocities in ONE call; CSV
       note,velocity,h_db,m_db,ratio_db,verdict)
  both: [--device N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_note_range(text):
    """`a..b` (inclusive) or a comma-separated list."""
    from openwurli_amd._rust_text import parse_csv_u8
    if ".." in text:
        lo, hi = text.split("..", 1)
        return list(range(int(lo), int(hi) + 1))
    return parse_csv_u8(text)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", nargs="?", default="audit", choices=("audit", "grid"),
                    help="`audit` (default) is the reference's command; `grid` is this project's addition")
    ap.add_argument("--threshold", type=float, default=0.07)
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--duration", type=float, default=3.0)
    ap.add_argument("--notes", default=None)
    ap.add_argument("--velocities", default="20,35,50,65,80,95,110,127")
    ap.add_argument("--csv", default="")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None):
    from openwurli_amd import intermod_audit as ia
    a = parse_args(argv)
    if a.command == "grid":
        notes = parse_note_range(a.notes) if a.notes is not None else list(range(ia.MIDI_LO, ia.MIDI_HI + 1))
        rows = ia.audit(notes, ia.parse_csv_u8(a.velocities), a.duration, a.device)
        text = ia.format_grid_csv(rows)
        if a.csv:
            with open(a.csv, "w", newline="") as f:
                f.write(text)
            print(f"Intermod grid: {rows.size} (note, velocity) pairs, CSV written to {a.csv}")
        else:
            sys.stdout.write(text)
        return
    notes = ia.parse_csv_u8(a.notes) if a.notes is not None else None          # has_flag(--notes): parse_csv_list(args, "--notes", "")
    sys.stdout.write(ia.report(a.threshold, a.render, a.duration, notes, a.device))


if __name__ == "__main__":
    main()
