"""`preamp-bench bark-audit` on the device (tools/preamp-bench/src/main.rs:551-664): the reference's flags and defaults, its stdout.

  python tools/bark_audit.py [--notes 36,48,60,72,84] [--velocities 40,80,100,127]
  python tools/bark_audit.py grid --csv FILE [--notes 33..96] [--velocities 20,35,50,65,80,95,110,127]
      (this project's addition, not a command of the reference: notes x velocity layers x both preamp models, one call per model; CSV
       note,velocity,model,reed_peak,y_peak,pu_h2_h1_pct,pu_peak_mv,pre_h2_h1_pct)
  both: [--model dk|dk-legacy] [--preamp legacy|melange]: what `--model dk` means (the reference's `melange-preamp` cargo feature;
        dk-legacy is always legacy; `grid` runs both models and ignores the two flags) [--device N]
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
    ap.add_argument("--notes", default=None)
    ap.add_argument("--velocities", default=None)
    ap.add_argument("--model", default="dk", choices=("dk", "dk-legacy"))
    ap.add_argument("--preamp", default="legacy", choices=("legacy", "melange"))
    ap.add_argument("--csv", default="")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None):
    from openwurli_amd import bark_audit as ba
    a = parse_args(argv)
    if a.command == "grid":
        notes = parse_note_range(a.notes) if a.notes is not None else list(range(33, 97))
        vels = ba.parse_csv_u8(a.velocities) if a.velocities is not None else list(ba.ML_VELOCITIES)
        by_kind, text = ba.grid(notes, vels, device=a.device)
        if a.csv:
            with open(a.csv, "w", newline="") as f:
                f.write(text)
            print(f"Bark grid: {sum(r.size for _, r in by_kind)} (note, velocity, model) rows, CSV written to {a.csv}")
        else:
            sys.stdout.write(text)
        return
    kind = ba.PREAMP_MELANGE12 if (a.model == "dk" and a.preamp == "melange") else ba.PREAMP_LEGACY8
    notes = ba.parse_csv_u8(a.notes if a.notes is not None else "36,48,60,72,84")
    vels = ba.parse_csv_u8(a.velocities if a.velocities is not None else "40,80,100,127")
    sys.stdout.write(ba.report(notes, vels, kind, device=a.device))


if __name__ == "__main__":
    main()
