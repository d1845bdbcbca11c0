"""`preamp-bench render-poly` on the device (tools/preamp-bench/src/main.rs:1397-1592): the reference's flags and defaults, its stdout
and its two WAV files (X.wav and X_residual.wav).

  python tools/render_poly.py [--notes 38,59,62,66] [--velocities 45,40,40,40] [--duration 3.0] [--volume 0.60] [--speaker 1.0]
                              [--ldr 1000000] [--no-poweramp] [--normalize] [--output FILE.wav]
  python tools/render_poly.py grid [--lo 33] [--hi 96] [--velocities 80,80] [--duration 3.0] [--volume 0.60] [--speaker 1.0]
                              [--ldr 1000000] [--no-poweramp] --csv FILE
      (this project's addition, not a command of the reference: every dyad of the notes lo..hi in ONE call; CSV
       note_a,note_b,vel_a,vel_b,intermod_ratio_db)
  both: [--device N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from openwurli_amd import render_poly as rp
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", nargs="?", default="render", choices=("render", "grid"),
                    help="`render` (default) is the reference's command; `grid` is this project's addition")
    ap.add_argument("--notes", default="38,59,62,66")
    ap.add_argument("--velocities", default=None)
    ap.add_argument("--duration", type=float, default=3.0)
    ap.add_argument("--volume", type=float, default=0.60)
    ap.add_argument("--speaker", type=float, default=1.0)
    ap.add_argument("--ldr", type=float, default=1_000_000.0)
    ap.add_argument("--no-poweramp", action="store_true")
    ap.add_argument("--normalize", action="store_true")
    ap.add_argument("--output", default=None)
    ap.add_argument("--lo", type=int, default=33)
    ap.add_argument("--hi", type=int, default=96)
    ap.add_argument("--csv", default="")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.command == "grid":
        vel = rp.parse_csv_u8(a.velocities if a.velocities is not None else "80,80")
        chords = rp.dyad_grid(a.lo, a.hi, vel, a.volume, a.speaker, a.ldr, a.no_poweramp)
        rows = rp.run_chords(chords, a.duration, a.device)
        print(f"Intermod grid: {chords.size} dyads of notes {a.lo}..{a.hi}, {a.duration:.1f}s each")
        if a.csv:
            with open(a.csv, "w", newline="") as f:
                f.write(rp.format_grid_csv(chords, rows))
            print(f"CSV written to {a.csv}")
        else:
            sys.stdout.write(rp.format_grid_csv(chords, rows))
        return
    notes = rp.parse_csv_u8(a.notes)
    vel = rp.parse_csv_u8(a.velocities if a.velocities is not None else "45,40,40,40")
    r = rp.render_poly(notes, vel, a.duration, a.volume, a.speaker, a.ldr, a.no_poweramp, a.normalize, a.output or rp.default_output(), a.device)
    sys.stdout.write(r["report"])


if __name__ == "__main__":
    main()
