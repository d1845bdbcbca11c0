"""`preamp-bench centroid-track` on the device (tools/preamp-bench/src/main.rs:1925-2135): the reference's flags and defaults, its stdout
and its CSV.

  python tools/centroid_track.py [--note 60] [--velocity 100] [--duration 1.0] [--window-ms 5.0] [--hop-ms 2.5] [--end-ms 500.0]
                                 [--ldr 1000000] [--volume 0.60] [--speaker 1.0] [--no-poweramp] [--no-preamp]
                                 [--displacement-scale [0.30]] [--csv FILE]
  python tools/centroid_track.py grid [--lo 33] [--hi 96] [--velocities 20,35,50,65,80,95,110,127] [the flags above but --note /
                                 --velocity] [--csv FILE]
      (this project's addition, not a command of the reference: notes x velocities in ONE call; CSV
       note,velocity,c10,c300,drift,attack_status,sustain_status,drift_status)
  both: [--device N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from openwurli_amd import centroid_track as ct
    from openwurli_amd.render_poly import parse_csv_u8
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", nargs="?", default="track", choices=("track", "grid"),
                    help="`track` (default) is the reference's command; `grid` is this project's addition")
    ap.add_argument("--note", type=int, default=60)
    ap.add_argument("--velocity", type=int, default=100)
    ap.add_argument("--duration", type=float, default=1.0)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--hop-ms", type=float, default=2.5)
    ap.add_argument("--end-ms", type=float, default=500.0)
    ap.add_argument("--ldr", type=float, default=1_000_000.0)
    ap.add_argument("--volume", type=float, default=0.60)
    ap.add_argument("--speaker", type=float, default=1.0)
    ap.add_argument("--no-poweramp", action="store_true")
    ap.add_argument("--no-preamp", action="store_true")
    ap.add_argument("--displacement-scale", type=float, nargs="?", const=0.30, default=None)
    ap.add_argument("--csv", default="")
    ap.add_argument("--lo", type=int, default=33)
    ap.add_argument("--hi", type=int, default=96)
    ap.add_argument("--velocities", default=",".join(str(v) for v in ct.ML_VELOCITIES))
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.command == "grid":
        jobs = ct.grid_jobs(range(a.lo, a.hi + 1), parse_csv_u8(a.velocities), a.volume, a.speaker, a.ldr, a.no_preamp, a.no_poweramp, a.displacement_scale)
        rows, frames = ct.run_jobs(jobs, a.duration, a.window_ms, a.hop_ms, a.end_ms, a.device)
        print(f"Centroid grid: {jobs.size} (note, velocity) pairs, {frames.shape[1]} frames of {ct.rust_display(a.window_ms)}ms each")
        if a.csv:
            with open(a.csv, "w", newline="") as f:
                f.write(ct.format_grid_csv(jobs, rows))
            print(f"CSV written to {a.csv}")
        else:
            sys.stdout.write(ct.format_grid_csv(jobs, rows))
        return
    r = ct.centroid_track(a.note, a.velocity, a.duration, a.window_ms, a.hop_ms, a.end_ms, a.ldr, a.volume, a.speaker, a.no_poweramp, a.no_preamp, a.csv,
                          a.displacement_scale, a.device)
    sys.stdout.write(r["report"])


if __name__ == "__main__":
    main()
