"""`preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep` on the device (tools/preamp-bench/src/main.rs:150-369): the reference's
flags and defaults, its stdout and its CSV.  Every point of a command runs in one ow_preamp_measure call.

  python tools/preamp_bench.py gain          [--freq 1000] [--amplitude 0.001] [--ldr 1000000]
  python tools/preamp_bench.py sweep         [--start 20] [--end 20000] [--points 50] [--ldr 1000000] [--amplitude 0.001] [--csv FILE]
  python tools/preamp_bench.py harmonics     [--freq 440] [--amplitude 0.005] [--ldr 1000000]
  python tools/preamp_bench.py tremolo-sweep [--ldr-min 19000] [--ldr-max 1000000] [--steps 20] [--freq 1000] [--amplitude 0.001] [--csv FILE]
  python tools/preamp_bench.py surface       [--start 20] [--end 20000] [--points 50] [--ldr-min 19000] [--ldr-max 1000000] [--steps 20]
                                             [--amplitude 0.001] [--csv FILE]
      (this project's addition, not a command of the reference: the gain over the frequency x LDR plane in one call; row R of the
       surface is `sweep --ldr R` over the same frequencies.  CSV ldr_ohm,freq_hz,gain_db with {:.0},{:.1},{:.2})
  all: [--model dk|dk-legacy] [--preamp legacy|melange]: what `--model dk` means (the reference's `melange-preamp` cargo feature;
       dk-legacy is always legacy) [--device N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _count(x):
    """`parse_flag(..) as usize`: truncation toward zero, negative values saturate to 0."""
    return int(x) if x > 0 else 0


def main(argv=None):
    from openwurli_amd import preamp_bench as pb
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", choices=("gain", "sweep", "harmonics", "tremolo-sweep", "surface"),
                    help="the reference's four commands; `surface` is this project's addition (not a command of the reference)")
    ap.add_argument("--freq", type=float)
    ap.add_argument("--amplitude", type=float)
    ap.add_argument("--ldr", type=float, default=1_000_000.0)
    ap.add_argument("--start", type=float, default=20.0)
    ap.add_argument("--end", type=float, default=20000.0)
    ap.add_argument("--points", type=float, default=50.0)
    ap.add_argument("--ldr-min", type=float, default=19_000.0)
    ap.add_argument("--ldr-max", type=float, default=1_000_000.0)
    ap.add_argument("--steps", type=float, default=20.0)
    ap.add_argument("--csv", default="")
    ap.add_argument("--model", default="dk", choices=("dk", "dk-legacy"))
    ap.add_argument("--preamp", default="legacy", choices=("legacy", "melange"))
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    kind = pb.PREAMP_MELANGE12 if (a.model == "dk" and a.preamp == "melange") else pb.PREAMP_LEGACY8
    csv = None
    if a.command == "gain":
        row = pb.measure_gain(a.freq if a.freq is not None else 1000.0, a.amplitude if a.amplitude is not None else 0.001, a.ldr, kind, a.device)
        sys.stdout.write(pb.format_gain(row))
    elif a.command == "sweep":
        rows = pb.sweep(a.start, a.end, _count(a.points), a.ldr, a.amplitude if a.amplitude is not None else 0.001, kind, a.device)
        sys.stdout.write(pb.format_sweep(rows, a.ldr))
        csv = pb.format_sweep_csv(rows)
    elif a.command == "harmonics":
        row = pb.harmonics(a.freq if a.freq is not None else 440.0, a.amplitude if a.amplitude is not None else 0.005, a.ldr, kind, a.device)
        sys.stdout.write(pb.format_harmonics(row))
    elif a.command == "tremolo-sweep":
        rows = pb.tremolo_sweep(a.ldr_min, a.ldr_max, _count(a.steps), a.freq if a.freq is not None else 1000.0,
                                a.amplitude if a.amplitude is not None else 0.001, kind, a.device)
        sys.stdout.write(pb.format_tremolo_sweep(rows))
        csv = pb.format_tremolo_sweep_csv(rows)
    else:
        freqs = pb.log_spaced(a.start, a.end, _count(a.points))
        rs = pb.log_spaced(a.ldr_min, a.ldr_max, _count(a.steps))
        g = pb.response_surface(freqs, rs, a.amplitude if a.amplitude is not None else 0.001, kind, a.device)
        csv = pb.format_surface_csv(freqs, rs, g)
        print(f"Response surface: {len(rs)} LDR x {len(freqs)} frequencies = {g.size} points")
    if csv is not None and a.csv:
        with open(a.csv, "w", newline="") as f:
            f.write(csv)
        print(f"\nCSV written to {a.csv}")


if __name__ == "__main__":
    main()
