"""`preamp-bench calibrate` / `preamp-bench sensitivity` on the device (tools/preamp-bench/src/main.rs:1069-1395): the reference's
flags, the reference's CSV.  Every grid point of a run -- a whole sensitivity sweep included -- renders in one ow_calibrate call.

  python tools/calibrate.py calibrate   [--notes 36,40,...] [--velocities 40,80,127] [--ds-at-c4 0.75] [--ds-clamp-max 0.82] [--zero-trim]
  python tools/calibrate.py sensitivity [--notes ...] [--velocities ...] [--ds-range 0.50,...,0.85] [--scale-mode track|zero-trim|freeze]
                                        [--zero-trim]
  both: [--volume 0.40] [--speaker 1.0] [--model dk|dk-legacy] [--output FILE] [--mlp (parsed and ignored, as in the reference)]
        [--preamp legacy|melange]: what `--model dk` means (the reference's `melange-preamp` cargo feature; dk-legacy is always legacy)
        [--power-amp behavioral|melange]: the build's PowerAmp (the `legacy-power-amp` cargo feature) [--device N]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ints(s):
    return [int(v) for v in s.split(",") if v.strip()]


def _floats(s):
    return [float(v) for v in s.split(",") if v.strip()]


def main(argv=None):
    from openwurli_amd import calibrate as cal
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", choices=("calibrate", "sensitivity"))
    ap.add_argument("--notes")
    ap.add_argument("--velocities", default="40,80,127")
    ap.add_argument("--ds-at-c4", type=float, default=0.75)
    ap.add_argument("--ds-clamp-max", type=float, default=0.82)
    ap.add_argument("--ds-range", default=",".join("%.2f" % d for d in cal.SENSITIVITY_DS))
    ap.add_argument("--scale-mode", default="track")
    ap.add_argument("--zero-trim", action="store_true")
    ap.add_argument("--volume", type=float, default=0.40)
    ap.add_argument("--speaker", type=float, default=1.0)
    ap.add_argument("--model", default="dk", choices=("dk", "dk-legacy"))
    ap.add_argument("--preamp", default="legacy", choices=("legacy", "melange"))
    ap.add_argument("--power-amp", default="behavioral", choices=("behavioral", "melange"))
    ap.add_argument("--mlp", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--output")
    a = ap.parse_args(argv)
    preamp = cal.PREAMP_MELANGE12 if (a.model == "dk" and a.preamp == "melange") else cal.PREAMP_LEGACY8
    pa = cal.POWER_AMP_MELANGE if a.power_amp == "melange" else cal.POWER_AMP_BEHAVIORAL
    vels = _ints(a.velocities)
    t0 = time.perf_counter()
    if a.command == "calibrate":
        notes = _ints(a.notes) if a.notes else list(cal.CALIBRATE_NOTES)
        rows = cal.calibrate(notes, vels, a.ds_at_c4, a.ds_clamp_max, a.volume, a.speaker, a.zero_trim, preamp, pa, a.device)
        what = f"Calibrate: {len(notes)} notes × {len(vels)} velocities = {len(rows)} rows"
    else:
        notes = _ints(a.notes) if a.notes else list(cal.SENSITIVITY_NOTES)
        ds = _floats(a.ds_range)
        rows = cal.sensitivity(notes, vels, ds, a.scale_mode, a.zero_trim, a.volume, a.speaker, preamp, pa, a.device)
        what = f"Sensitivity: {len(ds)} DS × {len(notes)} notes × {len(vels)} vel = {len(rows)} rows"
    dt = time.perf_counter() - t0
    out = a.output or os.path.join(tempfile.gettempdir(), a.command + ".csv")
    cal.write_calibrate_csv(out, rows)
    print(f"{what} → {out}  ({dt * 1e3:.1f} ms)", file=sys.stderr)


if __name__ == "__main__":
    main()
