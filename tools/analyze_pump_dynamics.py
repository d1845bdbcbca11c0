"""The reference's tools/analyze_pump_dynamics.py on the device: fit its six pump predictors to slewed-R captures by Nelder-Mead, every
fit of the run in one library call (openwurli_amd/pump_fit.py, `ow_pump_fit`).

  python tools/analyze_pump_dynamics.py [--lut /tmp/pump_sweep_88k2.csv] [--sin-dir /tmp/pump_sin] [--results /tmp/pump_fit_results.csv]
        the reference's script: its two kinds of CSV in, its table, its "fitted parameters" section and its results CSV out
  python tools/analyze_pump_dynamics.py --from-device --freqs 2,4,5.6,8 [--ldr-min 19000] [--ldr-max 1000000] [--cycles 10]
        [--sample-rate 88200] [--settle 750000] [--lut-points 256] [--lut-settle 60000] [--lut-avg 4096] [--write-csv DIR]
        the table (pump-sweep at the captures' rate) and the captures (pump-sinusoid per frequency) are measured on the device in
        two `ow_pump_measure` calls and fitted at once; the numbers are those the commands' CSV files carry.  --write-csv also writes
        those files (DIR/pump_sweep_88k2.csv, DIR/pump_sin/sin_<freq>.csv).
  python tools/analyze_pump_dynamics.py grid --starts K --csv FILE [--seed 0] [either input]
        K starts per (capture, model): the reference's x0, then seeded log-uniform draws in the per-model boxes of
        openwurli_amd/pump_fit.py (START_BOXES).  One CSV row per start, the best of each (capture, model) marked.
  all: [--device N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sin_name(freq) -> str:
    return f"sin_{int(round(float(freq) * 1000)):08d}.csv"      # sorted by path = sorted by frequency


def main(argv=None):
    from openwurli_amd import pump_fit
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", nargs="?", choices=["grid"])
    ap.add_argument("--lut", default=pump_fit.LUT_CSV)
    ap.add_argument("--sin-dir", default=pump_fit.SIN_DIR)
    ap.add_argument("--results", default=pump_fit.RESULTS_CSV)
    ap.add_argument("--from-device", action="store_true")
    ap.add_argument("--freqs", type=lambda s: [float(x) for x in s.split(",")], default=None)
    ap.add_argument("--ldr-min", type=float, default=19_000.0)
    ap.add_argument("--ldr-max", type=float, default=1_000_000.0)
    ap.add_argument("--cycles", type=float, default=10.0)
    ap.add_argument("--sample-rate", type=float, default=88_200.0)
    ap.add_argument("--settle", type=int, default=750_000)
    ap.add_argument("--lut-points", type=int, default=256)
    ap.add_argument("--lut-settle", type=int, default=60_000)
    ap.add_argument("--lut-avg", type=int, default=4_096)
    ap.add_argument("--write-csv", default=None)
    ap.add_argument("--starts", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--csv", default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.command == "grid" and (a.starts is None or a.csv is None):
        ap.error("grid needs --starts K and --csv FILE")

    inputs = None
    if a.from_device:
        if not a.freqs:
            ap.error("--from-device needs --freqs")
        inputs = pump_fit.device_inputs(sorted(a.freqs), a.ldr_min, a.ldr_max, a.cycles, a.sample_rate, a.settle, a.lut_points, a.lut_settle, a.lut_avg,
                                        a.device)
        table, traces = inputs["lut"], inputs["traces"]
        if a.write_csv:
            os.makedirs(os.path.join(a.write_csv, "pump_sin"), exist_ok=True)
            with open(os.path.join(a.write_csv, "pump_sweep_88k2.csv"), "w", newline="") as f:
                f.write(inputs["lut_csv"])
            for freq, text in zip(sorted(a.freqs), inputs["sin_csvs"]):
                with open(os.path.join(a.write_csv, "pump_sin", sin_name(freq)), "w", newline="") as f:
                    f.write(text)
    elif a.command == "grid":
        import glob
        table = pump_fit.load_lut(a.lut)
        traces = [pump_fit.load_sinusoid(p) for p in sorted(glob.glob(os.path.join(a.sin_dir, "sin_*.csv")))]

    if a.command == "grid":
        rows = pump_fit.grid(traces, table, a.starts, a.seed, device=a.device)
        text = pump_fit.format_grid_csv(rows, traces)
        with open(a.csv, "w", newline="") as f:
            f.write(text)
        for q in rows:
            if q["best"]:
                print(f"{traces[q['trace']].get('freq'):>7.1f}  {q['model']:>12s}  best of {a.starts}: start {q['start']:3d}  RMSE = {q['fun']:9.3f} mV  "
                      f"({pump_fit.STATUS_NAMES[q['status']]}, nit {q['nit']})")
        print(f"\nWrote grid CSV → {a.csv}")
        return {"rows": rows, "csv_text": text, "traces": traces, "lut": table, "inputs": inputs}

    if a.from_device:
        rows = pump_fit.analyze(traces, table, a.device)
        text = pump_fit.format_results_csv(rows)
        with open(a.results, "w", newline="") as f:
            f.write(text)
        out = {"lut": table, "traces": traces, "rows": rows, "report": pump_fit.format_report(table, rows, a.results), "csv_text": text, "csv": a.results,
               "inputs": inputs}
    else:
        try:
            out = pump_fit.analyze_files(a.lut, a.sin_dir, a.results, a.device)
        except FileNotFoundError as e:
            print(e, file=sys.stderr)
            sys.exit(1)
    sys.stdout.write(out["report"])
    return out


if __name__ == "__main__":
    main()
