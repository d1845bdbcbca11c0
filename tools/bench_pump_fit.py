"""Times the pump-dynamics fitter on the device and sets the reference's algorithm on the CPU beside it.  Prints one JSON line.

Device (each step in a child process under its own time limit; the tool stops at the first that fails):
  inputs    the table (pump-sweep, 256 points at 88.2 kHz) and one pump-sinusoid capture per frequency (10 cycles: 157 500 samples at
            5.6 Hz), made on the device and kept for the other steps
  default   the reference's default workload: captures x 6 models from its x0, one `ow_pump_fit` call      (timed: the whole call)
  starts    the same with --starts starts per (capture, model), one call                                   (timed: the whole call)
  lone      one fit (iir1_dlnR on the 5.6 Hz capture, or the capture nearest to it), one call             (timed: the whole call)
  The per-sample cost of the eight-lane pass is lone's time over (nit x samples): upload, table preparation and the start pass included.

CPU: the reference runs every loss evaluation as an interpreted loop over the trace.  Timed here: --cpu-evals loss evaluations per
(capture, model) of the restatement (tests/pump_fit_ref.py: the same recurrences as plain Python loops over lists, which run faster than
the reference's loops over numpy scalars), one process, one thread.  SCALED BY COUNT, not timed: that time per evaluation times the nfev
the device reports for each fit, summed -- what the same search costs at that rate.

  python tools/bench_pump_fit.py [--freqs 2,4,5.6,8] [--starts 64] [--settle 750000] [--cpu-evals 2] [--no-cpu] [--limit 600] [--device N]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

_STEP = """
import json, sys, time
import numpy as np
sys.path.insert(0, %r)
from openwurli_amd import pump_fit
which, path, dev, starts, settle = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
freqs = [float(x) for x in sys.argv[6].split(",")]
t0 = time.perf_counter()
if which == "inputs":
    d = pump_fit.device_inputs(freqs, settle=settle, device=dev)
    np.savez(path, lut_r=d["lut"][0], lut_v=d["lut"][1], n=len(freqs), **{"r%%d" %% i: t["r"] for i, t in enumerate(d["traces"])},
             **{"y%%d" %% i: t["target"] for i, t in enumerate(d["traces"])})
    out = {"samples": [int(t["r"].size) for t in d["traces"]]}
else:
    z = np.load(path)
    traces = [{"r": z["r%%d" %% i], "target": z["y%%d" %% i], "sr": 88200.0, "freq": f} for i, f in enumerate(freqs)]
    lut = (z["lut_r"], z["lut_v"])
    pump_fit.evaluate(traces[:1], lut, [(0, 0, [50.0])], device=dev)          # loads the library, creates the context
    t0 = time.perf_counter()
    if which == "default":
        rows = pump_fit.fit(traces, lut, [(t, m, pump_fit.X0[m]) for t in range(len(traces)) for m in range(6)], device=dev)
    elif which == "starts":
        rows = pump_fit.grid(traces, lut, starts, device=dev)
    else:
        i = min(range(len(freqs)), key=lambda k: abs(freqs[k] - 5.6))
        rows = pump_fit.fit(traces[i:i + 1], lut, [(0, 3, pump_fit.X0[3])], device=dev)
        for q in rows:
            q["trace"] = i
    out = {"fits": len(rows), "nit_max": max(q["nit"] for q in rows), "nit_sum": sum(q["nit"] for q in rows), "nfev_sum": sum(q["nfev"] for q in rows),
           "status": [sum(q["status"] == s for q in rows) for s in range(3)],
           "nfev": [[q["trace"], pump_fit.MODELS.index(q["model"]), q["nfev"], q["nit"]] for q in rows] if which != "starts" else None}
out["wall_s"] = round(time.perf_counter() - t0, 4)
print(json.dumps(out))
"""


def device_step(which, path, a):
    try:
        p = subprocess.run([sys.executable, "-c", _STEP % ROOT, which, path, str(a.device), str(a.starts), str(a.settle), a.freqs], capture_output=True,
                           text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_pump_fit: the {which} step exceeded its limit of {a.limit} s; stopping")
    if p.returncode != 0:
        raise SystemExit(f"bench_pump_fit: the {which} step ended with status {p.returncode}; stopping\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def cpu_seconds_per_eval(path, freqs, n_evals):
    """[trace][model] seconds of one loss evaluation of the restatement at the reference's x0 (a valid neighbour for the biquad)."""
    import numpy as np
    import pump_fit_ref as ref
    z = np.load(path)
    table = ref.Table(z["lut_r"], z["lut_v"])
    out = []
    for i in range(len(freqs)):
        prob = ref.Problem(z[f"r{i}"], 88200.0, z[f"y{i}"], table)
        row = []
        for m in range(6):
            p = ref.X0[m] if m < 5 else [1.9, -0.905, -1.0, 0.5]
            t0 = time.perf_counter()
            for _ in range(n_evals):
                prob.loss(m, p)
            row.append((time.perf_counter() - t0) / n_evals)
        out.append(row)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--freqs", default="2,4,5.6,8")
    ap.add_argument("--starts", type=int, default=64)
    ap.add_argument("--settle", type=int, default=750_000)
    ap.add_argument("--cpu-evals", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    freqs = [float(x) for x in a.freqs.split(",")]
    out = {"freqs": freqs, "starts": a.starts}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "inputs.npz")
        for which in ("inputs", "default", "starts", "lone"):
            out[which] = device_step(which, path, a)
            print(f"bench_pump_fit: {which} {out[which]['wall_s']} s", file=sys.stderr, flush=True)
        lone = out["lone"]
        n = out["inputs"]["samples"][lone["nfev"][0][0]]
        out["ns_per_sample_pass"] = round(lone["wall_s"] / (lone["nit_sum"] * n) * 1e9, 2)
        if not a.no_cpu:
            per = cpu_seconds_per_eval(path, freqs, a.cpu_evals)
            out["cpu_s_per_eval_timed"] = [[round(v, 4) for v in row] for row in per]
            scaled = sum(per[t][m] * nfev for t, m, nfev, _ in out["default"]["nfev"])
            out["cpu_default_s_scaled_by_nfev"] = round(scaled, 1)
            out["default_speedup_scaled"] = round(scaled / out["default"]["wall_s"], 1)
            t, m, nfev, _ = lone["nfev"][0]
            out["cpu_lone_s_scaled_by_nfev"] = round(per[t][m] * nfev, 1)
    for k in ("default", "lone"):
        out[k].pop("nfev")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
