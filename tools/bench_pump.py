"""Times the default `pump-sweep` (256 points, 64 096 samples each) and the default `pump-spike` (832 points of about 408 000 samples, and
the slew) once on the device, and the CPU restatement (tests/c/pump_ref.cpp) of the same points on at most 16 host threads.  Prints one
JSON line.

Every device step runs in a child process under its own time limit, and the tool stops at the first one that fails.  A step is one or two
library calls that say nothing until they return (the 48 kHz launch of pump-spike alone runs for minutes: its 47.5 kOhm points exhaust Newton's
265 sweeps on most of their 408 192 samples), so the tool reports on stderr every 30 s that the step is still inside its limit.

  python tools/bench_pump.py [--no-cpu] [--cpu-points N] [--sweep-limit S] [--spike-limit S] [--device N]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

_STEP = """
import json, sys, time
sys.path.insert(0, %r)
from openwurli_amd import pump
dev = int(sys.argv[2])
pump.run_points(pump.static_points(48000.0, [19000.0], 16, 16), dev)          # loads the library, creates the context
t0 = time.perf_counter()
if sys.argv[1] == "sweep":
    rows = pump.run_points(pump.sweep_points(), dev)
    out = {"points": int(rows.size), "fallback_points": int((rows["be_fallbacks"] > 0).sum())}
else:
    rows = pump.run_points(pump.spike_points(), dev)
    t1 = time.perf_counter()
    srow, _ = pump.run_points(pump.slew_point(), dev, trace=True)
    out = {"points": int(rows.size), "spike_points": int((rows["raw_std"] > 0.1).sum()), "grids_s": round(t1 - t0, 4), "slew_max_step": float(srow[0]["max_step"])}
out["gpu_wall_s"] = round(time.perf_counter() - t0, 4)
print(json.dumps(out))
"""


def device_step(which, device, limit):
    """One device step in a child under its own time limit: its JSON, or SystemExit with what went wrong."""
    p = subprocess.Popen([sys.executable, "-c", _STEP % ROOT, which, str(device)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    t0 = time.perf_counter()
    while True:
        try:
            out, err = p.communicate(timeout=30)
            break
        except subprocess.TimeoutExpired:
            spent = time.perf_counter() - t0
            if spent > limit:
                p.kill()
                p.communicate()
                raise SystemExit(f"bench_pump: the {which} step exceeded its limit of {limit} s; stopping")
            print(f"bench_pump: {which} step running, {spent:.0f} s of at most {limit} s", file=sys.stderr, flush=True)
    p = subprocess.CompletedProcess(p.args, p.returncode, out, err)
    if p.returncode != 0:
        raise SystemExit(f"bench_pump: the {which} step ended with status {p.returncode}; stopping\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def cpu_time(points, n):
    """The restatement on the first n points spread evenly over `points`, 16 threads at most; scaled to all of them."""
    import pump_ref as ref
    ref.lib()
    sub = points[:: max(1, points.size // n)][:n] if n and n < points.size else points
    t0 = time.perf_counter()
    ref.run_points(sub, trace=False, threads=16)
    s = time.perf_counter() - t0
    return {"cpu_points_timed": int(sub.size), "cpu_wall_s_16_threads": round(s, 3), "cpu_wall_s_scaled": round(s * points.size / sub.size, 3)}


def main(argv=None):
    from openwurli_amd import pump
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-points", type=int, default=0, help="time only N points of each command on the CPU and scale (0: all)")
    ap.add_argument("--sweep-limit", type=int, default=120)
    ap.add_argument("--spike-limit", type=int, default=600)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    res = {"pump_sweep": device_step("sweep", a.device, a.sweep_limit)}
    res["pump_spike"] = device_step("spike", a.device, a.spike_limit)
    if not a.no_cpu:
        res["pump_sweep"].update(cpu_time(pump.sweep_points(), a.cpu_points))
        res["pump_spike"].update(cpu_time(pump.spike_points(), a.cpu_points))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
