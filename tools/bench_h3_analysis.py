"""Times the pickup-law study on the device and sets the reference's arithmetic on the CPU beside it.  Prints one JSON line.

Workload: 512 carriers (the 64 notes 33..96 x 8 velocity layers) x 256 law points (128 alphas over 1.0..2.5, 64 k over 0..5, 64 blends
over 0..1) at the script's 22 050 samples and 8 harmonics, in ONE `ow_pickup_law` call: 131 072 jobs, 2.9e9 lane-samples.

Device: a warm-up call at a small size (loads the library, creates the context), then --repeats whole calls, each timed with the host
clock around the call (it ends in a stream synchronise after the copy back).  `ns_per_lane_sample` is the best call's time over
jobs x samples: uploads, the 8 MB copy back and the carrier side of every tile included, so it bounds the kernel's from above.

CPU: the numpy restatement (tests/pickup_law_ref.py, reference form: the script's operations, its high-pass loop vectorised over a
carrier's 256 laws, which runs faster than the script's per-law Python loop) timed on --cpu-carriers carriers x the 256 laws, one
process, one thread.  SCALED BY COUNT, not timed: that time per carrier times 512.

  python tools/bench_h3_analysis.py [--repeats 3] [--cpu-carriers 2] [--no-cpu] [--device N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_SAMPLES, N_HARMONICS = 22050, 8
VELOCITIES = (16, 32, 48, 64, 80, 96, 112, 127)


def workload():
    import numpy as np
    from openwurli_amd import pickup_law as pl
    rows, _ = pl.carriers(range(33, 97), VELOCITIES, variants=("midi",))
    kinds, params = pl.grid_laws(np.linspace(1.0, 2.5, 128), np.linspace(0.0, 5.0, 64), np.linspace(0.0, 1.0, 64))
    return rows, kinds, params


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-carriers", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    import numpy as np
    from openwurli_amd import pickup_law as pl
    rows, kinds, params = workload()
    jobs = rows.shape[0] * kinds.size
    out = {"carriers": int(rows.shape[0]), "laws": int(kinds.size), "samples": N_SAMPLES, "harmonics": N_HARMONICS, "jobs": jobs}

    pl.pickup_law(rows[:2], kinds[:3], params[:3], n_samples=256, n_harmonics=N_HARMONICS, device=a.device)      # warm-up
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        amps, peak = pl.pickup_law(rows, kinds, params, n_samples=N_SAMPLES, n_harmonics=N_HARMONICS, device=a.device)
        walls.append(time.perf_counter() - t0)
        print(f"bench_h3_analysis: call {walls[-1]:.4f} s", file=sys.stderr, flush=True)
    assert np.all(np.isfinite(amps)) and np.all(amps[..., 0] > 0) and np.all(peak > 0)
    out["call_s"] = [round(w, 4) for w in walls]
    out["ns_per_lane_sample"] = round(min(walls) / (jobs * N_SAMPLES) * 1e9, 4)

    if not a.no_cpu:
        import pickup_law_ref as ref
        pick = np.linspace(0, rows.shape[0] - 1, a.cpu_carriers).astype(int)
        t0 = time.perf_counter()
        want, _ = ref.jobs(rows[pick], kinds, params)
        cpu = (time.perf_counter() - t0) / a.cpu_carriers
        out["cpu_s_per_carrier_timed"] = round(cpu, 3)
        out["cpu_s_scaled_by_count"] = round(cpu * rows.shape[0], 1)
        out["speedup_scaled"] = round(cpu * rows.shape[0] / min(walls), 1)
        out["worst_amp_difference_v"] = float(np.max(np.abs(amps[pick] - want)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
