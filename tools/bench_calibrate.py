"""Wall time of the calibration sweep (ow_calibrate) in a warm process, against the CPU restatement (tests/c/calibrate_ref.cpp, the
reference's run_calibrate over the oracle) on 16 host threads.  Prints ONE JSON line:
  gpu_192_ms      the default `sensitivity` grid (8 DS x 8 notes x 3 velocities, track), median of --reps calls
  gpu_65536_s     64 notes x 128 velocities x 8 DS values (track) in one call, median of --reps-big calls
  cpu_192_s       the same 192 points on the restatement, 16 threads (one point per task)
  csv             the 192-row CSV of both: cells that differ in the printed precision, and how many of those lie within 1e-4 (dB) of a
                  rounding boundary of the printed precision (the only place the two may differ)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _near_boundary(x, decimals, eps=1e-4):
    s = abs(x) * 10 ** decimals
    return abs((s - int(s)) - 0.5) <= eps * 10 ** decimals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-big", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from openwurli_amd import calibrate as cal

    cal.sensitivity()                                            # warm: library, device context, code objects
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); rows = cal.sensitivity(); t.append(time.perf_counter() - t0)
    gpu_192 = float(np.median(t))
    notes, vels = list(range(33, 97)), list(range(128))
    tb = []
    for _ in range(a.reps_big):
        t0 = time.perf_counter(); big = cal.sensitivity(notes, vels); tb.append(time.perf_counter() - t0)
    assert len(big) == 65536
    res = {"metric": "calibrate_sweep_wall", "gpu_192_ms": gpu_192 * 1e3, "gpu_192_all_ms": [x * 1e3 for x in t],
           "gpu_65536_s": float(np.median(tb)), "gpu_65536_all_s": tb, "gpu_65536_points_per_s": 65536 / float(np.median(tb))}
    if not a.no_cpu:
        import calibrate_ref
        pts = [(n, v, cal.sensitivity_config(ds)) for ds in cal.SENSITIVITY_DS for n in cal.SENSITIVITY_NOTES for v in cal.SENSITIVITY_VELOCITIES]
        calibrate_ref.run_points(pts[:1], 0.40, 1.0)             # build + warm
        t0 = time.perf_counter()
        ref, _ = calibrate_ref.run_points(pts, 0.40, 1.0, threads=a.threads)
        res["cpu_192_s"] = time.perf_counter() - t0
        res["cpu_threads"] = a.threads
        res["gpu_speedup_192"] = res["cpu_192_s"] / gpu_192
        ref[:, 0] = [p[2].ds_at_c4 for p in pts]
        ref_rows = [cal.CalibrateRow(n, v, *r) for (n, v, _), r in zip(pts, ref.tolist())]
        g = [ln.split(",") for ln in cal.format_calibrate_csv(rows).splitlines()]
        c = [ln.split(",") for ln in cal.format_calibrate_csv(ref_rows).splitlines()]
        diff, near = 0, 0
        for i in range(1, len(c)):
            vals = [getattr(ref_rows[i - 1], f) for f in cal.CALIBRATE_ROW_FIELDS]
            for k in range(3, len(c[i])):
                if g[i][k] != c[i][k]:
                    diff += 1
                    near += _near_boundary(vals[k - 3], 4 if k < 6 else 2)
        res["csv"] = {"rows": len(c) - 1, "cells_differ": diff, "cells_differ_near_boundary": near}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
