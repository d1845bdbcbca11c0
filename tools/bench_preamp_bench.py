"""Wall time of the preamp measurements (ow_preamp_measure) in a warm process, against the CPU restatement
(tests/c/preamp_bench_ref.cpp, the reference's measure_gain_at over the oracle) on 16 host threads.  Prints ONE JSON line:
  sweep_50_ms / trem_20_ms     the default `sweep` (50 points) and `tremolo-sweep` (20 steps), legacy, on the row kernel
                               (OW_PBENCH_ROW=1) and on the lane-pair kernel (OW_PBENCH_ROW=0), and the melange preamp (lane pair);
                               medians of --reps calls
  grid_1024_ms                 1 024 points (a 32 x 32 surface) on both legacy kernels: where the size rule switches
  surface_16384_s              a 128-frequency x 128-R response surface (16 384 points) in one call, legacy and melange
  cpu_*                        the restatement on --threads threads, one point per task (independent points with r_reset: the same
                               numbers as the sequential run): both default sweeps, and --cpu-cells cells of the surface scaled to 16 384
  csv                          the default sweep / tremolo-sweep CSVs of the device against the restatement: cells that differ, and how
                               many of those lie within 1e-4 dB of a rounding boundary of the printed precision
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


def _median_ms(fn, reps):
    import numpy as np
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, [x * 1e3 for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-big", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-cells", type=int, default=256)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from openwurli_amd import preamp_bench as pb

    res = {"metric": "preamp_bench_wall"}
    sw, tw = pb.sweep_points(), pb.tremolo_sweep_points()
    g32 = pb.surface_points(pb.log_spaced(20.0, 20000.0, 32), pb.log_spaced(19_000.0, 1e6, 32))
    for tag, v in (("row", "1"), ("lanepair", "0")):
        os.environ["OW_PBENCH_ROW"] = v
        res[f"sweep_50_{tag}_ms"], res[f"sweep_50_{tag}_all_ms"] = _median_ms(lambda: pb.run_points(sw), a.reps)
        res[f"trem_20_{tag}_ms"], res[f"trem_20_{tag}_all_ms"] = _median_ms(lambda: pb.run_points(tw), a.reps)
        res[f"grid_1024_{tag}_ms"], _ = _median_ms(lambda: pb.run_points(g32), a.reps_big)
    os.environ.pop("OW_PBENCH_ROW")
    res["sweep_50_melange_ms"], _ = _median_ms(lambda: pb.run_points(sw, pb.PREAMP_MELANGE12), a.reps)
    res["trem_20_melange_ms"], _ = _median_ms(lambda: pb.run_points(tw, pb.PREAMP_MELANGE12), a.reps)
    freqs, rs = pb.log_spaced(20.0, 20000.0, 128), pb.log_spaced(19_000.0, 1e6, 128)
    for kind, tag in ((pb.PREAMP_LEGACY8, "legacy"), (pb.PREAMP_MELANGE12, "melange")):
        ms, allms = _median_ms(lambda: pb.response_surface(freqs, rs, 0.001, kind), a.reps_big)
        res[f"surface_16384_{tag}_s"] = ms / 1e3
        res[f"surface_16384_{tag}_points_per_s"] = 16384 / (ms / 1e3)
    if not a.no_cpu:
        import preamp_bench_ref as ref
        for kind, tag in ((0, "legacy"), (1, "melange")):
            for name, pts in (("sweep_50", sw), ("trem_20", tw)):
                q = [tuple(x) for x in pts.tolist()]
                ref.points(kind, q[:1])
                t0 = time.perf_counter(); met = ref.points(kind, q, threads=a.threads); dt = time.perf_counter() - t0
                res[f"cpu_{name}_{tag}_ms"] = dt * 1e3
                if kind == 0:
                    rows = pb.run_points(pts)
                    cr = rows.copy()
                    cr["gain_db"] = met[:, 1]
                    fmt = pb.format_sweep_csv if name == "sweep_50" else pb.format_tremolo_sweep_csv
                    gl, cl = fmt(rows).splitlines(), fmt(cr).splitlines()
                    diff = sum(x != y for x, y in zip(gl[1:], cl[1:]))
                    near = sum(x != y and _near_boundary(v, 2) for x, y, v in zip(gl[1:], cl[1:], met[:, 1]))
                    res.setdefault("csv", {})[name] = {"rows": len(cl) - 1, "cells_differ": diff, "cells_differ_near_boundary": near,
                                                       "max_abs_gain_db_dev": float(np.abs(rows["gain_db"] - met[:, 1]).max())}
            sp = pb.surface_points(freqs, rs, 0.001)
            idx = np.random.default_rng(7).choice(sp.size, a.cpu_cells, replace=False)
            q = [tuple(x) for x in sp[idx].tolist()]
            t0 = time.perf_counter(); ref.points(kind, q, threads=a.threads); dt = time.perf_counter() - t0
            res[f"cpu_surface_16384_{tag}_s_scaled"] = dt * 16384 / a.cpu_cells
        res["cpu_threads"] = a.threads
        res["cpu_surface_cells_timed"] = a.cpu_cells
    print(json.dumps(res))


if __name__ == "__main__":
    main()
