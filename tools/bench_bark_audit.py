"""Times `bark-audit` on the device: the command's default 5 notes x 4 velocities (20 jobs), and the keyboard x the eight velocity layers
(64 x 8 = 512 jobs) on both preamp kinds, the legacy grid in both forms of its chain kernel (OW_BARK_ROW=1: a row of sixteen lanes per
solver state; =0: the lane pair), against the CPU restatement (tests/c/bark_audit_ref.cpp) on 16 host threads.  One process; every shape
is warmed up once, then timed --repeats times with the forms alternating; a call's time is the host clock around ow_bark_audit, which
ends in a stream synchronise.  A call of the default size is some tens of milliseconds: the spread is printed with the median.  Prints one
JSON line.

  python tools/bench_bark_audit.py [--repeats 5] [--sweep 1024,2048,4096] [--no-cpu] [--cpu-jobs N] [--device N]
      --sweep: both legacy forms at these job counts too (the grid repeated), for the threshold between them (bark::chain_row)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def _stat(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3)}


def main(argv=None):
    from openwurli_amd import bark_audit as ba
    from openwurli_amd.intermod_audit import note_jobs
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sweep", default="", help="job counts at which both legacy forms are timed as well")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-jobs", type=int, default=0, help="time only the first N grid jobs on the CPU and scale (0: all)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    default = note_jobs(list(ba.DEFAULT_NOTES), list(ba.DEFAULT_VELOCITIES))
    grid = note_jobs(list(range(33, 97)), list(ba.ML_VELOCITIES))
    saved = os.environ.pop("OW_BARK_ROW", None)

    def call(jobs, kind, form=None):
        def go():
            if form is None:
                os.environ.pop("OW_BARK_ROW", None)
            else:
                os.environ["OW_BARK_ROW"] = form
            return ba.run_jobs(jobs, kind, device=a.device)
        return go

    shapes = {"default_legacy": call(default, 0), "default_legacy_lane_pair": call(default, 0, "0"), "default_melange": call(default, 1),
              "grid_legacy_row": call(grid, 0, "1"), "grid_legacy_lane_pair": call(grid, 0, "0"), "grid_melange": call(grid, 1)}
    for count in [int(x) for x in a.sweep.split(",") if x.strip()]:
        jobs = np.resize(grid, count)
        shapes[f"sweep_{count}_row"], shapes[f"sweep_{count}_lane_pair"] = call(jobs, 0, "1"), call(jobs, 0, "0")
    rows = {k: fn() for k, fn in shapes.items()}                  # warm-up: library, context, code objects, settled states
    same = rows["grid_legacy_row"].tobytes() == rows["grid_legacy_lane_pair"].tobytes()
    times = {k: [] for k in shapes}
    for _ in range(a.repeats):                                    # alternating: drift of the shared host lands on every shape alike
        for k, fn in shapes.items():
            times[k] += _timed(fn, 1)
    os.environ.pop("OW_BARK_ROW", None)
    if saved is not None:
        os.environ["OW_BARK_ROW"] = saved
    res = {"repeats": a.repeats, "samples_per_job": ba.samples(ba.DURATION), "default_jobs": int(default.size), "grid_jobs": int(grid.size),
           "forms_bit_identical": bool(same)}
    res.update({k: _stat(v) for k, v in times.items()})
    res["row_over_lane_pair_grid"] = round(statistics.median(times["grid_legacy_row"]) / statistics.median(times["grid_legacy_lane_pair"]), 4)
    if not a.no_cpu:
        import bark_audit_ref as ref
        for kind, name in ((0, "legacy"), (1, "melange")):
            ref.run(60, 100, ref.DEFAULT_SIZE, kind)              # builds the library and the oracle's settled states
            sub = grid[:a.cpu_jobs] if a.cpu_jobs else grid
            pairs = [(int(j["note"]), int(j["velocity"])) for j in sub if (int(j["note"]), int(j["velocity"])) != (60, 100)]
            t0 = time.perf_counter()
            ref.run_many(pairs, ref.DEFAULT_SIZE, kind, threads=16)
            cpu_s = time.perf_counter() - t0
            res[f"cpu_{name}"] = {"jobs_timed": len(pairs), "wall_s_16_threads": round(cpu_s, 3), "wall_s_scaled_to_grid": round(cpu_s * grid.size / len(pairs), 3)}
            ref._RUNS.clear()                                     # 512 x 3 rows of 22 050 doubles per kind need not stay
    print(json.dumps(res))


if __name__ == "__main__":
    main()
