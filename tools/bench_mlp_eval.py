#!/usr/bin/env python3
"""Times a training sweep's closed-loop render: --sets perturbed weight sets (default 64) x the 512-job grid of tools/bench_batch.py
(64 notes x 8 velocity layers) at 2 s and 44.1 kHz, MLP on, in ONE ow_batch_render_mlp call into a device buffer; next to it the same
grid with one set, ow_mlp_infer alone (sets x 512 points: the host clock around the call, i.e. the kernel plus its uploads and the
download of the table -- an upper bound of what k_mlp_infer adds to the render), and the CPU restatement (tests/c/mlp_eval_ref.cpp) for
one set x 16 jobs on 16 host threads, scaled to the sweep.  Every shape is warmed up once, then timed --repeats times.  Prints one JSON line.

  python tools/bench_mlp_eval.py [--sets 64] [--duration 2.0] [--repeats 3] [--no-cpu] [--device N]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

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
    from openwurli_amd import binding, mlp
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--duration", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    lib = binding.load_library()
    sr = 44100.0
    pairs = [(m, v) for m in range(33, 97) for v in (20, 35, 50, 65, 80, 95, 110, 127)]
    base = mlp.MlpWeights.builtin()
    sets = [base.perturbed(0.02, 100 + k) for k in range(a.sets)]
    n = int(a.duration * sr)
    jobs_all = [dict(note=m, velocity=v) for _ in sets for m, v in pairs]
    soj_all = np.repeat(np.arange(a.sets, dtype=np.uint32), len(pairs))
    jobs_one = jobs_all[:len(pairs)]
    buf = lib.ow_device_alloc(8 * len(jobs_all) * n, a.device)
    if not buf:
        raise SystemExit(binding.take_error(lib))
    notes = np.array([m for m, _ in pairs], dtype=np.uint8)
    vels = np.array([v / 127.0 for _, v in pairs])
    shapes = {
        "sweep": lambda: mlp.batch_render_mlp(jobs_all, sets, soj_all, sample_rate=sr, duration_s=a.duration, device=a.device, out_device_ptr=buf, stride=n),
        "one_set": lambda: mlp.batch_render_mlp(jobs_one, sets[:1], soj_all[:len(pairs)], sample_rate=sr, duration_s=a.duration, device=a.device, out_device_ptr=buf, stride=n),
        "infer_alone": lambda: mlp.infer(sets, notes, vels, device=a.device),
    }
    try:
        for fn in shapes.values():
            fn()                                                  # warm-up: library, context, code objects
        times = {k: [] for k in shapes}
        for _ in range(a.repeats):
            for k, fn in shapes.items():
                times[k] += _timed(fn, 1)
    finally:
        lib.ow_device_free(buf, a.device)
    res = {"sets": a.sets, "jobs_per_set": len(pairs), "jobs": len(jobs_all), "samples_per_job": n, "repeats": a.repeats}
    res.update({k: _stat(v) for k, v in times.items()})
    sweep = statistics.median(times["sweep"])
    res["sweep_over_one_set"] = round(sweep / statistics.median(times["one_set"]), 3)
    res["infer_alone_share_of_sweep"] = round(statistics.median(times["infer_alone"]) / sweep, 5)
    res["sweep_samples_per_s"] = round(len(jobs_all) * n / sweep, 1)
    if not a.no_cpu:
        import mlp_eval_ref as ref
        sub = pairs[::32][:16]
        corr = [ref.infer(sets[0].flat(), m, v / 127.0) for m, v in sub]
        ref.render(60, 100, 0.01, ref.IDENTITY)                   # builds the library
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as ex:
            list(ex.map(lambda k: ref.render(sub[k][0], sub[k][1], a.duration, corr[k]), range(len(sub))))
        cpu_s = time.perf_counter() - t0
        res["cpu"] = {"jobs_timed": len(sub), "wall_s_16_threads": round(cpu_s, 3), "wall_s_scaled_to_sweep": round(cpu_s * len(jobs_all) / len(sub), 1)}
        res["speedup_over_cpu_16_threads"] = round(cpu_s * len(jobs_all) / len(sub) / sweep, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
