"""Wall time of ONE ow_centroid_track call over the 512-point default grid (notes 33..96 x the ML pipeline's eight velocity layers, 1 s
each), rows and frames only, in a warm process, against the CPU restatement (tests/c/centroid_track_ref.cpp over the oracle) on
--threads host threads.  Run once per configuration: the command's defaults, and --window-ms 50 --hop-ms 10.  Prints ONE JSON line:
  device_s / device_all_s / device_spread   median, every one of --reps calls (after one warm-up call), (max - min) / median
  render_s                                  the same grid with a window that leaves ONE frame per job: what the renders alone cost
  cpu_s_scaled                              the restatement on --cpu-jobs jobs spread over the grid, scaled to 512 (cpu_s_timed: as measured)
  c_max_abs_dev_hz                          the largest |c(device) - c(restatement)| over the frames of the jobs the CPU ran
It measures; it does not gate.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-jobs", type=int, default=64)
    ap.add_argument("--duration", type=float, default=1.0)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--hop-ms", type=float, default=2.5)
    ap.add_argument("--end-ms", type=float, default=500.0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from openwurli_amd import centroid_track as ct

    jobs = ct.grid_jobs()
    kw = dict(duration=a.duration, window_ms=a.window_ms, hop_ms=a.hop_ms, end_ms=a.end_ms)
    res = {"metric": "centroid_track_wall", "jobs": int(jobs.size), **kw}
    ct.run_jobs(jobs[:64], **kw)                           # warm-up: library, context, kernels
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); rows, frames = ct.run_jobs(jobs, **kw); t.append(time.perf_counter() - t0)
    res["frames"] = int(frames.shape[1])
    res["device_s"], res["device_all_s"] = float(np.median(t)), t
    res["device_spread"] = (max(t) - min(t)) / res["device_s"]
    t = []
    for _ in range(max(2, a.reps // 2)):
        t0 = time.perf_counter(); ct.run_jobs(jobs, a.duration, a.window_ms, a.hop_ms, 0.5 * a.window_ms); t.append(time.perf_counter() - t0)
    res["render_s"] = float(np.median(t))
    res["status_counts"] = {k: [int((rows[k] == s).sum()) for s in (0, 1, 2)] for k in ("attack_status", "sustain_status", "drift_status")}
    if not a.no_cpu:
        import centroid_track_ref as ref
        idx = np.linspace(0, jobs.size - 1, min(a.cpu_jobs, jobs.size)).astype(int)
        js = [ref.Job(int(j["note"]), int(j["velocity"])) for j in jobs[idx]]
        ref.track(js[0], duration=0.05, end_ms=40.0)       # compile / load
        t0 = time.perf_counter(); rr = ref.track_many(js, threads=a.threads, **kw); dt = time.perf_counter() - t0
        res["cpu_s_timed"], res["cpu_jobs_timed"], res["cpu_threads"] = dt, len(js), a.threads
        res["cpu_s_scaled"] = dt * jobs.size / len(js)
        res["c_max_abs_dev_hz"] = float(max(np.abs(r.frames - frames[i]).max() for r, i in zip(rr, idx)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
