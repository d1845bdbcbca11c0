"""Times the render analysis of `intermod-audit` for the keyboard x the ML pipeline's eight velocity layers (64 x 8 = 512 jobs, 3 s each)
in ONE device call against the CPU restatement (tests/c/note_audit_ref.cpp) on 16 host threads.  Prints one JSON line.

  python tools/bench_intermod_audit.py [--duration 3.0] [--no-cpu] [--cpu-jobs N] [--device N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    from openwurli_amd import intermod_audit as ia
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--duration", type=float, default=3.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-jobs", type=int, default=0, help="time only the first N jobs on the CPU and scale (0: all)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    jobs = ia.note_jobs(list(range(ia.MIDI_LO, ia.MIDI_HI + 1)), [20, 35, 50, 65, 80, 95, 110, 127])
    ia.run_jobs(jobs[:1], 0.6, a.device)                     # loads the library, creates the context
    t0 = time.perf_counter()
    rows = ia.run_jobs(jobs, a.duration, a.device)
    gpu_s = time.perf_counter() - t0
    res = {"jobs": int(jobs.size), "duration_s": a.duration, "gpu_wall_s": round(gpu_s, 4), "verdicts": {v: int((rows["verdict"] == i).sum()) for i, v in enumerate(ia.VERDICTS)}}
    if not a.no_cpu:
        import note_audit_ref as ref
        ref.lib()
        sub = jobs[:a.cpu_jobs] if a.cpu_jobs else jobs
        t0 = time.perf_counter()
        ref.many(lambda j: ref.intermod_audit(ref.render(int(j["note"]), int(j["velocity"]), a.duration), int(j["note"])), sub, threads=16)
        cpu_s = time.perf_counter() - t0
        res.update({"cpu_jobs_timed": int(sub.size), "cpu_wall_s_16_threads": round(cpu_s, 4), "cpu_wall_s_scaled": round(cpu_s * jobs.size / sub.size, 4)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
