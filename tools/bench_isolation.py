#!/usr/bin/env python3
"""Times the isolation sub-scores of F synthetic recordings of N notes each (default 8 x 4 096) in ONE ow_isolation_score call: the wall
time of the call (planned records in, scores out) and the kernel's own device time; and the Python restatement of tests/isolation_ref.py
on the CPU for one file of --cpu-notes notes (default 512), scaled by pair count (notes squared per file) to the whole set -- the CPU
figure is an extrapolation, and the output says so.  The restatement makes one pass over a target's others where the reference makes
three; the reference itself is not run here.  Prints one JSON line: files, notes, pairs, wall and kernel time per call, pairs per second,
the CPU figures and how the GPU's scores of the CPU file compare with the restatement's.

  python tools/bench_isolation.py [--files 8] [--notes 4096] [--repeats 3] [--cpu-notes 512] [--no-cpu] [--device 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic_file(rng, name, n, notes_per_second=4.0):
    """n notes as a transcriber gives them: onsets spread at notes_per_second, 0.1 to 3 s long, times and amplitudes at four places."""
    import numpy as np
    notes = []
    for k in range(n):
        onset = rng.uniform(0.0, n / notes_per_second)
        dur = float(np.exp(rng.uniform(np.log(0.1), np.log(3.0))))
        notes.append({"id": f"{name}_{k:05d}", "onset_s": round(onset, 4), "offset_s": round(onset + dur, 4), "midi_note": int(rng.integers(36, 97)),
                      "amplitude": round(float(rng.uniform(0.05, 1.0)), 4), "source_file": name, "source_type": "basic_pitch"})
    notes.sort(key=lambda x: x["onset_s"])
    return notes


def main(argv=None):
    import numpy as np
    import isolation_ref as ref
    from openwurli_amd import isolation
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--notes", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-notes", type=int, default=512)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(11)
    files = [synthetic_file(rng, f"take_{f:02d}.wav", a.notes) for f in range(a.files)]
    notes = [n for f in files for n in f]
    rec, file_first, _ = isolation.plan_notes(notes)
    isolation.isolation_scores(rec[:2], [0, 2], a.device)                    # warm-up: library, context, code object
    wall, kern = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        got = isolation.isolation_scores(rec, file_first, a.device, kernel_ms=True)
        wall.append(time.perf_counter() - t0)
        kern.append(got[4])
    pairs = a.files * a.notes * a.notes
    med = statistics.median(wall)
    res = {"files": a.files, "notes_per_file": a.notes, "scored_notes": int(np.sum(rec["score"] != 0)), "pairs": pairs, "repeats": a.repeats,
           "wall_ms": round(1e3 * med, 3), "wall_min_ms": round(1e3 * min(wall), 3), "wall_max_ms": round(1e3 * max(wall), 3),
           "kernel_ms": round(statistics.median(kern), 3), "pairs_per_s_wall": round(pairs / med, 1)}
    if not a.no_cpu:
        one = synthetic_file(np.random.default_rng(12), "cpu_take.wav", a.cpu_notes)
        r1, ff1, _ = isolation.plan_notes(one)
        g = isolation.isolation_scores(r1, ff1, a.device)
        t0 = time.perf_counter()
        raw = ref.score_notes(json.loads(json.dumps(one)))
        cpu_s = time.perf_counter() - t0
        scaled = cpu_s * pairs / (a.cpu_notes * a.cpu_notes)
        live = [k for k, r in enumerate(raw) if r is not None]
        res["python_restatement_cpu"] = {"notes_timed": a.cpu_notes, "wall_s": round(cpu_s, 3), "us_per_pair": round(1e6 * cpu_s / (a.cpu_notes * a.cpu_notes), 3),
                                         "wall_s_scaled_by_pair_count_to_all_files": round(scaled, 2),
                                         "note": "timed on one file of notes_timed notes, scaled by pair count: an extrapolation; one pass per target, not the reference's three",
                                         "collision_identical_to_the_gpu": f"{sum(1 for k in live if g[1][k] == raw[k][1])}/{len(live)}",
                                         "largest_difference_temporal": float(max(abs(g[0][k] - raw[k][0]) for k in live)),
                                         "largest_difference_dominance": float(max(abs(g[2][k] - raw[k][2]) for k in live))}
        res["speedup_over_python_restatement_scaled"] = round(scaled / med, 1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
