"""Wall time of ONE ow_render_poly call over the 2 016 dyads of notes 33..96 at 3 s (6 048 chains of 132 300 samples), rows only, in a
warm process, against the CPU restatement (tests/c/render_poly_ref.cpp over the oracle) on --threads host threads.  Prints ONE JSON line:
  device_s / device_all_s      median and every one of --reps calls (after one warm-up call)
  device_dyads_per_s
  cpu_s_scaled                 the restatement on --cpu-chords dyads spread over the grid, scaled to 2 016 (cpu_s_timed: as measured)
  ratio_db_max_abs_dev         the largest |intermod_ratio_db(device) - intermod_ratio_db(restatement)| over the dyads the CPU ran
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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-chords", type=int, default=128)
    ap.add_argument("--duration", type=float, default=3.0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from openwurli_amd import render_poly as rp

    chords = rp.dyad_grid(33, 96, (80, 80))
    res = {"metric": "render_poly_wall", "dyads": int(chords.size), "duration_s": a.duration}
    rp.run_chords(chords[:64], a.duration)                 # warm-up: library, context, kernels
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); rows = rp.run_chords(chords, a.duration); t.append(time.perf_counter() - t0)
    res["device_s"], res["device_all_s"] = float(np.median(t)), t
    res["device_dyads_per_s"] = chords.size / res["device_s"]
    res["ratio_db_min_max"] = [float(rows["intermod_ratio_db"].min()), float(rows["intermod_ratio_db"].max())]
    if not a.no_cpu:
        import render_poly_ref as ref
        idx = np.linspace(0, chords.size - 1, min(a.cpu_chords, chords.size)).astype(int)
        cs = [ref.Chord(tuple(c["notes"][:2]), tuple(c["velocities"][:2]), a.duration, float(c["volume"]), float(c["speaker"]), float(c["r_ldr"]), False)
              for c in chords[idx]]
        ref.render_chord(cs[0], audio=False)               # compile / load
        t0 = time.perf_counter(); rr = ref.render_many(cs, threads=a.threads, audio=False); dt = time.perf_counter() - t0
        res["cpu_s_timed"], res["cpu_chords_timed"], res["cpu_threads"] = dt, len(cs), a.threads
        res["cpu_s_scaled"] = dt * chords.size / len(cs)
        res["ratio_db_max_abs_dev"] = float(max(abs(r.row["intermod_ratio_db"] - rows["intermod_ratio_db"][i]) for r, i in zip(rr, idx)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
