#!/usr/bin/env python3
"""Times the Goertzel harmonics of N synthetic gold notes (1.7 s each: 3 windows x 8 harmonics and 6 decay points, as
ml/extract_harmonics.py walks a gold note) in ONE ow_goertzel_harmonics call, host audio in, amplitudes out; and the numpy restatement
of tests/harmonics_ref.py on the CPU for --cpu-notes of the notes (default 2), scaled by count to N -- the CPU figure is an
extrapolation, and the output says so.  The restatement advances all recurrences of a note together, one numpy operation per operation of
the loop; the reference's own loop is interpreted Python, one recurrence after the other, and is not run here.  Prints one JSON line:
notes, segments, recurrences, recurrence steps (recurrences x samples), wall time per call, steps per second, the CPU figures and how many
of the CPU notes' amplitudes the GPU reproduced bit for bit.

  python tools/bench_harmonics.py [--notes 256] [--repeats 3] [--cpu-notes 2] [--no-cpu] [--device 0]
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


def synthetic_notes(n, sr, seconds=1.7):
    """n decaying harmonic series with noise, MIDI 33..96 in turn: (rows [n, samples], f0 [n])."""
    import numpy as np
    from openwurli_amd.features import midi_to_freq
    rng = np.random.default_rng(7)
    m = int(seconds * sr)
    t = np.arange(m) / sr
    rows, f0s = np.empty((n, m)), []
    for j in range(n):
        f0 = midi_to_freq(33 + j % 64)
        x = np.zeros(m)
        for h in range(1, 9):
            if f0 * h < sr / 2:
                x += 0.5 / h ** 1.5 * np.exp(-t * (1.5 + 0.7 * h)) * np.sin(2 * np.pi * f0 * h * t * (1.0 + rng.uniform(-2e-3, 2e-3)) + rng.uniform(0, 6.28))
        rows[j] = 0.3 * x + 1e-4 * rng.standard_normal(m)
        f0s.append(f0)
    return rows, f0s


def main(argv=None):
    import numpy as np
    import harmonics_ref as ref
    from openwurli_amd import features, harmonics
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--notes", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-notes", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    sr = 44100.0
    rows, f0s = synthetic_notes(a.notes, sr)
    segs, first = [], []
    for j, f0 in enumerate(f0s):
        _, plan = harmonics.plan_note(rows.shape[1], sr, {"onset_s": 0.0, "offset_s": rows.shape[1] / sr})
        first.append(len(segs))
        segs += [(j, s[0], s[1], s[2], f0) for s in plan[:9] if s is not None]
    first.append(len(segs))
    features.goertzel_segments(rows[:1], sr, segs[:first[1]], device=a.device)                  # warm-up: library, context, code object
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        amps, coeffs, bins = features.goertzel_segments(rows, sr, segs, device=a.device, plan=True)
        wall.append(time.perf_counter() - t0)
    n_rec = [sum(len({int(k) for k in bins[i, h] if k >= 0}) for h in range(8)) for i in range(len(segs))]
    steps = sum(r * (s[2] - s[1]) for r, s in zip(n_rec, segs))
    med = statistics.median(wall)
    res = {"notes": a.notes, "segments": len(segs), "recurrences": sum(n_rec), "recurrence_steps": steps, "repeats": a.repeats,
           "wall_ms": round(1e3 * med, 3), "wall_min_ms": round(1e3 * min(wall), 3), "wall_max_ms": round(1e3 * max(wall), 3),
           "ms_per_note": round(1e3 * med / a.notes, 4), "recurrence_steps_per_s": round(steps / med, 1),
           "audio_bytes_copied_per_call": int(rows.nbytes)}
    if not a.no_cpu:
        pick = list(range(min(a.cpu_notes, a.notes)))
        same = total = 0
        t0 = time.perf_counter()
        for j in pick:
            mine = range(first[j], first[j + 1])
            got = ref.goertzel_amps_many([rows[j, segs[i][1]:segs[i][2]] for i in mine],
                                         [(coeffs[i, :segs[i][3]], bins[i, :segs[i][3]], ref.past_cut(sr, segs[i][4], segs[i][3])) for i in mine])
            for i, g in zip(mine, got):
                total += len(g)
                same += int(np.sum(g == amps[i, :len(g)]))
        cpu_s = time.perf_counter() - t0
        scaled = cpu_s * a.notes / len(pick)
        res["numpy_restatement_cpu"] = {"notes_timed": len(pick), "wall_s": round(cpu_s, 3), "s_per_note": round(cpu_s / len(pick), 4),
                                        "wall_s_scaled_by_count_to_all_notes": round(scaled, 2),
                                        "note": "timed on notes_timed of the notes, scaled by count: an extrapolation; vectorised numpy, not the reference's interpreted loop",
                                        "amplitudes_bit_identical_to_the_gpu": f"{same}/{total}"}
        res["speedup_over_numpy_restatement_scaled"] = round(scaled / med, 1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
