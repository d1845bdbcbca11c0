#!/usr/bin/env python3
"""Closed-loop check of candidate note-on MLP weights without rebuilding anything: renders (weight sets x notes x velocities) in ONE batch
call with the ML pipeline's render flags (ml/render_model_notes.py:57-73: --volume 1.0 --no-poweramp --speaker 0.0, but the MLP on) and
extracts the pipeline's harmonic features from the audio while it is still on the GPU.

  python tools/mlp_eval.py --weights a.json,b.json,builtin,identity --notes 65-97 --velocities 40,80,120 --duration 2.0 \
         --corrections-csv c.csv --features-dir out/

  --weights         model_weights.json files (ml/train_mlp.py's export), `builtin` (the set compiled into the library) and `identity`
                    (the --no-mlp baseline: all-identity corrections)
  --features-dir    writes <dir>/<set>/model_harmonics.json in the layout ml/render_model_notes.py writes ("<midi>_<velocity>" keys), so
                    ml/compute_residuals.py --model reads it
  --corrections-csv one row of the eleven corrections per (set, note, velocity)
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_ints(text):
    """"65-97" / "60,76" / "33-40,60" -> [int]."""
    out = []
    for part in text.split(","):
        part = part.strip()
        if not part:
            continue
        if "-" in part:
            lo, hi = part.split("-", 1)
            out.extend(range(int(lo), int(hi) + 1))
        else:
            out.append(int(part))
    return out


def set_name(spec, taken):
    name = spec if spec in ("builtin", "identity") else os.path.splitext(os.path.basename(spec))[0]
    base, k = name, 1
    while name in taken:
        k += 1
        name = f"{base}_{k}"
    return name


def main(argv=None):
    import numpy as np
    from openwurli_amd import mlp
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--notes", default="65-97")
    ap.add_argument("--velocities", default="40,80,120")
    ap.add_argument("--duration", type=float, default=2.0)
    ap.add_argument("--sample-rate", type=float, default=44100.0)
    ap.add_argument("--preamp-kind", type=int, default=0)
    ap.add_argument("--corrections-csv", default=None)
    ap.add_argument("--features-dir", default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    specs = [s.strip() for s in a.weights.split(",") if s.strip()]
    names, sets = [], []
    for spec in specs:
        names.append(set_name(spec, names))
        sets.append(None if spec == "identity" else (mlp.MlpWeights.builtin() if spec == "builtin" else mlp.MlpWeights.from_json(spec)))
    pairs = [(m, v) for m in parse_ints(a.notes) for v in parse_ints(a.velocities)]
    if not sets or not pairs:
        ap.error("no weight set or no (note, velocity) pair")
    if a.corrections_csv:
        real = [s for s in sets if s is not None]
        notes = np.array([m for m, _ in pairs], dtype=np.uint8)
        vels = np.array([v / 127.0 for _, v in pairs])
        inferred = iter(mlp.infer(real, notes, vels, device=a.device)) if real else iter(())
        os.makedirs(os.path.dirname(os.path.abspath(a.corrections_csv)), exist_ok=True)
        with open(a.corrections_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(("set", "midi_note", "velocity_midi") + mlp.CORRECTION_NAMES)
            for name, s in zip(names, sets):
                rows = np.tile(mlp.IDENTITY, (len(pairs), 1)) if s is None else next(inferred)
                for (m, v), row in zip(pairs, rows):
                    w.writerow([name, m, v] + [repr(float(x)) for x in row])
    feats = mlp.render_and_extract(pairs, sets, sample_rate=a.sample_rate, duration_s=a.duration, device=a.device, preamp_kind=a.preamp_kind)
    written = []
    if a.features_dir:
        for name, feat in zip(names, feats):
            d = os.path.join(a.features_dir, name)
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, "model_harmonics.json")
            with open(path, "w") as f:
                json.dump({f"{m}_{v}": feat[(m, v)] for m, v in pairs}, f, indent=2)
            written.append(path)
    print(json.dumps({"sets": names, "pairs": len(pairs), "jobs": len(pairs) * len(sets), "duration_s": a.duration, "features": written,
                      "corrections_csv": a.corrections_csv}))


if __name__ == "__main__":
    main()
