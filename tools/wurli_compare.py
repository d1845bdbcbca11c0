#!/usr/bin/env python3
"""The reference's tools/wurli_compare.py on the GPU: A/B comparison of extracted real Wurlitzer notes with renders of the same notes.

  python tools/wurli_compare.py DIR [DIR ...] -o OUT --top-per-pitch 3          # best notes per pitch against renders
  python tools/wurli_compare.py DIR -o OUT --notes B4,G5,C3 [--velocity 90] [--tier3]
  python tools/wurli_compare.py DIR --summary-only
  python tools/wurli_compare.py rank DIR [DIR ...] --weights a.json,builtin,identity -o ranks.csv

The reference's arguments, progress lines (minus the cargo build), report text, comparison_report.json and <note>_real.wav /
<note>_synth.wav.  All selected notes are rendered in one batch call per distinct duration (MLP on, 44 100 Hz; tier 2 = --no-poweramp
--speaker 0.0 --volume 1.0, --tier3 = --volume 0.40 --speaker 1.0) and analysed where the render left them, as the 24-bit file the
command writes.  The recorded clip is analysed as the 16-bit file the reference makes of it (--real-as-is: as read).

`rank` renders the same selected notes under every (weight set, tier) configuration in one batch and writes one CSV row per
configuration: mean / median / worst harmonic distance, mean decay and centroid differences -- the number a training sweep is ranked by.
"""
import argparse
import csv
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _common(ap):
    ap.add_argument("extraction_dirs", nargs="+", help="Directories with extraction_metadata.json from recording_analyzer")
    ap.add_argument("--top-per-pitch", type=int, default=1, help="Number of best notes to compare per pitch (default: 1)")
    ap.add_argument("--notes", type=str, default=None, help="Comma-separated note names to compare (e.g. B4,G5,C3)")
    ap.add_argument("--velocity", type=int, default=None, help="Override synth velocity (default: estimate from extraction)")
    ap.add_argument("--real-as-is", action="store_true", help="Analyse the recorded clip as read, not as the 16-bit file the reference makes of it")
    ap.add_argument("--device", type=int, default=0)


def _select(a, wc):
    print("Loading extractions...")
    all_notes = wc.load_extractions(a.extraction_dirs)
    print(f"  {len(all_notes)} total notes from {len(a.extraction_dirs)} source(s)")
    return all_notes


def main_compare(argv):
    from openwurli_amd import wurli_compare as wc
    from openwurli_amd.features import write_wav_24bit
    ap = argparse.ArgumentParser(description="A/B comparison: real Wurlitzer vs OpenWurli synthesis")
    _common(ap)
    ap.add_argument("-o", "--output", default=os.path.join(tempfile.gettempdir(), "wurli_comparison"),
                    help="Output directory for comparison results (default: $TMPDIR/wurli_comparison)")
    ap.add_argument("--summary-only", action="store_true", help="Just print extraction summary, no rendering")
    ap.add_argument("--tier3", action="store_true", help="Render with full chain (power amp + speaker + volume) instead of Tier 2")
    a = ap.parse_args(argv)
    all_notes = _select(a, wc)
    if a.summary_only:
        wc.print_summary(all_notes)
        return
    selected = wc.select_best_notes(all_notes, a.top_per_pitch, a.notes.split(",") if a.notes else None)
    print(f"  Selected {sum(len(v) for v in selected.values())} notes across {len(selected)} pitches")
    os.makedirs(a.output, exist_ok=True)
    plan = wc.plan_run(selected, a.top_per_pitch, a.output, a.velocity, a.tier3)
    have = [p for p in plan if not p["missing"]]
    for p in have:                                    # the copy of the recorded clip, as the script writes it
        wc.write_wav16(p["real_wav"], wc.read_wav(p["info"]["_wav_path"]), wc.SR)
        p["real"] = wc.load_real(p["info"]["_wav_path"], a.real_as_is)
    ok = [p for p in have if p["job"] is not None]
    audio = []
    comps = wc.compare_rendered([p["real"] for p in ok], [p["info"]["f0_hz"] for p in ok], [p["job"] for p in ok], [p["duration"] for p in ok],
                                device=a.device, audio_out=audio) if ok else []
    for k, (p, comp) in enumerate(zip(ok, comps)):
        p["comparison"] = comp
        write_wav_24bit(p["synth_wav"], audio[0][k, :int(audio[1][k])], wc.SR, 1.0)          # as `preamp-bench render` writes it
    comparisons = []
    for p in plan:                                    # the script's progress lines, in its order
        if p["missing"]:
            print(p["head"] + " SKIP (wav missing)")
        elif p["job"] is None:
            print(p["head"] + " RENDER FAILED")
        else:
            comparisons.append(wc.result_entry(p, p["comparison"]))
            print(p["head"] + " " + wc.progress_tail(p["comparison"]["harmonic_distance_db"]))
    with open(os.path.join(a.output, "comparison_report.json"), "w") as f:
        json.dump({"n_comparisons": len(comparisons), "sources": a.extraction_dirs, "comparisons": comparisons}, f, indent=2, default=str)
    wc.print_comparison_report(comparisons, a.output)


def main_rank(argv):
    from openwurli_amd import mlp, wurli_compare as wc
    ap = argparse.ArgumentParser(prog="wurli_compare.py rank", description="Rank weight sets x tiers by their distance to the recorded notes")
    _common(ap)
    ap.add_argument("--weights", required=True, help="model_weights.json files, `builtin`, `identity` (comma-separated)")
    ap.add_argument("--tiers", default="2,3")
    ap.add_argument("-o", "--output", default="wurli_rank.csv", help="CSV, one row per (weight set, tier)")
    a = ap.parse_args(argv)
    specs = [s.strip() for s in a.weights.split(",") if s.strip()]
    names, sets = [], []
    for spec in specs:
        base = spec if spec in ("builtin", "identity") else os.path.splitext(os.path.basename(spec))[0]
        name, k = base, 1
        while name in names:
            k += 1
            name = f"{base}_{k}"
        names.append(name)
        sets.append(None if spec == "identity" else ("builtin" if spec == "builtin" else mlp.MlpWeights.from_json(spec)))
    tiers = [int(t) for t in a.tiers.split(",") if t.strip()]
    if not sets or not tiers or any(t not in (2, 3) for t in tiers):
        ap.error("--weights needs at least one set, --tiers takes 2 and / or 3")
    all_notes = _select(a, wc)
    selected = wc.select_best_notes(all_notes, a.top_per_pitch, a.notes.split(",") if a.notes else None)
    plan = [p for p in wc.plan_run(selected, a.top_per_pitch, ".", a.velocity, False) if p["job"] is not None]
    print(f"  Selected {len(plan)} notes; {len(sets) * len(tiers)} configurations, {len(plan) * len(sets) * len(tiers)} renders")
    reals = [wc.load_real(p["info"]["_wav_path"], a.real_as_is) for p in plan]
    rows = wc.rank(reals, [p["info"]["f0_hz"] for p in plan], [p["midi"] for p in plan], [p["velocity_midi"] for p in plan],
                   [p["duration"] for p in plan], sets, names, tiers, device=a.device)
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        for r in rows:
            w.writerow({k: ("" if v is None else v) for k, v in r.items()})
    print(json.dumps({"configurations": len(rows), "notes": len(plan), "csv": a.output}))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == "rank":
        return main_rank(argv[1:])
    return main_compare(argv)


if __name__ == "__main__":
    main()
