"""The reference's ml/h3_analysis_v2.py on the device: should the pickup's y / (1 - y) law change?  Every law point of every note of a run
is one lane of ONE library call (openwurli_amd/pickup_law.py, `ow_pickup_law`); step 1's inter-harmonic SNR goes through
`ow_dft_magnitudes`.

  python tools/h3_analysis.py --harmonics harmonics.json [--model model_harmonics.json]
        the reference's script: its sections 1 to 6 character for character (SNR table, anomalous patterns, y_peak / HPF table, reliable
        and unreliable notes, alpha sweep with "Best alpha", k list, blend list).  Its closing SUMMARY is prose about one data set
        and is not reproduced.
  python tools/h3_analysis.py grid --harmonics harmonics.json --csv g.csv [--per-note n.csv] [--alphas lo:hi:step] [--ks lo:hi:step]
        [--blends lo:hi:step] [--velocities 40,80,120]
        every law point x the notes of harmonics.json x the velocity layers in one call.  g.csv: one row per law point (family,
        parameter, n, H2 mean / std, H3 mean / std, H3 RMS, total RMS, dB).  n.csv: per (note, velocity) the law point with the smallest
        sqrt(h2e^2 + h3e^2).  An axis is lo:hi:step (hi included) or a comma list.
  both: [--device N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from openwurli_amd import pickup_law as pl
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", nargs="?", choices=["grid"])
    ap.add_argument("--harmonics", required=True)
    ap.add_argument("--model", default=None)
    ap.add_argument("--alphas", default="")
    ap.add_argument("--ks", default="")
    ap.add_argument("--blends", default="")
    ap.add_argument("--velocities", type=lambda s: [int(x) for x in s.split(",")], default=[pl.VEL_MIDI])
    ap.add_argument("--csv", default=None)
    ap.add_argument("--per-note", default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)

    if a.command == "grid":
        if a.csv is None:
            ap.error("grid needs --csv FILE")
        alphas, ks, blends = pl.parse_axis(a.alphas), pl.parse_axis(a.ks), pl.parse_axis(a.blends)
        if alphas.size + ks.size + blends.size == 0:
            ap.error("grid needs at least one of --alphas, --ks, --blends")
        law_csv, note_csv, amps = pl.grid(pl.load_obm(a.harmonics), alphas, ks, blends, a.velocities, a.device)
        with open(a.csv, "w", newline="") as f:
            f.write(law_csv)
        print(f"Wrote {alphas.size + ks.size + blends.size} law points x {amps.shape[0]} carriers → {a.csv}")
        if a.per_note:
            with open(a.per_note, "w", newline="") as f:
                f.write(note_csv)
            print(f"Wrote the best law point per (note, velocity) → {a.per_note}")
        return {"law_csv": law_csv, "note_csv": note_csv, "amps": amps}

    text = pl.analyse(a.harmonics, a.model, a.device)
    sys.stdout.write(text)
    return {"report": text}


if __name__ == "__main__":
    main()
