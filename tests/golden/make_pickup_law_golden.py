#!/usr/bin/env python3
"""Generate tests/golden/pickup_law_golden.json and pickup_law_clips.npz by running the REFERENCE's own ml/h3_analysis_v2.py on the
fixture of tests/pickup_law_ref.py.  The reference checkout is not part of this repository and is absent where the GPU tests run, so its
outputs travel as this fixture.

    python tests/golden/make_pickup_law_golden.py --reference <checkout of the reference>

`soundfile` is not installed.  The script needs sf.read only, so a stand-in over the standard library's `wave` is registered before the
import: PCM as int / 2^(bits - 1) in float64, soundfile's default.  The module's __file__ is pointed at a temporary directory that holds
the fixture's harmonics.json, model_harmonics.json and clips.

What the JSON holds:
  harmonics, model   the two input files (source_file as a bare file name: the tests write the clips where they like)
  vel_scale          per note the script's two scales: compute_harmonics' (from midi_approx) and the inline variants' (from the note)
  alpha              compute_harmonics(f0, ds, alpha=a) for every note and every a of np.arange(1.0, 2.51, 0.1): amps [16][8], y_peak
  k, blend           the script's own inline blocks (:291-319, :346-375, executed from its source text) for every note and list entry: [n][3]
  snr                measure_interharmonic_floor per clip: h_amps, snr (null for NaN)
  report             main()'s stdout
  movement           tests/pickup_law_ref.py's movement on all of these jobs, per class of figure; the GPU test's floors are 2.5 x these
The generator asserts what the tests rely on: three reliable notes or more and one that is not, an H3 > H2 note, every printed figure at
least 10 x its class's movement away from a rounding boundary, the best alpha ahead of the runner-up by as much.  Replace a seed if not.
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import textwrap
import types
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pickup_law_ref as own  # noqa: E402
from openwurli_amd import pickup_law as pl  # noqa: E402

SNR_MOVEMENT_DB = 1e-6      # step 1's figures: far above what ow_dft_magnitudes' floor ((n + 4) 2^-52 of the scale) moves a 10+ dB ratio


def _sf_read(path):
    with wave.open(str(path), "rb") as w:
        ch, width, sr, raw = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.readframes(w.getnframes())
    assert width == 2
    data = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    return (data.reshape(-1, ch) if ch > 1 else data), sr


def load_reference(root, workdir):
    sf = types.ModuleType("soundfile")
    sf.read = _sf_read
    sys.modules["soundfile"] = sf
    spec = importlib.util.spec_from_file_location("h3_analysis_v2_reference", os.path.join(root, "ml", "h3_analysis_v2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.__file__ = os.path.join(workdir, "h3_analysis_v2.py")
    return mod


def inline_block(root, first, last, marker):
    """Lines first..last (1-based) of the script as a code object: its inline k / blend variants, which are no function."""
    with open(os.path.join(root, "ml", "h3_analysis_v2.py")) as f:
        lines = f.read().split("\n")[first - 1:last]
    assert marker in lines[0], lines[0]
    assert "amps.append" in lines[-1], lines[-1]
    return compile(textwrap.dedent("\n".join(lines)), f"h3_analysis_v2.py:{first}-{last}", "exec")


def margin(x, decimals):
    """How far x lies from the nearest boundary between two printed values."""
    return abs((abs(float(x)) * 10 ** decimals) % 1.0 - 0.5) / 10 ** decimals


def write_wav(path, q, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(q.astype("<i2").tobytes())


def plain(x):
    return None if x != x else float(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "pickup_law_golden.json"))
    ap.add_argument("--clips", default=os.path.join(HERE, "pickup_law_clips.npz"))
    args = ap.parse_args()

    clips = {note[0]: own.fixture_clip(*note) for note in own.FIXTURE_NOTES}
    midis = sorted(clips)
    with tempfile.TemporaryDirectory() as tmp:
        entries = []
        for midi, _, amps, _, _, _ in own.FIXTURE_NOTES:
            path = os.path.join(tmp, f"note_{midi}.wav")
            write_wav(path, clips[midi], own.SR)
            entries.append(own.fixture_entry(midi, amps, path))
        model = {str(e["midi_note"]): {"midi_note": e["midi_note"], "f0": e["f0"],
                                       "windows": {"early_sustain": {"amps_dB_rel_H1": e["windows"]["early_sustain"]["amps_dB_rel_H1"]}}} for e in entries}
        with open(os.path.join(tmp, "harmonics.json"), "w") as f:
            json.dump(entries, f)
        with open(os.path.join(tmp, "model_harmonics.json"), "w") as f:
            json.dump(model, f)
        ref = load_reference(args.reference, tmp)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ref.main()
        report = buf.getvalue()
        snr = {}
        for e in entries:
            h, s = ref.measure_interharmonic_floor(e["source_file"], e["f0"])
            snr[str(e["midi_note"])] = {"h_amps": [plain(v) for v in h], "snr": [plain(v) for v in s]}
        for e in entries:
            e["source_file"] = os.path.basename(e["source_file"])

    alphas = np.arange(1.0, 2.51, 0.1)
    assert np.array_equal(alphas, pl.ALPHAS)
    block_k = inline_block(args.reference, 291, 319, "# Custom nonlinearity")
    block_b = inline_block(args.reference, 346, 375, "vel = 80/127.0")
    out_alpha, out_k, out_b, scales = {}, {}, {}, {}
    for midi in midis:
        f0, ds = ref.midi_to_freq(midi), ref.pickup_ds(midi)
        rows, peak = [], None
        for a in alphas:
            amps, y_peak = ref.compute_harmonics(f0, ds, alpha=a)
            rows.append([float(v) for v in amps])
            assert peak is None or peak == float(y_peak)
            peak = float(y_peak)
        out_alpha[str(midi)] = {"amps": rows, "y_peak": peak}
        base = {"np": np, "velocity_exponent": ref.velocity_exponent, "SENSITIVITY": ref.SENSITIVITY, "HPF_FC": ref.HPF_FC, "midi": midi, "f0": f0, "ds": ds}
        out_k[str(midi)], out_b[str(midi)] = [], []
        for k in pl.KS:
            ns = dict(base, k=k)
            exec(block_k, ns)
            out_k[str(midi)].append([float(v) for v in ns["amps"]])
        for blend in pl.BLENDS:
            ns = dict(base, blend=blend)
            exec(block_b, ns)
            out_b[str(midi)].append([float(v) for v in ns["amps"]])
        midi_approx = 69 + 12 * np.log2(f0 / 440.0)
        scales[str(midi)] = {"approx": float((80 / 127.0) ** ref.velocity_exponent(midi_approx)), "midi": float((80 / 127.0) ** ref.velocity_exponent(midi)),
                             "f0": float(f0), "ds": float(ds)}

    # the restatement's movement on every job of the run (both carriers of every note, the 29 laws)
    carrier_rows, keys = pl.carriers(midis)
    kinds, params = pl.script_laws()
    obm = {e["midi_note"]: {"f0": e["f0"], "db": e["windows"]["early_sustain"]["amps_dB_rel_H1"], "source_file": ""} for e in entries}
    recorded = [obm[m]["db"][1:3] for m, _, _ in keys]
    movement = own.movement(carrier_rows, kinds, params, recorded)
    print("movement", movement)

    # what the tests rely on
    numbers = {"midis": midis, "amps": np.zeros((len(midis), 2, 29, 8)), "y_peak": np.zeros((len(midis), 2))}
    for i, m in enumerate(midis):
        numbers["amps"][i, 0, :16] = out_alpha[str(m)]["amps"]
        numbers["amps"][i, 1, 16:23, :3] = out_k[str(m)]
        numbers["amps"][i, 1, 23:, :3] = out_b[str(m)]
        numbers["y_peak"][i, 0] = out_alpha[str(m)]["y_peak"]
    snr_pairs = {m: tuple(float("nan") if snr[str(m)]["snr"][i] is None else snr[str(m)]["snr"][i] for i in (1, 2)) for m in midis}
    head = report.split("=" * 95 + "\nSUMMARY")[0]
    mine = pl.report(obm, snr_pairs, numbers)
    assert mine.rstrip("\n") == head.rstrip("\n"), "the tool's report differs from the script's"
    reliable = [m for m in midis if snr_pairs[m][1] > 10.0]
    assert len(reliable) >= 3 and len(reliable) < len(midis), reliable
    assert any(obm[m]["db"][2] > obm[m]["db"][1] for m in midis)
    for m in midis:
        for v in snr_pairs[m]:
            assert v != v or margin(v, 1) > 10 * SNR_MOVEMENT_DB, (m, v)
        h3_snr = snr_pairs[m][1]
        assert h3_snr != h3_snr or abs(h3_snr - 10.0) > 10 * SNR_MOVEMENT_DB, (m, h3_snr)
        assert margin(numbers["y_peak"][midis.index(m), 0], 3) > 10 * movement["y_peak"], (m, "y_peak")
    totals = []
    for law in range(29):
        h2e, h3e = pl.law_errors(obm, numbers, reliable, 0 if law < 16 else 1, law)
        a2, a3 = np.array(h2e), np.array(h3e)
        figures = [np.mean(a2), np.std(a2), np.mean(a3), np.std(a3), np.sqrt(np.mean(a2 ** 2 + a3 ** 2))] + ([np.sqrt(np.mean(a3 ** 2))] if law < 16 else [])
        for v in figures:
            assert margin(v, 1) > 10 * movement["stats"], (law, v, margin(v, 1))
        if law < 16:
            totals.append(float(figures[4]))
    order = np.argsort(totals)
    assert totals[order[1]] - totals[order[0]] > 10 * movement["stats"], totals

    golden = {"source": "ml/h3_analysis_v2.py of the reference, numpy " + np.__version__, "sample_rate": own.SR, "midis": midis, "harmonics": entries,
              "model": model, "vel_scale": scales, "alpha": out_alpha, "k": out_k, "blend": out_b, "snr": snr, "report": report, "movement": movement,
              "reliable": reliable}
    with open(args.out, "w") as f:
        json.dump(golden, f)
    np.savez_compressed(args.clips, **{f"note_{m}": clips[m] for m in midis})
    print("reliable", reliable, "best alpha", float(alphas[order[0]]))
    print(head)


if __name__ == "__main__":
    main()
