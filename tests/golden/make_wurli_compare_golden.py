#!/usr/bin/env python3
"""Generate tests/golden/wurli_compare_golden.json / .npz by running the REFERENCE's own tools/wurli_compare.py functions (compare_note,
select_best_notes, print_comparison_report, print_summary) here (build container only: /root/reference does not exist on the GPU box, so
the outputs travel as a fixture).

`soundfile` is not installed.  The script needs it for sf.read / sf.write only, so a small stand-in over the standard library's `wave`
is registered before the import.  It applies libsndfile's PCM rules as read from its source: write = PCM_16, lrint(x * 32767); read =
int / 2^(bits - 1) as float32.  openwurli_amd.wurli_compare.pcm16_roundtrip states the same rule, so golden and tool agree on it BY
CONSTRUCTION: the fixture does not confirm it.

Inputs: seeded synthetic pairs (tests/wurli_compare_ref.golden_clip: decaying harmonic series, 10 ms onset ramp, 1e-4 noise floor), kept
in the .npz as the integers of the files the reference read (16-bit "recorded" side, 24-bit "render" side).  Outputs: the reference's
comparison dictionaries, both report texts, the selection, and `movement`: per class of figure the largest float32 -> float64 difference
of our restatement on these clips.
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import wurli_compare_ref as own  # noqa: E402


def _sf_read(path, dtype="float32"):
    with wave.open(str(path), "rb") as w:
        ch, width, sr, raw = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.readframes(w.getnframes())
    if width == 2:
        ints = np.frombuffer(raw, dtype="<i2").astype(np.int64)
    else:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        ints = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        ints = ints - ((ints & 0x800000) << 1)
    y = (ints.astype(np.float64) / float(1 << (8 * width - 1))).astype(dtype)
    return (y.reshape(-1, ch) if ch > 1 else y), sr


def _sf_write(path, y, sr):
    q = np.clip(np.rint(np.asarray(y, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(sr))
        w.writeframes(q.tobytes())


def write_pcm24(path, q, sr):
    b = (q.astype(np.int64) & 0xFFFFFF)
    raw = np.stack([b & 0xFF, (b >> 8) & 0xFF, (b >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(3); w.setframerate(int(sr))
        w.writeframes(raw)


sf = types.ModuleType("soundfile")
sf.read, sf.write = _sf_read, _sf_write
sys.modules["soundfile"] = sf
sys.path.insert(0, "/root/reference/tools")
import wurli_compare as ref  # noqa: E402

NOTE_NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
# (midi, seed of the recorded side, seed of the render side, isolation, velocity_norm, duration)
PAIRS = [(40, 11, 12, 0.91, 0.62, 0.6), (60, 21, 22, 0.84, 0.35, 0.6), (77, 31, 33, 0.77, 0.80, 0.6), (96, 41, 42, 0.66, 0.004, 0.6)]


def plain(x):
    """The reference's values as JSON numbers (numpy scalars -> float; its rms figures are np.float32 under numpy 2)."""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.floating):
        return round(float(x), 1) if isinstance(x, np.float32) else float(x)
    if isinstance(x, np.integer):
        return int(x)
    return x


def main():
    arrays, comparisons, figs32, figs64 = {}, [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for i, (midi, s_real, s_synth, iso, vel, dur) in enumerate(PAIRS):
            f0 = 440.0 * 2.0 ** ((midi - 69) / 12.0)
            name = f"{NOTE_NAMES[midi % 12]}{midi // 12 - 1}"
            real_path, synth_path = os.path.join(tmp, f"{i}_real.wav"), os.path.join(tmp, f"{i}_synth.wav")
            sf.write(real_path, own.golden_clip(s_real, f0, dur), own.SR)                 # as the tool re-writes the recorded clip
            q24 = np.rint(own.golden_clip(s_synth, f0 * 1.001, dur, level=0.25) * 8388607.0).astype(np.int32)
            write_pcm24(synth_path, q24, own.SR)
            y_real, _ = sf.read(real_path)
            y_synth, _ = sf.read(synth_path)
            arrays[f"real{i}"] = np.rint(y_real.astype(np.float64) * 32768.0).astype(np.int16)
            arrays[f"synth{i}"] = q24
            comp = ref.compare_note(real_path, synth_path, f0)
            comparisons.append({"note_name": name, "midi_note": midi, "f0_hz": f0, "isolation": iso, "velocity_norm": vel,
                                "velocity_midi": max(1, min(127, int(vel * 127))), "duration": dur, "source": "take_a",
                                "real_wav": f"OUT/{name}_real.wav", "synth_wav": f"OUT/{name}_synth.wav", "comparison": comp})
            a, b = own.pair_figures(y_real.astype(np.float64), y_synth.astype(np.float64), f0, np.float32)
            c, d = own.pair_figures(y_real.astype(np.float64), y_synth.astype(np.float64), f0, np.float64)
            figs32 += [a, b]; figs64 += [c, d]
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            ref.print_comparison_report(comparisons, "OUT")
        report_text = out.getvalue()

        # selection and summary: two source directories, several takes per pitch, equal scores, a name filter
        meta = {"take_a": [("C4", 60, 0.84, 0.35, 0.9), ("C4", 60, 0.91, 0.50, 1.2), ("C4", 60, 0.84, 0.20, 0.4), ("E2", 40, 0.91, 0.62, 2.0),
                           ("F5", 77, 0.30, 0.80, 0.7), ("A#3", 58, 0.55, 0.44, 1.0)],
                "take_b": [("C4", 60, 0.95, 0.61, 0.3), ("C7", 96, 0.66, 0.004, 0.6), ("F5", 77, 0.77, 0.99, 1.5), ("C8", 108, 0.5, 1.0, 0.5),
                           ("E1", 28, 0.41, 0.1, 3.0)]}
        dirs = []
        for d, notes in meta.items():
            os.makedirs(os.path.join(tmp, d))
            dirs.append(os.path.join(tmp, d))
            with open(os.path.join(tmp, d, "extraction_metadata.json"), "w") as f:
                json.dump({"notes": [{"note_name": n, "midi_note": m, "isolation_score": iso, "velocity_norm": v, "duration": du,
                                      "f0_hz": 440.0 * 2.0 ** ((m - 69) / 12.0), "filename": f"{d}_{n}_{k}.wav"}
                                     for k, (n, m, iso, v, du) in enumerate(notes)]}, f)
        all_notes = ref.load_extractions(dirs + [os.path.join(tmp, "missing")])
        selections = {}
        for key, (top, names) in {"top1": (1, None), "top2": (2, None), "named": (3, ["C4", "F5"])}.items():
            sel = ref.select_best_notes(ref.load_extractions(dirs), top, names)
            selections[key] = [[midi, [n["filename"] for n in notes]] for midi, notes in sel.items()]
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            ref.print_summary(all_notes)
        summary_text = out.getvalue()

    golden = {"pairs": [list(p) for p in PAIRS], "comparisons": plain(comparisons), "report_text": report_text, "meta": meta,
              "selections": selections, "summary_text": summary_text, "movement": own.movement(figs32, figs64),
              "numpy": np.__version__}
    with open(os.path.join(HERE, "wurli_compare_golden.json"), "w") as f:
        json.dump(golden, f, indent=1, ensure_ascii=False)
    np.savez_compressed(os.path.join(HERE, "wurli_compare_golden.npz"), **arrays)
    print("wrote", len(PAIRS), "pairs; movement", golden["movement"])


if __name__ == "__main__":
    main()
