#!/usr/bin/env python3
"""ml/compute_residuals.py on the GPU: the same flags and report, training_data.npz as the result (what tools/train_mlp.py --data
reads).  The inter-harmonic SNR of all notes is measured in two calls, see openwurli_amd/residuals.py.

  python tools/compute_residuals.py --real harmonics.json --model model_harmonics.json [--output-dir ml_data] [--no-snr-filter]
         [--snr-threshold 10]

Against the reference: paths are taken as given (not relative to the script); source files are PCM WAV read with the standard library.
As there, --snr-threshold changes the printed line only: the masks use the module's SNR_THRESHOLD_DB.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from openwurli_amd import harmonics, residuals
    ap = argparse.ArgumentParser(description="Compute residuals and assemble training data")
    ap.add_argument("--real", default="harmonics.json", help="Real harmonic features JSON")
    ap.add_argument("--model", default="model_harmonics.json", help="Model harmonic features JSON")
    ap.add_argument("--output-dir", default="ml_data", help="Output directory for training_data.npz")
    ap.add_argument("--no-snr-filter", action="store_true", help="Disable SNR-based filtering (not recommended)")
    ap.add_argument("--snr-threshold", type=float, default=residuals.SNR_THRESHOLD_DB, help=f"SNR threshold in dB (default: {residuals.SNR_THRESHOLD_DB})")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    with open(a.real) as f:
        real = json.load(f)
    with open(a.model) as f:
        model = json.load(f)
    print(f"Real observations: {len(real)}")
    print(f"Model note/vel combos: {len(model)}")
    cache = None
    if not a.no_snr_filter:
        print(f"\nComputing inter-harmonic SNR (threshold: {a.snr_threshold:.0f} dB)...")
        audio = {}
        for feat in real:
            path = feat.get("source_file", "")
            if path and path not in audio and os.path.exists(path):
                try:
                    audio[path] = harmonics.load_audio(path)
                except Exception as e:
                    print(f"  WARNING: Could not load {path}: {e}")
        cache = residuals.load_audio_for_snr(real, audio, device=a.device)
        print(f"  SNR computed for {len(cache)} notes")
        print(residuals.format_snr_table(real, cache), end="")
    else:
        print("\nSNR filtering DISABLED (--no-snr-filter)")
    inputs, targets, mask, weights, note_ids, stats = residuals.assemble_dataset(real, model, cache)
    residuals.print_dataset_summary(inputs, targets, mask, weights, note_ids, stats)
    path = residuals.save_npz(a.output_dir, inputs, targets, mask, weights)
    print(f"\nSaved to {path}")
    print(f"  inputs:  {inputs.shape}")
    print(f"  targets: {targets.shape}")
    print(f"  mask:    {mask.shape}")
    print(f"  weights: {weights.shape}")
    return path


if __name__ == "__main__":
    main()
