#!/usr/bin/env python3
"""ml/train_mlp.py on the GPU: the same flags, the same report, model_weights.json as the result -- and `sweep`, which trains a whole grid
of models in ONE call and exports the best of them for tools/mlp_eval.py.

  python tools/train_mlp.py --data ml_data/training_data.npz [--epochs 2000 --lr 3e-3 --hidden 16 --patience 150 --huber-delta 5.0
         --weight-decay 1e-4 --seed 42 --export ml_data/model_weights.json --no-split --mask-decay-h3]
  python tools/train_mlp.py sweep --data d.npz --seeds 0-63 --lrs 1e-3,3e-3 --weight-decays 0,1e-4 --huber-deltas 5.0 [--folds 5]
         [--csv sweep.csv] [--export-dir sets/ --top 8]

Against the reference: --hidden defaults to 16 and takes at most 16 (the weight set the library evaluates has 16 hidden units; a smaller
network is the same set with zero padding, and the exported JSON always says hidden_size 16); the training runs in float64 from the
initial values torch draws for --seed; paths are taken as given (not relative to the script); no model_checkpoint.pt is written.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_ints(text):
    """"0-63" / "1,2,5" / "0-3,42" -> [int]."""
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


def parse_floats(text):
    return [float(p) for p in text.split(",") if p.strip()]


def _common(ap):
    ap.add_argument("--data", default="ml_data/training_data.npz", help="Training data path")
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--patience", type=int, default=150)
    ap.add_argument("--no-split", action="store_true", help="Train on all data (no train/val split)")
    ap.add_argument("--mask-decay-h3", action="store_true", help="Mask decay_H3 targets (too noisy)")
    ap.add_argument("--device", type=int, default=0)


def report_lines(data, result, a, n_params):
    """The reference's report of one run (train_mlp.py:299-320 and evaluate), from a result with its history."""
    from openwurli_amd import mlp_train as mt
    tr, va = (data.split & 1) != 0, (data.split & 2) != 0
    lines = [f"Loading data from {a.data}..."]
    if a.mask_decay_h3:
        lines.append(f"  Masked decay_H3 (index {mt.N_FREQ + 1}): {a.n_masked} entries zeroed")
    if bool((tr & va).all()):
        lines.append(f"  Small dataset ({len(data.inputs)} points) — training on all data (no split)")
    lines += [f"  Train: {int(tr.sum())}, Val: {int(va.sum())}",
              f"  Train mask coverage: {data.mask[tr].mean():.1%}",
              f"  Val mask coverage: {data.mask[va].mean():.1%}",
              "",
              f"Model: {n_params} parameters (hidden={a.hidden})",
              f"Training: epochs={a.epochs}, lr={a.lr}, patience={a.patience}, huber_delta={a.huber_delta}, wd={a.weight_decay}",
              ""]
    lines += mt.format_epoch_lines(result, a.patience)
    lines += ["", f"  Best validation loss: {result.best_val_loss:.4f}"]
    lines += mt.format_evaluation(mt.evaluate(result.weights, data))
    return lines


def run_single(a):
    import numpy as np
    from openwurli_amd import mlp_train as mt
    a.n_masked = int(np.load(a.data)["mask"][:, mt.N_FREQ + 1].sum()) if a.mask_decay_h3 else 0
    data = mt.load_data(a.data, no_split=a.no_split, mask_decay_h3=a.mask_decay_h3)
    init = mt.init_like_reference(a.seed, a.hidden)
    m = mt.model(lr=a.lr, weight_decay=a.weight_decay, huber_delta=a.huber_delta, epochs=a.epochs, patience=a.patience)
    result = mt.train(data, [init], [m], device=a.device, history=True)[0]
    h = a.hidden
    print("\n".join(report_lines(data, result, a, 2 * h + h + h * h + h + h * 11 + 11)))
    os.makedirs(os.path.dirname(os.path.abspath(a.export)), exist_ok=True)
    with open(a.export, "w") as f:
        json.dump(result.weights.to_json(), f, indent=2)
    print(f"\n  Exported weights to {a.export}")
    print(f"  Total parameters: {2 * h + h + h * h + h + h * 11 + 11}")
    return result


def run_sweep(a):
    from openwurli_amd import mlp_train as mt
    data = mt.load_data(a.data, no_split=a.no_split, mask_decay_h3=a.mask_decay_h3)
    splits = mt.kfold_splits(len(data.inputs), a.folds, a.fold_seed) if a.folds else None
    fixed = dict(epochs=a.epochs, patience=a.patience)
    if a.mask_decay_h3:
        fixed["mask_decay_h3"] = True
    models, inits, rows, labels = mt.sweep(data, parse_ints(a.seeds), parse_floats(a.lrs), parse_floats(a.weight_decays), parse_floats(a.huber_deltas),
                                           splits=splits, hidden=a.hidden, **fixed)
    results = mt.train(data, inits, models, splits=rows, device=a.device)
    text = mt.format_sweep_csv(labels, results)
    if a.csv:
        os.makedirs(os.path.dirname(os.path.abspath(a.csv)), exist_ok=True)
        with open(a.csv, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    paths = mt.export_top(results, a.top, a.export_dir) if a.export_dir else []
    best = min(range(len(results)), key=lambda i: (results[i].best_val_loss, i))
    print(json.dumps({"models": len(results), "best_model": best, "best_val_loss": results[best].best_val_loss, "csv": a.csv, "exported": paths}))
    return results


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "sweep":
        ap = argparse.ArgumentParser(prog="train_mlp.py sweep", description="Train seeds x lrs x weight decays x Huber deltas x folds in one call")
        _common(ap)
        ap.add_argument("--seeds", default="0-63")
        ap.add_argument("--lrs", default="3e-3")
        ap.add_argument("--weight-decays", default="1e-4")
        ap.add_argument("--huber-deltas", default="5.0")
        ap.add_argument("--folds", type=int, default=0, help="K > 1: K-fold splits of the rows instead of the 80/20 split")
        ap.add_argument("--fold-seed", type=int, default=42)
        ap.add_argument("--csv", default=None, help="one row per model (default: standard output)")
        ap.add_argument("--export-dir", default=None)
        ap.add_argument("--top", type=int, default=8)
        return run_sweep(ap.parse_args(argv[1:]))
    ap = argparse.ArgumentParser(description="Train MLP for parameter corrections")
    _common(ap)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--huber-delta", type=float, default=5.0, help="Huber loss delta (switch from quadratic to linear)")
    ap.add_argument("--weight-decay", type=float, default=1e-4, help="Weight decay for Adam optimizer")
    ap.add_argument("--seed", type=int, default=42, help="Random seed for reproducibility")
    ap.add_argument("--export", default="ml_data/model_weights.json", help="Export path for weights JSON")
    return run_single(ap.parse_args(argv))


if __name__ == "__main__":
    main()
