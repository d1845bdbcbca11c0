#!/usr/bin/env python3
"""Times the training sweep: 1 024 models (64 seeds x 4 learning rates x 4 weight decays) on 512 synthetic rows (tests/mlp_train_ref.py's
synthetic, 80 / 20 split), 2 000 epochs with patience 150, in ONE ow_mlp_train call; one of the models alone as a second case; and the
torch float64 loop of tests/mlp_train_ref.py on the CPU (16 threads) for --cpu-models of the models (default 8), scaled by count to the
sweep -- the CPU figure is an extrapolation, and the output says so.  Prints one JSON line: wall time and k_mlp_train's own time (device
events) per case, ns per row-epoch (of the model alone: time / rows of a pass / epochs run; of the sweep: time / the sum over the models),
the ratio sweep / one model, the speed-up over torch.

  python tools/bench_mlp_train.py [--models 1024] [--rows 512] [--epochs 2000] [--patience 150] [--repeats 3] [--cpu-models 8] [--no-cpu]
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


def main(argv=None):
    import mlp_train_ref as ref
    from openwurli_amd import mlp_train as mt
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--patience", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-models", type=int, default=8)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    inputs, targets, mask, weights = ref.synthetic(a.rows, 1)
    data = mt.Data(inputs, targets, mask, weights, ref.split_80_20(a.rows), [0.0] * 11, [1.0] * 11)
    lrs, wds = (1e-3, 2e-3, 3e-3, 6e-3), (0.0, 1e-5, 1e-4, 1e-3)
    seeds = list(range(max(1, -(-a.models // 16))))
    models, inits, rows, labels = mt.sweep(data, seeds, lrs, wds, epochs=a.epochs, patience=a.patience)
    models, inits, rows, labels = models[:a.models], inits[:a.models], rows[:a.models], labels[:a.models]
    rows_per_epoch = int(((data.split & 1) != 0).sum() + ((data.split & 2) != 0).sum())      # a train pass and a validation pass

    def case(ms, ins, sp):
        mt.train(data, ins, ms, splits=sp, device=a.device)                                 # warm-up: library, context, code object
        wall, kern, results = [], [], None
        for _ in range(a.repeats):
            k = []
            t0 = time.perf_counter()
            results = mt.train(data, ins, ms, splits=sp, device=a.device, kernel_ms=k)
            wall.append(time.perf_counter() - t0)
            kern.append(k[0] * 1e-3)
        row_epochs = sum(r.epochs_run for r in results) * rows_per_epoch
        return results, {"wall_ms": round(1e3 * statistics.median(wall), 3), "wall_min_ms": round(1e3 * min(wall), 3), "wall_max_ms": round(1e3 * max(wall), 3),
                         "k_mlp_train_ms": round(1e3 * statistics.median(kern), 3), "epochs_run_total": sum(r.epochs_run for r in results),
                         "epochs_run_max": max(r.epochs_run for r in results), "ns_per_row_epoch": round(1e9 * statistics.median(kern) / row_epochs, 3)}

    results, sweep = case(models, inits, rows)
    longest = max(range(len(results)), key=lambda i: results[i].epochs_run)                   # the model that bounds the sweep's time
    _, alone = case([models[longest]], [inits[longest]], rows[longest:longest + 1])
    res = {"models": len(models), "rows": a.rows, "rows_per_epoch": rows_per_epoch, "epochs": a.epochs, "patience": a.patience, "repeats": a.repeats,
           "sweep": sweep, "one_model_alone": dict(alone, model=longest),
           "sweep_over_one_model_kernel": round(sweep["k_mlp_train_ms"] / alone["k_mlp_train_ms"], 3)}
    if not a.no_cpu:
        import torch
        torch.set_num_threads(16)
        pick = list(range(0, len(models), max(1, len(models) // max(a.cpu_models, 1))))[:a.cpu_models]
        t0 = time.perf_counter()
        same = 0
        for i in pick:
            m = {k: v for k, v in models[i].items()}
            r = ref.train(ref.make_net(labels[i]["seed"]), inputs, targets, mask, weights, rows[i], **m)
            same += int(r["epochs_run"] == results[i].epochs_run and r["best_epoch"] == results[i].best_epoch)
        cpu_s = time.perf_counter() - t0
        scaled = cpu_s * len(models) / len(pick)
        res["torch_cpu_f64_16_threads"] = {"models_timed": len(pick), "wall_s": round(cpu_s, 3), "wall_s_scaled_by_count_to_the_sweep": round(scaled, 1),
                                            "note": "timed on models_timed of the models, scaled by count: an extrapolation, not a measurement of the sweep",
                                            "models_with_the_gpu_run_s_best_epoch_and_epochs_run": same}
        res["speedup_over_torch_cpu_scaled"] = round(scaled / (sweep["wall_ms"] * 1e-3), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
