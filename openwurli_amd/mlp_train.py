"""Training note-on MLP weight sets on the GPU (ml/train_mlp.py; stage 6 of ml/pipeline.py), many models per call.

`train` runs every model's whole training loop -- Adam, the validation pass, ReduceLROnPlateau, early stopping, the best-state snapshot --
inside ONE kernel launch (k_mlp_train: one wavefront per model, float64), so seeds x learning rates x weight decays x Huber deltas x splits
cost about what one model costs.  The results are `MlpWeights` that `mlp.infer` / `mlp.batch_render_mlp` / tools/mlp_eval.py take as they
stand.  `load_data` and `init_like_reference` are the reference's host-side preparation (numpy, and torch's own initialiser on the CPU);
there is no CPU fallback for the training itself.
"""
import collections
import ctypes as C
import itertools
import json
import os

import numpy as np

from . import binding
from .binding import OwError
from .mlp import HIDDEN, OUTPUTS, MlpWeights

N_FREQ, N_DECAY = 5, 5
DS_IDX = N_FREQ + N_DECAY                  # train_mlp.py:26-29
ALL_TARGETS = (1 << OUTPUTS) - 1
DECAY_H3_BIT = 1 << (N_FREQ + 1)           # --mask-decay-h3: target 6
TARGET_NAMES = tuple(f"freq_H{h}" for h in range(2, 2 + N_FREQ)) + tuple(f"decay_H{h}" for h in range(2, 2 + N_DECAY)) + ("ds_corr",)
TARGET_UNITS = ("cents",) * N_FREQ + ("ratio",) * N_DECAY + ("",)
# train_mlp.py's defaults: main()'s flags, train()'s min_lr and scheduler
DEFAULTS = dict(lr=3e-3, min_lr=1e-5, weight_decay=1e-4, huber_delta=5.0, sched_factor=0.5, epochs=2000, patience=150, sched_patience=30,
                target_mask=ALL_TARGETS)

Data = collections.namedtuple("Data", "inputs targets mask weights split target_means target_stds")
Data.__doc__ = """load_data's result: inputs [n, 2], targets [n, 11] (standardised), mask [n, 11] bool, weights [n], split [n] uint8 (bit 0 = train
row, bit 1 = validation row), target_means / target_stds [11] -- float64."""


class TrainResult:
    """One trained model: `weights` (MlpWeights, the best state, with the data's means and stds), best_val_loss, best_epoch, epochs_run,
    last_lr, last_train_loss, last_val_loss, lr_reductions, status (0 = ok, 1 = no epoch improved: weights = the initial set) and
    history (None or [epochs_run, 3]: train loss, validation loss, learning rate in force during the epoch's step)."""

    def __init__(self, weights, row, history=None):
        self.weights = weights
        for name in ("best_val_loss", "last_train_loss", "last_val_loss", "last_lr"):
            setattr(self, name, float(row[name]))
        for name in ("best_epoch", "epochs_run", "lr_reductions", "status"):
            setattr(self, name, int(row[name]))
        self.history = history


def load_data(path_or_arrays, no_split=False, mask_decay_h3=False):
    """train_mlp.py:73-137, statement by statement, in float64: decay targets clipped to +-20, ds to [0.5, 2.0], per-target mean and
    population standard deviation over masked-in entries (std floored at 1e-6; mean 0 and std 1 with <= 1 valid entry), the 80 / 20 split
    of np.random.RandomState(42).permutation(n), or every row in both parts with no_split or n < 20.  path_or_arrays: an .npz path, or a
    mapping / 4-tuple of inputs, targets, mask, weights (not modified)."""
    if isinstance(path_or_arrays, (str, os.PathLike)):
        d = np.load(os.fspath(path_or_arrays))
        d = {k: d[k] for k in ("inputs", "targets", "mask", "weights")}
    elif isinstance(path_or_arrays, dict):
        d = path_or_arrays
    else:
        d = dict(zip(("inputs", "targets", "mask", "weights"), path_or_arrays))
    inputs = np.array(d["inputs"], dtype=np.float64)
    targets = np.array(d["targets"], dtype=np.float64)
    mask = np.array(d["mask"], dtype=bool)
    weights = np.array(d["weights"], dtype=np.float64)
    n_targets = targets.shape[1]
    if inputs.ndim != 2 or inputs.shape[1] != 2 or n_targets != OUTPUTS or mask.shape != targets.shape or weights.shape != (len(inputs),) or len(targets) != len(inputs):
        raise ValueError(f"training data: inputs {inputs.shape}, targets {targets.shape}, mask {mask.shape}, weights {weights.shape}; "
                         f"expected [n, 2], [n, {OUTPUTS}], [n, {OUTPUTS}], [n]")
    if mask_decay_h3:
        mask[:, N_FREQ + 1] = False
    decay = slice(N_FREQ, N_FREQ + N_DECAY)
    targets[:, decay] = np.clip(targets[:, decay], -20.0, 20.0)
    targets[:, DS_IDX] = np.clip(targets[:, DS_IDX], 0.5, 2.0)
    means, stds = np.zeros(n_targets), np.ones(n_targets)
    for i in range(n_targets):
        valid = mask[:, i]
        if valid.sum() > 1:
            means[i] = targets[valid, i].mean()
            stds[i] = max(targets[valid, i].std(), 1e-6)
    targets_norm = (targets - means) / stds
    n = len(inputs)
    split = np.zeros(n, dtype=np.uint8)
    if no_split or n < 20:
        split[:] = 3
    else:
        perm = np.random.RandomState(42).permutation(n)
        cut = int(0.8 * n)
        split[perm[:cut]] |= 1
        split[perm[cut:]] |= 2
    return Data(np.ascontiguousarray(inputs), np.ascontiguousarray(targets_norm), mask, weights, split, means, stds)


def init_like_reference(seed, hidden=16):
    """The initial values train_mlp.py starts from: torch.manual_seed(seed), then nn.Sequential(Linear(2, hidden), ReLU, Linear(hidden,
    hidden), ReLU, Linear(hidden, 11)) on the CPU -- as float64 in an MlpWeights, zero-padded to 16 hidden units (a padded unit stays
    exactly zero through training), target_means 0 and target_stds 1.  The caller's torch random state is left as it was."""
    hidden = int(hidden)
    if not 1 <= hidden <= HIDDEN:
        raise ValueError(f"hidden must be 1..{HIDDEN}, got {hidden}")
    import torch
    import torch.nn as nn
    with torch.random.fork_rng(devices=[]):           # the CPU generator alone: no device is asked for its state
        torch.manual_seed(int(seed))
        net = nn.Sequential(nn.Linear(2, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, OUTPUTS))
    p = [q.detach().numpy().astype(np.float64) for q in net.parameters()]
    w1, b1, w2, b2, w3, b3 = np.zeros((HIDDEN, 2)), np.zeros(HIDDEN), np.zeros((HIDDEN, HIDDEN)), np.zeros(HIDDEN), np.zeros((OUTPUTS, HIDDEN)), np.zeros(OUTPUTS)
    w1[:hidden], b1[:hidden], w2[:hidden, :hidden], b2[:hidden], w3[:, :hidden], b3[:] = p
    return MlpWeights(w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, target_means=np.zeros(OUTPUTS), target_stds=np.ones(OUTPUTS))


def model(**kw):
    """One model's hyper-parameters: train_mlp.py's defaults with the given keys replaced (lr, min_lr, weight_decay, huber_delta,
    sched_factor, epochs, patience, sched_patience, target_mask; mask_decay_h3=True clears target 6)."""
    m = dict(DEFAULTS)
    if kw.pop("mask_decay_h3", False):
        m["target_mask"] = ALL_TARGETS & ~DECAY_H3_BIT
    unknown = set(kw) - set(m)
    if unknown:
        raise ValueError(f"unknown hyper-parameter {sorted(unknown)}")
    m.update(kw)
    return m


def _model_array(models):
    if isinstance(models, dict):
        models = [models]
    if isinstance(models, np.ndarray) and models.dtype.names:
        return np.ascontiguousarray(models.astype(np.dtype(binding.MLP_TRAIN_MODEL_DTYPE)))
    models = list(models)
    arr = np.zeros(len(models), dtype=np.dtype(binding.MLP_TRAIN_MODEL_DTYPE))
    for i, m in enumerate(models):
        m = model(**m)
        for name in arr.dtype.names:
            arr[name][i] = m[name]
    return arr


def train(data, inits, models, splits=None, device=0, history=False, kernel_ms=None):
    """Train len(models) models in one call of ow_mlp_train.  data: load_data's result (or anything with its fields); inits: one MlpWeights
    per model (or one for all); models: dictionaries of `model`'s keys (or a structured array of binding.MLP_TRAIN_MODEL_DTYPE); splits:
    None (data.split for every model), one row, or [n_models, n_rows] uint8 with bit 0 = train row, bit 1 = validation row.
    kernel_ms: a list that receives the kernel's time in ms.  Returns a list of TrainResult."""
    lib = binding.load_library()
    marr = _model_array(models)
    n_models = marr.size
    inputs = np.ascontiguousarray(data.inputs, dtype=np.float64)
    targets = np.ascontiguousarray(data.targets, dtype=np.float64)
    mask = np.ascontiguousarray(np.asarray(data.mask) != 0, dtype=np.uint8)
    weights = np.ascontiguousarray(data.weights, dtype=np.float64)
    n = inputs.shape[0]
    if inputs.shape != (n, 2) or targets.shape != (n, OUTPUTS) or mask.shape != (n, OUTPUTS) or weights.shape != (n,):
        raise ValueError(f"training data: inputs {inputs.shape}, targets {targets.shape}, mask {mask.shape}, weights {weights.shape}")
    sp = np.asarray(data.split if splits is None else splits, dtype=np.uint8)
    if sp.ndim == 1:
        sp = np.broadcast_to(sp, (n_models, sp.size))
    sp = np.ascontiguousarray(sp)
    if sp.shape != (n_models, n):
        raise ValueError(f"splits: shape {sp.shape}, expected {(n_models, n)}")
    if isinstance(inits, MlpWeights):
        inits = [inits] * n_models
    inits = list(inits)
    if len(inits) != n_models:
        raise ValueError(f"{len(inits)} initial sets for {n_models} models")
    means = np.asarray(data.target_means, dtype=np.float64)
    stds = np.asarray(data.target_stds, dtype=np.float64)
    init = np.ascontiguousarray(np.stack([w.flat() for w in inits])) if inits else np.zeros((0, 529))
    if n_models:
        init[:, 507:518] = means          # the normalisation travels with the set: best_out is complete
        init[:, 518:529] = stds
    best = np.zeros_like(init)
    results = np.zeros(n_models, dtype=np.dtype(binding.MLP_TRAIN_RESULT_DTYPE))
    hist_epochs = int(marr["epochs"].max()) if (history and n_models) else 0
    hist = np.zeros((n_models, hist_epochs, 3)) if history else None
    ms = C.c_double(0.0)
    cfg = binding.OwMlpTrainCfg(n, hist_epochs, int(device), C.pointer(ms) if kernel_ms is not None else None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.ow_mlp_train(p(inputs), p(targets), p(mask), p(weights), p(sp), p(init), p(marr), n_models, C.byref(cfg), p(best), p(results),
                          p(hist) if history else None)
    if rc != 0:
        raise OwError(binding.take_error(lib))
    if kernel_ms is not None:
        kernel_ms.append(ms.value)
    return [TrainResult(MlpWeights.from_flat(best[i]), results[i], hist[i, :int(results["epochs_run"][i])].copy() if history else None)
            for i in range(n_models)]


def kfold_splits(n, k, seed):
    """[k, n] uint8: the rows in a RandomState(seed) permutation cut into k folds (np.array_split); fold f's rows are the validation rows
    of split f, all the others its train rows."""
    if not 2 <= k <= n:
        raise ValueError(f"k-fold: k must be 2..n, got k = {k}, n = {n}")
    perm = np.random.RandomState(seed).permutation(n)
    out = np.full((k, n), 1, dtype=np.uint8)
    for f, rows in enumerate(np.array_split(perm, k)):
        out[f, rows] = 2
    return out


def sweep(data, seeds, lrs=(DEFAULTS["lr"],), weight_decays=(DEFAULTS["weight_decay"],), huber_deltas=(DEFAULTS["huber_delta"],), splits=None,
          hidden=16, **fixed):
    """The product seeds x lrs x weight_decays x huber_deltas x splits, in that order (splits varies fastest): (models, inits, splits,
    labels) for `train`.  splits: None (data.split) or [n_splits, n_rows]; fixed: further `model` keys, the same for every model;
    labels: one dictionary per model (seed, lr, weight_decay, huber_delta, split)."""
    sp = np.asarray(data.split, dtype=np.uint8)[None, :] if splits is None else np.atleast_2d(np.asarray(splits, dtype=np.uint8))
    init_of = {s: init_like_reference(s, hidden) for s in seeds}
    models, inits, rows, labels = [], [], [], []
    for seed, lr, wd, delta, k in itertools.product(seeds, lrs, weight_decays, huber_deltas, range(len(sp))):
        models.append(model(lr=lr, weight_decay=wd, huber_delta=delta, **fixed))
        inits.append(init_of[seed])
        rows.append(sp[k])
        labels.append(dict(seed=seed, lr=lr, weight_decay=wd, huber_delta=delta, split=k))
    return models, inits, np.stack(rows), labels


# ---- the command's text (train_mlp.py:179-186, 193-223) and the sweep's files ---------------------------------------------------------
def format_epoch_lines(result, patience):
    """The `Epoch` lines at epoch 1 and every 100th, and the early-stopping line, from a result's history.  The lr printed is the one
    after the epoch's scheduler step, as the reference prints it."""
    h = result.history
    lines, best, stale = [], float("inf"), 0
    for e in range(len(h)):
        if h[e, 1] < best:
            best, stale = h[e, 1], 0
        else:
            stale += 1
        lr_after = h[e + 1, 2] if e + 1 < len(h) else result.last_lr
        if (e + 1) % 100 == 0 or e == 0:
            lines.append(f"  Epoch {e + 1:>5}: train={h[e, 0]:.4f}  val={h[e, 1]:.4f}  best={best:.4f}  lr={lr_after:.1e}  stale={stale}")
        if stale >= patience:
            lines.append(f"  Early stopping at epoch {e + 1} (patience={patience})")
            break
    return lines


def forward(weights, inputs):
    """The network's standardised outputs [n, 11] at inputs [n, 2], on the host (numpy): for the report's error table."""
    h = np.maximum(np.asarray(inputs, dtype=np.float64) @ weights.w1.T + weights.b1, 0.0)
    h = np.maximum(h @ weights.w2.T + weights.b2, 0.0)
    return h @ weights.w3.T + weights.b3


def evaluate(weights, data, split=None, target_mask=ALL_TARGETS):
    """train_mlp.py's evaluate(): per target (name, n_val, MAE, RMSE, unit) over the validation rows, in original units; targets without
    a valid validation entry are left out."""
    sp = np.asarray(data.split if split is None else split)
    rows = (sp & 2) != 0
    pred = forward(weights, data.inputs[rows]) * weights.target_stds + weights.target_means
    actual = data.targets[rows] * weights.target_stds + weights.target_means
    out = []
    for i, (name, unit) in enumerate(zip(TARGET_NAMES, TARGET_UNITS)):
        valid = np.asarray(data.mask)[rows, i] & bool((target_mask >> i) & 1)
        if valid.sum() == 0:
            continue
        err = (pred[:, i] - actual[:, i])[valid]
        out.append((name, int(valid.sum()), float(np.abs(err).mean()), float(np.sqrt((err ** 2).mean())), unit))
    return out


def format_evaluation(rows):
    lines = ["", "  Per-target validation error (original units):", f"  {'Target':>12} {'N_val':>5} {'MAE':>8} {'RMSE':>8} {'Unit'}", f"  {'-' * 45}"]
    lines += [f"  {name:>12} {n:>5} {mae:>8.2f} {rmse:>8.2f}  {unit}" for name, n, mae, rmse, unit in rows]
    return lines


SWEEP_HEADER = "model,seed,lr,weight_decay,huber_delta,split,best_val_loss,best_epoch,epochs_run,last_lr,lr_reductions,status"


def format_sweep_csv(labels, results):
    """One row per model, in the call's order."""
    lines = [SWEEP_HEADER]
    for i, (lab, r) in enumerate(zip(labels, results)):
        lines.append(f"{i},{lab['seed']},{lab['lr']:g},{lab['weight_decay']:g},{lab['huber_delta']:g},{lab['split']},{r.best_val_loss:.9g},{r.best_epoch},"
                     f"{r.epochs_run},{r.last_lr:g},{r.lr_reductions},{r.status}")
    return "\n".join(lines) + "\n"


def export_top(results, top, directory):
    """The `top` models with the lowest best validation loss (ties: the lower index) as rank01_model0007.json, ... in `directory`, each a
    model_weights.json that tools/mlp_eval.py --weights takes.  Returns the paths, best first."""
    order = sorted(range(len(results)), key=lambda i: (results[i].best_val_loss, i))[:max(int(top), 0)]
    os.makedirs(directory, exist_ok=True)
    paths = []
    for rank, i in enumerate(order, 1):
        path = os.path.join(directory, f"rank{rank:02d}_model{i:04d}.json")
        with open(path, "w") as f:
            json.dump(results[i].weights.to_json(), f, indent=2)
        paths.append(path)
    return paths
