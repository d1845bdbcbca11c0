"""MLP training without a device: the binding's struct sizes and cfg defaults, every refusal of ow_mlp_train with its message, load_data and
init_like_reference against direct restatements, the precondition of the GPU tests' whole runs (torch's own result does not move with the
order of the rows), and the tool's text from canned results.

The precondition tests and test_synthetic_data_is_what_it_says exercise tests/mlp_train_ref.py and torch alone, so they would pass without
the feature too (twelve cases); every other test here needs the new symbol or the new module."""
import ctypes as C
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import mlp_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "ow_mlp_train"


# ---- the binding's sizes, cfg defaults and exports (against the header: tests/test_abi_layout.py) ----------------------------------------------
def test_struct_layouts_header_binding_numpy():
    import openwurli_amd
    from openwurli_amd import binding as b, mlp_train
    assert [56, 32, 48] == [C.sizeof(b.OwMlpTrainModel), C.sizeof(b.OwMlpTrainCfg), C.sizeof(b.OwMlpTrainResult)]
    assert b.MLP_TRAIN_MODEL_DTYPE.itemsize == 56 and b.MLP_TRAIN_RESULT_DTYPE.itemsize == 48 and b.MLP_TRAIN_MAX_ROW_EPOCHS == 1 << 26
    cfg = b.OwMlpTrainCfg(70, 12, 1)
    assert (cfg.struct_size, cfg.model_size, cfg.n_rows, cfg.history_epochs, cfg.device) == (32, 56, 70, 12, 1) and not cfg.kernel_ms_out
    assert openwurli_amd.mlp_train is mlp_train and "mlp_train" in openwurli_amd.__all__ and "ow_mlp_train" in b.SYMBOLS


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.5


class _Call:
    """A valid call of ow_mlp_train on 24 rows and 3 models; `run` replaces arguments by name and returns (rc, message)."""

    def __init__(self, lib):
        from openwurli_amd import binding as b, mlp_train as mt
        self.lib, self.b = lib, b
        x, t, m, w = ref.synthetic(24, 5)
        self.args = dict(inputs=x, targets=t, mask=np.ascontiguousarray(m, dtype=np.uint8), row_weights=w,
                         split=np.ascontiguousarray(np.stack([ref.split_80_20(24)] * 3)),
                         init=np.ascontiguousarray(np.stack([mt.init_like_reference(s).flat() for s in (1, 2, 3)])),
                         models=mt._model_array([mt.model(epochs=5)] * 3), n_models=3, cfg=b.OwMlpTrainCfg(24, 0),
                         best_out=np.full((3, 529), SENTINEL), results=np.zeros(3, dtype=np.dtype(b.MLP_TRAIN_RESULT_DTYPE)), history_out=None)

    def run(self, **over):
        a = dict(self.args)
        a.update(over)
        p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
        self.lib.ow_clear_error()
        rc = self.lib.ow_mlp_train(p(a["inputs"]), p(a["targets"]), p(a["mask"]), p(a["row_weights"]), p(a["split"]), p(a["init"]), p(a["models"]),
                                   a["n_models"], None if a["cfg"] is None else C.byref(a["cfg"]), p(a["best_out"]), p(a["results"]), p(a["history_out"]))
        msg = self.lib.ow_last_error().decode()
        self.lib.ow_clear_error()
        return rc, msg

    def changed(self, name, index, value):
        v = self.args[name].copy()
        v[index] = value
        return {name: v}

    def model(self, i, **kw):
        v = self.args["models"].copy()
        for k, x in kw.items():
            v[k][i] = x
        return {"models": v}


def test_refusals(hiplib):
    c = _Call(hiplib)
    b = c.b
    for field, bad in (("struct_size", 24), ("model_size", 48)):
        cfg = b.OwMlpTrainCfg(24, 0)
        setattr(cfg, field, bad)
        assert c.run(cfg=cfg) == (-1, f"{FN}: ABI mismatch: ow_mlp_train_cfg.struct_size / model_size do not match this library's openwurli_hip.h (OW_ABI_VERSION 8)")
    for name in ("inputs", "targets", "mask", "row_weights", "split", "init", "models", "cfg", "best_out", "results"):
        assert c.run(**{name: None}) == (-1, f"{FN}: null argument"), name
    assert c.run(cfg=b.OwMlpTrainCfg(0, 0)) == (-1, f"{FN}: n_rows is 0")
    assert c.run(n_models=65536) == (-1, f"{FN}: more than 65535 models in one call")
    # the call's memory: the models' row lists, the history table (refused before any array is read)
    assert c.run(n_models=60000, cfg=b.OwMlpTrainCfg(4096, 0)) == (-1, f"{FN}: n_models x n_rows is above 2^27 (the models' row lists would pass 1 GiB)")
    assert c.run(history_out=np.zeros(3), cfg=b.OwMlpTrainCfg(24, (1 << 26))) == (-1, f"{FN}: n_models x history_epochs is above 2^27 (history_out would pass 3 GiB)")
    # non-finite data: the row and the field
    for value in (float("nan"), float("inf"), float("-inf")):
        assert c.run(**c.changed("inputs", (7, 1), value)) == (-1, f"{FN}: row 7: inputs[1] is not finite")
        assert c.run(**c.changed("targets", (23, 10), value)) == (-1, f"{FN}: row 23: targets[10] is not finite")
        assert c.run(**c.changed("row_weights", 0, value)) == (-1, f"{FN}: row 0: row_weights is not finite")
    # non-finite initial weights: the model and the field
    at = {"w1[3][1]": 3 * 2 + 1, "b1[15]": 32 + 15, "w2[2][5]": 48 + 2 * 16 + 5, "b2[0]": 304, "w3[10][15]": 320 + 10 * 16 + 15, "b3[4]": 496 + 4,
          "target_means[10]": 507 + 10, "target_stds[0]": 518}
    for field, k in at.items():
        assert c.run(**c.changed("init", (2, k), float("nan"))) == (-1, f"{FN}: model 2: init.{field} is not finite")
    # hyper-parameters: the model and the field
    nan, inf = float("nan"), float("inf")
    for value in (0.0, -1e-3, nan, inf):
        assert c.run(**c.model(1, lr=value)) == (-1, f"{FN}: model 1: lr is not a finite positive number")
        assert c.run(**c.model(2, huber_delta=value)) == (-1, f"{FN}: model 2: huber_delta is not a finite positive number")
    for value in (-1e-9, nan, inf):
        assert c.run(**c.model(0, min_lr=value)) == (-1, f"{FN}: model 0: min_lr is not a finite non-negative number")
        assert c.run(**c.model(1, weight_decay=value)) == (-1, f"{FN}: model 1: weight_decay is not a finite non-negative number")
    for value in (0.0, 1.0, -0.5, 1.5, nan, inf):
        assert c.run(**c.model(2, sched_factor=value)) == (-1, f"{FN}: model 2: sched_factor is not inside (0, 1)")
    assert c.run(**c.model(1, epochs=0)) == (-1, f"{FN}: model 1: epochs is 0")
    # the launch cap: n_rows x epochs
    too_many = (1 << 26) // 24 + 1
    assert c.run(**c.model(2, epochs=too_many)) == \
           (-1, f"{FN}: model 2: n_rows x epochs = {24 * too_many} is above 67108864 (OW_MLP_TRAIN_MAX_ROW_EPOCHS: a model is one serial wavefront)")
    # a model without a masked-in entry among its train rows / its validation rows
    sp = c.args["split"].copy()
    sp[1] &= 2
    assert c.run(split=sp) == (-1, f"{FN}: model 1: split / target_mask leave no masked-in entry among the train rows")
    sp = c.args["split"].copy()
    sp[2] &= 1
    assert c.run(split=sp) == (-1, f"{FN}: model 2: split / target_mask leave no masked-in entry among the validation rows")
    assert c.run(**c.model(0, target_mask=0)) == (-1, f"{FN}: model 0: split / target_mask leave no masked-in entry among the train rows")
    assert c.run(**c.model(0, target_mask=1 << 11)) == (-1, f"{FN}: model 0: split / target_mask leave no masked-in entry among the train rows")
    m = c.args["mask"].copy()
    val_rows = (c.args["split"][0] & 2) != 0
    m[val_rows, 1:] = 0
    assert c.run(mask=m, **c.model(1, target_mask=0x7FE)) == (-1, f"{FN}: model 1: split / target_mask leave no masked-in entry among the validation rows")
    # history_out given, history_epochs below a model's epochs
    hist = np.full((3, 4, 3), SENTINEL)
    assert c.run(history_out=hist, cfg=b.OwMlpTrainCfg(24, 4)) == (-1, f"{FN}: model 0: epochs 5 is above history_epochs 4")
    assert c.run(history_out=hist, cfg=b.OwMlpTrainCfg(24, 4), **c.model(0, epochs=4)) == (-1, f"{FN}: model 1: epochs 5 is above history_epochs 4")
    # nothing was written
    assert np.all(c.args["best_out"] == SENTINEL) and np.all(hist == SENTINEL)
    # no model: nothing to do, no device needed
    assert c.run(n_models=0) == (0, "")


def test_valid_call_reaches_the_device_check(hiplib):
    """Everything is validated before the device is asked for: without one, a valid call fails there and nowhere earlier; with one, the
    same call trains (the library itself says which: torch's view of the device is another runtime's)."""
    c = _Call(hiplib)
    buf = hiplib.ow_device_alloc(8, 0)
    hiplib.ow_clear_error()
    rc, msg = c.run()
    if buf:
        hiplib.ow_device_free(buf, 0)
        assert (rc, msg) == (0, "") and np.all(c.args["best_out"] != SENTINEL) and np.all(c.args["results"]["epochs_run"] == 5)
    else:
        assert rc == -1 and msg.startswith(f"{FN}: ") and "device" in msg and np.all(c.args["best_out"] == SENTINEL)


# ---- load_data -------------------------------------------------------------------------------------------------------------------------
def _raw(n, seed):
    """Unstandardised training data in the reference's layout, with outliers beyond every clip and a column with a single valid entry."""
    rng = np.random.RandomState(seed)
    inputs = rng.uniform(size=(n, 2))
    targets = rng.normal(0.0, 3.0, size=(n, 11))
    targets[:, 5:10] = np.exp(rng.normal(0.0, 1.5, size=(n, 5))) * rng.choice([-1.0, 1.0], size=(n, 5), p=[0.1, 0.9])
    targets[0, 5], targets[1, 6], targets[2, 9] = 55.0, -31.0, 20.5
    targets[:, 10] = rng.uniform(0.2, 2.6, size=n)
    mask = rng.uniform(size=(n, 11)) < 0.7
    mask[:, 3] = False
    mask[min(4, n - 1), 3] = True                      # one valid entry: mean 0, std 1
    mask[:, 4] = False                                 # none
    weights = rng.choice([1.0, 0.6, 0.3], size=n)
    return dict(inputs=inputs, targets=targets, mask=mask, weights=weights)


def _restated(d, no_split, mask_decay_h3):
    inputs, targets, mask, weights = d["inputs"].copy(), d["targets"].copy(), d["mask"].copy(), d["weights"].copy()
    if mask_decay_h3:
        mask[:, 6] = False
    targets[:, 5:10] = np.minimum(np.maximum(targets[:, 5:10], -20.0), 20.0)
    targets[:, 10] = np.minimum(np.maximum(targets[:, 10], 0.5), 2.0)
    means, stds = np.zeros(11), np.ones(11)
    for i in range(11):
        v = targets[mask[:, i], i]
        if v.size > 1:
            means[i] = v.sum() / v.size
            stds[i] = max(np.sqrt(((v - v.mean()) ** 2).sum() / v.size), 1e-6)
    n = len(inputs)
    split = np.zeros(n, dtype=np.uint8)
    if no_split or n < 20:
        split[:] = 3
    else:
        perm = np.random.RandomState(42).permutation(n)
        split[perm[:int(0.8 * n)]] = 1
        split[perm[int(0.8 * n):]] = 2
    return inputs, (targets - means) / stds, mask, weights, split, means, stds


@pytest.mark.parametrize("n,no_split,h3", [(50, False, False), (50, False, True), (50, True, False), (19, False, False), (20, False, True)])
def test_load_data_is_the_references(n, no_split, h3, tmp_path):
    from openwurli_amd import mlp_train as mt
    d = _raw(n, 3)
    keep = {k: v.copy() for k, v in d.items()}
    got = mt.load_data(d, no_split=no_split, mask_decay_h3=h3)
    for k in d:
        assert np.array_equal(d[k], keep[k]), k                     # the caller's arrays are not modified
    want = _restated(d, no_split, h3)
    assert np.array_equal(got.inputs, want[0]) and np.array_equal(got.mask, want[2]) and np.array_equal(got.weights, want[3])
    assert np.array_equal(got.split, want[4])
    assert np.allclose(got.target_means, want[5], rtol=1e-14, atol=0) and np.allclose(got.target_stds, want[6], rtol=1e-14, atol=0)
    assert np.allclose(got.targets, want[1], rtol=1e-12, atol=1e-14)
    for a in (got.inputs, got.targets, got.weights, got.target_means, got.target_stds):
        assert a.dtype == np.float64
    # the clips happened before the statistics: the clipped outliers are what is standardised
    assert got.targets[0, 5] * got.target_stds[5] + got.target_means[5] == pytest.approx(20.0) and got.targets[1, 6] * got.target_stds[6] + got.target_means[6] == pytest.approx(-20.0)
    raw_ds = got.targets[:, 10] * got.target_stds[10] + got.target_means[10]
    assert raw_ds.min() == pytest.approx(0.5) and raw_ds.max() == pytest.approx(2.0)
    # standardisation from masked-in entries only; one or no valid entry: mean 0, std 1
    for i in (0, 7, 10):
        v = got.targets[got.mask[:, i], i]
        assert abs(v.mean()) < 1e-12 and abs(v.std() - 1.0) < 1e-12
    assert (got.target_means[3], got.target_stds[3], got.target_means[4], got.target_stds[4]) == (0.0, 1.0, 0.0, 1.0)
    assert bool(got.mask[:, 6].any()) == (not h3)
    if no_split or n < 20:
        assert np.all(got.split == 3)
    else:
        assert ((got.split & 1) != 0).sum() == int(0.8 * n) and np.all((got.split == 1) | (got.split == 2))
        assert np.array_equal(np.nonzero(got.split == 2)[0], np.sort(np.random.RandomState(42).permutation(n)[int(0.8 * n):]))
    # the same through a file, and as a tuple
    path = tmp_path / "d.npz"
    np.savez(path, **d)
    again = mt.load_data(path, no_split=no_split, mask_decay_h3=h3)
    third = mt.load_data((d["inputs"], d["targets"], d["mask"], d["weights"]), no_split=no_split, mask_decay_h3=h3)
    for a, b_, c_ in zip(got, again, third):
        assert np.array_equal(a, b_) and np.array_equal(a, c_)


def test_std_floor():
    from openwurli_amd import mlp_train as mt
    d = _raw(30, 4)
    d["targets"][:, 2] = 1.25
    got = mt.load_data(d)
    assert got.target_stds[2] == 1e-6 and got.target_means[2] == 1.25


# ---- init_like_reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [42, 7])
def test_init_is_torchs_own(seed):
    import torch
    import torch.nn as nn
    from openwurli_amd import mlp_train as mt
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(2, 16), nn.ReLU(), nn.Linear(16, 16), nn.ReLU(), nn.Linear(16, 11))
    want = [p.detach().numpy().astype(np.float64) for p in net.parameters()]
    torch.manual_seed(1234)
    before = torch.random.get_rng_state().clone()
    got = mt.init_like_reference(seed, 16)
    assert torch.equal(torch.random.get_rng_state(), before)         # the caller's global state is untouched
    for a, b in zip((got.w1, got.b1, got.w2, got.b2, got.w3, got.b3), want):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert np.array_equal(got.flat()[:507], ref.flat507(ref.params_of(ref.make_net(seed))))
    assert np.all(got.target_means == 0.0) and np.all(got.target_stds == 1.0)
    assert mt.init_like_reference(seed) == got and mt.init_like_reference(seed + 1) != got


def test_init_hidden_8_is_zero_in_exactly_the_padding():
    from openwurli_amd import mlp_train as mt
    got = mt.init_like_reference(42, hidden=8)
    want = ref.pad16(ref.params_of(ref.make_net(42, 8)))
    for a, b in zip((got.w1, got.b1, got.w2, got.b2, got.w3, got.b3), want):
        assert np.array_equal(a, b)
    pad = np.ones((16, 16), dtype=bool)
    pad[:8, :8] = False
    assert np.array_equal(got.w2 == 0.0, pad) and np.array_equal(got.w1 == 0.0, np.repeat(np.arange(16) >= 8, 2).reshape(16, 2))
    assert np.array_equal(got.b1 == 0.0, np.arange(16) >= 8) and np.array_equal(got.b2 == 0.0, np.arange(16) >= 8)
    assert np.array_equal(got.w3 == 0.0, np.tile(np.arange(16) >= 8, (11, 1))) and np.all(got.b3 != 0.0)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="hidden"):
            mt.init_like_reference(42, hidden=bad)


def test_kfold_and_sweep():
    from openwurli_amd import mlp_train as mt
    f = mt.kfold_splits(70, 5, 3)
    assert f.shape == (5, 70) and f.dtype == np.uint8 and np.array_equal(f, ref.kfold(70, 5, 3))
    assert np.all((f == 2).sum(axis=0) == 1) and np.all((f == 2).sum(axis=1) == 14) and np.all((f == 1) | (f == 2))
    assert not np.array_equal(f, mt.kfold_splits(70, 5, 4))
    with pytest.raises(ValueError):
        mt.kfold_splits(3, 5, 0)
    x, t, m, w = ref.synthetic(30, 1)
    data = mt.Data(x, t, m, w, ref.split_80_20(30), np.zeros(11), np.ones(11))
    folds = mt.kfold_splits(30, 3, 0)
    models, inits, rows, labels = mt.sweep(data, [5, 6], lrs=(1e-3, 3e-3), weight_decays=(0.0, 1e-4), huber_deltas=(5.0,), splits=folds, epochs=77, mask_decay_h3=True)
    assert len(models) == len(inits) == len(labels) == 2 * 2 * 2 * 1 * 3 and rows.shape == (24, 30)
    assert [(l["seed"], l["lr"], l["weight_decay"], l["split"]) for l in labels[:7]] == \
           [(5, 1e-3, 0.0, 0), (5, 1e-3, 0.0, 1), (5, 1e-3, 0.0, 2), (5, 1e-3, 1e-4, 0), (5, 1e-3, 1e-4, 1), (5, 1e-3, 1e-4, 2), (5, 3e-3, 0.0, 0)]
    assert labels[12]["seed"] == 6 and inits[0] == mt.init_like_reference(5) and inits[12] == mt.init_like_reference(6)
    assert np.array_equal(rows[4], folds[1]) and models[6]["lr"] == 3e-3 and models[3]["weight_decay"] == 1e-4
    assert all(mo["epochs"] == 77 and mo["target_mask"] == 0x7FF & ~(1 << 6) and mo["patience"] == 150 and mo["min_lr"] == 1e-5 for mo in models)
    one = mt.sweep(data, [1])
    assert len(one[0]) == 1 and np.array_equal(one[2][0], data.split) and one[0][0] == mt.DEFAULTS == ref.DEFAULTS
    with pytest.raises(ValueError, match="unknown"):
        mt.model(learning_rate=1.0)


# ---- the precondition of the GPU tests' whole runs -------------------------------------------------------------------------------------
def _same_under_reversal(a, b):
    assert (a["best_epoch"], a["epochs_run"], a["lr_reductions"], a["last_lr"]) == (b["best_epoch"], b["epochs_run"], b["lr_reductions"], b["last_lr"])
    assert abs(a["best_val_loss"] - b["best_val_loss"]) <= 1e-12 * a["best_val_loss"]


@pytest.mark.parametrize("seed", ref.WHOLE_SEEDS)
@pytest.mark.parametrize("case", sorted(ref.WHOLE_RUNS))
def test_whole_runs_do_not_move_with_the_row_order(case, seed):
    """torch's own loop on the rows as given and reversed: the same best_epoch, epochs_run and lr reductions, the best validation loss to
    1e-12 relative -- otherwise the data set is no yardstick for another summation order, and another data seed is chosen."""
    a = ref.whole_run(case, seed)
    _same_under_reversal(a, ref.whole_run(case, seed, reverse=True))
    assert a["epochs_run"] < 2000 and a["lr_reductions"] >= 1           # what the GPU test wants of the case: early stopping, a reduction


def test_hidden_8_run_does_not_move_with_the_row_order():
    _same_under_reversal(ref.whole_run("A", 42, hidden=8), ref.whole_run("A", 42, reverse=True, hidden=8))


@pytest.mark.parametrize("i", ref.MANY_TORCH)
def test_compared_models_of_many_do_not_move_with_the_row_order(i):
    x, t, m, w, _ = ref.dataset(ref.MANY_CASE)
    seed, hp, sp = ref.many_models()[i]
    _same_under_reversal(ref.train(ref.make_net(seed), x, t, m, w, sp, **hp), ref.train(ref.make_net(seed), x, t, m, w, sp, reverse=True, **hp))


def test_synthetic_data_is_what_it_says():
    x, t, m, w = ref.synthetic(4000, 9)
    assert x.shape == (4000, 2) and t.shape == m.shape == (4000, 11) and w.shape == (4000,)
    notes = x[:, 0] * 87.0 + 21.0
    assert np.allclose(notes, np.round(notes)) and notes.min() >= 33 - 1e-9 and notes.max() <= 96 + 1e-9 and 0.0 <= x[:, 1].min() and x[:, 1].max() <= 1.0
    assert 0.68 < m.mean() < 0.72 and set(np.unique(w)) == {1.0, 0.6, 0.3}
    assert 0.01 < (np.abs(t) > 5.0).mean() < 0.03                       # the entries times 15: beyond the default Huber delta
    a = ref.synthetic(70, 1)
    assert all(np.array_equal(p, q) for p, q in zip(a, ref.synthetic(70, 1)))


# ---- the tool's text -------------------------------------------------------------------------------------------------------------------
class _Canned:
    def __init__(self, history, last_lr, best_val_loss, best_epoch, weights=None, status=0, lr_reductions=0):
        self.history, self.last_lr, self.best_val_loss, self.best_epoch = np.asarray(history, dtype=np.float64), last_lr, best_val_loss, best_epoch
        self.epochs_run, self.weights, self.status, self.lr_reductions = len(history), weights, status, lr_reductions


def test_report_text_from_canned_results():
    """train_mlp.py:179-186: `Epoch` lines at epoch 1 and every 100th with the lr after the epoch's scheduler step, the early-stopping
    line; evaluate()'s table."""
    from openwurli_amd import mlp_train as mt
    hist = [(1.0 / (e + 1), 2.0 / (e + 1) if e < 120 else 0.5, 3e-3 if e < 199 else 1.5e-3) for e in range(270)]
    r = _Canned(hist, 1.5e-3, 2.0 / 120, 119)
    assert mt.format_epoch_lines(r, 150) == [
        "  Epoch     1: train=1.0000  val=2.0000  best=2.0000  lr=3.0e-03  stale=0",
        "  Epoch   100: train=0.0100  val=0.0200  best=0.0200  lr=3.0e-03  stale=0",
        "  Epoch   200: train=0.0050  val=0.5000  best=0.0167  lr=1.5e-03  stale=80",
        "  Early stopping at epoch 270 (patience=150)"]
    assert mt.format_epoch_lines(_Canned(hist[:100], 3e-3, 0.02, 99), 150)[-1].startswith("  Epoch   100:")      # ran out of epochs: no stopping line
    assert mt.format_evaluation([("freq_H2", 14, 1.23456, 2.5, "cents"), ("ds_corr", 3, 0.004, 0.0051, "")]) == [
        "", "  Per-target validation error (original units):", "        Target N_val      MAE     RMSE Unit", "  " + "-" * 45,
        "       freq_H2    14     1.23     2.50  cents", "       ds_corr     3     0.00     0.01  "]
    # evaluate: in original units, over the validation rows' valid entries only
    x, t, m, w = ref.synthetic(40, 2)
    init = mt.init_like_reference(3)
    init.target_means[:] = np.arange(11.0)
    init.target_stds[:] = 2.0
    data = mt.Data(x, t, m, w, ref.split_80_20(40), init.target_means, init.target_stds)
    rows = mt.evaluate(init, data)
    val = data.split == 2
    pred = ref.forward_numpy(init.flat(), x[val]) * 2.0 + np.arange(11.0)
    act = t[val] * 2.0 + np.arange(11.0)
    assert [r_[0] for r_ in rows] == [mt.TARGET_NAMES[i] for i in range(11) if m[val, i].any()]
    name, n_val, mae, rmse, unit = rows[0]
    e = (pred[:, 0] - act[:, 0])[m[val, 0]]
    assert (name, n_val, unit) == ("freq_H2", int(m[val, 0].sum()), "cents") and mae == pytest.approx(np.abs(e).mean()) and rmse == pytest.approx(np.sqrt((e ** 2).mean()))
    assert mt.TARGET_NAMES == ("freq_H2", "freq_H3", "freq_H4", "freq_H5", "freq_H6", "decay_H2", "decay_H3", "decay_H4", "decay_H5", "decay_H6", "ds_corr")


def test_sweep_csv_and_export_naming(tmp_path):
    from openwurli_amd import mlp_train as mt
    from openwurli_amd.mlp import MlpWeights
    sets = [mt.init_like_reference(s) for s in (1, 2, 3)]
    res = [_Canned([(1, 1, 1)] * 5, 3e-3, 0.25, 4, sets[0]), _Canned([(1, 1, 1)] * 9, 1.5e-3, 0.125, 2, sets[1], lr_reductions=1),
           _Canned([(1, 1, 1)] * 2, 3e-3, 0.125, 1, sets[2], status=0)]
    labels = [dict(seed=1, lr=3e-3, weight_decay=1e-4, huber_delta=5.0, split=0), dict(seed=2, lr=1e-3, weight_decay=0.0, huber_delta=0.5, split=1),
              dict(seed=3, lr=3e-3, weight_decay=1e-4, huber_delta=5.0, split=0)]
    assert mt.format_sweep_csv(labels, res) == mt.SWEEP_HEADER + "\n0,1,0.003,0.0001,5,0,0.25,4,5,0.003,0,0\n1,2,0.001,0,0.5,1,0.125,2,9,0.0015,1,0\n2,3,0.003,0.0001,5,0,0.125,1,2,0.003,0,0\n"
    assert mt.SWEEP_HEADER == "model,seed,lr,weight_decay,huber_delta,split,best_val_loss,best_epoch,epochs_run,last_lr,lr_reductions,status"
    paths = mt.export_top(res, 2, str(tmp_path / "sets"))
    assert [os.path.basename(p) for p in paths] == ["rank01_model0001.json", "rank02_model0002.json"]            # ties: the lower index first
    assert sorted(os.listdir(tmp_path / "sets")) == ["rank01_model0001.json", "rank02_model0002.json"]
    back = MlpWeights.from_json(paths[0])                                                                       # what tools/mlp_eval.py --weights reads
    assert back == sets[1] and json.load(open(paths[0]))["hidden_size"] == 16
    assert mt.export_top(res, 0, str(tmp_path / "none")) == []


def test_tool_flags(monkeypatch, tmp_path):
    """tools/train_mlp.py: the reference's flags and defaults (--hidden 16), its report around a canned training, the export; `sweep`."""
    from openwurli_amd import mlp_train as mt
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_mlp as tool
    d = _raw(40, 8)
    path = tmp_path / "training_data.npz"
    np.savez(path, **d)
    seen = {}

    def fake_train(data, inits, models, splits=None, device=0, history=False, kernel_ms=None):
        seen["call"] = (data, list(inits), [dict(m) for m in models], splits, device, history)
        return [_Canned([(0.5, 0.25, m["lr"])] * 3, m["lr"], 0.25 - 0.01 * i, 0, w) for i, (m, w) in enumerate(zip(models, inits))]
    monkeypatch.setattr(mt, "train", fake_train)
    out = tmp_path / "out" / "model_weights.json"
    buf = io.StringIO()
    with redirect_stdout(buf):
        tool.main(["--data", str(path), "--export", str(out), "--mask-decay-h3"])
    data, inits, models, splits, device, history = seen["call"]
    assert models == [mt.model(lr=3e-3, weight_decay=1e-4, huber_delta=5.0, epochs=2000, patience=150)] and history and device == 0 and splits is None
    assert inits == [mt.init_like_reference(42, 16)] and not data.mask[:, 6].any()
    text = buf.getvalue().splitlines()
    assert text[0] == f"Loading data from {path}..." and text[1] == f"  Masked decay_H3 (index 6): {int(d['mask'][:, 6].sum())} entries zeroed"
    assert text[2:5] == ["  Train: 32, Val: 8", f"  Train mask coverage: {data.mask[data.split == 1].mean():.1%}", f"  Val mask coverage: {data.mask[data.split == 2].mean():.1%}"]
    assert text[5:9] == ["", "Model: 507 parameters (hidden=16)", "Training: epochs=2000, lr=0.003, patience=150, huber_delta=5.0, wd=0.0001", ""]
    assert text[9] == "  Epoch     1: train=0.5000  val=0.2500  best=0.2500  lr=3.0e-03  stale=0" and "  Best validation loss: 0.2500" in text
    assert "  Per-target validation error (original units):" in text and text[-2:] == [f"  Exported weights to {out}", "  Total parameters: 507"]
    assert json.load(open(out))["hidden_size"] == 16
    with redirect_stdout(io.StringIO()) as quiet:
        tool.main(["--data", str(path), "--export", str(out), "--hidden", "8", "--seed", "7", "--lr", "1e-3", "--epochs", "50", "--patience", "5", "--huber-delta", "0.5",
                   "--weight-decay", "0", "--no-split", "--device", "2"])
    data, inits, models, splits, device, history = seen["call"]
    assert models == [mt.model(lr=1e-3, weight_decay=0.0, huber_delta=0.5, epochs=50, patience=5)] and device == 2 and np.all(data.split == 3)
    assert inits == [mt.init_like_reference(7, 8)] and "Model: 195 parameters (hidden=8)" in quiet.getvalue() and "training on all data (no split)" in quiet.getvalue()
    assert json.load(open(out))["hidden_size"] == 16                                                            # the set is the 16-unit shape, zero-padded
    csv_path, top = tmp_path / "s" / "sweep.csv", tmp_path / "top"
    with redirect_stdout(io.StringIO()) as line:
        tool.main(["sweep", "--data", str(path), "--seeds", "0-2", "--lrs", "1e-3,3e-3", "--weight-decays", "0,1e-4", "--huber-deltas", "5.0", "--folds", "4",
                   "--csv", str(csv_path), "--export-dir", str(top), "--top", "3", "--epochs", "60"])
    data, inits, models, splits, device, history = seen["call"]
    assert len(models) == 3 * 2 * 2 * 1 * 4 == len(inits) and splits.shape == (48, 40) and np.array_equal(splits[:4], mt.kfold_splits(40, 4, 42))
    rows = open(csv_path).read().splitlines()
    assert rows[0] == mt.SWEEP_HEADER and len(rows) == 49 and rows[1].startswith("0,0,0.001,0,5,0,") and rows[48].startswith("47,2,0.003,0.0001,5,3,")
    assert sorted(os.listdir(top)) == ["rank01_model0047.json", "rank02_model0046.json", "rank03_model0045.json"]
    summary = json.loads(line.getvalue().splitlines()[-1])
    assert summary["models"] == 48 and summary["best_model"] == 47 and len(summary["exported"]) == 3
