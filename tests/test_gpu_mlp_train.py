"""ow_mlp_train / k_mlp_train on the device against torch itself (tests/mlp_train_ref.py: nn.Sequential.double(), torch.optim.Adam,
ReduceLROnPlateau, autograd, on the CPU).

The bounds are conditions against torch set from the deviation a float64 restatement with another summation order shows against it
(measured on the CPU): <= 2e-16 after one epoch, <= 2e-15 at 50 epochs, <= 1.1e-10 for the best state of whole runs of 330-470 epochs,
with equal best_epoch / epochs_run / learning rates.  The data sets of the whole runs are those for which torch's own result does not
move with the order of the rows (tests/test_mlp_train_host.py checks that on the CPU).
"""
import numpy as np
import pytest

import mlp_train_ref as ref

pytestmark = pytest.mark.gpu

W_BOUND, LOSS_REL = 1e-8, 1e-9          # whole runs: every weight, the best validation loss


@pytest.fixture(scope="module")
def mt(hiplib):
    """The module, with the library's device opened before torch runs anything: torch's autograd engine asks its own HIP runtime for
    the device count at the first backward(), and of two runtimes in one process only the one that opened the device first sees it.
    (In the whole suite the library has rendered long before; this keeps the module runnable on its own.)"""
    from openwurli_amd import binding, mlp_train
    buf = hiplib.ow_device_alloc(8, 0)
    if not buf:
        raise binding.OwError(binding.take_error(hiplib))
    hiplib.ow_device_free(buf, 0)
    return mlp_train


def _data(mt, x, t, m, w, s):
    return mt.Data(x, t, m, w, s, np.zeros(11), np.ones(11))


def _flat(result):
    return result.weights.flat()[:507]


def _show(*a):
    print(*a, flush=True)


@pytest.mark.parametrize("n", [5, 16, 64, 65, 70])
def test_one_epoch(mt, n):
    """One step from init_like_reference(42): every parameter within 1e-13 of torch, the losses to 1e-12 relative.  n = 5 has a one-row
    validation part; 16 and 64 end on tile edges, 65 and 70 spill into a second tile of the train rows."""
    x, t, m, w = ref.synthetic(n, 10 + n)
    s = ref.split_80_20(n) if n >= 20 else _small_split(n)
    want = ref.train(ref.make_net(42), x, t, m, w, s, epochs=1)
    got = mt.train(_data(mt, x, t, m, w, s), [mt.init_like_reference(42)], [mt.model(epochs=1)], history=True)[0]
    dev = np.abs(_flat(got) - ref.flat507(want["last"])).max()
    _show("one epoch", n, "max weight deviation", dev, "losses", got.history[0], want["history"][0])
    assert (got.epochs_run, got.best_epoch, got.status) == (1, 0, 0)
    assert dev <= 1e-13
    assert abs(got.history[0, 0] - want["history"][0, 0]) <= 1e-12 * abs(want["history"][0, 0])
    assert abs(got.history[0, 1] - want["history"][0, 1]) <= 1e-12 * abs(want["history"][0, 1])
    assert got.history[0, 2] == want["history"][0, 2] == 3e-3
    assert abs(got.best_val_loss - want["best_val_loss"]) <= 1e-12 * want["best_val_loss"] and got.last_val_loss == got.best_val_loss
    assert got.last_train_loss == got.history[0, 0]


def _small_split(n):
    """80 / 20 of fewer than 20 rows (load_data would not split them): the permutation's first 80 % train, the rest validate."""
    perm = np.random.RandomState(42).permutation(n)
    s = np.zeros(n, dtype=np.uint8)
    s[perm[:int(0.8 * n)]] |= 1
    s[perm[int(0.8 * n):]] |= 2
    return s


@pytest.mark.parametrize("seed", [42, 7])
def test_fifty_epochs(mt, seed):
    x, t, m, w, s = ref.dataset("A")
    want = ref.train(ref.make_net(seed), x, t, m, w, s, epochs=50, patience=50)
    got = mt.train(_data(mt, x, t, m, w, s), [mt.init_like_reference(seed)], [mt.model(epochs=50, patience=50)], history=True)[0]
    dev = np.abs(_flat(got) - ref.flat507(want["best"])).max()
    rel = np.abs(got.history[:, :2] - want["history"][:, :2]) / np.abs(want["history"][:, :2])
    _show("fifty epochs", seed, "max weight deviation", dev, "max relative loss deviation", rel.max())
    assert got.epochs_run == want["epochs_run"] == 50 and got.best_epoch == want["best_epoch"]
    assert got.history.shape == (50, 3)
    assert dev <= 1e-10
    assert rel.max() <= 1e-10
    assert np.array_equal(got.history[:, 2], want["history"][:, 2])


@pytest.fixture(scope="module")
def whole(mt):
    """Every whole run of the module in ONE call: (case, seed) as the cases say, and the same with patience = epochs."""
    out = {}
    for case, c in ref.WHOLE_RUNS.items():
        x, t, m, w, s = ref.dataset(case)
        models, inits, keys = [], [], []
        for seed in ref.WHOLE_SEEDS:
            for patience in (c["patience"], 2000):
                models.append(mt.model(patience=patience, sched_patience=c["sched_patience"]))
                inits.append(mt.init_like_reference(seed))
                keys.append((case, seed, patience == 2000))
        for key, r in zip(keys, mt.train(_data(mt, x, t, m, w, s), inits, models, history=True)):
            out[key] = r
    return out


def _against_torch(got, want, label):
    dev = np.abs(_flat(got) - ref.flat507(want["best"])).max()
    rel = abs(got.best_val_loss - want["best_val_loss"]) / want["best_val_loss"]
    _show(label, "torch: best_epoch", want["best_epoch"], "epochs_run", want["epochs_run"], "lr reductions", want["lr_reductions"],
          "| max weight deviation", dev, "best validation loss deviation (relative)", rel)
    assert (got.best_epoch, got.epochs_run, got.lr_reductions) == (want["best_epoch"], want["epochs_run"], want["lr_reductions"])
    assert got.last_lr == want["last_lr"]
    assert rel <= LOSS_REL
    assert dev <= W_BOUND
    return dev


@pytest.mark.parametrize("seed", ref.WHOLE_SEEDS)
@pytest.mark.parametrize("case", sorted(ref.WHOLE_RUNS))
def test_whole_run(mt, whole, case, seed):
    """Early stopping, a learning-rate reduction and the best-state restore, against torch."""
    want = ref.whole_run(case, seed)
    got = whole[(case, seed, False)]
    assert want["epochs_run"] < 2000 and want["lr_reductions"] >= 1 and want["best_epoch"] == want["epochs_run"] - 1 - ref.WHOLE_RUNS[case]["patience"]
    _against_torch(got, want, f"whole run {case} seed {seed}")
    assert got.status == 0 and got.history.shape == (want["epochs_run"], 3)
    # the best state, not the last: the run that never stops early walks the same path (its history starts with this one's), its
    # snapshot at this run's end would be the same -- and it differs from it exactly when a later epoch was better still
    on = whole[(case, seed, True)]
    assert on.epochs_run == 2000
    assert np.array_equal(on.history[:got.epochs_run], got.history)
    later_better = on.history[got.epochs_run:, 1].min() < got.best_val_loss
    assert (on.best_epoch != got.best_epoch) == later_better
    assert np.array_equal(_flat(on), _flat(got)) == (not later_better)
    assert np.abs(_flat(got) - ref.flat507(want["last"])).max() > 1e-6                  # forty epochs on, the weights had moved


@pytest.fixture(scope="module")
def many(mt):
    x, t, m, w, _ = ref.dataset(ref.MANY_CASE)
    spec = ref.many_models()
    data = _data(mt, x, t, m, w, spec[0][2])
    models = [mt.model(**hp) for _, hp, _ in spec]
    inits = [mt.init_like_reference(seed) for seed, _, _ in spec]
    splits = np.stack([sp for _, _, sp in spec])
    return data, spec, models, inits, splits, mt.train(data, inits, models, splits=splits, history=True)


def test_many_unequal_models_are_independent(mt, many):
    """70 models of unequal lifetimes in one call: each bit-identical to the same model trained alone in its own call."""
    data, spec, models, inits, splits, together = many
    assert len(models) == 70
    runs = sorted(r.epochs_run for r in together)
    assert runs[0] == 1 and runs[-1] >= 400 and len(set(runs)) > 10
    assert np.array_equal(splits[6:11], mt.kfold_splits(70, 5, 3)) and np.array_equal(splits[6:11], ref.kfold(70, 5, 3))
    for i in range(len(models)):
        alone = mt.train(data, [inits[i]], [models[i]], splits=splits[i:i + 1], history=True)[0]
        r = together[i]
        assert alone.weights.flat().tobytes() == r.weights.flat().tobytes(), i
        assert alone.history.tobytes() == r.history.tobytes(), i
        assert (alone.best_val_loss, alone.last_train_loss, alone.last_val_loss, alone.last_lr, alone.best_epoch, alone.epochs_run, alone.lr_reductions, alone.status) == \
               (r.best_val_loss, r.last_train_loss, r.last_val_loss, r.last_lr, r.best_epoch, r.epochs_run, r.lr_reductions, r.status), i


@pytest.mark.parametrize("i", ref.MANY_TORCH)
def test_many_models_against_torch(mt, many, i):
    """Huber delta 0.5, a masked target, a fold, no weight decay, no split: within the whole runs' bounds of torch."""
    data, spec, models, inits, splits, together = many
    seed, hp, sp = spec[i]
    want = ref.train(ref.make_net(seed), data.inputs, data.targets, data.mask, data.weights, sp, **hp)
    _against_torch(together[i], want, f"model {i} of many {hp}")
    if i == 1:                       # the linear branch dominates: most residuals of the first epoch lie beyond delta
        d = np.abs(ref.forward_numpy(inits[i].flat(), data.inputs) - data.targets)[np.asarray(data.mask)]
        assert (d >= 0.5).mean() > 0.5


def test_hidden_8_zero_padded(mt):
    """A network of 8 hidden units is the 16-unit set with zero padding: the padding stays exactly 0.0 through a whole run, the rest is
    torch's 8-unit network."""
    c = ref.WHOLE_RUNS["A"]
    x, t, m, w, s = ref.dataset("A")
    init = mt.init_like_reference(42, hidden=8)
    got = mt.train(_data(mt, x, t, m, w, s), [init], [mt.model(patience=c["patience"], sched_patience=c["sched_patience"])])[0]
    want = ref.whole_run("A", 42, hidden=8)
    _against_torch(got, want, "hidden 8")
    g = got.weights
    for pad in (g.w1[8:], g.b1[8:], g.w2[8:, :], g.w2[:, 8:], g.b2[8:], g.w3[:, 8:]):
        assert pad.size and np.all(pad == 0.0)
    assert np.all(g.w1[:8] != 0.0) and np.all(g.w3[:, :8] != 0.0)


def test_same_call_twice_same_bytes(mt, many):
    data, spec, models, inits, splits, first = many
    again = mt.train(data, inits[:24], models[:24], splits=splits[:24], history=True)
    for a, b in zip(first, again):
        assert a.weights.flat().tobytes() == b.weights.flat().tobytes() and a.history.tobytes() == b.history.tobytes()
        assert (a.best_val_loss, a.last_train_loss, a.last_val_loss, a.last_lr, a.best_epoch, a.epochs_run, a.lr_reductions) == \
               (b.best_val_loss, b.last_train_loss, b.last_val_loss, b.last_lr, b.best_epoch, b.epochs_run, b.lr_reductions)
    again_all = mt.train(data, inits, models, splits=splits, history=True)
    assert all(a.weights.flat().tobytes() == b.weights.flat().tobytes() and a.history.tobytes() == b.history.tobytes() for a, b in zip(first, again_all))


def test_trained_set_closes_the_loop(mt, whole):
    """A trained set carries the data's normalisation and is what ow_mlp_infer and the batch render take."""
    from openwurli_amd import mlp
    x, t, m, w, s = ref.dataset("A")
    means, stds = np.linspace(-2.0, 3.0, 11), np.linspace(0.5, 4.0, 11)
    c = ref.WHOLE_RUNS["A"]
    got = mt.train(mt.Data(x, t, m, w, s, means, stds), [mt.init_like_reference(42)], [mt.model(patience=c["patience"], sched_patience=c["sched_patience"])])[0]
    assert np.array_equal(got.weights.target_means, means) and np.array_equal(got.weights.target_stds, stds)
    assert np.array_equal(_flat(got), _flat(whole[("A", 42, False)]))                   # the normalisation is not a parameter
    notes = np.arange(33, 97, dtype=np.uint8)
    vels = np.linspace(0.05, 1.0, notes.size)
    _, raw = mlp.infer([got.weights], notes, vels, raw=True)
    inputs = np.stack([(notes - 21.0) / 87.0, vels], axis=1)
    want = ref.forward_numpy(got.weights.flat(), inputs) * stds + means
    dev = np.abs(raw[0] - want).max()
    _show("infer on a trained set: max deviation from the numpy forward pass", dev)
    assert dev <= 1e-12
    audio = mlp.batch_render_mlp([dict(note=72, velocity=100)], [got.weights], [0], duration_s=0.02)
    assert audio.shape == (1, 882) and np.all(np.isfinite(audio)) and np.abs(audio).max() > 0.0


def test_history_is_optional_and_may_be_longer(mt, hiplib):
    """history_out == NULL works; history_epochs above a model's epochs works, the rows from epochs_run on stay zero."""
    import ctypes as C
    from openwurli_amd import binding
    x, t, m, w, s = ref.dataset("A")
    data = _data(mt, x, t, m, w, s)
    models = [mt.model(epochs=12, patience=3, lr=0.05), mt.model(epochs=30, patience=30)]
    inits = [mt.init_like_reference(1), mt.init_like_reference(2)]
    plain = mt.train(data, inits, models)
    assert all(r.history is None for r in plain)
    with_h = mt.train(data, inits, models, history=True)                                # history_epochs = 30 > the first model's 12
    for a, b in zip(plain, with_h):
        assert a.weights.flat().tobytes() == b.weights.flat().tobytes() and (a.epochs_run, a.best_epoch) == (b.epochs_run, b.best_epoch)
    assert with_h[0].epochs_run <= 12 and with_h[1].epochs_run == 30
    # the raw table: 40 epochs wide, zero from each model's epochs_run on
    marr = mt._model_array(models)
    init = np.ascontiguousarray(np.stack([i.flat() for i in inits]))
    best, res = np.zeros_like(init), np.zeros(2, dtype=np.dtype(binding.MLP_TRAIN_RESULT_DTYPE))
    hist = np.full((2, 40, 3), -7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mask8 = np.ascontiguousarray(m, dtype=np.uint8)
    sp = np.ascontiguousarray(np.stack([s, s]))
    cfg = binding.OwMlpTrainCfg(70, 40)
    assert hiplib.ow_mlp_train(p(x), p(t), p(mask8), p(w), p(sp), p(init), p(marr), 2, C.byref(cfg), p(best), p(res), p(hist)) == 0
    for k, r in enumerate(with_h):
        assert np.array_equal(hist[k, :r.epochs_run], r.history) and np.all(hist[k, r.epochs_run:] == 0.0)
        assert np.all(hist[k, :r.epochs_run, 2] > 0.0)
