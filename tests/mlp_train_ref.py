"""The yardstick of the MLP training tests: ml/train_mlp.py's train() written with torch itself, in float64 on the CPU --
nn.Sequential(...).double(), torch.optim.Adam, torch.optim.lr_scheduler.ReduceLROnPlateau and autograd.  Independent of the code under test:
it imports neither the package's mlp_train nor anything else of it.  Also the synthetic data the tests (and tools/bench_mlp_train.py) use.
"""
import numpy as np

N_OUT = 11
DEFAULTS = dict(lr=3e-3, min_lr=1e-5, weight_decay=1e-4, huber_delta=5.0, sched_factor=0.5, epochs=2000, patience=150, sched_patience=30,
                target_mask=0x7FF)


def synthetic(n, seed):
    """(inputs [n, 2], targets [n, 11] standardised-like, mask [n, 11] bool, weights [n]): (note - 21) / 87 for notes 33..96 plus a uniform
    velocity; eleven smooth functions of the inputs plus N(0, 0.3) noise, about 2 % of the entries times 15 (the Huber linear branch is
    live), about 70 % of the mask set, tier weights from {1.0, 0.6, 0.3}."""
    rng = np.random.RandomState(seed)
    note = rng.randint(33, 97, size=n)
    x0 = (note - 21.0) / 87.0
    x1 = rng.uniform(0.0, 1.0, size=n)
    inputs = np.stack([x0, x1], axis=1)
    k = np.arange(N_OUT)
    targets = (np.sin((1.0 + 0.37 * k)[None, :] * x0[:, None] * 3.0 + 0.5 * k[None, :]) * (0.6 + 0.8 * x1[:, None])
               + (x1[:, None] - 0.5) * np.cos(0.9 * k)[None, :] + 0.5 * (x0[:, None] ** 2) * ((k % 3) - 1.0)[None, :])
    targets = targets + rng.normal(0.0, 0.3, size=targets.shape)
    targets = np.where(rng.uniform(size=targets.shape) < 0.02, targets * 15.0, targets)
    mask = rng.uniform(size=targets.shape) < 0.7
    weights = rng.choice(np.array([1.0, 0.6, 0.3]), size=n)
    return np.ascontiguousarray(inputs), np.ascontiguousarray(targets), mask, weights


def split_80_20(n):
    """train_mlp.py's split as a row of the split table: bit 0 = train, bit 1 = validation."""
    perm = np.random.RandomState(42).permutation(n)
    cut = int(0.8 * n)
    s = np.zeros(n, dtype=np.uint8)
    s[perm[:cut]] |= 1
    s[perm[cut:]] |= 2
    return s


def make_net(seed, hidden=16):
    """The reference's network with torch's own initial values under torch.manual_seed(seed), float64 (the draw is float32: exact in f64)."""
    import torch
    import torch.nn as nn
    with torch.random.fork_rng(devices=[]):           # the CPU generator alone: no device is asked for its state
        torch.manual_seed(seed)
        net = nn.Sequential(nn.Linear(2, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, N_OUT))
    return net.double()


def params_of(net):
    """(w1, b1, w2, b2, w3, b3) as float64 arrays."""
    return [p.detach().numpy().copy() for p in net.parameters()]


def masked_huber(pred, target, mask, weights, delta):
    import torch
    diff = pred - target
    a = diff.abs()
    loss = torch.where(a < delta, 0.5 * diff ** 2, delta * (a - 0.5 * delta))
    loss = loss * mask.double()
    loss = loss * weights.unsqueeze(1)
    return loss.sum() / mask.double().sum()


def train(net, inputs, targets, mask, weights, split, lr=3e-3, min_lr=1e-5, weight_decay=1e-4, huber_delta=5.0, sched_factor=0.5, epochs=2000,
          patience=150, sched_patience=30, target_mask=0x7FF, reverse=False):
    """train_mlp.py:140-190 in float64.  split: bit 0 = train row, bit 1 = validation row; target_mask bit i = target i is trained on.
    reverse: the rows of both parts in reversed order (the same sums in another order).  Returns a dictionary: best (the six arrays of the best
    state), best_val_loss, best_epoch, epochs_run, last_lr, lr_reductions, history [epochs_run, 3] (train loss, validation loss, the lr in
    force during the step)."""
    import torch
    split = np.asarray(split)
    m = np.asarray(mask, dtype=bool) & np.array([(target_mask >> i) & 1 for i in range(N_OUT)], dtype=bool)[None, :]

    def part(bit):
        idx = np.nonzero(split & bit)[0]
        if reverse:
            idx = idx[::-1].copy()
        return (torch.tensor(np.asarray(inputs)[idx], dtype=torch.float64), torch.tensor(np.asarray(targets)[idx], dtype=torch.float64),
                torch.tensor(m[idx]), torch.tensor(np.asarray(weights)[idx], dtype=torch.float64))
    tr, va = part(1), part(2)
    opt = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=sched_factor, patience=sched_patience, min_lr=min_lr)
    best_val, best_state, best_epoch, stale, reductions, history = float("inf"), None, 0, 0, 0, []
    epochs_run = 0
    for epoch in range(epochs):
        lr_now = opt.param_groups[0]["lr"]
        net.train()
        opt.zero_grad()
        loss = masked_huber(net(tr[0]), tr[1], tr[2], tr[3], huber_delta)
        loss.backward()
        opt.step()
        net.eval()
        with torch.no_grad():
            val = masked_huber(net(va[0]), va[1], va[2], va[3], huber_delta)
        sched.step(val)
        if opt.param_groups[0]["lr"] != lr_now:
            reductions += 1
        history.append((loss.item(), val.item(), lr_now))
        epochs_run = epoch + 1
        if val.item() < best_val:
            best_val, best_epoch, stale = val.item(), epoch, 0
            best_state = params_of(net)
        else:
            stale += 1
        if stale >= patience:
            break
    return dict(best=best_state, best_val_loss=best_val, best_epoch=best_epoch, epochs_run=epochs_run, last_lr=opt.param_groups[0]["lr"],
                lr_reductions=reductions, history=np.array(history, dtype=np.float64).reshape(-1, 3), last=params_of(net))


def pad16(params):
    """The six arrays of a hidden-H network zero-padded to the 16-unit shapes of a weight set."""
    w1, b1, w2, b2, w3, b3 = params
    h = b1.shape[0]
    o = [np.zeros((16, 2)), np.zeros(16), np.zeros((16, 16)), np.zeros(16), np.zeros((N_OUT, 16)), np.zeros(N_OUT)]
    o[0][:h] = w1; o[1][:h] = b1; o[2][:h, :h] = w2; o[3][:h] = b2; o[4][:, :h] = w3; o[5][:] = b3
    return o


def flat507(params):
    return np.concatenate([a.ravel() for a in pad16(params)])


def forward_numpy(flat, inputs):
    """The network of a 529-double weight set (or its first 507) at inputs [n, 2]: standardised outputs [n, 11]."""
    flat = np.asarray(flat, dtype=np.float64)
    w1, b1, w2, b2 = flat[0:32].reshape(16, 2), flat[32:48], flat[48:304].reshape(16, 16), flat[304:320]
    w3, b3 = flat[320:496].reshape(11, 16), flat[496:507]
    h = np.maximum(np.asarray(inputs) @ w1.T + b1, 0.0)
    h = np.maximum(h @ w2.T + b2, 0.0)
    return h @ w3.T + b3


# ---- the cases the GPU tests run whole, shared with the host test that checks their precondition on the CPU -----------------------------
# A data set qualifies when torch's own result does not move with the order of the rows (tests/test_mlp_train_host.py): the data seeds
# below were chosen for that -- seed 2 at 70 rows, for one, moves torch's best validation loss by 4e-10 under a reversal and is not used.
WHOLE_RUNS = {"A": dict(n=70, data_seed=1, patience=40, sched_patience=30), "B": dict(n=150, data_seed=2, patience=60, sched_patience=30)}
WHOLE_SEEDS = (42, 7)
_CACHE = {}


def dataset(case):
    c = WHOLE_RUNS[case]
    key = ("data", case)
    if key not in _CACHE:
        _CACHE[key] = synthetic(c["n"], c["data_seed"]) + (split_80_20(c["n"]),)
    return _CACHE[key]


def whole_run(case, seed, reverse=False, hidden=16, **over):
    """torch's run of a WHOLE_RUNS case from make_net(seed, hidden), computed once per process."""
    key = ("run", case, seed, reverse, hidden, tuple(sorted(over.items())))
    if key not in _CACHE:
        c = WHOLE_RUNS[case]
        x, t, m, w, s = dataset(case)
        kw = dict(patience=c["patience"], sched_patience=c["sched_patience"])
        kw.update(over)
        _CACHE[key] = train(make_net(seed, hidden), x, t, m, w, s, reverse=reverse, **kw)
    return _CACHE[key]


def kfold(n, k, seed):
    """The package's kfold_splits, restated: a RandomState(seed) permutation cut by np.array_split; fold f's rows validate split f."""
    perm = np.random.RandomState(seed).permutation(n)
    out = np.full((k, n), 1, dtype=np.uint8)
    for f, rows in enumerate(np.array_split(perm, k)):
        out[f, rows] = 2
    return out


MANY_CASE = "A"            # the data of the many-models test
MANY_TORCH = (0, 1, 2, 3, 4, 5)      # the models of many_models() that are compared with torch


def many_models():
    """70 unequal models on MANY_CASE's data: (seed, hyper-parameters, split row) each.  The first six are the ones compared with torch:
    0 the reference's defaults at patience 40, 1 Huber delta 0.5 (the linear branch dominates), 2 without target 6 (--mask-decay-h3),
    3 fold 1 of five, 4 no weight decay, 5 --no-split (150 epochs: nothing stops it early).  Then the five folds, and a mix of seeds, learning rates, weight decays and
    lifetimes from one epoch to no early stop."""
    n = WHOLE_RUNS[MANY_CASE]["n"]
    base, folds, both = split_80_20(n), kfold(n, 5, 3), np.full(n, 3, dtype=np.uint8)
    out = [(42, dict(patience=40), base),
           (7, dict(patience=40, huber_delta=0.5), base),
           (42, dict(patience=40, target_mask=0x7FF & ~(1 << 6)), base),
           (11, dict(patience=40), folds[1]),
           (5, dict(patience=40, weight_decay=0.0), base),
           (3, dict(patience=40, epochs=150), both)]
    out += [(20 + f, dict(patience=30, epochs=300), folds[f]) for f in range(5)]
    lrs, wds = (1e-3, 3e-3, 1e-2), (0.0, 1e-4, 1e-2)
    k = 0
    while len(out) < 70:
        patience = (1, 2, 5, 17, 40, 400)[k % 6]
        out.append((100 + k, dict(lr=lrs[k % 3], weight_decay=wds[(k // 3) % 3], huber_delta=(5.0, 0.5, 1.5)[(k // 9) % 3], patience=patience,
                                  epochs=(1, 3, 64, 150, 400)[k % 5], sched_patience=(30, 5)[k % 2]), (base, both, folds[k % 5])[k % 3]))
        k += 1
    return out
