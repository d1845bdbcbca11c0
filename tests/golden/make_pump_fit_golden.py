#!/usr/bin/env python3
"""Generate tests/golden/pump_fit_golden.json by running the REFERENCE's own tools/analyze_pump_dynamics.py (its model_* functions, rmse,
fit_model, and main() with its three path constants pointed at a temporary directory) and the scipy installed beside it on the fixture of
tests/pump_fit_ref.py.  The reference checkout is not part of this repository and is absent where the GPU tests run, so its outputs
travel as this fixture.

    python tests/golden/make_pump_fit_golden.py --reference <checkout of the reference>

What the file holds:
  inputs      the table, the three traces (R, target) and their rates
  evals       per model a fixed list of parameter vectors with the reference's loss on every trace: its x0, ordinary vectors, one vector
              per guard ("guard"), vectors whose prediction overflows ("nonfinite": 1e9) and vectors whose prediction stays finite
              while its squared error overflows ("overflow": the loss is inf)
  movement    the restatement's own movement on these evaluations: every exp / log result moved by one ulp (up, down, alternating, two
              seeded random patterns) and the loss summed in sample order instead of pairwise.  The largest |difference| of a prediction
              (V) and of a loss (mV): the GPU test's floors are 2.5 x these.
  fits        the 18 fits from the reference's x0: x as float.hex, fun, nit, nfev, and
                path_stable   x bitwise equal and nit equal with the target scaled by 1 + eps, eps in {0, +-1e-13, 3e-12}
                fun_spread    max - min of fun over those four runs
              At least 16 of the 18 must be path_stable (asserted): if another scipy breaks that, change the fixture, not the cap.
                stable_order  the same minimize call with scipy's `np.argsort(fsim)` made a stable sort.  numpy's default argsort does not
                              promise to keep ties in order (its vectorised small-array sort does not), so a fit that meets equal
                              losses can order them either way; the library and the restatement keep them in order.  Where the two
                              runs differ the fit is not path_stable (asserted).
  maxiter5    every fit again with maxiter = 5
  invalid     starts whose whole simplex is invalid, and what scipy returns for them
  report, csv main()'s stdout (the results path replaced by {results}) and its results CSV
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import random
import sys
import tempfile

import numpy as np
import scipy
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pump_fit_ref as own  # noqa: E402

EPS = (0.0, 1e-13, -1e-13, 3e-12)

EVALS = {
    0: [([50.0], ""), ([0.4], ""), ([3.0], ""), ([1e-300], ""), ([0.0], "guard"), ([-3.0], "guard")],
    1: [([50.0], ""), ([0.4], ""), ([2.5], ""), ([0.0], "guard"), ([-1e-3], "guard")],
    2: [([0.999, 1e-6], ""), ([0.9, -2e-7], ""), ([0.0, 1e-7], ""), ([-0.1, 1e-6], "guard"), ([1.0, 1e-6], "guard"), ([0.5, 1e308], "nonfinite")],
    3: [([0.999, -1.0], ""), ([0.99, -0.04], ""), ([-1e-9, -1.0], "guard"), ([1.5, -1.0], "guard"), ([0.5, 1e308], "overflow"),
        ([0.9999, 1.7e308], "nonfinite")],
    4: [([0.999, -1.0, 1.0], ""), ([0.99, -0.05, 0.02], ""), ([1.0, -1.0, 1.0], "guard"), ([-0.5, -1.0, 1.0], "guard"),
        ([0.5, 1e308, -1e308], "overflow"), ([0.9999, 1.7e308, 1.7e308], "nonfinite")],
    5: [([1.99, -0.99, -1.0, 0.5], "guard"), ([1.9, -0.905, -0.04, 0.03], ""), ([0.3, 0.2, 0.1, -0.1], ""),
        ([2.1, -1.0, -1.0, 0.5], "guard"), ([-1.5, 0.6, -1.0, 0.5], "guard"), ([1.0, -1.0, -1.0, 0.5], "guard"),
        ([0.0, -1.2, -1.0, 0.5], "guard"), ([1.9, -0.905, 1e308, 1e308], "nonfinite")],
}
INVALID_STARTS = [(0, [-1.0]), (3, [1.5, -1.0]), (5, [2.5, -1.0, -1.0, 0.5])]


def load_reference(root):
    spec = importlib.util.spec_from_file_location("analyze_pump_dynamics_reference", os.path.join(root, "tools", "analyze_pump_dynamics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "pump_fit_golden.json"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    ref_models = [ref.model_lpf_on_R, ref.model_lpf_on_lnR, ref.model_iir1_dR, ref.model_iir1_dlnR, ref.model_iir1_asym, ref.model_iir2_dlnR]

    lut_r, lut_v = own.fixture_table()
    lut_fn = ref.make_lut_interp(lut_r, lut_v)
    traces = []
    for n, f, model, params in own.FIXTURE_TRACES:
        R = own.fixture_resistance(n, f)
        target = ref_models[model](R, own.FIXTURE_SR, list(params), lut_fn) + own.fixture_noise(n)
        traces.append({"n": n, "freq": f, "sr": own.FIXTURE_SR, "r": R.tolist(), "target": target.tolist()})

    def ref_loss(model, t, p, target=None):
        pred = ref_models[model](np.asarray(t["r"]), t["sr"], p, lut_fn)
        if not np.all(np.isfinite(pred)):
            return 1e9
        return float(ref.rmse(pred, np.asarray(t["target"]) if target is None else target))

    # ---- evaluations and the restatement's own movement on them
    table = own.Table(lut_r, lut_v)
    evals, move_pred, move_loss = [], 0.0, 0.0
    with np.errstate(all="ignore"):
        for model, cases in EVALS.items():
            for p, kind in cases:
                for ti, t in enumerate(traces):
                    evals.append({"trace": ti, "model": model, "p": p, "kind": kind, "loss": ref_loss(model, t, p)})
    plain = own.Table(lut_r, lut_v)
    base_rows = {}
    for e in evals:
        t = traces[e["trace"]]
        prob = own.Problem(t["r"], t["sr"], t["target"], plain)
        row = prob.predict(e["model"], e["p"])
        base_rows[(e["trace"], e["model"], tuple(e["p"]))] = (row, own.loss(row, t["target"]))
        if e["kind"] == "":
            move_loss = max(move_loss, abs(own.loss_sequential(row, t["target"]) - own.loss(row, t["target"])))

    class pattern:                   # one-ulp patterns beyond ulp_nudge's up / down
        def __init__(self, choose):
            self.choose = choose

        def __enter__(self):
            self.saved = own._nudged

            def nudged(v, choose=self.choose):
                d = choose()
                if d == 0 or not np.isfinite(v):
                    return v
                return float(np.nextafter(v, np.inf if d > 0 else -np.inf))
            own._nudged = nudged

        def __exit__(self, *exc):
            own._nudged = self.saved

    def alternating():
        state = [1]

        def choose():
            state[0] = -state[0]
            return state[0]
        return choose

    def seeded(seed):
        rng = random.Random(seed)
        return lambda: rng.choice((-1, 0, 1))

    for ctx in (own.ulp_nudge(1), own.ulp_nudge(-1), pattern(alternating()), pattern(seeded(1)), pattern(seeded(2))):
        with ctx:
            moved = own.Table(lut_r, lut_v)
            for e in evals:
                if e["kind"] != "":
                    continue
                t = traces[e["trace"]]
                row = own.Problem(t["r"], t["sr"], t["target"], moved).predict(e["model"], e["p"])
                row0, loss0 = base_rows[(e["trace"], e["model"], tuple(e["p"]))]
                move_pred = max(move_pred, float(np.max(np.abs(np.asarray(row) - np.asarray(row0)))))
                move_loss = max(move_loss, abs(own.loss(row, t["target"]) - loss0))

    # ---- fits
    def ref_fit(model, t, x0, target, maxiter=5000):
        def loss(p):
            pred = ref_models[model](np.asarray(t["r"]), t["sr"], p, lut_fn)
            if not np.all(np.isfinite(pred)):
                return 1e9
            return ref.rmse(pred, target)
        with np.errstate(all="ignore"):
            return minimize(loss, x0, method="Nelder-Mead", options={"xatol": 1e-6, "fatol": 1e-6, "maxiter": maxiter})

    import scipy.optimize._optimize as so

    class stable_argsort:            # scipy's own code, its ordering pinned to a stable sort
        class proxy:
            def __getattr__(self, name):
                return getattr(np, name)

            def argsort(self, a, *a_, **kw):
                return np.argsort(a, kind="stable")

        def __enter__(self):
            self.saved, so.np = so.np, self.proxy()

        def __exit__(self, *exc):
            so.np = self.saved

    def record(r):
        return {"x": [float(v).hex() for v in r.x], "fun": float(r.fun), "nit": int(r.nit), "nfev": int(r.nfev), "status": int(r.status)}

    def both(model, t, x0, maxiter=5000):
        r = ref_fit(model, t, x0, np.asarray(t["target"]), maxiter)
        with stable_argsort():
            rs = ref_fit(model, t, x0, np.asarray(t["target"]), maxiter)
        return r, dict(record(r), stable_order=record(rs))

    fits, maxiter5 = [], []
    for ti, t in enumerate(traces):
        for model in range(6):
            x0 = own.X0[model]
            runs = [ref_fit(model, t, x0, np.asarray(t["target"]) * (1.0 + eps)) for eps in EPS]
            r0 = runs[0]
            with np.errstate(all="ignore"):
                x_ref, f_ref = ref.fit_model(ref_models[model], np.asarray(t["r"]), t["sr"], np.asarray(t["target"]), lut_fn, x0)
            assert np.array_equal(x_ref, r0.x) and f_ref == r0.fun            # fit_model is that minimize call
            stable = all(np.array_equal(r.x, r0.x) and r.nit == r0.nit for r in runs)
            funs = [float(r.fun) for r in runs]
            rb, rec = both(model, t, x0)
            assert record(rb) == record(r0)
            assert rec["stable_order"] == record(r0) or not stable, "a path_stable fit depends on how ties are ordered: change the fixture"
            fits.append(dict(rec, trace=ti, model=model, x0=x0, path_stable=bool(stable), fun_spread=max(funs) - min(funs)))
            maxiter5.append(dict(both(model, t, x0, maxiter=5)[1], trace=ti, model=model, x0=x0))
            print(own.MODELS[model], ti, r0.nit, r0.nfev, r0.fun, stable, file=sys.stderr)
    n_stable = sum(f["path_stable"] for f in fits)
    assert n_stable >= 16, f"only {n_stable} of {len(fits)} fits are path_stable: change the fixture"

    invalid = []
    for model, x0 in INVALID_STARTS:
        r, rec = both(model, traces[0], x0)
        invalid.append(dict(rec, trace=0, model=model, x0=x0, success=bool(r.success)))

    # ---- the reference's main() on the fixture written as its two kinds of CSV
    with tempfile.TemporaryDirectory() as tmp:
        sin_dir = os.path.join(tmp, "pump_sin")
        os.mkdir(sin_dir)
        ref.LUT_CSV = os.path.join(tmp, "pump_sweep_88k2.csv")
        ref.SIN_DIR = sin_dir
        ref.RESULTS_CSV = os.path.join(tmp, "pump_fit_results.csv")
        with open(ref.LUT_CSV, "w") as f:
            f.write(own.fixture_lut_csv(lut_r, lut_v))
        for t in traces:
            with open(os.path.join(sin_dir, own.fixture_sin_name(t["freq"])), "w") as f:
                f.write(own.fixture_sin_csv(t["r"], t["target"], t["freq"], t["sr"]))
        out = io.StringIO()
        with contextlib.redirect_stdout(out), np.errstate(all="ignore"):
            ref.main()
        report = out.getvalue().replace(ref.RESULTS_CSV, "{results}")
        with open(ref.RESULTS_CSV, newline="") as f:
            csv_text = f.read()

    golden = {"scipy": scipy.__version__, "numpy": np.__version__, "skip": own.SKIP, "lut_r": lut_r.tolist(), "lut_v": lut_v.tolist(), "traces": traces,
              "evals": evals, "movement": {"pred": move_pred, "loss": move_loss}, "fits": fits, "maxiter5": maxiter5, "invalid": invalid,
              "report": report, "csv": csv_text}
    with open(args.out, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print(f"{args.out}: {n_stable} of {len(fits)} path_stable, movement {golden['movement']}", file=sys.stderr)


if __name__ == "__main__":
    main()
