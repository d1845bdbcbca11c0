"""ow_pump_fit_eval / ow_pump_fit (k_pump_fit_eval, k_pump_fit) against the reference's own results on the fixture of
tests/golden/pump_fit_golden.json and against the restatement (tests/pump_fit_ref.py).

Floors.  The golden's `movement` is the restatement's own movement on the fixture's evaluations with every exp / log result moved by one
ulp (five patterns) and with the loss summed in sample order instead of pairwise: 7.24e-14 V on a prediction, 2.39e-11 mV on a loss.  The
floors are 2.5 x those (the project's rule).  The device's distances are printed by test_evaluations; DESIGN.md (section 10, the pump-dynamics fitter) has them: 1.78e-15 V and 7.28e-12 mV on one MI355X.

Fits.  A `path_stable` fit (17 of 18: the reference returns the same bits with the target scaled by 1 + eps, |eps| <= 3e-12, 1e4 times
what summation order and one-ulp functions move the loss) must return the golden's x bit for bit with equal nit and nfev.  The other fit
must reach the golden's fun within the reference's own spread over its perturbed runs.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pump_fit_ref as ref
from openwurli_amd import binding, pump, pump_fit

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "pump_fit_golden.json")) as f:
        g = json.load(f)
    g["table"] = (g["lut_r"], g["lut_v"])
    g["floor_pred"], g["floor_loss"] = 2.5 * g["movement"]["pred"], 2.5 * g["movement"]["loss"]
    return g


@pytest.fixture(scope="module")
def problems(golden):
    table = ref.Table(golden["lut_r"], golden["lut_v"])
    return [ref.Problem(t["r"], t["sr"], t["target"], table) for t in golden["traces"]]


@pytest.fixture(scope="module")
def fitted(golden):
    """The 18 fits in one call, shared."""
    return pump_fit.fit(golden["traces"], golden["table"], [(f["trace"], f["model"], f["x0"]) for f in golden["fits"]])


def bits(rows):
    return [([float(v).hex() for v in q["x"]], float(q["fun"]).hex(), q["nit"], q["nfev"], q["status"]) for q in rows]


def test_evaluations(golden, problems):
    evals = golden["evals"]
    loss, pred = pump_fit.evaluate(golden["traces"], golden["table"], [(e["trace"], e["model"], e["p"]) for e in evals], predictions=True)
    assert np.array_equal(loss, pump_fit.evaluate(golden["traces"], golden["table"], [(e["trace"], e["model"], e["p"]) for e in evals]))
    worst_pred = worst_loss = 0.0
    for i, e in enumerate(evals):
        n = golden["traces"][e["trace"]]["n"]
        assert np.all(pred[i, n:] == 0.0)
        if e["kind"] == "guard":
            assert loss[i] == 1e9 and np.all(np.isnan(pred[i, :n])), e
        elif e["kind"] == "nonfinite":
            assert loss[i] == 1e9 and not np.all(np.isfinite(pred[i, :n])), e
        elif e["kind"] == "overflow":
            assert loss[i] == np.inf and np.all(np.isfinite(pred[i, :n])), e
        else:
            row = np.asarray(problems[e["trace"]].predict(e["model"], e["p"]))
            worst_pred = max(worst_pred, float(np.max(np.abs(pred[i, :n] - row))))
            worst_loss = max(worst_loss, abs(float(loss[i]) - e["loss"]))
    print("device against the reference: prediction %.3e V (floor %.3e), loss %.3e mV (floor %.3e)"
          % (worst_pred, golden["floor_pred"], worst_loss, golden["floor_loss"]))
    assert worst_pred <= golden["floor_pred"] and worst_loss <= golden["floor_loss"]


def test_stable_fits_are_the_references_bit_for_bit(golden, fitted):
    for f, q in zip(golden["fits"], fitted):
        print(q["model"], f["trace"], q["nit"], q["nfev"], q["fun"], f["fun"], "stable" if f["path_stable"] else "other")
    for f, q in zip(golden["fits"], fitted):
        if f["path_stable"]:
            assert [float(v).hex() for v in q["x"]] == f["x"] and (q["nit"], q["nfev"]) == (f["nit"], f["nfev"]), (f, q)
            assert abs(q["fun"] - f["fun"]) <= golden["floor_loss"] and q["status"] == pump_fit.CONVERGED, (f, q)


def test_other_fits_reach_the_references_loss(golden, problems, fitted):
    others = [(f, q) for f, q in zip(golden["fits"], fitted) if not f["path_stable"]]
    assert len(others) <= 2
    for f, q in others:
        own = problems[f["trace"]].loss(f["model"], q["x"])
        print(q["model"], f["trace"], "device fun %.17g, golden %.17g, spread %.3e, loss at the device's x %.17g" % (q["fun"], f["fun"], f["fun_spread"], own))
        assert q["fun"] <= f["fun"] + f["fun_spread"] + golden["floor_loss"]
        assert abs(own - q["fun"]) <= golden["floor_loss"]


def test_packing_does_not_change_a_fit(golden, fitted):
    jobs = [(f["trace"], f["model"], f["x0"]) for f in golden["fits"]]
    want = bits(fitted)
    alone = [pump_fit.fit(golden["traces"], golden["table"], [j])[0] for j in jobs]
    assert bits(alone) == want
    assert bits(pump_fit.fit(golden["traces"], golden["table"], jobs[::-1])[::-1]) == want
    nine = pump_fit.fit(golden["traces"], golden["table"], [jobs[10]] * 9)          # straddles a wavefront
    assert bits(nine) == [want[10]] * 9
    g = pump_fit.grid(golden["traces"][:1], golden["table"], 3, seed=5, models=("iir1_asym", "lpf_lnR"))
    assert [q["start"] for q in g] == [0, 1, 2] * 2 and sum(q["best"] for q in g) == 2
    single = [pump_fit.fit(golden["traces"][:1], golden["table"], [(0, q["model"], q["x0"])])[0] for q in g]
    assert bits(g) == bits(single)


def test_maxiter_and_invalid_starts(golden):
    five = pump_fit.fit(golden["traces"], golden["table"], [(f["trace"], f["model"], f["x0"]) for f in golden["maxiter5"]], maxiter=5)
    for f, q in zip(golden["maxiter5"], five):
        assert q["status"] == pump_fit.MAXITER_REACHED and [float(v).hex() for v in q["x"]] == f["x"] and (q["nit"], q["nfev"]) == (5, f["nfev"]), (f, q)
    inv = pump_fit.fit(golden["traces"], golden["table"], [(f["trace"], f["model"], f["x0"]) for f in golden["invalid"]])
    for f, q in zip(golden["invalid"], inv):
        # scipy: success after the simplex has shrunk below xatol, the f test passing on equal 1e9 losses
        assert q["status"] == pump_fit.START_INVALID and q["fun"] == 1e9 and [float(v).hex() for v in q["x"]] == f["x"], (f, q)
        assert (q["nit"], q["nfev"]) == (f["nit"], f["nfev"])
    one = pump_fit.fit(golden["traces"], golden["table"], [(0, 0, [50.0])], maxiter=1)[0]
    assert (one["nit"], one["nfev"], one["status"]) == (1, 2, pump_fit.MAXITER_REACHED)


def test_refusals(golden, hiplib):
    t = golden["traces"][0]
    good = dict(r=np.array(t["r"]), y=np.array(t["target"]), offs=np.array([0, t["n"]], dtype=np.uint64), rates=np.array([t["sr"]]),
                lut_r=np.array(golden["lut_r"]), lut_v=np.array(golden["lut_v"]), tr=np.zeros(1, dtype=np.uint32), mo=np.zeros(1, dtype=np.uint32),
                x0=np.array([[50.0, 0, 0, 0]]), skip=200, maxiter=100)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)                          # noqa: E731

    def run(entry, **kw):
        a = dict(good, **kw)
        x, fun = np.full((1, 4), -7.0), np.full(1, -7.0)
        nit, nfev, status = (np.full(1, 77, dtype=np.uint32) for _ in range(3))
        pred = np.full((1, 700), -7.0)
        head = (p(a["r"]), p(a["y"]), p(a["offs"]), p(a["rates"]), 1, p(a["lut_r"]), p(a["lut_v"]), 0 if a["lut_r"] is None else a["lut_r"].size, p(a["tr"]),
                p(a["mo"]), p(a["x0"]), 1, a["skip"])
        if entry == "fit":
            rc = hiplib.ow_pump_fit(*head, 1e-6, 1e-6, a["maxiter"], 0, p(x), p(fun), p(nit), p(nfev), p(status))
        else:
            rc = hiplib.ow_pump_fit_eval(*head, 0, p(fun), p(pred), a.get("stride", 700))
        err = binding.take_error(hiplib)
        assert np.all(x == -7.0) and np.all(fun == -7.0) and np.all(pred == -7.0) and nit[0] == nfev[0] == status[0] == 77      # untouched
        return rc, err

    def changed(name, i, v):
        a = good[name].copy()
        a.flat[i] = v
        return {name: a}
    cases = [(dict(skip=t["n"] - 1), "samples: skip + 1"), (dict(skip=t["n"]), "samples: skip + 1"),
             (changed("lut_r", 3, golden["lut_r"][2]), "not strictly ascending"), (changed("lut_r", 0, 0.0), "lut_r is not a finite positive"),
             (changed("r", 5, 0.0), "r is not a finite positive"), (changed("r", 5, -1.0), "r is not a finite positive"),
             (changed("mo", 0, 6), "model 6 above 5"), (changed("tr", 0, 1), "trace 1 out of range"),
             (changed("r", 9, np.nan), "r is not a finite positive"), (changed("y", 9, np.inf), "target is not finite"),
             (changed("lut_v", 1, np.nan), "lut_v"), (changed("rates", 0, np.inf), "sample_rate"), (changed("x0", 0, np.nan), "parameter"),
             (dict(lut_r=good["lut_r"][:1], lut_v=good["lut_v"][:1]), "fewer than 2 points")]
    cases += [({name: None}, "null argument") for name in ("r", "y", "offs", "rates", "lut_r", "lut_v", "tr", "mo", "x0")]
    for entry in ("fit", "eval"):
        for kw, text in cases:
            rc, err = run(entry, **kw)
            assert rc < 0 and err.startswith("ow_pump_fit: " if entry == "fit" else "ow_pump_fit_eval: ") and text in err, (entry, kw.keys(), err)
    rc, err = run("fit", maxiter=0)
    assert rc < 0 and "maxiter is 0" in err
    rc, err = run("eval", stride=t["n"] - 1)
    assert rc < 0 and "pred_stride" in err
    assert hiplib.ow_pump_fit(*[None] * 4, 1, *[None] * 2, 2, *[None] * 3, 1, 200, 1e-6, 1e-6, 10, 0, *[None] * 5) < 0
    assert "null argument" in binding.take_error(hiplib)


def test_from_device_equals_the_written_files(tmp_path):
    """One short point (settle 2 000, 2 cycles at 400 Hz; the table from 8 points): the tool's captures are pump-sinusoid's, and its
    fit from the device equals the fit of the files it wrote."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("analyze_pump_dynamics_tool", os.path.join(ROOT, "tools", "analyze_pump_dynamics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    flags = ["--from-device", "--freqs", "400", "--settle", "2000", "--cycles", "2", "--lut-points", "8", "--lut-settle", "2000", "--lut-avg", "64"]
    a = tool.main(flags + ["--write-csv", str(tmp_path), "--results", str(tmp_path / "a.csv")])
    single = pump.pump_sinusoid(freq=400.0, cycles=2.0, settle=2000, csv=str(tmp_path / "single.csv"))
    assert a["inputs"]["sin_csvs"][0] == single["csv_text"] and np.array_equal(a["inputs"]["raw"][0], single["trace"])
    assert a["traces"][0]["r"].size == 441 and a["traces"][0]["sr"] == 88200.0 and a["traces"][0]["freq"] == 400.0
    b = tool.main(["--lut", str(tmp_path / "pump_sweep_88k2.csv"), "--sin-dir", str(tmp_path / "pump_sin"), "--results", str(tmp_path / "b.csv")])
    assert a["csv_text"] == b["csv_text"] and a["report"].replace("a.csv", "b.csv") == b["report"]
    for ra, rb in zip(a["rows"], b["rows"]):
        for name in pump_fit.MODELS:
            assert bits([ra[name + "_fit"]]) == bits([rb[name + "_fit"]])
    assert (tmp_path / "a.csv").read_text().replace("\r\n", "\n") == a["csv_text"].replace("\r\n", "\n")
