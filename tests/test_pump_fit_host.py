"""The pump-dynamics fitter without a device: the restatement (tests/pump_fit_ref.py) against the reference's own results
(tests/golden/pump_fit_golden.json, written by tests/golden/make_pump_fit_golden.py from the reference's functions and scipy), the CSV
readers and the report text, the start boxes, the wavefront packing and the Python layer's argument checks.

Ordering of ties.  scipy orders the simplex with numpy's default argsort, which does not promise to keep equal losses in order (its
vectorised small-array sort does not); the library and the restatement use a stable ordering.  The golden therefore carries, beside
scipy's run, the same scipy code with a stable argsort (`stable_order`).  The two differ for one fit of the fixture only: iir2_dlnR on the
first trace, the fit that is not path_stable (it ends on the stability boundary a2 = -1 and meets three equal finite losses at iteration
347; scipy: nit 355, nfev 635; stable ordering: nit 359, nfev 644).  Every fit is checked bit for bit against scipy's code: against the
unmodified run wherever ties did not matter, against the stable-order run always.
"""
import json
import math
import os

import numpy as np
import pytest

import pump_fit_ref as ref
from openwurli_amd import pump_fit

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "pump_fit_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def problems(golden):
    table = ref.Table(golden["lut_r"], golden["lut_v"])
    return [ref.Problem(t["r"], t["sr"], t["target"], table) for t in golden["traces"]]


def hexes(x):
    return [float(v).hex() for v in x]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_golden_meets_the_fixtures_condition(golden):
    assert len(golden["fits"]) == 18 and sum(f["path_stable"] for f in golden["fits"]) >= 16
    assert golden["skip"] == ref.SKIP == pump_fit.SKIP
    kinds = {(e["model"], e["kind"]) for e in golden["evals"]}
    assert all((m, "guard") in kinds for m in range(6)) and any(k == "nonfinite" for _, k in kinds)
    assert all(e["loss"] == ref.INVALID_LOSS for e in golden["evals"] if e["kind"] in ("guard", "nonfinite"))
    assert all(e["loss"] == math.inf for e in golden["evals"] if e["kind"] == "overflow") and (3, "overflow") in kinds
    assert all(e["loss"] < ref.INVALID_LOSS for e in golden["evals"] if not e["kind"])
    assert golden["movement"]["pred"] > 0 and golden["movement"]["loss"] > 0


def test_restatement_losses_are_the_references(golden, problems):
    for e in golden["evals"]:
        assert problems[e["trace"]].loss(e["model"], e["p"]) == e["loss"], e


@pytest.mark.parametrize("key,maxiter", [("fits", 5000), ("maxiter5", 5), ("invalid", 5000)])
def test_restatement_fits_are_scipys_bit_for_bit(golden, problems, key, maxiter):
    differ = []
    for f in golden[key]:
        r = ref.nelder_mead(lambda p: problems[f["trace"]].loss(f["model"], p), f["x0"], maxiter=maxiter)
        got = {"x": hexes(r["x"]), "fun": r["fun"], "nit": r["nit"], "nfev": r["nfev"]}
        stable = {k: f["stable_order"][k] for k in got}
        assert got == stable, (key, f["trace"], f["model"], got, stable)
        if got != {k: f[k] for k in got}:
            differ.append((f["trace"], f["model"]))
            assert not f.get("path_stable", False)
        # scipy's status: 0 success, 2 maxiter; a start that never leaves the invalid region is a success to scipy
        want = ref.MAXITER if f["status"] == 2 else (ref.START_INVALID if f["fun"] == ref.INVALID_LOSS else ref.CONVERGED)
        assert r["status"] == want, (key, f["trace"], f["model"], r["status"], f["status"])
    print(key, "fits whose ties scipy ordered otherwise:", differ)
    assert differ == ([(0, 5)] if key == "fits" else [])


def test_invalid_starts_end_as_scipy_ends_them(golden):
    """What scipy returns for a start whose whole simplex is invalid: success, fun = 1e9, after the simplex has shrunk below xatol (the
    f test passes on equal 1e9 losses); the restatement names it START_INVALID (checked above)."""
    for f in golden["invalid"]:
        assert f["success"] and f["status"] == 0 and f["fun"] == ref.INVALID_LOSS and 15 <= f["nit"] <= 20


def test_restatement_matches_scipy_directly(golden, problems):
    optimize = pytest.importorskip("scipy.optimize")
    for f in golden["fits"][:5] + golden["maxiter5"][:6] + golden["invalid"][:1]:
        maxiter = 5 if f in golden["maxiter5"] else 5000
        loss = lambda p: problems[f["trace"]].loss(f["model"], p)                              # noqa: E731
        with np.errstate(all="ignore"):
            s = optimize.minimize(loss, f["x0"], method="Nelder-Mead", options={"xatol": 1e-6, "fatol": 1e-6, "maxiter": maxiter})
        r = ref.nelder_mead(loss, f["x0"], maxiter=maxiter)
        assert hexes(s.x) == hexes(r["x"]) and float(s.fun) == r["fun"] and (s.nit, s.nfev) == (r["nit"], r["nfev"]), (f["trace"], f["model"])


def test_lookup_is_numpys_interp(golden):
    r, v = np.asarray(golden["lut_r"]), np.asarray(golden["lut_v"])
    table = ref.Table(r, v)
    xs = np.concatenate([r, r * (1 + 1e-9), [1.0, 999.0, 1e6 + 1, 1e9, 31_000.0, math.inf]])
    want = np.interp(np.log(np.clip(xs, r[0], r[-1])), np.log(r), v)
    assert [table(x) for x in xs] == want.tolist()
    assert [table(x) for x in r] == v.tolist() and table(1.0) == v[0] and table(1e9) == v[-1]      # exact on a knot, the ends held
    assert math.isnan(table(math.nan))


def test_guards(golden):
    assert not ref.valid(0, [0.0]) and not ref.valid(1, [-1.0]) and ref.valid(0, [1e-300]) and ref.valid(0, [math.nan])
    assert ref.valid(2, [0.0, 1.0]) and not ref.valid(3, [1.0, 1.0]) and not ref.valid(4, [-1e-300, 1.0, 1.0]) and not ref.valid(2, [math.nan, 1.0])
    assert not ref.valid(5, [1.99, -0.99])                  # the reference's own start: z1 = 0.5 (1.99 + 0.01) = 1
    assert ref.valid(5, [1.9, -0.905]) and not ref.valid(5, [1.0, -1.0]) and not ref.valid(5, [0.0, -1.2]) and not ref.valid(5, [-1.5, 0.6])
    row = ref.predict(5, golden["traces"][0]["r"][:8], 88200.0, [1.99, -0.99, -1.0, 0.5], ref.Table(golden["lut_r"], golden["lut_v"]))
    assert all(math.isnan(x) for x in row)


def test_start_indices(golden, problems):
    """The residual is zero at sample 0, and at samples 0 and 1 for the biquad."""
    p = problems[0]
    for model, params in ((2, [0.5, 1e-6]), (3, [0.5, 1.0]), (4, [0.5, 1.0, 2.0])):
        row = p.predict(model, params)
        assert row[0] == p.base[0] and row[1] != p.base[1]
    row = p.predict(5, [0.3, 0.2, 1.0, 1.0])
    assert row[0] == p.base[0] and row[1] == p.base[1] and row[2] != p.base[2]


# ---- the readers, the report and the results CSV -------------------------------------------------------------------------------------
def fixture_files(golden, tmp_path):
    (tmp_path / "pump_sin").mkdir()
    (tmp_path / "lut.csv").write_text(ref.fixture_lut_csv(golden["lut_r"], golden["lut_v"]))
    for t in golden["traces"]:
        (tmp_path / "pump_sin" / ref.fixture_sin_name(t["freq"])).write_text(ref.fixture_sin_csv(t["r"], t["target"], t["freq"], t["sr"]))
    return str(tmp_path / "lut.csv"), str(tmp_path / "pump_sin")


def test_readers_take_the_references_files(golden, tmp_path):
    lut, sin_dir = fixture_files(golden, tmp_path)
    r, v = pump_fit.load_lut(lut)
    assert r.tolist() == golden["lut_r"] and v.tolist() == golden["lut_v"]
    t = golden["traces"][1]
    d = pump_fit.load_sinusoid(os.path.join(sin_dir, ref.fixture_sin_name(t["freq"])))
    assert d["sr"] == t["sr"] and d["freq"] == t["freq"] and d["r"].tolist() == t["r"] and d["target"].tolist() == t["target"]
    # what the commands write: pump-sweep's header and five columns; pump-sinusoid's header tokens, the pair mean in the last column
    r2, v2 = pump_fit.parse_lut("r_ldr,pump_v,pump_std,pump_min,pump_max\n# note\n2.000000e3,1.5e0,0,0,0\n1.000000e3,5.000000000e-1,0,0,0\n")
    assert r2.tolist() == [1000.0, 2000.0] and v2.tolist() == [0.5, 1.5]                         # sorted by resistance
    d = pump_fit.parse_sinusoid("# pump-sinusoid  ldr_min=1.9e4  ldr_max=1e6  freq=5.600000  sr=88200  cycles=10\nsample,r_ldr,pump_v,pump_avg2\n"
                                "0,1.000000e6,2.0e0,2.5e0\n1,9.9e5,3.0e0,2.5e0\n")
    assert (d["sr"], d["freq"]) == (88200.0, 5.6) and d["target"].tolist() == [2.5, 2.5] and d["pump"].tolist() == [2.0, 3.0]
    assert (pump_fit.LUT_CSV, pump_fit.SIN_DIR, pump_fit.RESULTS_CSV) == ("/tmp/pump_sweep_88k2.csv", "/tmp/pump_sin", "/tmp/pump_fit_results.csv")


def test_report_and_results_csv_are_the_references(golden, problems):
    """The reference's stdout and results CSV from the reference's numbers, character for character (files in path order)."""
    rows = []
    for ti in sorted(range(3), key=lambda i: ref.fixture_sin_name(golden["traces"][i]["freq"])):
        p = problems[ti]
        row = {"freq": golden["traces"][ti]["freq"], "baseline_mv": ref.loss(p.base, p.target)}
        for f in golden["fits"]:
            if f["trace"] == ti:
                name = ref.MODELS[f["model"]]
                row[name + "_rmse_mv"], row[name + "_params"] = f["fun"], [float.fromhex(h) for h in f["x"]]
        rows.append(row)
    assert pump_fit.format_report((golden["lut_r"], golden["lut_v"]), rows, "{results}") == golden["report"]
    assert pump_fit.format_results_csv(rows) == golden["csv"]


# ---- start boxes, packing, argument checks -------------------------------------------------------------------------------------------
def test_start_boxes():
    assert pump_fit.MODELS == ref.MODELS and pump_fit.N_PARAMS == ref.N_PARAMS and list(pump_fit.X0) == list(ref.X0)
    for m, name in enumerate(pump_fit.MODELS):
        starts = pump_fit.grid_starts(name, 200, seed=3)
        assert starts[0] == list(pump_fit.X0[m]) and starts == pump_fit.grid_starts(m, 200, seed=3) and starts[:7] == pump_fit.grid_starts(m, 7, seed=3)
        assert starts[1:] != pump_fit.grid_starts(m, 200, seed=4)[1:]
        box = pump_fit.START_BOXES
        for x in starts[1:]:
            assert len(x) == pump_fit.N_PARAMS[m] and ref.valid(m, x), (name, x)
            if m < 2:
                assert box["tau_ms"][0] <= x[0] <= box["tau_ms"][1]
            elif m < 5:
                assert box["one_minus_a"][0] * (1 - 1e-9) <= 1.0 - x[0] <= box["one_minus_a"][1]
                b = box["b_dR" if m == 2 else "b_dlnR"]
                assert all(b[0] <= abs(v) <= b[1] for v in x[1:])
            else:
                rho = math.sqrt(-x[1])
                assert box["one_minus_rho"][0] * (1 - 1e-6) <= 1.0 - rho <= box["one_minus_rho"][1] * (1 + 1e-9) and x[0] * x[0] + 4 * x[1] < 0
                assert all(box["b_dlnR"][0] <= abs(v) <= box["b_dlnR"][1] for v in x[2:])
        if m >= 2:
            assert {v > 0 for x in starts[1:] for v in x[-1:]} == {True, False}                   # either sign


def test_wavefront_packing():
    trace = [1, 0, 1, 0, 0, 1] + [2] * 19
    model = [5, 3, 5, 3, 0, 0] + [4] * 19
    order, inverse, waves = pump_fit.pack_waves(trace, model)
    assert order.tolist()[:6] == [4, 1, 3, 5, 0, 2] and order.tolist()[6:] == list(range(6, 25))   # stable inside a (trace, model)
    assert inverse[order].tolist() == list(range(25)) and order[inverse].tolist() == list(range(25))
    assert waves == [(0, 0, 0, 1), (0, 3, 1, 2), (1, 0, 3, 1), (1, 5, 4, 2), (2, 4, 6, 8), (2, 4, 14, 8), (2, 4, 22, 3)]
    assert pump_fit.pack_waves([0] * 9, [1] * 9)[2] == [(0, 1, 0, 8), (0, 1, 8, 1)]              # nine copies straddle a wavefront
    assert pump_fit.pack_waves([], [])[2] == []
    with pytest.raises(ValueError):
        pump_fit.pack_waves([0, 1], [0])


def test_python_argument_checks(golden):
    t = {"r": [1e4] * 300, "target": [1.0] * 300, "sr": 88200.0}
    lut = ([1e3, 1e6], [0.5, 3.0])
    for call, what in ((lambda: pump_fit.fit([t], lut, [(0, "lpf_R", [1.0, 2.0])]), "takes 1 parameters, got 2"),
                       (lambda: pump_fit.fit([t], lut, [(0, "iir2_dlnR", [1.0])]), "takes 4 parameters, got 1"),
                       (lambda: pump_fit.fit([t], lut, [(0, "biquad", [1.0])]), "unknown model 'biquad'"),
                       (lambda: pump_fit.fit([t], lut, [(0, 6, [1.0])]), "model id 6 outside 0..5"),
                       (lambda: pump_fit.fit([t], lut, [(1, 0, [1.0])]), "trace 1 outside 0..0"),
                       (lambda: pump_fit.fit([t], lut, [(0, 0, [1.0])], maxiter=0), "maxiter must be at least 1"),
                       (lambda: pump_fit.fit([], lut, []), "no traces"),
                       (lambda: pump_fit.evaluate([dict(t, target=[1.0] * 299)], lut, [(0, 0, [1.0])]), "r has 300 samples, target 299"),
                       (lambda: pump_fit.evaluate([t], ([1e3, 1e6], [0.5]), [(0, 0, [1.0])]), "2 resistances and 1 values"),
                       (lambda: pump_fit.grid([t], lut, 0), "starts must be at least 1")):
        with pytest.raises(ValueError) as e:
            call()
        assert what in str(e.value), (what, str(e.value))
    assert pump_fit.model_id("iir1_asym") == 4 and pump_fit.model_id(np.uint32(2)) == 2
