"""The pump-dynamics fitter on the device: host mirror of the reference's ``tools/analyze_pump_dynamics.py`` over the C-ABI
(``ow_pump_fit_eval``, ``ow_pump_fit``).

The reference takes the static pump table of ``pump-sweep`` and the slewed-R captures of ``pump-sinusoid``, fits a ladder of six cheap
predictors R(t) -> pump(t) by Nelder-Mead and reports the RMSE per (model, frequency): can the 12-node melange shadow solver be replaced
by an analytical predictor?  Here every fit of a run -- files x models, or files x models x starts -- is one row of eight lanes in ONE
``ow_pump_fit`` call; include/openwurli_hip.h states the models, the lookup, the loss and the Nelder-Mead contract.

A trace is a dict ``{"r", "target", "sr"}`` (``freq`` too where a report needs it); the table is ``(lut_r, lut_v)``.
"""
import csv
import ctypes as C
import glob
import io
import os

import numpy as np

from .binding import (PUMP_FIT_CONVERGED, PUMP_FIT_MAX_LUT, PUMP_FIT_MAXITER, PUMP_FIT_START_INVALID, OwError, check,  # noqa: F401
                      load_library)

MODELS = ("lpf_R", "lpf_lnR", "iir1_dR", "iir1_dlnR", "iir1_asym", "iir2_dlnR")
N_PARAMS = (1, 1, 2, 2, 3, 4)
X0 = ([50.0], [50.0], [0.999, 1e-6], [0.999, -1.0], [0.999, -1.0, 1.0], [1.99, -0.99, -1.0, 0.5])      # the reference's starts
SKIP = 200                                    # the reference's rmse(skip=200)
XATOL = FATOL = 1e-6                          # its minimize options
MAXITER = 5000
CONVERGED, MAXITER_REACHED, START_INVALID = PUMP_FIT_CONVERGED, PUMP_FIT_MAXITER, PUMP_FIT_START_INVALID
STATUS_NAMES = ("converged", "maxiter", "start_invalid")
FITS_PER_WAVE = 8                             # OW_PF_ROWS: a wavefront holds eight fits of one (trace, model)
LUT_CSV, SIN_DIR, RESULTS_CSV = "/tmp/pump_sweep_88k2.csv", "/tmp/pump_sin", "/tmp/pump_fit_results.csv"      # the reference's constants


def model_id(model) -> int:
    if isinstance(model, str):
        if model not in MODELS:
            raise ValueError(f"unknown model {model!r}: one of {', '.join(MODELS)}")
        return MODELS.index(model)
    m = int(model)
    if not 0 <= m < len(MODELS):
        raise ValueError(f"model id {model} outside 0..{len(MODELS) - 1}")
    return m


# ---- the reference's two kinds of CSV -------------------------------------------------------------------------------------------------
def parse_lut(text: str):
    """load_lut: `#` and header lines skipped, (r_ldr, pump_v) of every other line, sorted."""
    rows = []
    for line in text.splitlines(True):
        if line.startswith("#") or line.startswith("r_ldr"):
            continue
        parts = line.strip().split(",")
        rows.append((float(parts[0]), float(parts[1])))
    rows.sort()
    return np.array([x[0] for x in rows]), np.array([x[1] for x in rows])


def parse_sinusoid(text: str):
    """load_sinusoid: the `sr=` and `freq=` tokens of the `#` lines; sample, r_ldr, pump_v, pair mean per data line."""
    r, pump, pump_pm = [], [], []
    sr = freq = None
    for line in text.splitlines():
        line = line.strip()
        if line.startswith("#"):
            for tok in line.split():
                if tok.startswith("sr="):
                    sr = float(tok[3:])
                elif tok.startswith("freq="):
                    freq = float(tok[5:])
            continue
        if line.startswith("sample"):
            continue
        parts = line.split(",")
        int(parts[0])
        r.append(float(parts[1]))
        pump.append(float(parts[2]))
        pump_pm.append(float(parts[3]))
    return {"sr": sr, "freq": freq, "r": np.array(r), "pump": np.array(pump), "target": np.array(pump_pm)}      # the fit is against the pair mean


def load_lut(path):
    with open(path) as f:
        return parse_lut(f.read())


def load_sinusoid(path):
    with open(path) as f:
        return parse_sinusoid(f.read())


# ---- wavefront packing ----------------------------------------------------------------------------------------------------------------
def pack_waves(trace_idx, model_ids, per_wave=FITS_PER_WAVE):
    """How the library lays work out: a stable sort by (trace, model), then wavefronts of at most `per_wave` items of one (trace, model).
    Returns (order, inverse, waves): order[i] = the caller's index of sorted item i, inverse[order[i]] = i, waves = (trace, model, first,
    count) tuples over the sorted list."""
    trace_idx = np.asarray(trace_idx, dtype=np.int64).ravel()
    model_ids = np.asarray(model_ids, dtype=np.int64).ravel()
    if trace_idx.size != model_ids.size:
        raise ValueError("trace and model lists differ in length")
    order = np.lexsort((np.arange(trace_idx.size), model_ids, trace_idx))
    inverse = np.empty_like(order)
    inverse[order] = np.arange(order.size)
    waves, i = [], 0
    while i < order.size:
        t, m = int(trace_idx[order[i]]), int(model_ids[order[i]])
        j = i
        while j < order.size and j - i < per_wave and trace_idx[order[j]] == t and model_ids[order[j]] == m:
            j += 1
        waves.append((t, m, i, j - i))
        i = j
    return order, inverse, waves


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())


def _stage(traces, lut):
    if not len(traces):
        raise ValueError("no traces")
    rs, ts, offs, rates = [], [], [0], []
    for i, t in enumerate(traces):
        r, y = _f64(t["r"]), _f64(t["target"])
        if r.size != y.size:
            raise ValueError(f"trace {i}: r has {r.size} samples, target {y.size}")
        rs.append(r); ts.append(y); offs.append(offs[-1] + r.size); rates.append(float(t["sr"]))
    lut_r, lut_v = _f64(lut[0]), _f64(lut[1])
    if lut_r.size != lut_v.size:
        raise ValueError(f"the table has {lut_r.size} resistances and {lut_v.size} values")
    return (np.concatenate(rs), np.concatenate(ts), np.asarray(offs, dtype=np.uint64), np.asarray(rates, dtype=np.float64), lut_r, lut_v)


def _items(items, n_traces, what):
    """[(trace, model, parameters)] -> (trace u32, model u32, rows f64 [n][4]); the parameter count must be the model's."""
    tr = np.zeros(len(items), dtype=np.uint32)
    mo = np.zeros(len(items), dtype=np.uint32)
    rows = np.zeros((len(items), 4))
    for i, (t, m, p) in enumerate(items):
        m = model_id(m)
        p = np.asarray(p, dtype=np.float64).ravel()
        if p.size != N_PARAMS[m]:
            raise ValueError(f"{what} {i}: {MODELS[m]} takes {N_PARAMS[m]} parameters, got {p.size}")
        if not 0 <= int(t) < n_traces:
            raise ValueError(f"{what} {i}: trace {t} outside 0..{n_traces - 1}")
        tr[i], mo[i] = int(t), m
        rows[i, :p.size] = p
    return tr, mo, rows


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def evaluate(traces, lut, evals, skip=SKIP, predictions=False, device=0):
    """``ow_pump_fit_eval``: the loss (mV) of every (trace, model, parameters) of `evals`; with predictions also the rows, f64 [n][longest
    trace] (NaN rows for an invalid vector, 0 beyond a trace)."""
    L = load_library()
    r, y, offs, rates, lut_r, lut_v = _stage(traces, lut)
    tr, mo, rows = _items(evals, len(traces), "evaluation")
    loss = np.zeros(len(evals))
    stride = int(np.max(np.diff(offs.astype(np.int64)))) if predictions else 0
    pred = np.zeros((len(evals), stride)) if predictions else None
    check(L, L.ow_pump_fit_eval(_p(r), _p(y), _p(offs), _p(rates), len(traces), _p(lut_r), _p(lut_v), lut_r.size, _p(tr), _p(mo), _p(rows), len(evals),
                                int(skip), int(device), _p(loss), _p(pred) if predictions else None, stride))
    return (loss, pred) if predictions else loss


def fit(traces, lut, fits, xatol=XATOL, fatol=FATOL, maxiter=MAXITER, skip=SKIP, device=0):
    """``ow_pump_fit``: scipy's Nelder-Mead from every (trace, model, x0) of `fits`, all in one call.  Returns a list of dicts: model
    (name), trace, x (list of the model's parameters), fun (mV), nit, nfev, status (CONVERGED / MAXITER_REACHED / START_INVALID)."""
    L = load_library()
    if int(maxiter) < 1:
        raise ValueError("maxiter must be at least 1")
    r, y, offs, rates, lut_r, lut_v = _stage(traces, lut)
    tr, mo, rows = _items(fits, len(traces), "fit")
    n = len(fits)
    x = np.zeros((n, 4))
    fun = np.zeros(n)
    nit, nfev, status = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    check(L, L.ow_pump_fit(_p(r), _p(y), _p(offs), _p(rates), len(traces), _p(lut_r), _p(lut_v), lut_r.size, _p(tr), _p(mo), _p(rows), n, int(skip),
                           float(xatol), float(fatol), int(maxiter), int(device), _p(x), _p(fun), _p(nit), _p(nfev), _p(status)))
    return [{"trace": int(tr[i]), "model": MODELS[mo[i]], "x": x[i, :N_PARAMS[mo[i]]].tolist(), "fun": float(fun[i]), "nit": int(nit[i]),
             "nfev": int(nfev[i]), "status": int(status[i])} for i in range(n)]


def baseline(traces, lut, skip=SKIP, device=0):
    """The cost of doing nothing: the RMSE of the table alone, lut(R) against the target (iir1_dlnR with a = b = 0 adds an exact 0.0)."""
    return evaluate(traces, lut, [(i, "iir1_dlnR", [0.0, 0.0]) for i in range(len(traces))], skip, device=device)


# ---- multi-start ----------------------------------------------------------------------------------------------------------------------
# Where the seeded starts of `grid` are drawn, per model.  Every box lies inside the model's valid region.
#   tau_ms            log-uniform in [0.05, 500] ms
#   a                 1 - a log-uniform in [1e-4, 0.5]                          (a in [0.5, 0.9999])
#   b (iir1_dR)       |b| log-uniform in [1e-9, 1e-4] V / ohm, either sign
#   b (ln R drive)    |b| log-uniform in [1e-3, 10] V per unit of ln R, either sign (b_up, b_dn, b0, b1 independently)
#   a1, a2            a complex pole pair: a1 = 2 rho cos(theta), a2 = -rho^2 with 1 - rho log-uniform in [1e-4, 0.5] and theta
#                     log-uniform in [1e-4, 1] rad
START_BOXES = {"tau_ms": (0.05, 500.0), "one_minus_a": (1e-4, 0.5), "b_dR": (1e-9, 1e-4), "b_dlnR": (1e-3, 10.0), "one_minus_rho": (1e-4, 0.5),
               "theta": (1e-4, 1.0)}


def _log_uniform(rng, box):
    lo, hi = START_BOXES[box]
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _signed(rng, box):
    v = _log_uniform(rng, box)
    return v if rng.random() < 0.5 else -v


def draw_start(model, rng):
    m = model_id(model)
    if m < 2:
        return [_log_uniform(rng, "tau_ms")]
    if m == 2:
        return [1.0 - _log_uniform(rng, "one_minus_a"), _signed(rng, "b_dR")]
    if m == 3:
        return [1.0 - _log_uniform(rng, "one_minus_a"), _signed(rng, "b_dlnR")]
    if m == 4:
        return [1.0 - _log_uniform(rng, "one_minus_a"), _signed(rng, "b_dlnR"), _signed(rng, "b_dlnR")]
    rho, theta = 1.0 - _log_uniform(rng, "one_minus_rho"), _log_uniform(rng, "theta")
    return [2.0 * rho * float(np.cos(theta)), -rho * rho, _signed(rng, "b_dlnR"), _signed(rng, "b_dlnR")]


def grid_starts(model, starts, seed=0):
    """`starts` starts of a model: the reference's x0, then draws from the model's boxes, seeded by (seed, model) alone."""
    m = model_id(model)
    rng = np.random.default_rng([int(seed), m])
    return [list(X0[m])] + [draw_start(m, rng) for _ in range(int(starts) - 1)]


def grid(traces, lut, starts, seed=0, models=MODELS, device=0, **options):
    """`starts` fits per (trace, model) in one call.  Rows in (trace, model, start) order, each the dict of `fit` plus start, x0 and best
    (the lowest fun of its (trace, model); the first of equals)."""
    if int(starts) < 1:
        raise ValueError("starts must be at least 1")
    jobs = [(t, m, x0, k) for t in range(len(traces)) for m in models for k, x0 in enumerate(grid_starts(m, starts, seed))]
    rows = fit(traces, lut, [(t, m, x0) for t, m, x0, _ in jobs], device=device, **options)
    for row, (_, _, x0, k) in zip(rows, jobs):
        row.update(start=k, x0=list(x0), best=False)
    for i in range(0, len(rows), int(starts)):
        min(rows[i:i + int(starts)], key=lambda q: q["fun"])["best"] = True
    return rows


def format_grid_csv(rows, traces) -> str:
    out = io.StringIO()
    w = csv.writer(out)
    w.writerow(["freq", "model", "start", "best", "status", "rmse_mv", "nit", "nfev", "x0", "x"])
    for q in rows:
        w.writerow([traces[q["trace"]].get("freq"), q["model"], q["start"], int(q["best"]), STATUS_NAMES[q["status"]], q["fun"], q["nit"], q["nfev"],
                    " ".join(repr(float(v)) for v in q["x0"]), " ".join(repr(float(v)) for v in q["x"])])
    return out.getvalue()


# ---- the reference's main() -----------------------------------------------------------------------------------------------------------
def analyze(traces, lut, device=0):
    """All traces x the six models from the reference's starts in one ``ow_pump_fit`` call (and one ``ow_pump_fit_eval`` call for the
    baselines).  Rows as the reference's `results`: freq, baseline_mv, <model>_rmse_mv, <model>_params."""
    base = baseline(traces, lut, device=device)
    fits = fit(traces, lut, [(t, m, X0[m]) for t in range(len(traces)) for m in range(len(MODELS))], device=device)
    rows = []
    for t, tr in enumerate(traces):
        row = {"freq": tr.get("freq"), "baseline_mv": float(base[t])}
        for m, name in enumerate(MODELS):
            q = fits[t * len(MODELS) + m]
            row[name + "_rmse_mv"], row[name + "_params"], row[name + "_fit"] = q["fun"], q["x"], q
        rows.append(row)
    return rows


def format_report(lut, rows, results_path) -> str:
    """main()'s stdout, character for character."""
    lut_r, lut_v = np.asarray(lut[0], dtype=np.float64), np.asarray(lut[1], dtype=np.float64)
    out = [f"LUT loaded: {len(lut_r)} points, R ∈ [{lut_r[0]:.0f}, {lut_r[-1]:.0f}] Ω, pump ∈ [{lut_v.min():.3f}, {lut_v.max():.3f}] V", "",
           f"{'freq Hz':>8s}  {'baseline':>10s}  " + "".join(f"{name:>14s}  " for name in MODELS)]
    for r in rows:
        out.append(f"{r['freq']:>7.1f}   {r['baseline_mv']:>10.1f}  " + "".join(f"{r[name + '_rmse_mv']:>14.1f}  " for name in MODELS))
    out += ["", "=== fitted parameters ==="]
    for r in rows:
        out += ["", f"freq = {r['freq']} Hz   (baseline RMSE = {r['baseline_mv']:.1f} mV)"]
        for name in MODELS:
            ps = "  ".join(f"{p:.6e}" for p in r[name + "_params"])
            out.append(f"  {name:>12s}  RMSE = {r[name + '_rmse_mv']:7.2f} mV   params = [{ps}]")
    out += ["", f"Wrote results CSV → {results_path}"]
    return "\n".join(out) + "\n"


def format_results_csv(rows) -> str:
    """main()'s results CSV (csv.writer's text: \\r\\n line ends)."""
    out = io.StringIO()
    w = csv.writer(out)
    w.writerow(["freq", "baseline_mv"] + [name + "_rmse_mv" for name in MODELS])
    for r in rows:
        w.writerow([r["freq"], r["baseline_mv"]] + [r[name + "_rmse_mv"] for name in MODELS])
    return out.getvalue()


def analyze_files(lut=LUT_CSV, sin_dir=SIN_DIR, results=RESULTS_CSV, device=0):
    """The reference's script: its table CSV, every sin_*.csv of its capture directory (sorted by path), its report and results CSV."""
    if not os.path.exists(lut):
        raise FileNotFoundError(f"ERROR: missing {lut}")
    files = sorted(glob.glob(os.path.join(sin_dir, "sin_*.csv")))
    if not files:
        raise FileNotFoundError(f"ERROR: no sin_*.csv in {sin_dir}")
    table = load_lut(lut)
    traces = [load_sinusoid(p) for p in files]
    rows = analyze(traces, table, device)
    text = format_results_csv(rows)
    if results:
        with open(results, "w", newline="") as f:
            f.write(text)
    return {"lut": table, "traces": traces, "rows": rows, "report": format_report(table, rows, results), "csv_text": text, "csv": results}


# ---- --from-device --------------------------------------------------------------------------------------------------------------------
def device_inputs(freqs, ldr_min=19_000.0, ldr_max=1_000_000.0, cycles=10.0, sample_rate=88_200.0, settle=750_000, lut_points=256, lut_settle=60_000,
                  lut_avg=4_096, device=0):
    """The table (``pump.sweep_points`` at the captures' rate) and one capture per frequency (``pump.sinusoid_points``), all through
    ``ow_pump_measure``: one call for the table, one for the captures.  The numbers are the ones the commands' CSV files carry (their
    printed digits), so a fit from here equals the fit of the written files; the texts are returned as `lut_csv` / `sin_csvs`."""
    from . import pump
    lp = pump.sweep_points(1_000.0, 1_000_000.0, lut_points, lut_settle, lut_avg, sample_rate)
    lut_csv = pump.format_sweep_csv(lp["r_settle"], pump.run_points(lp, device))
    pts = np.concatenate([pump.sinusoid_points(ldr_min, ldr_max, f, cycles, sample_rate, settle) for f in freqs])
    _, tr = pump.run_points(pts, device, trace=True)
    sin_csvs, traces = [], []
    for i, f in enumerate(freqs):
        n = int(pts[i]["capture"])
        text = pump.format_sinusoid_csv(pump.sinusoid_resistances(pts[i]), tr[i, :n], ldr_min, ldr_max, f, sample_rate, cycles)
        sin_csvs.append(text)
        traces.append(parse_sinusoid(text))
    return {"lut": parse_lut(lut_csv), "traces": traces, "lut_csv": lut_csv, "sin_csvs": sin_csvs, "points": pts, "raw": tr}


__all__ = ["MODELS", "N_PARAMS", "X0", "SKIP", "XATOL", "FATOL", "MAXITER", "CONVERGED", "MAXITER_REACHED", "START_INVALID", "STATUS_NAMES",
           "FITS_PER_WAVE", "LUT_CSV", "SIN_DIR", "RESULTS_CSV", "START_BOXES", "model_id", "parse_lut", "parse_sinusoid", "load_lut", "load_sinusoid",
           "pack_waves", "evaluate", "fit", "baseline", "draw_start", "grid_starts", "grid", "format_grid_csv", "analyze", "format_report",
           "format_results_csv", "analyze_files", "device_inputs"]
