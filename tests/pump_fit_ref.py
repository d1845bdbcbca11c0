"""Restatement of tools/analyze_pump_dynamics.py (the reference's pump-dynamics fitter) and of the Nelder-Mead it calls, in plain loops:
the six predictors R(t) -> pump(t), the log-R table lookup, the loss, and scipy's non-adaptive Nelder-Mead.

Stated from the mathematics, one IEEE operation per statement where the order matters:

  lookup      numpy.interp on ln(clip(x, r[0], r[-1])) over ln(r): left of the table v[0], right of it and on its last knot v[-1], on a knot
              v[j], else slope * (x - x[j]) + v[j] with slope = (v[j+1] - v[j]) / (x[j+1] - x[j]).
  lpf_R       s[0] = R[0]; s[n] = s[n-1] + a (R[n] - s[n-1]); pred = lookup(s);        a = 1 - exp(-1 / (sr tau_ms 1e-3)); tau_ms <= 0: invalid
  lpf_lnR     the same on ln R, pred = lookup(exp(s))
  iir1_dR     xi[0] = 0; xi[n] = a xi[n-1] + b (R[n] - R[n-1]); pred = lookup(R) + xi;  a outside [0, 1): invalid
  iir1_dlnR   the same driven by ln R[n] - ln R[n-1]
  iir1_asym   the same with b = b_up where the drive is positive, b_dn elsewhere
  iir2_dlnR   xi[0] = xi[1] = 0; xi[n] = ((a1 xi[n-1] + a2 xi[n-2]) + b0 u[n]) + b1 u[n-1], u[0] = 0, u[n] = ln R[n] - ln R[n-1];
              invalid unless both roots of z^2 - a1 z - a2 lie inside the unit circle (real pair: both |z| < 1; complex pair: sqrt(-a2) < 1)
  loss        1e9 for an invalid vector or a prediction that is not finite at every sample (the skipped ones included), else
              1000 sqrt(mean(d d)) over samples skip..n.  `loss` sums as numpy's mean does (pairwise); `loss_sequential` in sample order, as
              the device does.
  Nelder-Mead scipy.optimize's `_minimize_neldermead` with its defaults (rho 1, chi 2, psi = sigma = 0.5, start simplex 1.05 x / 0.00025),
              a stable ordering, maxfun unbounded.

`ulp_nudge` moves every exp / log result by one ulp (the experiment that sets the floors of tests/test_gpu_pump_fit.py).
"""
import math

import numpy as np

MODELS = ("lpf_R", "lpf_lnR", "iir1_dR", "iir1_dlnR", "iir1_asym", "iir2_dlnR")
N_PARAMS = (1, 1, 2, 2, 3, 4)
X0 = ([50.0], [50.0], [0.999, 1e-6], [0.999, -1.0], [0.999, -1.0, 1.0], [1.99, -0.99, -1.0, 0.5])
SKIP = 200
INVALID_LOSS = 1e9
CONVERGED, MAXITER, START_INVALID = 0, 1, 2      # include/openwurli_hip.h: ow_pump_fit's status codes

_NUDGE = 0      # 0: the library's exp / log; +1 / -1: every result moved one ulp up / down


class ulp_nudge:
    def __init__(self, direction):
        self.direction = direction

    def __enter__(self):
        global _NUDGE
        self.saved, _NUDGE = _NUDGE, self.direction

    def __exit__(self, *exc):
        global _NUDGE
        _NUDGE = self.saved


def _nudged(v):
    if _NUDGE == 0 or not math.isfinite(v):
        return v
    return math.nextafter(v, math.inf if _NUDGE > 0 else -math.inf)


def _exp(x):
    try:
        return _nudged(math.exp(x))
    except OverflowError:
        return math.inf


def _log(x):
    if x != x:
        return x
    if x == 0.0:
        return -math.inf
    if x < 0.0:
        return math.nan
    if x == math.inf:
        return x
    return _nudged(math.log(x))


class Table:
    """The static pump table: strictly ascending r, its logarithms and slopes."""

    def __init__(self, r, v):
        self.r = [float(x) for x in r]
        self.v = [float(x) for x in v]
        self.ln = [_log(x) for x in self.r]
        self.slope = [(self.v[j + 1] - self.v[j]) / (self.ln[j + 1] - self.ln[j]) for j in range(len(self.r) - 1)]

    def __call__(self, x):
        r, v, ln = self.r, self.v, self.ln
        if x != x:
            return x
        c = r[0] if x < r[0] else (r[-1] if x > r[-1] else x)
        lx = _log(c)
        if lx > ln[-1]:
            return v[-1]
        if lx < ln[0]:
            return v[0]
        lo, hi = 0, len(ln) - 1                  # the last j with ln[j] <= lx
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if ln[mid] <= lx:
                lo = mid
            else:
                hi = mid - 1
        j = lo
        if j == len(ln) - 1 or ln[j] == lx:
            return v[j]
        out = self.slope[j] * (lx - ln[j]) + v[j]
        if out != out:
            out = self.slope[j] * (lx - ln[j + 1]) + v[j + 1]
            if out != out and v[j] == v[j + 1]:
                out = v[j]
        return out


def _lpf_coeff(sr, tau_ms):
    return 1.0 - _exp(-1.0 / (sr * tau_ms * 1e-3))


def valid(model, p):
    """The reference's guards: False where it returns a row of NaN without running."""
    if model in (0, 1):
        return not (p[0] <= 0)
    if model in (2, 3, 4):
        return bool(0 <= p[0] < 1)
    a1, a2 = p[0], p[1]
    disc = a1 * a1 + 4 * a2
    if disc >= 0:
        z1 = 0.5 * (a1 + math.sqrt(disc))
        z2 = 0.5 * (a1 - math.sqrt(disc))
        return not (abs(z1) >= 1 or abs(z2) >= 1)
    mag = math.sqrt(-a2) if -a2 >= 0 else math.nan
    return not (mag >= 1)


class Problem:
    """One trace against one table: what every evaluation shares (ln R and the table's value at R)."""

    def __init__(self, R, sr, target, table, skip=SKIP):
        self.R = [float(x) for x in R]
        self.sr = float(sr)
        self.target = None if target is None else [float(x) for x in target]
        self.table = table
        self.skip = skip
        self.ln = [_log(x) for x in self.R]
        self.base = [table(x) for x in self.R]

    def predict(self, model, p):
        """The prediction row (list of floats); a row of NaN for an invalid vector."""
        R, ln, base, table = self.R, self.ln, self.base, self.table
        n = len(R)
        p = [float(x) for x in p]
        if not valid(model, p):
            return [math.nan] * n
        out = [0.0] * n
        if model == 0:
            a = _lpf_coeff(self.sr, p[0])
            s = R[0]
            out[0] = table(s)
            for k in range(1, n):
                s = s + a * (R[k] - s)
                out[k] = table(s)
        elif model == 1:
            a = _lpf_coeff(self.sr, p[0])
            s = ln[0]
            out[0] = table(_exp(s))
            for k in range(1, n):
                s = s + a * (ln[k] - s)
                out[k] = table(_exp(s))
        elif model == 2:
            a, b = p
            xi = 0.0
            out[0] = base[0] + xi
            for k in range(1, n):
                xi = a * xi + b * (R[k] - R[k - 1])
                out[k] = base[k] + xi
        elif model == 3:
            a, b = p
            xi = 0.0
            out[0] = base[0] + xi
            for k in range(1, n):
                xi = a * xi + b * (ln[k] - ln[k - 1])
                out[k] = base[k] + xi
        elif model == 4:
            a, b_up, b_dn = p
            xi = 0.0
            out[0] = base[0] + xi
            for k in range(1, n):
                du = ln[k] - ln[k - 1]
                xi = a * xi + (b_up if du > 0 else b_dn) * du
                out[k] = base[k] + xi
        else:
            a1, a2, b0, b1 = p
            x1 = x2 = 0.0
            out[0] = base[0] + 0.0
            if n > 1:
                out[1] = base[1] + 0.0
            for k in range(2, n):
                u1 = ln[k - 1] - ln[k - 2]
                xi = a1 * x1 + a2 * x2 + b0 * (ln[k] - ln[k - 1]) + b1 * u1
                x2, x1 = x1, xi
                out[k] = base[k] + xi
        return out

    def loss(self, model, p, sequential=False):
        return loss(self.predict(model, p), self.target, self.skip, sequential)


def predict(model, R, sr, p, table):
    return Problem(R, sr, None, table).predict(model, p)


def loss(pred, target, skip=SKIP, sequential=False):
    """1e9 unless the whole row is finite; else 1000 sqrt(mean(d d)) over skip..n."""
    if not all(math.isfinite(x) for x in pred):
        return INVALID_LOSS
    with np.errstate(all="ignore"):
        d = np.asarray(pred[skip:], dtype=np.float64) - np.asarray(target[skip:], dtype=np.float64)
        dd = d * d
        if sequential:
            acc = 0.0
            for x in dd.tolist():
                acc = acc + x
            return 1000.0 * math.sqrt(acc / len(dd))
        return float(1000.0 * np.sqrt(np.mean(dd)))


def loss_sequential(pred, target, skip=SKIP):
    return loss(pred, target, skip, sequential=True)


def make_loss(model, R, sr, target, table, skip=SKIP, sequential=False):
    prob = Problem(R, sr, target, table, skip)
    return lambda p: prob.loss(model, p, sequential)


def start_simplex(x0):
    x0 = [float(x) for x in x0]
    sim = [list(x0)]
    for k in range(len(x0)):
        y = list(x0)
        y[k] = (1 + 0.05) * y[k] if y[k] != 0 else 0.00025
        sim.append(y)
    return sim


def _fmax(values):
    """np.max: a NaN wins."""
    m = values[0]
    for v in values[1:]:
        if v != v or v > m:
            m = v
    return m


def nelder_mead(func, x0, xatol=1e-6, fatol=1e-6, maxiter=5000):
    """scipy.optimize.minimize(func, x0, method="Nelder-Mead", options=dict(xatol, fatol, maxiter)): x, fun, nit, nfev, status."""
    N = len(x0)
    sim = start_simplex(x0)
    fsim = [func(v) for v in sim]
    nfev = N + 1
    start_invalid = all(f == INVALID_LOSS for f in fsim)

    def order():
        ind = sorted(range(N + 1), key=lambda i: fsim[i])          # stable; every loss is a number (inf at the worst)
        return [sim[i] for i in ind], [fsim[i] for i in ind]

    sim, fsim = order()
    it = 1
    converged = False
    with np.errstate(all="ignore"):
        while it < maxiter:
            dx = _fmax([abs(sim[i][k] - sim[0][k]) for i in range(1, N + 1) for k in range(N)])
            df = _fmax([abs(float(np.float64(fsim[0]) - np.float64(fsim[i]))) for i in range(1, N + 1)])
            if dx <= xatol and df <= fatol:
                converged = True
                break
            xbar = []
            for k in range(N):
                s = sim[0][k]
                for i in range(1, N):
                    s = s + sim[i][k]
                xbar.append(s / N)
            last = sim[-1]
            xr = [2.0 * xbar[k] - 1.0 * last[k] for k in range(N)]
            fxr = func(xr)
            nfev += 1
            shrink = False
            if fxr < fsim[0]:
                xe = [3.0 * xbar[k] - 2.0 * last[k] for k in range(N)]
                fxe = func(xe)
                nfev += 1
                if fxe < fxr:
                    sim[-1], fsim[-1] = xe, fxe
                else:
                    sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-2]:
                sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-1]:
                xc = [1.5 * xbar[k] - 0.5 * last[k] for k in range(N)]
                fxc = func(xc)
                nfev += 1
                if fxc <= fxr:
                    sim[-1], fsim[-1] = xc, fxc
                else:
                    shrink = True
            else:
                xcc = [0.5 * xbar[k] + 0.5 * last[k] for k in range(N)]
                fxcc = func(xcc)
                nfev += 1
                if fxcc < fsim[-1]:
                    sim[-1], fsim[-1] = xcc, fxcc
                else:
                    shrink = True
            if shrink:
                for j in range(1, N + 1):
                    sim[j] = [sim[0][k] + 0.5 * (sim[j][k] - sim[0][k]) for k in range(N)]
                    fsim[j] = func(sim[j])
                    nfev += 1
            it += 1
            sim, fsim = order()
    # scipy reports success when the simplex of a start that never left the invalid region has shrunk below xatol; START_INVALID names it
    status = START_INVALID if start_invalid and fsim[0] == INVALID_LOSS else (CONVERGED if converged else MAXITER)
    return {"x": list(sim[0]), "fun": fsim[0], "nit": it, "nfev": nfev, "status": status}


def fit(model, R, sr, target, table, x0=None, xatol=1e-6, fatol=1e-6, maxiter=5000, skip=SKIP, sequential=False):
    return nelder_mead(make_loss(model, R, sr, target, table, skip, sequential), X0[model] if x0 is None else x0, xatol, fatol, maxiter)


# ---- the fixture of tests/golden/pump_fit_golden.json ---------------------------------------------------------------------------------
FIXTURE_SR = 88200.0
FIXTURE_TRACES = ((700, 600.0, 4, (0.99, -0.05, 0.02)), (1200, 300.0, 1, (0.4,)), (2048, 150.0, 5, (1.9, -0.905, -0.04, 0.03)))
FIXTURE_R = (19_000.0, 1_000_000.0)


def fixture_table():
    r = np.exp(np.linspace(np.log(1e3), np.log(1e6), 32))
    v = 2.0 + 1.5 * np.tanh((np.log(r) - 11.0) / 1.5)
    return r, v


def fixture_resistance(n, f, sr=FIXTURE_SR):
    ln_mid = 0.5 * (math.log(FIXTURE_R[1]) + math.log(FIXTURE_R[0]))
    ln_amp = 0.5 * (math.log(FIXTURE_R[1]) - math.log(FIXTURE_R[0]))
    k = np.arange(n)
    return np.exp(ln_mid + ln_amp * np.cos(2.0 * np.pi * f * k / sr))


def fixture_noise(n):
    return 2e-4 * np.random.default_rng(n).standard_normal(n)


def fixture_lut_csv(r, v):
    """The table as `pump-sweep` writes it (full precision, so that reading it back gives the same numbers)."""
    return "\n".join(["r_ldr,pump_v,pump_std,pump_min,pump_max"] + [f"{float(a)!r},{float(b)!r},0.0,{float(b)!r},{float(b)!r}" for a, b in zip(r, v)]) + "\n"


def fixture_sin_name(freq):
    return f"sin_{int(round(freq * 10)):05d}.csv"


def fixture_sin_csv(r, target, freq, sr):
    """A capture as `pump-sinusoid` writes it: the header's freq= and sr= tokens, the pair-mean column last (the fit's target)."""
    head = [f"# pump-sinusoid  ldr_min={FIXTURE_R[0]:.6e}  ldr_max={FIXTURE_R[1]:.6e}  freq={freq:.6f}  sr={sr:.0f}  cycles=1", "sample,r_ldr,pump_v,pump_avg2"]
    return "\n".join(head + [f"{i},{float(a)!r},{float(b)!r},{float(b)!r}" for i, (a, b) in enumerate(zip(r, target))]) + "\n"
