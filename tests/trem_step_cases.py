"""A corpus of single steps of the Twin-T tremolo oscillator (TremCircuit::process_sample(0.0), gen_tremolo.rs:2353-3116) that takes the
step's solver through everything the settled oscillation never does -- the junction limiter, the 3.5 V step cap, pivots off the usual
order, all fifty sweeps, the backward-Euler retry (converging and exhausted) and the NaN reset -- generated deterministically on the CPU
oracle (fixed seeds, nothing stored).  tests/test_oracle_trem_step_cases.py asserts its coverage on the oracle alone;
tests/test_gpu_trem_step.py takes the kernels' three forms of the step through it.

A case is a state [15] = v_prev[7], i_nl_prev[4], i_nl_prev_prev[4] at a chain rate.  The rates are the chain rates of hosts at 44.1, 48
and 192 kHz, whose matrices are rebuilt, and 48 kHz -- the chain rate of a 24 kHz host -- which is the solver's codegen rate: there the
reference, the oracle and the library copy the baked tables instead (gen_tremolo.rs:2117-2130).
"""
import math

import numpy as np

RATES = (48000.0, 88200.0, 96000.0, 192000.0)
CODEGEN_RATE = 48000.0
N_CLASSES = 10
CLASS_NAMES = ("converged at sweep 0", "converged at sweep 1-5", "converged at sweep 6-49", "retry converged", "retry exhausted", "pivot exchange",
               "singular sweep", "limited by pnjlim", "capped at 3.5 V", "NaN reset")
FAMILIES = ("settled", "growth", "node kick", "current kick", "multi kick", "extrapolation", "edge: convergence", "edge: 1e-4 V threshold",
            "edge: pnjlim", "edge: 3.5 V cap", "extreme")
EDGE_COLUMN = {"edge: convergence": 0, "edge: 1e-4 V threshold": 9, "edge: pnjlim": 7, "edge: 3.5 V cap": 8}     # the info column each edge family straddles
V_KICKS = np.logspace(-6.0, math.log10(40.0), 12)       # volts: one node voltage moved, microvolts to tens of volts
I_KICKS = np.logspace(-9.0, math.log10(4e-2), 12)       # amps: one junction current moved, nanoamps to tens of milliamps
MIN_CLASS = 256                                         # (dk_step_cases.MIN_CLASS)
MIN_COMPARABLE = 64
MAX_ILL_SHARE = 0.10
# the three kicks of test_gpu_trajectory.py::test_row_oscillator_kernels_equal_the_quad_lane_kernels (added to DC_OP, rows 0..14)
TRAJECTORY_KICKS = (np.array([0, 0, 2.0, 0, -1.5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0]),
                    np.array([-6.0, 3.0, 0, 4.0, 5.0, 0, 0.5, 1e-3, -1e-3, 2e-3, 1e-3, 0, 0, 0, 0.0]),
                    np.array([9.0, -9.0, 9.0, -9.0, 9.0, 0, 1.0, 5e-3, 5e-3, -5e-3, 5e-3, -1e-3, 1e-3, 1e-3, -1e-3]))


def dc_op(ob):
    """DC_OP / DC_NL_I as a state row: what the step's own NaN reset leaves (no second copy of the constants)."""
    bad = np.full((1, 15), np.nan)
    so, out, info = ob.trem_step_cases(96000.0, bad)
    assert info[0, 4] == 1 and np.isfinite(so).all()
    return so[0].copy()


class Cases:
    """Parallel arrays of one chain rate's cases."""

    def __init__(self, rate):
        self.rate = rate
        self.states, self.family, self.side = [], [], []

    def add(self, state, family, side=-1):
        self.states.append(np.array(state, dtype=np.float64)); self.family.append(FAMILIES.index(family)); self.side.append(side)

    def freeze(self):
        self.states = np.ascontiguousarray(np.stack(self.states)); self.family = np.array(self.family, dtype=np.int32)
        self.side = np.array(self.side, dtype=np.int32)       # edge families: 0 = the base's side of the decision, 1 = the other side
        self.n = self.states.shape[0]
        return self


def _bisect_edges(ob, rate, bases, rows, mags_hi, family, cs):
    """States on either side of one of the step's decisions: row `row` of a base state is moved, and the moved value is bisected between the
    base's own (info column EDGE_COLUMN[family] as the base has it) and one at which that column is larger, down to NEIGHBOURING doubles of
    the state row; those two and the next three doubles on either side become cases.  Every (base, row, sign, starting magnitude) is tried;
    the ones whose ends differ are kept."""
    col = EDGE_COLUMN[family]
    trials = [(b, r, s * m) for b in bases for r in rows for s in (1.0, -1.0) for m in mags_hi]
    st0 = np.stack([t[0] for t in trials]); row = np.array([t[1] for t in trials]); idx = np.arange(len(trials))
    lo = st0[idx, row].copy(); hi = lo + np.array([t[2] for t in trials])

    def count(x):
        st = st0.copy(); st[idx, row] = x
        return ob.trem_step_cases(rate, st)[2][:, col]
    c0 = count(lo)

    def f(x):
        return count(x) > c0
    ok = f(hi)
    for _ in range(1100):
        mid = 0.5 * (lo + hi)
        stop = (mid == lo) | (mid == hi)
        if stop.all():
            break
        t = f(mid)
        lo = np.where(~t & ~stop, mid, lo); hi = np.where(t & ~stop, mid, hi)
    n_added = 0
    for i in np.nonzero(ok)[0]:
        for side, (x0, away) in enumerate(((lo[i], -math.inf if hi[i] > lo[i] else math.inf), (hi[i], math.inf if hi[i] > lo[i] else -math.inf))):
            x = x0
            for _ in range(4):
                st = st0[i].copy(); st[row[i]] = x
                cs.add(st, family, side); n_added += 1
                x = math.nextafter(x, away)
    return n_added


def _build_rate(ob, rate):
    rng = np.random.default_rng(31337 + int(rate))
    cs = Cases(rate)
    dc = dc_op(ob)
    period = int(rate / 5.6)
    # the growth of the oscillation out of DC_OP (Tremolo::new's two seconds), then one full period of the settled oscillation
    growth = ob.trem_harvest(rate, int(2.0 * rate), int(2.0 * rate) // 48)
    last = ob.trem_harvest(rate, int(2.0 * rate) + 1, int(2.0 * rate))[1]
    settled = ob.trem_harvest(rate, period, max(period // 96, 1), state=last)[:96]
    for s in settled:
        cs.add(s, "settled")
    for s in growth:
        cs.add(s, "growth")
    bases = [settled[i] for i in (0, 12, 24, 36, 48, 60, 72, 84)] + [growth[0], growth[30]]
    # one node voltage moved, log-spaced, both signs, every node (node 5 is the supply: its row is overwritten by the source row)
    for b in bases:
        for node in range(7):
            for sign in (1.0, -1.0):
                for a in V_KICKS:
                    k = b.copy(); k[node] += sign * a
                    cs.add(k, "node kick")
    # one junction current of the previous step moved (it enters the right-hand side AND the extrapolated start)
    for b in bases:
        for j in range(4):
            for sign in (1.0, -1.0):
                for a in I_KICKS:
                    k = b.copy(); k[7 + j] += sign * a
                    cs.add(k, "current kick")
    # several rows at once: the trajectory test's three vectors on DC_OP and on settled states, and random volts / milliamps
    for kick in TRAJECTORY_KICKS:
        cs.add(dc + kick, "multi kick")
        for b in bases[:4]:
            cs.add(b + kick, "multi kick")
    for _ in range(160):
        b = bases[int(rng.integers(len(bases)))].copy()
        scale = 10.0 ** rng.uniform(-3.0, 1.0)
        b[:7] += scale * rng.standard_normal(7) * (rng.random(7) < 0.6)
        b[7:] += 1e-3 * scale * rng.standard_normal(8) * (rng.random(8) < 0.4)
        cs.add(b, "multi kick")
    # i_prev / i_pp pairs whose extrapolated start 2 i_prev - i_pp lies far from the solution while the right-hand side is the base's
    for b in bases[:6]:
        for j in range(4):
            for sign in (1.0, -1.0):
                for a in I_KICKS[3:]:
                    k = b.copy(); k[11 + j] -= sign * a
                    cs.add(k, "extrapolation")
    # states bisected to neighbouring doubles across a decision of the step: the convergence test at sweep 0, the limiter's 1e-4 V
    # threshold, pnjlim's own condition (its logarithm runs), the max_dv > 3.5 cap
    eb = bases[:3]
    for family, rows, mags in (("edge: convergence", (2, 4, 7, 9), (1e-3, 1e-2)),
                               ("edge: 1e-4 V threshold", (0, 2, 4, 8), (1e-3, 1e-2)),
                               ("edge: pnjlim", (2, 4, 0), (0.5, 5.0)),
                               ("edge: 3.5 V cap", (0, 2, 4, 3), (20.0, 40.0))):
        _bisect_edges(ob, rate, eb, rows, mags, family, cs)
    # far outside anything a circuit does, and non-finite: every row of the state in turn
    for b in (dc, settled[0], settled[40]):
        for row in range(15):
            for a in (1e300, -1e300, math.inf, -math.inf, math.nan, 1e308):
                k = b.copy(); k[row] = a
                cs.add(k, "extreme")
    return cs.freeze()


_CORPUS = None


def corpus(ob):
    """{rate: Cases}.  Built once per process."""
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = {rate: _build_rate(ob, rate) for rate in RATES}
    return _CORPUS


def state_row_ok(a, o, floors):
    """The state-row bar, per case: volts (v[7]) within 1e-5 relative + ABS_FLOOR_TREM_STEP_V, amps (i_prev[4], i_pp[4]) within 1e-5
    relative + ABS_FLOOR_TREM_STEP_I.  a, o: [n][15]; floors = (volts, amps)."""
    with np.errstate(invalid="ignore", over="ignore"):
        volts = np.abs(a[:, :7] - o[:, :7]) <= 1e-5 * np.abs(o[:, :7]) + floors[0]
        amps = np.abs(a[:, 7:] - o[:, 7:]) <= 1e-5 * np.abs(o[:, 7:]) + floors[1]
    return volts.all(axis=1) & amps.all(axis=1)


def floor_governed(a, o, floors):
    """(volts, amps): the largest |a - o| over the finite rows whose tolerance in state_row_ok is governed by the floor rather than by the
    relative term (1e-5 |o| < floor) -- what a floor has to cover."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(a - o)
        fin = np.isfinite(a) & np.isfinite(o)
        gv = fin[:, :7] & (1e-5 * np.abs(o[:, :7]) < floors[0])
        ga = fin[:, 7:] & (1e-5 * np.abs(o[:, 7:]) < floors[1])
    return (float(d[:, :7][gv].max()) if gv.any() else 0.0), (float(d[:, 7:][ga].max()) if ga.any() else 0.0)


class Reference:
    """The oracle's results on one rate's cases, the exit classes, and which cases the reference algorithm itself pins."""

    def __init__(self, ob, cs):
        floors = (ob.ABS_FLOOR_TREM_STEP_V, ob.ABS_FLOOR_TREM_STEP_I)
        self.states, self.out, self.info = ob.trem_step_cases(cs.rate, cs.states)
        self.perturbed = [ob.trem_step_cases(cs.rate, cs.states, log_ulp=u) for u in (1, -1)]
        f = self.info
        self.nan_reset = f[:, 4] > 0
        self.finite = np.isfinite(cs.states).all(axis=1) & np.isfinite(self.states).all(axis=1) & np.isfinite(self.out)
        # comparable: finite, and the oracle with pnjlim's logarithm one double away (either way) takes the same exits (retry, converged,
        # reset) and stays within the state-row bar of the unperturbed one (the output is v[OUT], a state row)
        comp = self.finite.copy()
        for sp, op, fp in self.perturbed:
            comp &= state_row_ok(sp, self.states, floors) & (fp[:, [1, 3, 4]] == f[:, [1, 3, 4]]).all(axis=1)
        self.comparable = comp
        self.no_log = f[:, 7] == 0                          # no pnjlim logarithm in the step: nothing but IEEE operations
        m = np.zeros((cs.n, N_CLASSES), dtype=bool)
        trap_ok = (f[:, 1] == 0) & (f[:, 3] == 1)
        m[:, 0] = trap_ok & (f[:, 0] == 0)
        m[:, 1] = trap_ok & (f[:, 0] >= 1) & (f[:, 0] <= 5)
        m[:, 2] = trap_ok & (f[:, 0] >= 6) & (f[:, 0] <= 49)
        m[:, 3] = (f[:, 1] == 1) & (f[:, 3] == 1)
        m[:, 4] = (f[:, 1] == 1) & (f[:, 3] == 0)
        m[:, 5] = f[:, 5] > 0
        m[:, 6] = f[:, 6] > 0
        m[:, 7] = f[:, 7] > 0
        m[:, 8] = f[:, 8] > 0
        m[:, :9] &= ~self.nan_reset[:, None]                # a step that ends in the reset sits in its own class only
        m[:, 9] = self.nan_reset
        self.classes = m


_REFS = None


def references(ob):
    global _REFS
    if _REFS is None:
        _REFS = {rate: Reference(ob, cs) for rate, cs in corpus(ob).items()}
    return _REFS


def coverage(ob):
    """Per exit class over all rates: (name, cases, comparable among them); the finite cases and the non-comparable ones among them."""
    refs = references(ob)
    rows = []
    for c in range(N_CLASSES):
        n = sum(int(r.classes[:, c].sum()) for r in refs.values())
        comp = sum(int((r.classes[:, c] & r.comparable).sum()) for r in refs.values())
        rows.append((CLASS_NAMES[c], n, comp))
    fin = sum(int(r.finite.sum()) for r in refs.values())
    return {"classes": rows, "finite": fin, "ill": fin - sum(int(r.comparable.sum()) for r in refs.values()),
            "cases": sum(r.finite.size for r in refs.values())}
