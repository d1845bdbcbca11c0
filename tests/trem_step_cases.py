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

import step_cases as sc

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
VARIANTS = ({"log_ulp": 1}, {"log_ulp": -1})            # the oracle's perturbed variants: pnjlim's logarithm one double away, either way
DECISIONS = [1, 3, 4]                                   # info columns of the exits a perturbed oracle has to keep: retry taken, converged, NaN reset
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


class Cases(sc.Cases):
    FAMILIES = FAMILIES


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
        for st, side in sc.bisect_edges(lambda s: ob.trem_step_cases(rate, s)[2][:, EDGE_COLUMN[family]], eb, rows, mags):
            cs.add(st, family, side)
    # far outside anything a circuit does, and non-finite: every row of the state in turn
    for b in (dc, settled[0], settled[40]):
        for row in range(15):
            for a in (1e300, -1e300, math.inf, -math.inf, math.nan, 1e308):
                k = b.copy(); k[row] = a
                cs.add(k, "extreme")
    return cs.freeze()


corpus = sc.cached(lambda ob: {rate: _build_rate(ob, rate) for rate in RATES})        # {rate: Cases}, built once per process
V_ROWS = slice(0, 7)
I_ROWS = slice(7, 15)


def groups(ob):
    """The state-row bar's groups: volts (v[7]) within 1e-5 relative + ABS_FLOOR_TREM_STEP_V, amps (i_prev[4], i_pp[4]) within 1e-5
    relative + ABS_FLOOR_TREM_STEP_I."""
    return ((V_ROWS, ob.ABS_FLOOR_TREM_STEP_V), (I_ROWS, ob.ABS_FLOOR_TREM_STEP_I))


def state_row_ok(a, o, ob):
    return sc.within_bar(a, o, groups(ob))


def out_ok(a, o, ob):
    return sc.within_bar(a, o, ((None, ob.ABS_FLOOR_TREM_STEP_V),))


def floor_governed(a, o, ob):
    """(volts, amps): what the two floors have to cover (step_cases.floor_governed)."""
    return sc.floor_governed(a, o, groups(ob))


class Reference:
    """The oracle's results on one rate's cases, the exit classes, and which cases the reference algorithm itself pins."""

    def __init__(self, ob, cs):
        self.states, self.out, self.info = ob.trem_step_cases(cs.rate, cs.states)
        self.perturbed = [ob.trem_step_cases(cs.rate, cs.states, **v) for v in VARIANTS]
        f = self.info
        self.nan_reset = f[:, 4] > 0
        self.finite = np.isfinite(cs.states).all(axis=1) & np.isfinite(self.states).all(axis=1) & np.isfinite(self.out)
        # comparable: finite, and the oracle with pnjlim's logarithm one double away (either way) takes the same exits (retry, converged,
        # reset) and stays within the state-row bar of the unperturbed one (the output is v[OUT], a state row)
        comp = self.finite.copy()
        for sp, op, fp in self.perturbed:
            comp &= state_row_ok(sp, self.states, ob) & (fp[:, DECISIONS] == f[:, DECISIONS]).all(axis=1)
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


references = sc.cached(lambda ob: {rate: Reference(ob, cs) for rate, cs in corpus(ob).items()})
