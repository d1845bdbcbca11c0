"""A corpus of single steps of the melange 12-node preamp solver (set_runtime_R; process_sample, gen_preamp.rs:1973-1984, 3399-3663) that
takes the step through everything a musical render never does -- the input clamp and a non-finite input, set_runtime_R's clamp, guard
and hysteresis, the junction limiter and the 0.1 A cap, all 265 sweeps, the 55 V ringing test, the backward-Euler fallback with its
never-rebuilt tables, the cooldown that forces it, the voltage-damp net, the NaN reset -- generated deterministically on the CPU oracle
(fixed seeds, nothing stored).  tests/test_oracle_mel_step_cases.py asserts its coverage on the oracle alone; tests/test_gpu_mel_step.py
takes the kernels' forms of the step through it.

A case is a state row [21] = v_prev[12], i_nl_prev[3], i_nl_prev_prev[3], input_prev, pot, be_cooldown, an input and a resistance, at a
chain rate.  Cases come in (main, shadow) pairs: case 2k+1 has input 0 and case 2k's resistance and pot -- what one engine's two solver
states can be (melange_adapter.rs:72-86).  The rates are 88.2, 96 and 192 kHz, whose matrices are rebuilt, and 48 kHz, the solver's
codegen rate, where a state that has never seen a resistance runs on the baked tables.
"""
import math

import numpy as np

import step_cases as sc

RATES = (48000.0, 88200.0, 96000.0, 192000.0)
CODEGEN_RATE = 48000.0
R_NOM = 9.99999999999999854e4
CLASS_NAMES = ("converged at sweep 0", "converged at sweep 1-9", "converged at sweep 10-264", "limited by pnjlim", "cut by the 0.1 A cap",
               "singular sweep", "all 265 sweeps", "ringing beyond 55 V", "forced by the cooldown", "fallback converged", "fallback exhausted",
               "damped", "NaN reset", "input clamped or non-finite", "resistance clamped", "resistance ignored", "matrices rebuilt")
N_CLASSES = len(CLASS_NAMES)
SINGULAR = CLASS_NAMES.index("singular sweep")
FAMILIES = ("base", "node kick", "current kick", "multi kick", "input", "cooldown", "resistance", "edge: ringing", "edge: damp",
            "edge: 1e-4 V threshold", "edge: convergence", "extreme")
EDGE_COLUMN = {"edge: ringing": 4, "edge: damp": 9, "edge: 1e-4 V threshold": 12, "edge: convergence": 0}   # the info column each edge family straddles
V_KICKS = np.logspace(-6.0, math.log10(80.0), 12)       # volts: one node moved, microvolts to beyond the 55 V ringing test
I_KICKS = np.logspace(-9.0, 0.0, 12)                    # amps: one junction current moved, nanoamps to an ampere
INPUTS = (1e-6, 1e-4, 1e-2, 0.3, 2.0, 10.0, 60.0, 99.0, 100.0, 100.00000000000001, 101.0, 150.0, 1e3, 1e6, 1e300, math.inf)
COOLDOWNS = (0, 1, 2, 63, 64)
R_OUTSIDE = (-5.0, 0.0, 1.0, 500.0, 999.9999999999999, 1000000.0000000001, 1.5e6, 5e6, 1e300)     # below 1 kOhm / above 1 MOhm: clamped
R_INSIDE = (1000.0, 1900.0, 19000.0, 100001.0, 470000.0, 1e6)
R_NONFINITE = (math.inf, -math.inf, math.nan)
MIN_CLASS = 256                                         # (dk_step_cases.MIN_CLASS)
MIN_COMPARABLE = 64
MAX_ILL_SHARE = 0.10
V_ROWS = slice(0, 12)
I_ROWS = slice(12, 18)
DECISIONS = (1, 3, 4, 5, 10, 13)                         # info columns of the fallback, reset and cooldown decisions: fallback taken, nr_failed,
                                                        # ringing (either sets the cooldown), forced, NaN reset, the fallback's solve exhausted


class Cases(sc.Cases):
    """One chain rate's cases, in pair order."""
    FAMILIES = FAMILIES
    COLUMNS = ("x", "r")

    def add(self, state, family, x=0.0, r=None, side=-1):
        super().add(state, family, side, x=x, r=state[19] if r is None else r)

    def freeze(self):
        """Pairs: single i is main 2i; its shadow 2i+1 is the state of the next single of the same family (its own for an edge family, so
        that the bisected state stays what it is) with the main's pot and resistance, and input 0."""
        singles = self._rows         # (state, family, side, x, r); side on mains only
        by_family = {}
        for i, s in enumerate(singles):
            by_family.setdefault(s[1], []).append(i)
        nxt = {}
        for fam, idx in by_family.items():
            edge = FAMILIES[fam].startswith("edge")
            for k, i in enumerate(idx):
                nxt[i] = i if edge else idx[(k + 1) % len(idx)]
        self._rows = []
        for i, (s, f, sd, xi, ri) in enumerate(singles):
            sh = singles[nxt[i]][0].copy(); sh[19] = s[19]
            self._rows += [(s, f, sd, xi, ri), (sh, f, -1, 0.0, ri)]
        return super().freeze()


def _build_rate(ob, rate):
    rng = np.random.default_rng(52525 + int(rate))
    cs = Cases(rate)
    # base states: the settled state; an overdriven run (2 V at 1 kHz into an input that clips at tens of millivolts); a depth-1 tremolo
    # run (the Twin-T's resistance over one period, a 50 mV tone)
    settled = ob.melange_harvest(rate, 1, 1)[0][0]
    n_od = int(rate * 0.004)
    od = ob.melange_harvest(rate, n_od, max(n_od // 48, 1), x=2.0 * np.sin(2.0 * math.pi * 1000.0 * np.arange(n_od) / rate))[0][:48]
    n_tr = int(rate / 5.6)
    r_tr = np.zeros(n_tr)
    ob.lib().owo_tremolo_run(ob.C.c_double(1.0), ob.C.c_double(rate if rate >= 88200.0 else 96000.0), ob._p(r_tr), ob.C.c_size_t(n_tr))
    tr = ob.melange_harvest(rate, n_tr, max(n_tr // 48, 1), x=0.05 * np.sin(2.0 * math.pi * 440.0 * np.arange(n_tr) / rate), r=r_tr)[0][:48]
    cs.add(settled, "base")
    for s in od:
        cs.add(s, "base", x=0.01)
    for s in tr:
        cs.add(s, "base", r=float(s[19]) * 1.001)
    bases = [settled, od[5], od[17], od[29], tr[7], tr[31]]
    # one node moved, log-spaced, both signs, every node (row 11 is the supply source's row)
    for b in bases[:5]:
        for node in range(12):
            for sign in (1.0, -1.0):
                for a in V_KICKS:
                    k = b.copy(); k[node] += sign * a
                    cs.add(k, "node kick")
    # one junction current of the previous step or of the one before (they enter the right-hand side and the extrapolated start)
    for b in bases:
        for j in range(6):
            for sign in (1.0, -1.0):
                for a in I_KICKS:
                    k = b.copy(); k[12 + j] += sign * a
                    cs.add(k, "current kick")
    # several rows at once, with an input and a resistance of their own
    for _ in range(320):
        b = bases[int(rng.integers(len(bases)))].copy()
        scale = 10.0 ** rng.uniform(-3.0, 1.3)
        b[:12] += scale * rng.standard_normal(12) * (rng.random(12) < 0.5)
        b[12:18] += 1e-3 * scale * rng.standard_normal(6) * (rng.random(6) < 0.4)
        b[18] = float(rng.choice((0.0, 0.01, -0.3)))
        cs.add(b, "multi kick", x=float(rng.choice((0.0, 0.02, -1.0, 30.0))), r=float(rng.choice(R_INSIDE)))
    # inputs from microvolts to beyond the +-100 V clamp, and non-finite ones; input_prev follows for half of them
    for b in bases:
        for a in INPUTS:
            for sign in (1.0, -1.0):
                cs.add(b, "input", x=sign * a)
                k = b.copy(); k[18] = sign * min(a, 100.0) * 0.9
                cs.add(k, "input", x=sign * a)
        cs.add(b, "input", x=math.nan)
    # the cooldown: every count on convergent states, on mild kicks and on kicks that ring
    for b in bases:
        for cd in COOLDOWNS:
            for node, a in ((4, 0.0), (4, 1e-3), (2, 0.05), (8, -0.5), (5, 3.0), (10, 70.0), (6, -60.0)):
                k = b.copy(); k[node] += a; k[20] = float(cd)
                cs.add(k, "cooldown", x=0.01 if node == 4 else 0.0)
    # resistances: outside the clamp range, non-finite, inside it, and within / just beyond 1e-12 of pot (at a pot of a few kOhm, where
    # doubles are finer than the hysteresis; at 100 kOhm the neighbouring doubles are already beyond it)
    for b in bases:
        for r in R_OUTSIDE + R_NONFINITE + R_INSIDE:
            cs.add(b, "resistance", x=0.01, r=r)
        for pot in (1000.0, 1500.0, 3000.0, 7000.0):
            k = b.copy(); k[19] = pot
            ulp = math.ulp(pot)
            for m in (0, 1, 2, 4, 8):
                for sign in (1.0, -1.0):
                    cs.add(k, "resistance", r=pot + sign * m * ulp)
            for d in (0.999e-12, 1e-12, 1.001e-12, 1.2e-12, 2e-12):
                for sign in (1.0, -1.0):
                    cs.add(k, "resistance", r=pot + sign * d)
        for pot in (R_NOM, float(tr[20][19])):
            k = b.copy(); k[19] = pot
            for r in (pot, math.nextafter(pot, math.inf), math.nextafter(pot, -math.inf)):
                cs.add(k, "resistance", r=r)
    # states bisected to neighbouring doubles across a decision of the step: the 55 V ringing test, the damp threshold, the limiter's
    # 1e-4 V threshold, convergence at sweep 0
    eb = [settled, tr[7]]
    for family, rows, mags in (("edge: ringing", (2, 4, 5, 8, 10), (80.0, 300.0)),
                               ("edge: damp", (2, 4, 5, 8, 10), (10.0, 40.0)),
                               ("edge: 1e-4 V threshold", (2, 4, 12, 13, 14), (1e-3, 1e-2)),
                               ("edge: convergence", (2, 4, 5, 13, 14), (1e-3, 1e-2))):
        for st, side in sc.bisect_edges(lambda s: ob.melange_step_cases(rate, s, np.zeros(len(s)), s[:, 19])[2][:, EDGE_COLUMN[family]], eb, rows, mags):
            cs.add(st, family, side=side)
    # far outside anything a circuit does, and non-finite: every row of the state but the cooldown in turn
    for b in (settled, od[17]):
        for row in range(20):
            for a in (1e300, -1e300, math.inf, -math.inf, math.nan, 1e308):
                k = b.copy(); k[row] = a
                cs.add(k, "extreme")
    return cs.freeze()


corpus = sc.cached(lambda ob: {rate: _build_rate(ob, rate) for rate in RATES})        # {rate: Cases}, built once per process


def state_row_ok(a, o, ob):
    """The state-row bar, per case: the twelve v rows within 1e-5 relative + ABS_FLOOR_MELANGE_STEP_V, the six junction-current rows
    within 1e-5 relative + ABS_FLOOR_MELANGE_STEP_I, and input_prev, pot and the cooldown EQUAL.  a, o: [n][21]."""
    return sc.within_bar(a, o, ((V_ROWS, ob.ABS_FLOOR_MELANGE_STEP_V), (I_ROWS, ob.ABS_FLOOR_MELANGE_STEP_I))) & (a[:, 18:] == o[:, 18:]).all(axis=1)


def out_ok(a, o, ob):
    return sc.within_bar(a, o, ((None, ob.ABS_FLOOR_MELANGE_STEP_V),))


# The oracle's perturbed variants: the four one-double moves, and -- what differs only at the codegen rate and the nominal pot -- the
# rebuilt tables in place of the baked ones.  Which of the two such a state runs on is history that a state row does not carry (the
# reference leaves the baked tables at its first resistance and never returns), the two differ by up to 4.7e-13 of the largest entry
# (DESIGN.md section 2), and the literal device forms always rebuild: a case is pinned only where both agree.
VARIANTS = ({"log_ulp": 1}, {"log_ulp": -1}, {"r_ulp": 1}, {"r_ulp": -1}, {"rebuilt": True})


class Reference:
    """The oracle's results on one rate's cases, the exit classes, and which cases the reference algorithm itself pins."""

    def __init__(self, ob, cs):
        self.states, self.out, self.info = ob.melange_step_cases(cs.rate, cs.states, cs.x, cs.r)
        self.perturbed = [ob.melange_step_cases(cs.rate, cs.states, cs.x, cs.r, **v) for v in VARIANTS]
        f = self.info
        self.nan_reset = f[:, 10] > 0
        # finite: the state going in and everything coming out (a non-finite input or resistance is one of the step's guarded exits)
        self.finite = np.isfinite(cs.states).all(axis=1) & np.isfinite(self.states).all(axis=1) & np.isfinite(self.out)
        # comparable: finite, and the oracle with pnjlim's logarithm or the rebuilt resistance one double away (either way) takes the same
        # fallback, reset and cooldown decisions and stays within the state-row bar of the unperturbed one
        comp = self.finite.copy()
        self.keeps = self.finite.copy()
        for sp, op, fp in self.perturbed:
            same = (fp[:, DECISIONS] == f[:, DECISIONS]).all(axis=1)
            self.keeps &= same
            comp &= same & state_row_ok(sp, self.states, ob) & out_ok(op, self.out, ob)
        self.comparable = comp
        m = np.zeros((cs.n, N_CLASSES), dtype=bool)
        trap_kept = f[:, 1] == 0
        m[:, 0] = trap_kept & (f[:, 0] == 1)
        m[:, 1] = trap_kept & (f[:, 0] >= 2) & (f[:, 0] <= 10)
        m[:, 2] = trap_kept & (f[:, 0] >= 11)
        m[:, 3] = f[:, 6] > 0
        m[:, 4] = f[:, 7] > 0
        m[:, 5] = f[:, 8] > 0
        m[:, 6] = f[:, 3] > 0
        m[:, 7] = f[:, 4] > 0
        m[:, 8] = f[:, 5] > 0
        m[:, 9] = (f[:, 1] > 0) & (f[:, 13] == 0)
        m[:, 10] = f[:, 13] > 0
        m[:, 11] = f[:, 9] > 0
        with np.errstate(invalid="ignore"):
            m[:, 13] = ~(np.abs(cs.x) <= 100.0)
            m[:, 14] = np.isfinite(cs.r) & ((cs.r < 1000.0) | (cs.r > 1000000.0))
            m[:, 15] = ~np.isfinite(cs.r) | (np.abs(np.clip(cs.r, 1000.0, 1000000.0) - cs.states[:, 19]) < 1e-12)
        m[:, 16] = f[:, 11] > 0
        m[:, :12] &= ~self.nan_reset[:, None]                # a step that ends in the reset sits in its own class (and its input / resistance ones)
        m[:, 12] = self.nan_reset
        self.classes = m


references = sc.cached(lambda ob: {rate: Reference(ob, cs) for rate, cs in corpus(ob).items()})
