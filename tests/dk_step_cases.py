"""A corpus of single steps of the legacy DK preamp (DkPreamp::dk_step, dk_preamp_legacy.rs:447-554) that takes the step's Newton loop
through every way it can end -- no update, one to five updates, six updates without convergence, the junction clamp at both edges --
generated deterministically on the CPU oracle (fixed seeds, nothing stored).  tests/test_oracle_dk_step_cases.py asserts its coverage on
the oracle alone; tests/test_gpu_dk_step.py takes the kernels' four forms of the step through it.

A case is (state[14], input, g_ldr, g_ldr_prev) at a chain rate.  Cases come in PAIRS (2k, 2k + 1) = (main, shadow) of one engine that
share g_ldr / g_ldr_prev, which is what dk_step_pair needs; every other form treats the two as independent cases.
"""
import math

import numpy as np

import step_cases as sc

RATES = (88200.0, 96000.0, 192000.0)            # chain rates: hosts at 44.1 kHz and 48 kHz (oversampled), and at 192 kHz
_HOST = {88200.0: 44100.0, 96000.0: 48000.0, 192000.0: 192000.0}
IS, VT, VBE_MAX = 3.03e-14, 0.026, 0.85
N_CLASSES = 9
CLASS_NAMES = ("0 updates", "1 update", "2 updates", "3 updates", "4 updates", "5 updates", "six updates, unconverged", "clamped at 0.85 V",
               "clamped at -1 V")
FAMILIES = ("play", "input", "kick", "g jump", "junction edge", "tolerance edge", "extreme")
KICK_MAGS = np.logspace(-6.0, math.log10(40.0), 20)      # volts: the finite kicks, microvolts to tens of volts
MIN_CLASS = 256
MAX_ILL_SHARE = 0.10
MIN_COMPARABLE = 230


def bjt_ic(v):
    return IS * (math.exp(min(max(v, -1.0), VBE_MAX) / VT) - 1.0)


class Cases(sc.Cases):
    """One chain rate's cases, in (main, shadow) pairs."""
    FAMILIES = FAMILIES
    COLUMNS = ("inputs", "g", "gp")

    def add_pair(self, main, shadow, in_main, in_shadow, g, gp, family):
        fam = FAMILIES.index(family)
        for st, x in ((main, in_main), (shadow, in_shadow)):
            self._rows.append((np.array(st, dtype=np.float64), fam, -1, float(x), float(g), float(gp)))

    def freeze(self):
        super().freeze()
        assert self.n % 2 == 0 and np.array_equal(self.g[0::2], self.g[1::2]) and np.array_equal(self.gp[0::2], self.gp[1::2])
        return self


def last_input(rate, st):
    """The input a state's last step saw, from its capacitor rows: cin_rhs_prev = g_cin x + j_cin' and j_cin = -g_cin (1 + c_cin) (x - v[BASE1])
    - c_cin j_cin' (dk_preamp_legacy.rs:469-471, 544-546) give x = (g_cin (1 + c_cin) v[BASE1] - c_cin cin_rhs_prev - j_cin) / g_cin."""
    alpha = 2.0 * 22000.0 * 0.022e-6 * rate
    g = (2.0 * 0.022e-6 * rate) / (1.0 + alpha); c = (1.0 - alpha) / (1.0 + alpha)
    return (g * (1.0 + c) * st[2] - c * st[1] - st[0]) / g


def _harvest(ob, rate):
    """(main[14], shadow[14], g_ldr) after every block of ordinary play on oracle engines: a chord and its release at tremolo depth 0 and 1 on
    engines as created (their solver states still settle from the 1 MOhm DC point), and at depth 0 after reset() (DC point at the cell's own
    R: the shadow state rests at a fixed point of the step).  Returns (pairs, pairs of the engine at rest)."""
    got, rest = [], []
    for depth, reset in ((0.0, False), (1.0, False), (0.0, True)):
        e = ob.OracleEngine(_HOST[rate])
        e.set_sample_rate(_HOST[rate])
        e.set_tremolo_depth(depth); e.set_volume(0.5)
        e.render(64)
        if reset:
            e.reset()
            e.render(16)
            rest.append((e.preamp_state(False)[:14].copy(), e.preamp_state(True)[:14].copy(), float(e.preamp_ldr()[1])))
        for note in (48, 60, 67):
            e.note_on(note, 0.9)
        for b in range(20):
            if b == 12:
                for note in (48, 60, 67):
                    e.note_off(note)
            e.render(37 if rate < 150000.0 else 149)
            (rest if reset else got).append((e.preamp_state(False)[:14].copy(), e.preamp_state(True)[:14].copy(), float(e.preamp_ldr()[1])))
        e.close()
    return got, rest


def _dc_pair(ob, rate, r):
    """Main and shadow at the DC point of R_ldr = r, as DkState::at_dc builds them (dk_preamp_legacy.rs:241-250) from the oracle's DC node
    voltages: a fixed point of the step at input 0 -- the opening residual is rounding noise and the loop leaves without an update."""
    alpha = 2.0 * 22000.0 * 0.022e-6 * rate
    g_cin = (2.0 * 0.022e-6 * rate) / (1.0 + alpha)
    v = ob.preamp_dc_nodes(rate, r)
    vnl = (v[0] - v[1], v[2] - v[3])
    st = np.concatenate([[g_cin * v[0], g_cin * v[0]], v, [bjt_ic(vnl[0]), bjt_ic(vnl[1])], vnl])
    return (st, st.copy(), 1.0 / r)


def _settle_at(ob, rate, base, r, steps=48):
    """The harvested pairs taken to a static R_ldr = r by the step itself: `steps` steps with a 1 kHz tone on the main state."""
    m = np.stack([b[0] for b in base]); s = np.stack([b[1] for b in base])
    g = np.full(len(base), 1.0 / r)
    for k in range(steps):
        x = 0.03 * math.sin(2.0 * math.pi * 1000.0 * k / rate)
        m = ob.dk_step_cases(rate, m, np.full(len(base), x), g, g)[0]
        s = ob.dk_step_cases(rate, s, np.zeros(len(base)), g, g)[0]
    return [(m[i].copy(), s[i].copy(), 1.0 / r) for i in range(len(base))]


def _tolerance_edges(ob, rate, quiet, cs):
    """Inputs on either side of the step's |f| < 1e-9 test: from a quiet pair (no update at the input the state last saw), the main input is
    bisected between a value that needs no update and one that needs one, down to NEIGHBOURING doubles; those two and the next three
    doubles on either side become cases.  (The residual is a sum of O(1 V) terms: a step of the input's last bit is the finest handle.)"""
    st = np.stack([q[0] for q in quiet]); g = np.array([q[2] for q in quiet]); n = len(quiet)
    upd = lambda x: ob.dk_step_cases(rate, st, x, g, g)[2][:, 0]
    for sign in (1.0, -1.0):
        lo = np.zeros(n); hi = np.full(n, sign * 1e-3)
        ok = (upd(lo) == 0) & (upd(hi) > 0)
        for _ in range(1100):
            mid = 0.5 * (lo + hi)
            stop = (mid == lo) | (mid == hi)
            if stop.all():
                break
            z = upd(mid) == 0
            lo = np.where(z & ~stop, mid, lo); hi = np.where(~z & ~stop, mid, hi)
        for i in np.nonzero(ok)[0]:
            for base_x, away in ((lo[i], 0.0), (hi[i], sign * math.inf)):
                x = base_x
                for _ in range(4):
                    cs.add_pair(quiet[i][0], quiet[i][1], x, 0.0, quiet[i][2], quiet[i][2], "tolerance edge")
                    x = math.nextafter(x, away)


def _build_rate(ob, rate):
    rng = np.random.default_rng(20240 + int(rate))
    cs = Cases(rate)
    play, rest = _harvest(ob, rate)
    rest = [_dc_pair(ob, rate, r) for r in np.logspace(3.0, 6.0, 13)] + rest
    base = rest + play + _settle_at(ob, rate, play[::2], 1000.0) + _settle_at(ob, rate, play[1::2], 1.0e6)     # R at set_ldr_resistance's floor, and dark
    # ordinary play: the state's next step at an input near the one its last step saw (a 50 mV tone at 1 kHz moves by ~3 mV per sample)
    for m, s, g in base:
        x0 = last_input(rate, m)
        for dx in (0.0, 1e-7, -2e-5, 3e-4, -3e-3):
            cs.add_pair(m, s, x0 + dx, 0.0, g, g, "play")
    # inputs from 0 to several volts (a hard strike is an input jump), both signs, shadow mostly at the production 0.0
    for m, s, g in base[::3]:
        for x in (1e-3, 5e-3, 0.02, 0.05, 0.1, 0.2, 0.35, 0.5, 0.8, 1.0, 1.5, 2.0, 3.0, 5.0):
            sg = 1.0 if rng.random() < 0.5 else -1.0
            cs.add_pair(m, s, sg * x, 0.0 if rng.random() < 0.8 else -sg * 0.3 * x, g, g, "input")
    # finite kicks: one node voltage of the main OR the shadow state moved, log-spaced from microvolts to tens of volts, both signs, every node
    mags = KICK_MAGS
    kick_bases = [rest[i] for i in (0, 7, 12, 20)] + [base[i] for i in rng.choice(np.arange(len(rest), len(base)), 6, replace=False)]
    for m, s, g in kick_bases:
        for role in (0, 1):
            for node in range(8):
                for sign in (1.0, -1.0):
                    for a in mags:
                        k = [m.copy(), s.copy()]
                        k[role][2 + node] += sign * a
                        cs.add_pair(k[0], k[1], last_input(rate, m) + float(rng.choice([0.0, 1e-4, 0.02])), 0.0, g, g, "kick")
    # g_ldr != g_ldr_prev: what a depth-knob ramp does per sample (relative steps of 1e-6 .. 1e-1) and what a reset / a depth jump does
    # (between the floor, the dark cell and the state's own)
    for m, s, g in base[::2]:
        for rel in (1e-6, -1e-5, 1e-4, -1e-3, 1e-2, -1e-1, 1e-1):
            cs.add_pair(m, s, last_input(rate, m) + 1e-4, 0.0, g * (1.0 + rel), g, "g jump")
        for g_new, g_old in ((1e-3, g), (1e-6, g), (g, 1e-3), (g, 1e-6), (1e-3, 1e-6), (1e-6, 1e-3)):
            cs.add_pair(m, s, last_input(rate, m) + 1e-4, 0.0, g_new, g_old, "g jump")
    # junction voltages within a few doubles of the clamp's edges, main or shadow, i_nl the junction law at that voltage as in every state
    for m, s, g in base[::12]:
        for role in (0, 1):
            for q in (0, 1):
                for edge in (-1.0, VBE_MAX):
                    for off in (-3, -2, -1, 0, 1, 2, 3):
                        v = edge
                        for _ in range(abs(off)):
                            v = math.nextafter(v, math.inf if off > 0 else -math.inf)
                        k = [m.copy(), s.copy()]
                        k[role][12 + q] = v; k[role][10 + q] = bjt_ic(v)
                        cs.add_pair(k[0], k[1], last_input(rate, m), 0.0, g, g, "junction edge")
    # (a shadow state has seen the input 0.0 all its life: with a steady R_ldr it needs no update at 0.0)
    _tolerance_edges(ob, rate, [(b[1], b[1], b[2]) for b in rest] + [(b[1], b[1], b[2]) for b in base[len(rest)::4]], cs)
    # far outside anything a circuit does: kept for the non-finite label
    for m, s, g in base[:2]:
        for role in (0, 1):
            for node, a in ((0, 1e300), (6, -1e308), (7, 1e306), (3, 1e200)):
                k = [m.copy(), s.copy()]
                k[role][2 + node] = a
                cs.add_pair(k[0], k[1], 0.0, 0.0, g, g, "extreme")
    return cs.freeze()


corpus = sc.cached(lambda ob: {rate: _build_rate(ob, rate) for rate in RATES})        # {rate: Cases}, built once per process
V_ROWS = list(range(2, 10)) + [12, 13]               # v[8], v_nl[2]
I_ROWS = [0, 1, 10, 11]                               # j_cin, cin_rhs_prev, i_nl[2]


def state_row_ok(a, o, ob):
    """The state-row bar of test_preamp_state_rows_are_the_references_fields_in_every_chain_kernel, per case: volts within 1e-5 relative +
    the preamp floor, currents within 1e-5 relative + 1e-12.  a, o: [n][14]."""
    return sc.within_bar(a, o, ((V_ROWS, ob.ABS_FLOOR_PREAMP), (I_ROWS, 1e-12)))


def out_ok(a, o, ob):
    return sc.within_bar(a, o, ((None, ob.ABS_FLOOR_PREAMP),))


class Reference:
    """The oracle's results on one rate's cases, the exit classes, and which cases the reference algorithm itself pins."""

    def __init__(self, ob, cs):
        self.states, self.out, self.info = ob.dk_step_cases(cs.rate, cs.states, cs.inputs, cs.g, cs.gp)
        sp, op, _ = ob.dk_step_cases(cs.rate, cs.states, cs.inputs, cs.g, cs.gp, perturbed=True)
        self.finite = np.isfinite(self.states).all(axis=1) & np.isfinite(self.out)
        # comparable: the one-ulp-exp oracle stays within the state-row bar of the unperturbed one (the output is v[OUT], a state row)
        self.comparable = self.finite & state_row_ok(sp, self.states, ob) & out_ok(op, self.out, ob)
        upd, ex = self.info[:, 0], self.info[:, 1]
        m = np.zeros((cs.n, N_CLASSES), dtype=bool)
        for u in range(6):
            m[:, u] = (upd == u) & (ex == ob.DK_EXIT_CONVERGED)
        m[:, 6] = ex == ob.DK_EXIT_SIX_UPDATES
        m[:, 7] = self.info[:, 3] > 0
        m[:, 8] = self.info[:, 2] > 0
        m &= self.finite[:, None]                       # non-finite results carry their own label and sit in no exit class
        self.classes = m
        self.singular = ex == ob.DK_EXIT_SINGULAR
        self.perturbed_states, self.perturbed_out = sp, op


references = sc.cached(lambda ob: {rate: Reference(ob, cs) for rate, cs in corpus(ob).items()})


def pair_statistics(refs):
    """(pairs whose update counts differ, pairs whose shadow needs more, singular exits) over all rates."""
    return (sum(int((r.info[0::2, 0] != r.info[1::2, 0]).sum()) for r in refs.values()), sum(int((r.info[1::2, 0] > r.info[0::2, 0]).sum()) for r in refs.values()),
            sum(int(r.singular.sum()) for r in refs.values()))
