"""ONE step of the melange 12-node preamp solver at a time, through each device form of it (mel_process, mel_process_lit fast / generic,
mel_process_col fast / generic, the lane-per-engine mel_eng_sample fast / generic: debug hook ow_debug_mel_step) on the corpus of
tests/mel_step_cases.py -- what a musical render never takes: the input clamp, set_runtime_R's clamp, guard and hysteresis, the limiter
and the 0.1 A cap, 265 sweeps, the 55 V ringing test, the backward-Euler fallback, the cooldown that forces it, the voltage-damp net,
the NaN reset.  tests/test_oracle_mel_step_cases.py fixes, on the CPU, which cases the reference algorithm itself pins."""
import ctypes as C

import numpy as np
import pytest

import mel_step_cases as mc
import oracle_binding as ob

pytestmark = pytest.mark.gpu

FORMS = ("mel_process", "mel_process_lit fast", "mel_process_lit generic", "mel_process_col fast", "mel_process_col generic", "mel_eng_sample fast",
         "mel_eng_sample generic")
ASSERTED_EQUAL = ((1, 2), (3, 5), (4, 6), (3, 4))     # lit fast = lit generic (test_melange_literal_fast_path_is_the_generic_rebuild_bit_for_bit), col = eng and
                                                      # generic col = generic eng (ow_melange_eng.h), col fast = col generic (ow_melange_col.h; eng_generic = col in test_melange_lane_engine_kernel_is_bit_identical)
REPORTED = ((1, 3),)                                  # lit against col: both restate invert_n's operations, neither header claims the other's bits


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _step(hiplib, form, rate, states, x, r):
    states = np.ascontiguousarray(states, dtype=np.float64); x = np.ascontiguousarray(x, dtype=np.float64); r = np.ascontiguousarray(r, dtype=np.float64)
    n = states.shape[0]
    so = np.full((n, 21), -7.0); out = np.full(n, -7.0); info = np.full((n, 2), 77, dtype=np.uint32)
    assert hiplib.ow_debug_mel_step(form, C.c_double(rate), _p(states), _p(x), _p(r), n, _p(so), _p(out), _p(info), 0) == 0, hiplib.ow_last_error()
    return so, out, info


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _differ(a, b):
    """Per case: any of the 21 state fields, the output or the two increments differs in its bits."""
    return (_bits(a[0]) != _bits(b[0])).any(axis=1) | (_bits(a[1]) != _bits(b[1])) | (a[2] != b[2]).any(axis=1)


_DEVICE = {}


def _device(hiplib, oracle, rate, form):
    """One form's results on the whole corpus of one rate, in corpus order (computed once, shared, never changed)."""
    if (rate, form) not in _DEVICE:
        cs = mc.corpus(oracle)[rate]
        _DEVICE[(rate, form)] = _step(hiplib, form, rate, cs.states, cs.x, cs.r)
    return _DEVICE[(rate, form)]


def _arrangements(ref, n):
    """Orders of the cases, PAIRS kept together: wavefronts uniform in their exits (pairs sorted by the main's reset, fallback, sweeps,
    limiter and cap counts), wavefronts that mix everything (a fixed shuffle), and a ragged tail (another shuffle cut so that the last
    wavefront of every form is partly filled and the last pair has no shadow)."""
    f = ref.info.astype(np.int64)[0::2]
    npairs = n // 2

    def cases(pairs):
        return np.stack([2 * pairs, 2 * pairs + 1], axis=1).reshape(-1)
    uniform = np.lexsort((np.arange(npairs), f[:, 7], f[:, 6], f[:, 2], f[:, 0], f[:, 1], f[:, 10]))
    return {"uniform": cases(uniform), "mixed": cases(np.random.default_rng(21).permutation(npairs)),
            "ragged": cases(np.random.default_rng(22).permutation(npairs))[: n - 64 - 13]}


def _where(cs, ref, order, pos, form):
    c = int(order[pos])
    return {"rate": cs.rate, "case": c, "family": mc.FAMILIES[cs.family[c]], "info": dict(zip(ob.MEL_INFO, ref.info[c].tolist())), "form": FORMS[form],
            "position": int(pos), "x": float(cs.x[c]), "r": float(cs.r[c]), "state": cs.states[c].tolist()}


def _tame(cs):
    """Cases whose state cannot overflow a right-hand side: the dense generic rebuild multiplies structural zeros of S with it (0 * inf
    is NaN) where the fast paths leave the product out, which the headers' identity claims do not cover."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(cs.states).all(axis=1) & (np.abs(cs.states[:, :19]).max(axis=1) < 1e100)


@pytest.mark.parametrize("rate", mc.RATES)
def test_forms_are_bit_identical_in_every_arrangement(hiplib, oracle, rate):
    """The same 21 state fields, the same output and the same fallback and reset increments, bit for bit (NaN payloads included), for
    every case -- non-comparable and non-finite ones too -- wherever in a wavefront its pair sits and whoever its neighbours are: every
    form against itself across the arrangements, and across forms wherever the code or an existing test claims it.  lit fast / generic,
    col / eng and generic col / generic eng on every case; col fast / generic on every case whose state cannot overflow (see _tame; the
    others are counted).  lit against col is not claimed anywhere: the worst difference is printed."""
    cs, ref = mc.corpus(oracle)[rate], mc.references(oracle)[rate]
    tame = _tame(cs)
    canon = {form: _device(hiplib, oracle, rate, form) for form in range(1, 7)}
    for a, b in ASSERTED_EQUAL:
        bad = _differ(canon[a], canon[b])
        if (a, b) == (3, 4):
            print("\n%g Hz: col fast against col generic differ on %d of %d cases whose state can overflow" % (rate, int((bad & ~tame).sum()), int((~tame).sum())))
            bad &= tame
        bad = np.nonzero(bad)[0]
        assert bad.size == 0, (FORMS[a], FORMS[b], int(bad.size), _where(cs, ref, np.arange(cs.n), bad[0], a), canon[a][0][bad[0]].tolist(), canon[b][0][bad[0]].tolist(),
                               canon[a][2][bad[0]].tolist(), canon[b][2][bad[0]].tolist())
    for a, b in REPORTED:
        with np.errstate(invalid="ignore"):
            d = np.abs(canon[a][0][tame] - canon[b][0][tame])
        print("%g Hz: %s against %s: %d of %d tame cases differ in some bit, worst |difference| %.3e" % (
            rate, FORMS[a], FORMS[b], int((_differ(canon[a], canon[b]) & tame).sum()), int(tame.sum()), float(np.nanmax(d))))
    for name, order in _arrangements(ref, cs.n).items():
        for form in range(1, 7):
            got = _step(hiplib, form, rate, cs.states[order], cs.x[order], cs.r[order])
            want = tuple(a[order] for a in canon[form])
            bad = np.nonzero(_differ(got, want))[0]               # (the ragged tail ends in a main without its shadow)
            assert bad.size == 0, (name, int(bad.size), _where(cs, ref, order, bad[0], form), got[0][bad[0]].tolist(), want[0][bad[0]].tolist())


@pytest.mark.parametrize("n", [1, 2, 3, 63, 65, 129])
def test_tiny_and_ragged_case_counts(hiplib, oracle, n):
    """n that fills no wavefront and, where odd, ends in a main state without its shadow: every form returns what it returns for those
    cases inside the full corpus."""
    rate = 96000.0
    cs = mc.corpus(oracle)[rate]
    pairs = np.random.default_rng(n).permutation(cs.n // 2)[: (n + 1) // 2]
    order = np.stack([2 * pairs, 2 * pairs + 1], axis=1).reshape(-1)[:n]
    for form in range(7):
        full = _device(hiplib, oracle, rate, form)
        got = _step(hiplib, form, rate, cs.states[order], cs.x[order], cs.r[order])
        bad = np.nonzero(_differ(got, tuple(a[order] for a in full)))[0]
        assert bad.size == 0, (n, FORMS[form], bad.tolist())


def _against_oracle(cs, ref, dev, floors, sel, what, exits=True):
    """Asserts the state-row bar (and the exits) on the cases `sel`; returns the per-case absolute errors."""
    so, out, info = dev
    ok = mc.state_row_ok(so, ref.states, floors) & mc.out_ok(out, ref.out, floors)
    with np.errstate(invalid="ignore"):
        err = np.abs(so - ref.states)
    if exits:
        want = np.stack([ref.info[:, 1], ref.info[:, 10]], axis=1).astype(np.uint32)
        bad = np.nonzero(sel & (info != want).any(axis=1))[0]
        assert bad.size == 0, (what, "fallback / reset increments", int(bad.size), _where(cs, ref, np.arange(cs.n), bad[0], 0), info[bad[0]].tolist())
    else:
        with np.errstate(invalid="ignore"):
            ok = (np.abs(so[:, mc.V_ROWS] - ref.states[:, mc.V_ROWS]) <= 1e-5 * np.abs(ref.states[:, mc.V_ROWS]) + floors[0]).all(axis=1) & mc.out_ok(out, ref.out, floors)
    bad = np.nonzero(sel & ~ok)[0]
    assert bad.size == 0, (what, "state-row bar", int(bad.size), _where(cs, ref, np.arange(cs.n), bad[0], 0), (so[bad[0]] - ref.states[bad[0]]).tolist(),
                           ref.states[bad[0]].tolist())
    return err


@pytest.mark.parametrize("rate", mc.RATES)
def test_every_comparable_case_is_the_oracles_step(hiplib, oracle, rate):
    """Every case the reference algorithm pins (CPU: the oracle with pnjlim's logarithm or the rebuilt resistance one double away keeps
    its decisions and stays within the state-row bar), through forms 1 to 6: the twelve v rows and the output within 1e-5 relative +
    ABS_FLOOR_MELANGE_STEP_V, the six junction currents within 1e-5 relative + ABS_FLOOR_MELANGE_STEP_I, input_prev, pot, the cooldown
    and the fallback and reset increments EQUAL.  Only non-comparable cases are excluded.  Form 0, the rank-one update of the nominal
    inverse, is held to the same bar where the resistance is the nominal one, and elsewhere to volts 1e-5 relative +
    ABS_FLOOR_MELANGE_PREAMP (its existing bar: a deliberate deviation), exits not asserted."""
    cs, ref = mc.corpus(oracle)[rate], mc.references(oracle)[rate]
    floors = (oracle.ABS_FLOOR_MELANGE_STEP_V, oracle.ABS_FLOOR_MELANGE_STEP_I)
    m = ref.comparable
    print("\n%g Hz: %d comparable of %d; by class: cases, then per form the worst volt / amp error" % (rate, int(m.sum()), cs.n))
    errs = {}
    failures = []
    for form in range(1, 7):
        try:
            errs[form] = _against_oracle(cs, ref, _device(hiplib, oracle, rate, form), floors, m, FORMS[form])
        except AssertionError as e:
            failures.append(e)
            with np.errstate(invalid="ignore"):
                errs[form] = np.abs(_device(hiplib, oracle, rate, form)[0] - ref.states)
    for c in range(mc.N_CLASSES):
        mcl = m & ref.classes[:, c]
        cells = ["%.1e/%.1e" % (float(errs[f][mcl][:, mc.V_ROWS].max()), float(errs[f][mcl][:, mc.I_ROWS].max())) if mcl.any() else "-" for f in range(1, 7)]
        print("  %-30s %6d  %s" % (mc.CLASS_NAMES[c], int(mcl.sum()), "  ".join(cells)))
    assert not failures, failures[0]
    # form 0
    nominal = m & (ref.states[:, 19] == mc.R_NOM) & (cs.states[:, 19] == mc.R_NOM)
    assert nominal.sum() >= 1024
    dev0 = _device(hiplib, oracle, rate, 0)
    _against_oracle(cs, ref, dev0, floors, nominal, FORMS[0] + " at the nominal resistance")
    # Off the nominal resistance the rank-one form is a deliberate deviation (ow_melange_dev.h: the same mathematics in a shorter operation
    # sequence, up to 1.8e-7 V from the LU at the preamp node) and its exits are not asserted.  A step that takes
    # another exit is another step, so the volt bar is held where the form's own fallback and reset increments are the oracle's, and
    # not on the families bisected to neighbouring doubles across a decision, which only a form that claims the reference's operations
    # can resolve (the damp and convergence decisions leave no trace in the increments).  Both exclusions are counted.
    edge = np.isin(cs.family, [mc.FAMILIES.index(f) for f in mc.EDGE_COLUMN])
    want = np.stack([ref.info[:, 1], ref.info[:, 10]], axis=1).astype(np.uint32)
    same_exit = (dev0[2] == want).all(axis=1)
    off = m & ~nominal
    print("  %s off the nominal resistance: %d comparable cases, %d of them bisected edges, %d others with another fallback / reset exit" % (
        FORMS[0], int(off.sum()), int((off & edge).sum()), int((off & ~edge & ~same_exit).sum())))
    with np.errstate(invalid="ignore"):
        okv = (np.abs(dev0[0][:, mc.V_ROWS] - ref.states[:, mc.V_ROWS]) <= 1e-5 * np.abs(ref.states[:, mc.V_ROWS]) + oracle.ABS_FLOOR_MELANGE_PREAMP).all(axis=1)
    bad = off & ~edge & same_exit & ~okv
    print("  outside the volt bar by family: %s" % {mc.FAMILIES[f]: int((bad & (cs.family == f)).sum()) for f in np.unique(cs.family[bad])})
    assert (off & ~edge & ~same_exit).sum() <= 0.01 * off.sum()
    _against_oracle(cs, ref, dev0, (oracle.ABS_FLOOR_MELANGE_PREAMP, 0.0), off & ~edge & same_exit, FORMS[0] + " off the nominal resistance", exits=False)


def _chain(hiplib, oracle, rate, sel, steps, what):
    """The pairs `sel` (indices of their mains) taken `steps` steps on, each side fed its own output state, inputs and resistances as in
    the first step; forms 1 to 6 held to the single step's bar at every step.  A pair drops out at the step at which the oracle with a
    knob one double away, chained the same way, changes a decision or leaves the bar of the unperturbed one, or at which a state resets
    (the matrices of a pair follow the main's pot; a reset parts the two)."""
    cs = mc.corpus(oracle)[rate]
    floors = (oracle.ABS_FLOOR_MELANGE_STEP_V, oracle.ABS_FLOOR_MELANGE_STEP_I)
    idx = np.stack([sel, sel + 1], axis=1).reshape(-1)
    x, r = cs.x[idx], cs.r[idx]
    dev = {form: cs.states[idx].copy() for form in range(1, 7)}
    cpu = cs.states[idx].copy(); cpu_p = [cpu.copy() for _ in mc.VARIANTS]
    alive = np.ones(idx.size, dtype=bool)
    seen_cd = set()
    for step in range(steps):
        cpu, out_c, info_c = oracle.melange_step_cases(rate, cpu, x, r)
        for k, (lu, ru, rb) in enumerate(mc.VARIANTS):
            cpu_p[k], out_p, info_p = oracle.melange_step_cases(rate, cpu_p[k], x, r, log_ulp=lu, r_ulp=ru, rebuilt=rb)
            alive &= mc.state_row_ok(cpu_p[k], cpu, floors) & mc.out_ok(out_p, out_c, floors) & (info_p[:, mc.DECISIONS] == info_c[:, mc.DECISIONS]).all(axis=1)
        alive &= (info_c[:, 10] == 0) & np.isfinite(cpu).all(axis=1)
        alive = np.repeat(alive.reshape(-1, 2).all(axis=1), 2)
        seen_cd |= set(cpu[alive, 20].tolist())
        want = np.stack([info_c[:, 1], info_c[:, 10]], axis=1).astype(np.uint32)
        for form in range(1, 7):
            dev[form], out_d, info_d = _step(hiplib, form, rate, dev[form], x, r)
            ok = mc.state_row_ok(dev[form], cpu, floors) & mc.out_ok(out_d, out_c, floors) & (info_d == want).all(axis=1)
            bad = np.nonzero(alive & ~ok)[0]
            assert bad.size == 0, (what, step, FORMS[form], int(bad.size), int(idx[bad[0]]), (dev[form][bad[0]] - cpu[bad[0]]).tolist(), cpu[bad[0]].tolist(),
                                   info_d[bad[0]].tolist(), want[bad[0]].tolist())
    print("\n%g Hz, %s: %d pairs chained over %d steps, %d dropped" % (rate, what, sel.size, steps, int((~alive).sum()) // 2))
    assert (~alive).sum() <= mc.MAX_ILL_SHARE * alive.size, (int((~alive).sum()), alive.size)
    return seen_cd


@pytest.mark.parametrize("rate", mc.RATES)
def test_eight_chained_steps(hiplib, oracle, rate):
    """What a step hands to the next one: the pairs whose two cases are comparable and converged in the trapezoidal solve, eight steps."""
    ref = mc.references(oracle)[rate]
    good = ref.comparable & (ref.info[:, 1] == 0) & ~ref.nan_reset
    sel = 2 * np.nonzero(good[0::2] & good[1::2])[0]
    assert sel.size >= 1024
    _chain(hiplib, oracle, rate, sel[:: max(sel.size // 1500, 1)], 8, "convergent pairs")


@pytest.mark.parametrize("rate", (mc.CODEGEN_RATE, 96000.0))
def test_cooldown_is_followed_to_its_end(hiplib, oracle, rate):
    """Pairs whose main starts in a fallback that arms the cooldown (ringing or 265 sweeps), followed for 66 steps: the count-down from 64
    to 0 with its forced backward-Euler steps, the last forced step and the first free one are crossed."""
    ref = mc.references(oracle)[rate]
    armed = ref.comparable & ((ref.info[:, 3] > 0) | (ref.info[:, 4] > 0)) & ~ref.nan_reset
    ok1 = ref.comparable & ~ref.nan_reset
    sel = 2 * np.nonzero(armed[0::2] & ok1[1::2])[0]
    assert sel.size >= 300
    seen = _chain(hiplib, oracle, rate, sel[:: sel.size // 300][:300], 66, "pairs that start in a fallback")
    assert {64.0, 63.0, 1.0, 0.0} <= seen, sorted(seen)
