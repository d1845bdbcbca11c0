"""ONE step of the melange 12-node preamp solver at a time, through each device form of it (mel_process, mel_process_lit fast / generic,
mel_process_col fast / generic, the lane-per-engine mel_eng_sample fast / generic: debug hook ow_debug_mel_step) on the corpus of
tests/mel_step_cases.py -- what a musical render never takes: the input clamp, set_runtime_R's clamp, guard and hysteresis, the limiter
and the 0.1 A cap, 265 sweeps, the 55 V ringing test, the backward-Euler fallback, the cooldown that forces it, the voltage-damp net,
the NaN reset.  tests/test_oracle_mel_step_cases.py fixes, on the CPU, which cases the reference algorithm itself pins; the test bodies
are tests/step_gpu.py's."""
import functools

import numpy as np
import pytest

import mel_step_cases as mc
import oracle_binding as ob
import step_cases as sc
import step_gpu as sg

pytestmark = pytest.mark.gpu

ASSERTED_EQUAL = ((1, 2), (3, 5), (4, 6), (3, 4))     # lit fast = lit generic (test_melange_literal_fast_path_is_the_generic_rebuild_bit_for_bit), col = eng and
                                                      # generic col = generic eng (ow_melange_eng.h), col fast = col generic (ow_melange_col.h; eng_generic = col in test_melange_lane_engine_kernel_is_bit_identical)
REPORTED = ((1, 3),)                                  # lit against col: both restate invert_n's operations, neither header claims the other's bits


def _sort_keys(ref):
    """Pairs sorted by the main's reset, fallback, sweeps, limiter and cap counts."""
    f = ref.info.astype(np.int64)[0::2]
    return f[:, 7], f[:, 6], f[:, 2], f[:, 0], f[:, 1], f[:, 10]


# The device reports the fallback and reset increments.  Form 0, the rank-one update of the nominal inverse, is a deliberate deviation
# and is not held to the oracle's step off the nominal resistance.  The ragged tail leaves the last wavefront of every form partly
# filled and ends in a main without its shadow.
SOLVER = sg.Solver(name="mel", mod=mc, forms=("mel_process", "mel_process_lit fast", "mel_process_lit generic", "mel_process_col fast", "mel_process_col generic",
                                              "mel_eng_sample fast", "mel_eng_sample generic"), info_names=ob.MEL_INFO,
                   outputs=(((21,), -7.0, np.float64), ((), -7.0, np.float64), ((2,), 77, np.uint32)),
                   oracle=lambda ob, rate, *args, **variant: ob.melange_step_cases(rate, *args, **variant), variants=mc.VARIANTS, decisions=list(mc.DECISIONS),
                   reset=10, exits=lambda info: np.stack([info[:, 1], info[:, 10]], axis=1).astype(np.uint32), held=range(1, 7), against=None,
                   sort_keys=_sort_keys, unit=2, seeds=(21, 22), ragged_cut=lambda n: n - 64 - 13,
                   convergent=lambda ob, ref: ref.comparable & (ref.info[:, 1] == 0) & ~ref.nan_reset)
FORMS = SOLVER.forms


@functools.lru_cache(maxsize=None)
def _call(hiplib):
    return sg.hook_call(hiplib.ow_debug_mel_step, hiplib.ow_last_error)


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
    canon = {form: sg.canonical(SOLVER, _call(hiplib), oracle, rate, form) for form in range(1, 7)}
    for a, b in ASSERTED_EQUAL:
        bad = SOLVER.differ(canon[a], canon[b])
        if (a, b) == (3, 4):
            print("\n%g Hz: col fast against col generic differ on %d of %d cases whose state can overflow" % (rate, int((bad & ~tame).sum()), int((~tame).sum())))
            bad &= tame
        bad = np.nonzero(bad)[0]
        assert bad.size == 0, (FORMS[a], FORMS[b], int(bad.size), sg.where(SOLVER, cs, ref, np.arange(cs.n), bad[0], a), canon[a][0][bad[0]].tolist(),
                               canon[b][0][bad[0]].tolist(), canon[a][2][bad[0]].tolist(), canon[b][2][bad[0]].tolist())
    for a, b in REPORTED:
        with np.errstate(invalid="ignore"):
            d = np.abs(canon[a][0][tame] - canon[b][0][tame])
        print("%g Hz: %s against %s: %d of %d tame cases differ in some bit, worst |difference| %.3e" % (
            rate, FORMS[a], FORMS[b], int((SOLVER.differ(canon[a], canon[b]) & tame).sum()), int(tame.sum()), float(np.nanmax(d))))
    sg.assert_arrangements_bit_identical(SOLVER, _call(hiplib), oracle, rate)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 65, 129])
def test_tiny_and_ragged_case_counts(hiplib, oracle, n):
    """n that fills no wavefront and, where odd, ends in a main state without its shadow: every form returns what it returns for those
    cases inside the full corpus."""
    sg.assert_subset_is_the_corpus(SOLVER, _call(hiplib), oracle, 96000.0, n)


@pytest.mark.parametrize("rate", mc.RATES)
def test_every_comparable_case_is_the_oracles_step(hiplib, oracle, rate):
    """Every case the reference algorithm pins (CPU: the oracle with pnjlim's logarithm or the rebuilt resistance one double away keeps
    its decisions and stays within the state-row bar), through forms 1 to 6: the twelve v rows and the output within 1e-5 relative +
    ABS_FLOOR_MELANGE_STEP_V, the six junction currents within 1e-5 relative + ABS_FLOOR_MELANGE_STEP_I, input_prev, pot, the cooldown
    and the fallback and reset increments EQUAL.  Only non-comparable cases are excluded.  Form 0, the rank-one update of the nominal
    inverse, is held to the same bar where the resistance is the nominal one, and elsewhere to volts 1e-5 relative +
    ABS_FLOOR_MELANGE_PREAMP (its existing bar: a deliberate deviation), exits not asserted."""
    cs, ref = mc.corpus(oracle)[rate], mc.references(oracle)[rate]
    m = ref.comparable
    dev = {form: sg.canonical(SOLVER, _call(hiplib), oracle, rate, form) for form in range(7)}
    errs = {form: sg.errors(dev[form], ref) for form in range(1, 7)}
    print("\n%g Hz: %d comparable of %d; by class: cases, then per form the worst volt / amp error" % (rate, int(m.sum()), cs.n))
    sg.class_table(SOLVER, ref, m, lambda mcl: "  ".join("%.1e/%.1e" % (float(errs[f][mcl][:, mc.V_ROWS].max()), float(errs[f][mcl][:, mc.I_ROWS].max())) if mcl.any() else "-"
                                                         for f in range(1, 7)), width=30)
    for form in range(1, 7):
        sg.against_oracle(SOLVER, oracle, cs, ref, dev[form], m, FORMS[form], form)
    # form 0
    nominal = m & (ref.states[:, 19] == mc.R_NOM) & (cs.states[:, 19] == mc.R_NOM)
    assert nominal.sum() >= 1024
    sg.against_oracle(SOLVER, oracle, cs, ref, dev[0], nominal, FORMS[0] + " at the nominal resistance")
    # Off the nominal resistance the rank-one form is a deliberate deviation (ow_melange_dev.h: the same mathematics in a shorter operation
    # sequence, up to 1.8e-7 V from the LU at the preamp node) and its exits are not asserted.  A step that takes
    # another exit is another step, so the volt bar is held where the form's own fallback and reset increments are the oracle's, and
    # not on the families bisected to neighbouring doubles across a decision, which only a form that claims the reference's operations
    # can resolve (the damp and convergence decisions leave no trace in the increments).  Both exclusions are counted.
    edge = np.isin(cs.family, [mc.FAMILIES.index(f) for f in mc.EDGE_COLUMN])
    same_exit = (dev[0][2] == SOLVER.exits(ref.info)).all(axis=1)
    off = m & ~nominal
    print("  %s off the nominal resistance: %d comparable cases, %d of them bisected edges, %d others with another fallback / reset exit" % (
        FORMS[0], int(off.sum()), int((off & edge).sum()), int((off & ~edge & ~same_exit).sum())))
    floor0 = oracle.ABS_FLOOR_MELANGE_PREAMP
    bad = off & ~edge & same_exit & ~sc.within_bar(dev[0][0], ref.states, ((mc.V_ROWS, floor0),))
    print("  outside the volt bar by family: %s" % {mc.FAMILIES[f]: int((bad & (cs.family == f)).sum()) for f in np.unique(cs.family[bad])})
    assert (off & ~edge & ~same_exit).sum() <= 0.01 * off.sum()
    sg.against_oracle(SOLVER, oracle, cs, ref, dev[0], off & ~edge & same_exit, FORMS[0] + " off the nominal resistance", exits=False,
                      bar=lambda got, want: sc.within_bar(got[0], want[0], ((mc.V_ROWS, floor0),)) & sc.within_bar(got[1], want[1], ((None, floor0),)))


def _chain(hiplib, oracle, rate, sel, steps, what):
    """The pairs `sel` taken `steps` steps on (step_gpu.chain, pairwise: the matrices of a pair follow the main's pot; a reset parts the
    two), forms 1 to 6.  Returns the cooldown values the oracle's states took while alive."""
    seen_cd = set()
    alive = sg.chain(SOLVER, _call(hiplib), oracle, rate, sc.cases_of(sel, 2), steps, what, pairwise=True,
                     after=lambda step, res, alive, rest: seen_cd.update(res[0][alive, 20].tolist()))
    print("\n%g Hz, %s: %d pairs chained over %d steps, %d dropped" % (rate, what, sel.size, steps, int((~alive).sum()) // 2))
    return seen_cd


@pytest.mark.parametrize("rate", mc.RATES)
def test_eight_chained_steps(hiplib, oracle, rate):
    """What a step hands to the next one: the pairs whose two cases are comparable and converged in the trapezoidal solve, eight steps."""
    ref = mc.references(oracle)[rate]
    sel = sc.whole_units(SOLVER.convergent(oracle, ref), 2)
    assert sel.size >= 1024
    _chain(hiplib, oracle, rate, sel[:: max(sel.size // 1500, 1)], 8, "convergent pairs")


@pytest.mark.parametrize("rate", (mc.CODEGEN_RATE, 96000.0))
def test_cooldown_is_followed_to_its_end(hiplib, oracle, rate):
    """Pairs whose main starts in a fallback that arms the cooldown (ringing or 265 sweeps), followed for 66 steps: the count-down from 64
    to 0 with its forced backward-Euler steps, the last forced step and the first free one are crossed."""
    ref = mc.references(oracle)[rate]
    armed = ref.comparable & ((ref.info[:, 3] > 0) | (ref.info[:, 4] > 0)) & ~ref.nan_reset
    ok1 = ref.comparable & ~ref.nan_reset
    sel = np.nonzero(armed[0::2] & ok1[1::2])[0]
    assert sel.size >= 300
    seen = _chain(hiplib, oracle, rate, sel[:: sel.size // 300][:300], 66, "pairs that start in a fallback")
    assert {64.0, 63.0, 1.0, 0.0} <= seen, sorted(seen)
