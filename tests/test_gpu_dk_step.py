"""ONE step of the legacy DK preamp at a time, through each of the kernels' four forms of it (dk_step, dk_step_pair, dk_step_wide,
dk_step_row: debug hook ow_debug_dk_step) on the corpus of tests/dk_step_cases.py -- the exits of the Newton loop that musical play
never takes: no update, six updates without convergence, the junction clamp at both edges, main and shadow states of a lane that need
different numbers of updates.  Long traces of an overdriven preamp are chaotic; one step from a common state is not: a difference is a
difference in the step.  tests/test_oracle_dk_step_cases.py fixes, on the CPU, which cases the reference algorithm itself pins; the
test bodies are tests/step_gpu.py's."""
import functools

import numpy as np
import pytest

import dk_step_cases as dk
import step_cases as sc
import step_gpu as sg

pytestmark = pytest.mark.gpu


def _sort_keys(ref):
    """Pairs sorted by their update counts: the ballot ends the loop early, or never."""
    um, us = ref.info[0::2, 0].astype(np.int64), ref.info[1::2, 0].astype(np.int64)
    return ref.info[0::2, 1].astype(np.int64), np.minimum(um, us), np.maximum(um, us)


# The ragged tail is cut to an odd number of cases: a last wavefront, quad and row partly filled, a last lane with a main state only.
SOLVER = sg.Solver(name="dk", mod=dk, forms=("dk_step", "dk_step_pair", "dk_step_wide", "dk_step_row"),
                   info_names=("updates", "exit", "clamped at -1 V", "clamped at 0.85 V"), outputs=(((14,), -7.0, np.float64), ((), -7.0, np.float64)),
                   oracle=lambda ob, rate, *args, **variant: ob.dk_step_cases(rate, *args, **variant), variants=({"perturbed": True},), decisions=[],
                   reset=None, exits=None, held=range(4), against=0, sort_keys=_sort_keys, unit=2, seeds=(11, 12), ragged_cut=lambda n: n - 2 * 37 - 1,
                   convergent=lambda ob, ref: ref.comparable & (ref.info[:, 1] == ob.DK_EXIT_CONVERGED))


@functools.lru_cache(maxsize=None)
def _call(hiplib):
    return sg.hook_call(hiplib.ow_debug_dk_step, hiplib.ow_last_error)


@pytest.mark.parametrize("rate", dk.RATES)
def test_four_forms_are_bit_identical_in_every_arrangement(hiplib, oracle, rate):
    """The same fourteen fields and the same output, bit for bit (NaN payloads included: the arrays are compared as integers), from all
    four forms, for every case of the corpus -- ill-conditioned and non-finite ones too -- wherever in a wavefront it sits and whoever its
    neighbours are.  A frozen lane that still moves, a pair loop that stops when one of its states is done, a different update cap in
    one form: each shows here as a case whose bits depend on the form or on the arrangement."""
    sg.assert_arrangements_bit_identical(SOLVER, _call(hiplib), oracle, rate)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 65, 129])
def test_tiny_and_ragged_case_counts(hiplib, oracle, n):
    """n that fills no wavefront, quad, row or pair: every form returns what the lane form returns for those cases inside the full corpus."""
    sg.assert_subset_is_the_corpus(SOLVER, _call(hiplib), oracle, 96000.0, n)


@pytest.mark.parametrize("rate", dk.RATES)
def test_every_comparable_case_is_the_oracles_step(hiplib, oracle, rate):
    """Every case the reference algorithm pins (CPU: one-ulp-exp oracle within the state-row bar) is within that bar of the oracle's step:
    volts 1e-5 relative + ABS_FLOOR_PREAMP, currents 1e-5 relative + 1e-12, the output as the node voltage it is.  No other exclusion."""
    cs, ref = dk.corpus(oracle)[rate], dk.references(oracle)[rate]
    dev = sg.canonical(SOLVER, _call(hiplib), oracle, rate, 0)
    m, err = ref.comparable, sg.errors(dev, ref)
    print("\n%g Hz: %d comparable of %d; worst volt error %.3e, worst current error %.3e; by class (cases, worst volt error):" % (
        rate, int(m.sum()), cs.n, float(err[m][:, dk.V_ROWS].max()), float(err[m][:, dk.I_ROWS].max())))
    sg.class_table(SOLVER, ref, m, lambda mc: "%.3e" % (float(err[mc][:, dk.V_ROWS].max()) if mc.any() else 0.0))
    sg.against_oracle(SOLVER, oracle, cs, ref, dev, m, "dk_step")
    # the same decisions: a comparable case left the loop after the oracle's number of updates unless its residual sat on the tolerance
    # (not asserted per case: the device's exponential differs from glibc's in the last place, which is what `comparable` allows for)


def _device_ic(hiplib, vnl):
    """IS (exp(clamp(v) / VT) - 1) with the kernels' own exponential (ow_debug_unary, which = 0); clamp, division and the rest are IEEE
    operations that numpy repeats bit for bit (tests/test_gpu_division.py pins the kernels' constant division to IEEE)."""
    x = np.ascontiguousarray(np.clip(vnl, -1.0, dk.VBE_MAX).ravel() / dk.VT)
    f = np.zeros_like(x); lib = np.zeros_like(x)
    assert hiplib.ow_debug_unary(0, sc.ptr(x), x.size, sc.ptr(f), sc.ptr(lib), 0) == 0
    return (dk.IS * (f - 1.0)).reshape(vnl.shape)


@pytest.mark.parametrize("rate", dk.RATES)
def test_carried_evaluation_is_the_junction_law_at_v_nl(hiplib, oracle, rate):
    """dk_step carries its last junction evaluation out of the Newton loop in place of the reference's bjt_ic(v_nl) after it
    (ow_chain_dev.h: "whichever way a lane left: converged, singular 2x2, six updates").  After every step with a finite result, in every
    form: i_nl[q] == IS (exp(clamp(v_nl[q]) / VT) - 1) bit for bit, with the kernels' own exponential.  The claim is inductive -- a step
    that takes no update hands its input's i_nl on -- so the states go in as the kernels would hold them: i_nl formed from v_nl by the
    device's junction law (an oracle state's i_nl is glibc's, one unit in the last place away here and there)."""
    cs, ref = dk.corpus(oracle)[rate], dk.references(oracle)[rate]
    states = cs.states.copy()
    states[:, 10:12] = _device_ic(hiplib, states[:, 12:14])
    for form in range(4):
        so, out = SOLVER.step(_call(hiplib), form, rate, states, cs.inputs, cs.g, cs.gp)
        fin = np.isfinite(so).all(axis=1) & np.isfinite(out)
        assert fin.sum() >= 0.99 * cs.n
        want = _device_ic(hiplib, so[fin][:, 12:14])
        bad = np.nonzero((sc.bits(so[fin][:, 10:12]) != sc.bits(want)).any(axis=1))[0]
        assert bad.size == 0, (int(bad.size), sg.where(SOLVER, cs, ref, np.nonzero(fin)[0], bad[0], form), so[fin][bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("rate", dk.RATES)
def test_eight_chained_steps(hiplib, oracle, rate):
    """What a step hands to the next one: the comparable, convergent cases of the corpus taken eight steps on, each side fed its own
    output state (g_ldr_prev = g_ldr from the second step, as process_sample leaves it), every form.  The bar is the single step's.  A case
    drops out at the step at which the one-ulp-exp oracle, chained the same way, leaves the bar of the unperturbed one; at most 10 % may."""
    ref = dk.references(oracle)[rate]
    sel = sc.cases_of(sc.whole_units(SOLVER.convergent(oracle, ref), 2), 2)       # whole (main, shadow) pairs: the pair form steps both
    assert sel.size >= 4096
    alive = sg.chain(SOLVER, _call(hiplib), oracle, rate, sel, 8, "convergent pairs", after=lambda step, res, alive, rest: (rest[0], rest[1], rest[1]))
    print("\n%g Hz: %d cases chained, %d dropped as ill-conditioned" % (rate, sel.size, int((~alive).sum())))
