"""ONE step of the Twin-T tremolo oscillator at a time, through each of the kernels' three forms of it (trem_osc_step, trem_osc_step_wide,
trem_osc_step_row: debug hook ow_debug_trem_step) on the corpus of tests/trem_step_cases.py -- what the settled oscillation never takes:
the junction limiter, the 3.5 V cap, pivots off the usual order, fifty sweeps, the backward-Euler retry, the NaN reset.  A kicked
oscillator is chaotic over a block; one step from a common state is not: a difference is a difference in the step.
tests/test_oracle_trem_step_cases.py fixes, on the CPU, which cases the reference algorithm itself pins; the test bodies are
tests/step_gpu.py's."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import step_cases as sc
import step_gpu as sg
import trem_step_cases as tc

pytestmark = pytest.mark.gpu


def _sort_keys(ref):
    """Cases sorted by reset, retry, sweeps, limiter and cap counts: the wave-wide ballots of the limiter, the pivot scan and the cap see
    agreeing lanes."""
    f = ref.info.astype(np.int64)
    return f[:, 8], f[:, 7], f[:, 2], f[:, 0], f[:, 1], f[:, 4]


# The device reports the fallback counter's increment.  The ragged tail leaves the last wavefront and the last quad partly filled.
SOLVER = sg.Solver(name="trem", mod=tc, forms=("trem_osc_step", "trem_osc_step_wide", "trem_osc_step_row"), info_names=ob.TREM_INFO,
                   outputs=(((15,), -7.0, np.float64), ((), -7.0, np.float64), ((), 77, np.uint64)),
                   oracle=lambda ob, rate, *args, **variant: ob.trem_step_cases(rate, *args, **variant), variants=tc.VARIANTS, decisions=tc.DECISIONS,
                   reset=4, exits=lambda info: info[:, 1].astype(np.uint64), held=range(3), against=0, sort_keys=_sort_keys, unit=1, seeds=(21, 22),
                   ragged_cut=lambda n: n - 64 - 13, convergent=lambda ob, ref: ref.comparable & (ref.info[:, 3] == 1) & ~ref.nan_reset)


@functools.lru_cache(maxsize=None)
def _call(hiplib):
    return sg.hook_call(hiplib.ow_debug_trem_step, hiplib.ow_last_error)


@pytest.mark.parametrize("rate", tc.RATES)
def test_three_forms_are_bit_identical_in_every_arrangement(hiplib, oracle, rate):
    """The same fifteen rows, the same output and the same fallback increment, bit for bit (NaN payloads included: the arrays are compared
    as integers), from all three forms, for every case of the corpus -- ill-conditioned and non-finite ones too -- wherever in a wavefront
    it sits and whoever its neighbours are.  The lane form's limiter divisions run only when some lane of the wavefront was limited, its
    pivot scan only when some lane disagrees with the usual order; the row form computes with zero coefficients where the others skip a
    term and redoes a sweep that trips a trigger: each shows here as a case whose bits depend on the form or on the arrangement."""
    sg.assert_arrangements_bit_identical(SOLVER, _call(hiplib), oracle, rate)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 15, 17, 63, 65])
def test_tiny_and_ragged_case_counts(hiplib, oracle, n):
    """n that fills no wavefront or quad: every form returns what the lane form returns for those cases inside the full corpus."""
    sg.assert_subset_is_the_corpus(SOLVER, _call(hiplib), oracle, 96000.0, n)


@pytest.mark.parametrize("rate", tc.RATES)
def test_every_comparable_case_is_the_oracles_step(hiplib, oracle, rate):
    """Every case the reference algorithm pins (CPU: the oracle with pnjlim's logarithm one double away keeps its exits and stays within the
    state-row bar) takes the oracle's exits -- the same increment of the fallback counter, the same NaN-reset outcome -- and is within
    that bar of the oracle's step: volts 1e-5 relative + ABS_FLOOR_TREM_STEP_V, amps 1e-5 relative + ABS_FLOOR_TREM_STEP_I, the output as
    the node voltage it is.  A case whose oracle step ran no pnjlim logarithm consists of IEEE operations only, and the kernels claim the
    oracle's bits (ow_trem_wide.h, ow_trem_row.h): those must be EQUAL, rows, output and all.  Non-finite states (in no class, not
    comparable) must still end in the reset, as the oracle's do."""
    cs, ref = tc.corpus(oracle)[rate], tc.references(oracle)[rate]
    dev = sg.canonical(SOLVER, _call(hiplib), oracle, rate, 0)
    so, out, info = dev
    m, err = ref.comparable, sg.errors(dev, ref)
    print("\n%g Hz: %d comparable of %d (%d of them without a logarithm); by class: cases, worst volt error, worst amp error" % (
        rate, int(m.sum()), cs.n, int((m & ref.no_log).sum())))
    sg.class_table(SOLVER, ref, m, lambda mc: "%.3e  %.3e" % ((float(err[mc][:, tc.V_ROWS].max()), float(err[mc][:, tc.I_ROWS].max())) if mc.any() else (0.0, 0.0)))
    sg.against_oracle(SOLVER, oracle, cs, ref, dev, m, "trem_osc_step")
    dc = tc.dc_op(oracle)
    is_reset = (sc.bits(so) == sc.bits(dc)[None, :]).all(axis=1) & (sc.bits(out) == sc.bits(dc[:1])[0])
    bad = np.nonzero((m | ~np.isfinite(cs.states).all(axis=1)) & (is_reset != ref.nan_reset))[0]
    assert bad.size == 0, ("NaN reset", int(bad.size), sg.where(SOLVER, cs, ref, np.arange(cs.n), bad[0], 0), so[bad[0]].tolist())
    exact = m & ref.no_log
    bad = np.nonzero(exact & ((sc.bits(so) != sc.bits(ref.states)).any(axis=1) | (sc.bits(out) != sc.bits(ref.out))))[0]
    assert bad.size == 0, ("bit identity without a logarithm", int(bad.size), int(exact.sum()), sg.where(SOLVER, cs, ref, np.arange(cs.n), bad[0], 0),
                           (so[bad[0]] - ref.states[bad[0]]).tolist())


@pytest.mark.parametrize("rate", tc.RATES)
def test_eight_chained_steps(hiplib, oracle, rate):
    """What a step hands to the next one: the comparable cases that converged (in the trapezoidal solve or in the retry) taken eight steps
    on, each side fed its own output state, every form.  The bar is the single step's.  A case drops out at the step at which the oracle
    with the logarithm one double away, chained the same way, changes an exit or leaves the bar of the unperturbed one; at most 10 % may."""
    ref = tc.references(oracle)[rate]
    sel = np.nonzero(SOLVER.convergent(oracle, ref))[0]
    assert sel.size >= 2048
    alive = sg.chain(SOLVER, _call(hiplib), oracle, rate, sel, 8, "converged cases")
    print("\n%g Hz: %d cases chained, %d dropped as ill-conditioned" % (rate, sel.size, int((~alive).sum())))
