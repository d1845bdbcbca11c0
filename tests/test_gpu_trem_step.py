"""ONE step of the Twin-T tremolo oscillator at a time, through each of the kernels' three forms of it (trem_osc_step, trem_osc_step_wide,
trem_osc_step_row: debug hook ow_debug_trem_step) on the corpus of tests/trem_step_cases.py -- what the settled oscillation never takes:
the junction limiter, the 3.5 V cap, pivots off the usual order, fifty sweeps, the backward-Euler retry, the NaN reset.  A kicked
oscillator is chaotic over a block; one step from a common state is not: a difference is a difference in the step.
tests/test_oracle_trem_step_cases.py fixes, on the CPU, which cases the reference algorithm itself pins."""
import ctypes as C

import numpy as np
import pytest

import trem_step_cases as tc

pytestmark = pytest.mark.gpu

FORMS = ("trem_osc_step", "trem_osc_step_wide", "trem_osc_step_row")
PER_WAVE = (64, 16, 1)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _step(hiplib, form, rate, states):
    states = np.ascontiguousarray(states, dtype=np.float64)
    n = states.shape[0]
    so = np.full((n, 15), -7.0); out = np.full(n, -7.0); info = np.full(n, 77, dtype=np.uint64)
    assert hiplib.ow_debug_trem_step(form, C.c_double(rate), _p(states), n, _p(so), _p(out), _p(info), 0) == 0, hiplib.ow_last_error()
    return so, out, info


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


_DEVICE = {}


def _device(hiplib, oracle, rate):
    """The lane = engine form's results on the whole corpus of one rate, in corpus order (computed once, shared, never changed)."""
    if rate not in _DEVICE:
        _DEVICE[rate] = _step(hiplib, 0, rate, tc.corpus(oracle)[rate].states)
    return _DEVICE[rate]


def _arrangements(ref, n):
    """Orders of the cases: wavefronts uniform in their exits (sorted by retry, sweeps, limiter and cap counts: the wave-wide ballots of the
    limiter, the pivot scan and the cap see agreeing lanes), wavefronts that mix everything (a fixed shuffle: limited beside unlimited
    lanes, converged beside retrying ones), and a ragged tail (another shuffle cut so that the last wavefront and the last quad are
    partly filled)."""
    f = ref.info.astype(np.int64)
    uniform = np.lexsort((np.arange(n), f[:, 8], f[:, 7], f[:, 2], f[:, 0], f[:, 1], f[:, 4]))
    return {"uniform": uniform, "mixed": np.random.default_rng(21).permutation(n), "ragged": np.random.default_rng(22).permutation(n)[: n - 64 - 13]}


def _where(cs, ref, order, pos, form):
    c = int(order[pos])
    return {"rate": cs.rate, "case": c, "family": tc.FAMILIES[cs.family[c]], "info": dict(zip(("trap_iter", "be", "be_iter", "conv", "nan", "pivot", "sing", "log",
            "cap", "thr"), ref.info[c].tolist())), "form": FORMS[form], "position": int(pos), "state": cs.states[c].tolist()}


@pytest.mark.parametrize("rate", tc.RATES)
def test_three_forms_are_bit_identical_in_every_arrangement(hiplib, oracle, rate):
    """The same fifteen rows, the same output and the same fallback increment, bit for bit (NaN payloads included: the arrays are compared
    as integers), from all three forms, for every case of the corpus -- ill-conditioned and non-finite ones too -- wherever in a wavefront
    it sits and whoever its neighbours are.  The lane form's limiter divisions run only when some lane of the wavefront was limited, its
    pivot scan only when some lane disagrees with the usual order; the row form computes with zero coefficients where the others skip a
    term and redoes a sweep that trips a trigger: each shows here as a case whose bits depend on the form or on the arrangement."""
    cs, ref = tc.corpus(oracle)[rate], tc.references(oracle)[rate]
    canon = _device(hiplib, oracle, rate)
    cb = (_bits(canon[0]), _bits(canon[1]), canon[2])
    for name, order in _arrangements(ref, cs.n).items():
        for form in range(3):
            so, out, info = _step(hiplib, form, rate, cs.states[order])
            bad = np.nonzero((_bits(so) != cb[0][order]).any(axis=1) | (_bits(out) != cb[1][order]) | (info != cb[2][order]))[0]
            assert bad.size == 0, (name, int(bad.size), _where(cs, ref, order, bad[0], form), so[bad[0]].tolist(), canon[0][order[bad[0]]].tolist(),
                                   int(info[bad[0]]), int(cb[2][order[bad[0]]]))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 15, 17, 63, 65])
def test_tiny_and_ragged_case_counts(hiplib, oracle, n):
    """n that fills no wavefront or quad: every form returns what the lane form returns for those cases inside the full corpus."""
    rate = 96000.0
    cs = tc.corpus(oracle)[rate]
    order = np.random.default_rng(n).permutation(cs.n)[:n]
    full = _device(hiplib, oracle, rate)
    for form in range(3):
        so, out, info = _step(hiplib, form, rate, cs.states[order])
        assert _bits(so).tobytes() == _bits(full[0][order]).tobytes() and _bits(out).tobytes() == _bits(full[1][order]).tobytes(), (n, FORMS[form])
        assert np.array_equal(info, full[2][order]), (n, FORMS[form])


@pytest.mark.parametrize("rate", tc.RATES)
def test_every_comparable_case_is_the_oracles_step(hiplib, oracle, rate):
    """Every case the reference algorithm pins (CPU: the oracle with pnjlim's logarithm one double away keeps its exits and stays within the
    state-row bar) takes the oracle's exits -- the same increment of the fallback counter, the same NaN-reset outcome -- and is within
    that bar of the oracle's step: volts 1e-5 relative + ABS_FLOOR_TREM_STEP_V, amps 1e-5 relative + ABS_FLOOR_TREM_STEP_I, the output as
    the node voltage it is.  A case whose oracle step ran no pnjlim logarithm consists of IEEE operations only, and the kernels claim the
    oracle's bits (ow_trem_wide.h, ow_trem_row.h): those must be EQUAL, rows, output and all.  Non-finite states (in no class, not
    comparable) must still end in the reset, as the oracle's do."""
    cs, ref = tc.corpus(oracle)[rate], tc.references(oracle)[rate]
    so, out, info = _device(hiplib, oracle, rate)
    floors = (oracle.ABS_FLOOR_TREM_STEP_V, oracle.ABS_FLOOR_TREM_STEP_I)
    with np.errstate(invalid="ignore"):
        ok = tc.state_row_ok(so, ref.states, floors) & (np.abs(out - ref.out) <= 1e-5 * np.abs(ref.out) + floors[0])
        err = np.abs(so - ref.states)
    m = ref.comparable
    dc = tc.dc_op(oracle)
    is_reset = (_bits(so) == _bits(dc)[None, :]).all(axis=1) & (_bits(out) == _bits(dc[:1])[0])
    print("\n%g Hz: %d comparable of %d (%d of them without a logarithm); by class: cases, worst volt error, worst amp error" % (
        rate, int(m.sum()), cs.n, int((m & ref.no_log).sum())))
    for c in range(tc.N_CLASSES):
        mc = m & ref.classes[:, c]
        print("  %-26s %6d  %.3e  %.3e" % (tc.CLASS_NAMES[c], int(mc.sum()), float(err[mc][:, :7].max()) if mc.any() else 0.0,
                                           float(err[mc][:, 7:].max()) if mc.any() else 0.0))
    bad = np.nonzero(m & (info != ref.info[:, 1].astype(np.uint64)))[0]
    assert bad.size == 0, ("fallback increment", int(bad.size), _where(cs, ref, np.arange(cs.n), bad[0], 0), int(info[bad[0]]))
    bad = np.nonzero((m | ~np.isfinite(cs.states).all(axis=1)) & (is_reset != ref.nan_reset))[0]
    assert bad.size == 0, ("NaN reset", int(bad.size), _where(cs, ref, np.arange(cs.n), bad[0], 0), so[bad[0]].tolist())
    bad = np.nonzero(m & ~ok)[0]
    assert bad.size == 0, ("state-row bar", int(bad.size), _where(cs, ref, np.arange(cs.n), bad[0], 0), (so[bad[0]] - ref.states[bad[0]]).tolist(),
                           ref.states[bad[0]].tolist())
    exact = m & ref.no_log
    bad = np.nonzero(exact & ((_bits(so) != _bits(ref.states)).any(axis=1) | (_bits(out) != _bits(ref.out))))[0]
    assert bad.size == 0, ("bit identity without a logarithm", int(bad.size), int(exact.sum()), _where(cs, ref, np.arange(cs.n), bad[0], 0),
                           (so[bad[0]] - ref.states[bad[0]]).tolist())


@pytest.mark.parametrize("rate", tc.RATES)
def test_eight_chained_steps(hiplib, oracle, rate):
    """What a step hands to the next one: the comparable cases that converged (in the trapezoidal solve or in the retry) taken eight steps
    on, each side fed its own output state, every form.  The bar is the single step's.  A case drops out at the step at which the oracle
    with the logarithm one double away, chained the same way, changes an exit or leaves the bar of the unperturbed one; at most 10 % may."""
    cs, ref = tc.corpus(oracle)[rate], tc.references(oracle)[rate]
    floors = (oracle.ABS_FLOOR_TREM_STEP_V, oracle.ABS_FLOOR_TREM_STEP_I)
    sel = np.nonzero(ref.comparable & (ref.info[:, 3] == 1) & ~ref.nan_reset)[0]
    assert sel.size >= 2048
    dev = [cs.states[sel].copy() for _ in range(3)]
    cpu = cs.states[sel].copy(); cpu_p = [cpu.copy(), cpu.copy()]
    alive = np.ones(sel.size, dtype=bool)
    for step in range(8):
        cpu, out_c, info_c = oracle.trem_step_cases(rate, cpu)
        for k, u in enumerate((1, -1)):
            cpu_p[k], _, info_p = oracle.trem_step_cases(rate, cpu_p[k], log_ulp=u)
            alive &= tc.state_row_ok(cpu_p[k], cpu, floors) & (info_p[:, [1, 3, 4]] == info_c[:, [1, 3, 4]]).all(axis=1)
        alive &= info_c[:, 4] == 0
        for form in range(3):
            dev[form], out_d, info_d = _step(hiplib, form, rate, dev[form])
            if form:
                assert _bits(dev[form]).tobytes() == _bits(dev[0]).tobytes(), (step, FORMS[form])
        with np.errstate(invalid="ignore"):
            ok = tc.state_row_ok(dev[0], cpu, floors) & (np.abs(out_d - out_c) <= 1e-5 * np.abs(out_c) + floors[0]) & (info_d == info_c[:, 1].astype(np.uint64))
        bad = np.nonzero(alive & ~ok)[0]
        assert bad.size == 0, (step, int(bad.size), _where(cs, ref, sel, bad[0], 0), (dev[0][bad[0]] - cpu[bad[0]]).tolist())
    print("\n%g Hz: %d cases chained, %d dropped as ill-conditioned" % (rate, sel.size, int((~alive).sum())))
    assert (~alive).sum() <= tc.MAX_ILL_SHARE * sel.size, (int((~alive).sum()), sel.size)
