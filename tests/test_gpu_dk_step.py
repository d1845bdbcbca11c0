"""ONE step of the legacy DK preamp at a time, through each of the kernels' four forms of it (dk_step, dk_step_pair, dk_step_wide,
dk_step_row: debug hook ow_debug_dk_step) on the corpus of tests/dk_step_cases.py -- the exits of the Newton loop that musical play
never takes: no update, six updates without convergence, the junction clamp at both edges, main and shadow states of a lane that need
different numbers of updates.  Long traces of an overdriven preamp are chaotic; one step from a common state is not: a difference is a
difference in the step.  tests/test_oracle_dk_step_cases.py fixes, on the CPU, which cases the reference algorithm itself pins."""
import ctypes as C

import numpy as np
import pytest

import dk_step_cases as dk

pytestmark = pytest.mark.gpu

FORMS = ("dk_step", "dk_step_pair", "dk_step_wide", "dk_step_row")
PER_WAVE = (64, 128, 16, 4)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _step(hiplib, form, rate, states, inputs, g, gp):
    states = np.ascontiguousarray(states, dtype=np.float64); inputs = np.ascontiguousarray(inputs, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64); gp = np.ascontiguousarray(gp, dtype=np.float64)
    n = states.shape[0]
    so = np.full((n, 14), -7.0); out = np.full(n, -7.0)
    assert hiplib.ow_debug_dk_step(form, C.c_double(rate), _p(states), _p(inputs), _p(g), _p(gp), n, _p(so), _p(out), 0) == 0
    return so, out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _arrangements(ref, n):
    """Orders of the (main, shadow) pairs, as case indices: wavefronts uniform in one exit class (pairs sorted by their update counts: the
    ballot ends the loop early, or never), wavefronts that mix all classes (a fixed shuffle: frozen lanes beside lanes still iterating),
    and a ragged tail (another shuffle cut to an odd number of cases: a last wavefront, quad and row partly filled, a last lane with a
    main state only)."""
    pairs = n // 2
    um, us = ref.info[0::2, 0].astype(np.int64), ref.info[1::2, 0].astype(np.int64)
    ex = ref.info[0::2, 1].astype(np.int64)
    uniform = np.lexsort((np.arange(pairs), ex, np.minimum(um, us), np.maximum(um, us)))
    mixed = np.random.default_rng(11).permutation(pairs)
    ragged = np.random.default_rng(12).permutation(pairs)
    to_cases = lambda p: np.stack([2 * p, 2 * p + 1], axis=1).ravel()
    return {"uniform": to_cases(uniform), "mixed": to_cases(mixed), "ragged": to_cases(ragged)[: n - 2 * 37 - 1]}


def _where(cs, ref, order, pos, form):
    """what an assert message says about the case at position `pos` of an arrangement"""
    c = int(order[pos])
    return {"rate": cs.rate, "case": c, "family": dk.FAMILIES[cs.family[c]], "updates": int(ref.info[c, 0]), "exit": int(ref.info[c, 1]),
            "clamped(-1 V, 0.85 V)": (int(ref.info[c, 2]), int(ref.info[c, 3])), "partner updates": int(ref.info[c ^ 1, 0]),
            "form": FORMS[form], "position": int(pos), "lane": int((pos % PER_WAVE[form]) * (64 // PER_WAVE[form]) if form != 1 else (pos // 2) % 64)}


@pytest.mark.parametrize("rate", dk.RATES)
def test_four_forms_are_bit_identical_in_every_arrangement(hiplib, oracle, rate):
    """The same fourteen fields and the same output, bit for bit (NaN payloads included: the arrays are compared as integers), from all
    four forms, for every case of the corpus -- ill-conditioned and non-finite ones too -- wherever in a wavefront it sits and whoever its
    neighbours are.  A frozen lane that still moves, a pair loop that stops when one of its states is done, a different update cap in
    one form: each shows here as a case whose bits depend on the form or on the arrangement."""
    cs, ref = dk.corpus(oracle)[rate], dk.references(oracle)[rate]
    canon_s = canon_o = None
    for name, order in _arrangements(ref, cs.n).items():
        for form in range(4):
            so, out = _step(hiplib, form, rate, cs.states[order], cs.inputs[order], cs.g[order], cs.gp[order])
            if canon_s is None:                 # the first run is a full permutation: every case has its bits
                assert order.size == cs.n
                canon_s = np.zeros((cs.n, 14), dtype=np.uint64); canon_o = np.zeros(cs.n, dtype=np.uint64)
                canon_s[order] = _bits(so); canon_o[order] = _bits(out)
                continue
            bad = np.nonzero((_bits(so) != canon_s[order]).any(axis=1) | (_bits(out) != canon_o[order]))[0]
            assert bad.size == 0, (name, int(bad.size), _where(cs, ref, order, bad[0], form),
                                   (so[bad[0]] - canon_s[order[bad[0]]].view(np.float64)).tolist())


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 65, 129])
def test_tiny_and_ragged_case_counts(hiplib, oracle, n):
    """n that fills no wavefront, quad, row or pair: every form returns what it returns for those cases inside the full corpus."""
    rate = 96000.0
    cs, ref = dk.corpus(oracle)[rate], dk.references(oracle)[rate]
    pick = np.random.default_rng(n).permutation(cs.n // 2)[: (n + 1) // 2]
    order = np.stack([2 * pick, 2 * pick + 1], axis=1).ravel()[:n]
    full_s, full_o = _step(hiplib, 0, rate, cs.states, cs.inputs, cs.g, cs.gp)
    for form in range(4):
        so, out = _step(hiplib, form, rate, cs.states[order], cs.inputs[order], cs.g[order], cs.gp[order])
        assert _bits(so).tobytes() == _bits(full_s[order]).tobytes() and _bits(out).tobytes() == _bits(full_o[order]).tobytes(), (n, FORMS[form])


@pytest.mark.parametrize("rate", dk.RATES)
def test_every_comparable_case_is_the_oracles_step(hiplib, oracle, rate):
    """Every case the reference algorithm pins (CPU: one-ulp-exp oracle within the state-row bar) is within that bar of the oracle's step:
    volts 1e-5 relative + ABS_FLOOR_PREAMP, currents 1e-5 relative + 1e-12, the output as the node voltage it is.  No other exclusion."""
    cs, ref = dk.corpus(oracle)[rate], dk.references(oracle)[rate]
    so, out = _step(hiplib, 0, rate, cs.states, cs.inputs, cs.g, cs.gp)
    ok = dk.state_row_ok(so, ref.states, oracle.ABS_FLOOR_PREAMP) & (np.abs(out - ref.out) <= 1e-5 * np.abs(ref.out) + oracle.ABS_FLOOR_PREAMP)
    m = ref.comparable
    with np.errstate(invalid="ignore"):
        err = np.abs(so - ref.states)
    print("\n%g Hz: %d comparable of %d; worst volt error %.3e, worst current error %.3e; by class (cases, worst volt error):" % (
        rate, int(m.sum()), cs.n, float(err[m][:, list(range(2, 10)) + [12, 13]].max()), float(err[m][:, [0, 1, 10, 11]].max())))
    for c in range(dk.N_CLASSES):
        mc = m & ref.classes[:, c]
        print("  %-26s %6d  %.3e" % (dk.CLASS_NAMES[c], int(mc.sum()), float(err[mc][:, list(range(2, 10)) + [12, 13]].max()) if mc.any() else 0.0))
    bad = np.nonzero(m & ~ok)[0]
    assert bad.size == 0, (int(bad.size), _where(cs, ref, np.arange(cs.n), bad[0], 0), (so[bad[0]] - ref.states[bad[0]]).tolist(), ref.states[bad[0]].tolist())
    # the same decisions: a comparable case left the loop after the oracle's number of updates unless its residual sat on the tolerance
    # (not asserted per case: the device's exponential differs from glibc's in the last place, which is what `comparable` allows for)


def _device_ic(hiplib, vnl):
    """IS (exp(clamp(v) / VT) - 1) with the kernels' own exponential (ow_debug_unary, which = 0); clamp, division and the rest are IEEE
    operations that numpy repeats bit for bit (tests/test_gpu_division.py pins the kernels' constant division to IEEE)."""
    x = np.ascontiguousarray(np.clip(vnl, -1.0, dk.VBE_MAX).ravel() / dk.VT)
    f = np.zeros_like(x); lib = np.zeros_like(x)
    assert hiplib.ow_debug_unary(0, _p(x), x.size, _p(f), _p(lib), 0) == 0
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
        so, out = _step(hiplib, form, rate, states, cs.inputs, cs.g, cs.gp)
        fin = np.isfinite(so).all(axis=1) & np.isfinite(out)
        assert fin.sum() >= 0.99 * cs.n
        want = _device_ic(hiplib, so[fin][:, 12:14])
        bad = np.nonzero((_bits(so[fin][:, 10:12]) != _bits(want)).any(axis=1))[0]
        assert bad.size == 0, (int(bad.size), _where(cs, ref, np.nonzero(fin)[0], bad[0], form), so[fin][bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("rate", dk.RATES)
def test_eight_chained_steps(hiplib, oracle, rate):
    """What a step hands to the next one: the comparable, convergent cases of the corpus taken eight steps on, each side fed its own
    output state (g_ldr_prev = g_ldr from the second step, as process_sample leaves it), every form.  The bar is the single step's.  A case
    drops out at the step at which the one-ulp-exp oracle, chained the same way, leaves the bar of the unperturbed one; at most 10 % may."""
    cs, ref = dk.corpus(oracle)[rate], dk.references(oracle)[rate]
    sel = np.nonzero(ref.comparable & (ref.info[:, 1] == oracle.DK_EXIT_CONVERGED))[0]
    sel = np.intersect1d(sel, sel ^ 1)                    # whole (main, shadow) pairs: the pair form steps both
    assert sel.size >= 4096
    x, g = cs.inputs[sel], cs.g[sel]
    dev = [cs.states[sel].copy() for _ in range(4)]
    cpu, cpu_p = cs.states[sel].copy(), cs.states[sel].copy()
    alive = np.ones(sel.size, dtype=bool)
    gp = cs.gp[sel]
    for step in range(8):
        cpu, out_c, _ = oracle.dk_step_cases(rate, cpu, x, g, gp)
        cpu_p, out_p, _ = oracle.dk_step_cases(rate, cpu_p, x, g, gp, perturbed=True)
        with np.errstate(invalid="ignore"):
            alive &= dk.state_row_ok(cpu_p, cpu, oracle.ABS_FLOOR_PREAMP) & np.isfinite(cpu).all(axis=1)
        for form in range(4):
            dev[form], out_d = _step(hiplib, form, rate, dev[form], x, g, gp)
            if form:
                assert _bits(dev[form]).tobytes() == _bits(dev[0]).tobytes(), (step, FORMS[form])
        ok = dk.state_row_ok(dev[0], cpu, oracle.ABS_FLOOR_PREAMP) & (np.abs(out_d - out_c) <= 1e-5 * np.abs(out_c) + oracle.ABS_FLOOR_PREAMP)
        bad = np.nonzero(alive & ~ok)[0]
        assert bad.size == 0, (step, int(bad.size), _where(cs, ref, sel, bad[0], 0), (dev[0][bad[0]] - cpu[bad[0]]).tolist())
        gp = g
    print("\n%g Hz: %d cases chained, %d dropped as ill-conditioned" % (rate, sel.size, int((~alive).sum())))
    assert (~alive).sum() <= dk.MAX_ILL_SHARE * sel.size, (int((~alive).sum()), sel.size)
