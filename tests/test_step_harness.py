"""The shared single-step test bodies of tests/step_gpu.py have teeth.  One rate per solver, the oracle's own step standing in for the
device: every routine passes; a slip seeded into that device makes the matching routine raise an AssertionError that names the
slipped case; and the same slip on a case the reference does not pin passes -- the exclusion is the reference's and nothing wider.
The solver descriptions are the GPU tests' own; the corpora come from the per-process caches the oracle tests fill."""
import collections

import numpy as np
import pytest

import oracle_binding as ob
import step_cases as sc
import step_gpu as sg
import test_gpu_dk_step
import test_gpu_mel_step
import test_gpu_trem_step

RATE = 96000.0
SOLVERS = {m.SOLVER.name: m.SOLVER for m in (test_gpu_dk_step, test_gpu_trem_step, test_gpu_mel_step)}
solvers = pytest.mark.parametrize("solver", SOLVERS.values(), ids=SOLVERS.keys())


def device(solver, slip=None):
    """The oracle's step as every form of the device; slip(form, k, ins, outs) then alters the results of that form's k-th call."""
    calls = collections.Counter()

    def call(form, rate, ins, outs):
        so, out, info = solver.oracle(ob, rate, *ins)
        outs[0][:] = so; outs[1][:] = out
        if solver.exits is not None:
            outs[2][:] = solver.exits(info)
        if slip is not None:
            slip(form, calls[form], ins, outs)
        calls[form] += 1
    return call


CLEAN = {name: device(s) for name, s in SOLVERS.items()}


def corpus(solver):
    return solver.mod.corpus(ob)[RATE], solver.mod.references(ob)[RATE]


def rows_of(solver, cs, c, ins):
    """The rows of a call's inputs that are case c: every argument equal in its bits."""
    hit = np.ones(ins[0].shape[0], dtype=bool)
    for a, want in zip(ins, solver.args(cs, c)):
        hit &= (sc.bits(a) == sc.bits(np.asarray(want))).reshape(hit.size, -1).all(axis=1)
    return np.nonzero(hit)[0]


def pick(solver, cs, ref, mask, unique=False):
    """(case, state row): the first case of `mask` that no earlier case (unique: no other case) shares its arguments with, and its volt
    row of largest magnitude (there 2e-5 of the value is beyond the bar's 1e-5 relative + floor)."""
    for c in np.nonzero(mask)[0]:
        hit = rows_of(solver, cs, c, solver.args(cs, slice(None)))
        if hit[0] == c and (hit.size == 1 or not unique):                        # (a later copy of the case carries the same slip)
            rows = np.arange(cs.states.shape[1])[solver.mod.V_ROWS]
            return int(c), int(rows[np.argmax(np.nan_to_num(np.abs(ref.states[c, rows]), posinf=0.0))])
    raise AssertionError("no such case")


def move(solver, cs, c, row):
    """Slip: state row `row` of case c comes out 2e-5 of its value away (1 V, where the value is not finite)."""
    def slip(form, k, ins, outs):
        hit = rows_of(solver, cs, c, ins)
        outs[0][hit, row] = np.where(np.isfinite(outs[0][hit, row]), outs[0][hit, row] * (1.0 + 2e-5), 1.0)
    return slip


def flip(solver, cs, c, row, only):
    """Slip: the last bit of state row `row` of case c flipped."""
    def slip(form, k, ins, outs):
        if only(form, k, ins):
            outs[0].view(np.uint64)[rows_of(solver, cs, c, ins), row] ^= np.uint64(1)
    return slip


def names(excinfo, c):
    return "'case': %d," % c in str(excinfo.value)


def chain_units(solver, ref):
    u = sc.whole_units(solver.convergent(ob, ref), solver.unit)
    return u[:: max(u.size // 256, 1)]


@solvers
def test_every_routine_passes_with_the_oracle_as_the_device(solver):
    cs, ref = corpus(solver)
    call = CLEAN[solver.name]
    sg.assert_arrangements_bit_identical(solver, call, ob, RATE)
    for n in (1, 3, 65):
        sg.assert_subset_is_the_corpus(solver, call, ob, RATE, n)
    err = sg.against_oracle(solver, ob, cs, ref, sg.canonical(solver, call, ob, RATE, 0), ref.comparable, "oracle")
    assert (err[ref.finite] == 0.0).all()
    sg.class_table(solver, ref, ref.comparable, lambda m: "%d" % int(m.sum()))
    alive = sg.chain(solver, call, ob, RATE, sc.cases_of(chain_units(solver, ref), solver.unit), 8, "oracle", pairwise=solver.unit == 2)
    assert alive.size >= 256 and alive.sum() >= 0.9 * alive.size


@solvers
def test_a_moved_state_row_is_caught_on_a_comparable_case_only(solver):
    cs, ref = corpus(solver)
    everything = solver.args(cs, slice(None))
    c, row = pick(solver, cs, ref, ref.comparable)
    dev = solver.step(device(solver, move(solver, cs, c, row)), 0, RATE, *everything)
    assert dev[0][c, row] != ref.states[c, row]
    with pytest.raises(AssertionError) as e:
        sg.against_oracle(solver, ob, cs, ref, dev, ref.comparable, "moved")
    assert names(e, c) and "state-row bar" in str(e.value)
    c, row = pick(solver, cs, ref, ~ref.comparable)
    dev = solver.step(device(solver, move(solver, cs, c, row)), 0, RATE, *everything)
    assert dev[0][c, row] != ref.states[c, row]
    sg.against_oracle(solver, ob, cs, ref, dev, ref.comparable, "moved, not comparable")


@pytest.mark.parametrize("solver", [s for s in SOLVERS.values() if s.exits is not None], ids=[n for n, s in SOLVERS.items() if s.exits is not None])
def test_a_changed_exit_increment_is_caught_on_a_comparable_case_only(solver):
    cs, ref = corpus(solver)
    everything = solver.args(cs, slice(None))

    def bump(c):
        def slip(form, k, ins, outs):
            outs[2].reshape(outs[2].shape[0], -1)[rows_of(solver, cs, c, ins), 0] += 1
        return slip
    c, _ = pick(solver, cs, ref, ref.comparable)
    with pytest.raises(AssertionError) as e:
        sg.against_oracle(solver, ob, cs, ref, solver.step(device(solver, bump(c)), 0, RATE, *everything), ref.comparable, "bumped")
    assert names(e, c) and "exit increments" in str(e.value)
    c, _ = pick(solver, cs, ref, ~ref.comparable)
    sg.against_oracle(solver, ob, cs, ref, solver.step(device(solver, bump(c)), 0, RATE, *everything), ref.comparable, "bumped, not comparable")


@solvers
def test_a_bit_flipped_in_one_arrangement_or_one_form_is_caught(solver):
    cs, ref = corpus(solver)
    ragged = sc.arrangements(solver.sort_keys(ref), cs.n, solver.unit, solver.seeds, solver.ragged_cut(cs.n))["ragged"]
    inside = np.zeros(cs.n, dtype=bool); inside[ragged] = True
    c, row = pick(solver, cs, ref, inside, unique=True)
    last = solver.held[-1]
    # the ragged arrangement alone (the only run of that many cases), one form
    call = device(solver, flip(solver, cs, c, row, lambda form, k, ins: form == last and ins[0].shape[0] == ragged.size))
    with pytest.raises(AssertionError) as e:
        sg.assert_arrangements_bit_identical(solver, call, ob, RATE)
    assert names(e, c) and "ragged" in str(e.value) and solver.forms[last] in str(e.value)
    # one form, in every run
    call = device(solver, flip(solver, cs, c, row, lambda form, k, ins: form == last))
    if solver.against is not None:
        with pytest.raises(AssertionError) as e:
            sg.assert_arrangements_bit_identical(solver, call, ob, RATE)
        assert names(e, c) and solver.forms[last] in str(e.value)
    else:                                   # each form is held to its own bits there: the solver's test compares the canonical runs
        sg.assert_arrangements_bit_identical(solver, call, ob, RATE)
        bad = solver.differ(sg.canonical(solver, call, ob, RATE, last), sg.canonical(solver, call, ob, RATE, last - 1))
        assert np.nonzero(bad)[0].tolist() == [c]


@solvers
def test_a_subset_run_that_returns_a_neighbours_row_is_caught(solver):
    cs, ref = corpus(solver)
    n = 65
    order = sg.subset(solver, cs, n)

    def slip(form, k, ins, outs):
        if form == 1 and ins[0].shape[0] == n:
            outs[0][7] = outs[0][8]
    assert not np.array_equal(ref.states[order[7]], ref.states[order[8]], equal_nan=True)
    with pytest.raises(AssertionError) as e:
        sg.assert_subset_is_the_corpus(solver, device(solver, slip), ob, RATE, n)
    assert names(e, order[7]) and "'position': 7," in str(e.value)


@solvers
def test_a_slip_at_step_five_of_a_chain_is_caught_on_a_live_case_only(solver):
    cs, ref = corpus(solver)
    idx = sc.cases_of(chain_units(solver, ref), solver.unit)
    pairwise = solver.unit == 2
    alive = sg.chain(solver, CLEAN[solver.name], ob, RATE, idx, 8, "clean", pairwise=pairwise)
    rows = np.arange(cs.states.shape[1])[solver.mod.V_ROWS]

    def at(pos, step, forms):
        def slip(form, k, ins, outs):
            if form in forms and k == step:
                outs[0][pos, rows[np.argmax(np.abs(outs[0][pos, rows]))]] *= 1.0 + 2e-5
        return slip
    pos = int(np.nonzero(alive)[0][0])
    with pytest.raises(AssertionError) as e:
        sg.chain(solver, device(solver, at(pos, 5, solver.held[-1:])), ob, RATE, idx, 8, "slipped", pairwise=pairwise)
    assert names(e, idx[pos]) and str(e.value).startswith("('slipped', 5,"), str(e.value)[:200]
    # a case that has dropped out by the last step carries the same slip there unnoticed, where this rate's selection has one (in every
    # form: the forms' state bits are compared on every case, dropped or not)
    for pos in np.nonzero(~alive)[0][:1]:
        sg.chain(solver, device(solver, at(int(pos), 7, solver.held)), ob, RATE, idx, 8, "slipped, dropped", pairwise=pairwise)
