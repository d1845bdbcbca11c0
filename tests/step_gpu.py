"""What the single-step tests of the three Newton solvers share (tests/test_gpu_dk_step.py, tests/test_gpu_trem_step.py,
tests/test_gpu_mel_step.py): a Solver record that describes one solver's step, and the four test bodies built on it -- forms
bit-identical in every arrangement, tiny and ragged counts, every comparable case against the oracle, chained steps.

`call(form, rate, inputs, outputs)` is whatever performs one device step on n cases: it reads the tuple of input arrays and fills the
tuple of output arrays.  The GPU tests pass hook_call() over a debug hook of the library; nothing here imports the library, so
tests/test_step_harness.py runs the same bodies with the oracle's own step as the device, and with slips seeded into it."""
import ctypes as C

import numpy as np

import step_cases as sc


class Solver:
    """One solver's step, as the routines below need it described:
    name, mod (its corpus module), forms (names of the device forms), info_names (the oracle's info columns);
    outputs: ((shape of one case, fill, dtype), ...) of the device's output arrays -- state row, output, then the exit increments if any;
    oracle(ob, rate, *args, **variant) -> (states, out, info), variants (keyword sets of the perturbed oracles), decisions (info columns
    a perturbed oracle has to keep), reset (info column of the NaN reset, or None);
    exits(info) -> what the device's increments have to be (None: the device reports none);
    held: the forms that claim the oracle's step; against: the form whose bits every form has to return (None: each its own);
    sort_keys(ref), unit, seeds, ragged_cut(n): its arrangements (step_cases.arrangements);
    convergent(ob, ref): mask of the cases a chain of steps may start from."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def args(self, cs, order):
        """The per-case input arrays of the cases `order`: states, then the corpus module's columns."""
        return (cs.states[order],) + tuple(getattr(cs, c)[order] for c in self.mod.Cases.COLUMNS)

    def step(self, call, form, rate, *args):
        ins = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in args)
        outs = tuple(np.full((ins[0].shape[0],) + shape, fill, dtype=dtype) for shape, fill, dtype in self.outputs)
        call(form, rate, ins, outs)
        return outs

    @staticmethod
    def differ(a, b):
        """Per case: any output differs in its bits (NaN payloads included: floats are compared as integers)."""
        bad = np.zeros(a[0].shape[0], dtype=bool)
        for x, y in zip(a, b):
            d = sc.bits(x) != sc.bits(y) if x.dtype == np.float64 else x != y
            bad |= d.reshape(bad.size, -1).any(axis=1)
        return bad

    def bar(self, ob, got, want):
        """Per case: state row and output within the solver's bar of the oracle's."""
        return self.mod.state_row_ok(got[0], want[0], ob) & self.mod.out_ok(got[1], want[1], ob)


def hook_call(hook, last_error):
    """`call` over a debug hook int hook(form, rate, inputs..., n, outputs..., device)."""
    def call(form, rate, ins, outs):
        assert hook(form, C.c_double(rate), *map(sc.ptr, ins), ins[0].shape[0], *map(sc.ptr, outs), 0) == 0, last_error()
    return call


_CANONICAL = {}


def canonical(solver, call, oracle, rate, form):
    """One form's results on the whole corpus of one rate, in corpus order (computed once per process, shared, never changed)."""
    key = (solver.name, call, rate, form)
    if key not in _CANONICAL:
        cs = solver.mod.corpus(oracle)[rate]
        _CANONICAL[key] = solver.step(call, form, rate, *solver.args(cs, slice(None)))
    return _CANONICAL[key]


def where(solver, cs, ref, order, pos, form):
    """What an assert message says about the case at position `pos` of the order `order`."""
    c = int(order[pos])
    return {"rate": cs.rate, "case": c, "family": solver.mod.FAMILIES[cs.family[c]], "info": dict(zip(solver.info_names, ref.info[c].tolist())),
            "form": solver.forms[form], "position": int(pos), "args": [a.tolist() for a in solver.args(cs, c)]}


def _same_as_canonical(solver, call, oracle, rate, order, forms, what):
    cs, ref = solver.mod.corpus(oracle)[rate], solver.mod.references(oracle)[rate]
    for form in forms:
        got = solver.step(call, form, rate, *solver.args(cs, order))
        want = tuple(a[order] for a in canonical(solver, call, oracle, rate, form if solver.against is None else solver.against))
        bad = np.nonzero(solver.differ(got, want))[0]
        assert bad.size == 0, (what, int(bad.size), where(solver, cs, ref, order, bad[0], form), [a[bad[0]].tolist() for a in got],
                               [a[bad[0]].tolist() for a in want])


def assert_arrangements_bit_identical(solver, call, oracle, rate):
    """Every held form returns, for every case of the corpus -- ill-conditioned and non-finite ones too -- the canonical bits (form
    `against`'s, or its own) wherever in a wavefront the case sits and whoever its neighbours are."""
    cs, ref = solver.mod.corpus(oracle)[rate], solver.mod.references(oracle)[rate]
    for name, order in sc.arrangements(solver.sort_keys(ref), cs.n, solver.unit, solver.seeds, solver.ragged_cut(cs.n)).items():
        _same_as_canonical(solver, call, oracle, rate, order, solver.held, name)


def subset(solver, cs, n):
    """n cases picked by a shuffle seeded with n: whole units but the last, where n is no multiple of the unit."""
    return sc.cases_of(np.random.default_rng(n).permutation(cs.n // solver.unit)[: (n + solver.unit - 1) // solver.unit], solver.unit)[:n]


def assert_subset_is_the_corpus(solver, call, oracle, rate, n):
    """n cases that fill no wavefront: every form returns what the canonical run returns for those cases inside the full corpus."""
    _same_as_canonical(solver, call, oracle, rate, subset(solver, solver.mod.corpus(oracle)[rate], n), range(len(solver.forms)), n)


def errors(dev, ref):
    with np.errstate(invalid="ignore"):
        return np.abs(dev[0] - ref.states)


def class_table(solver, ref, sel, cell, width=26):
    """One line per exit class: its name, the cases of `sel` in it, and cell(mask of those cases)."""
    for c, name in enumerate(solver.mod.CLASS_NAMES):
        m = sel & ref.classes[:, c]
        print("  %-*s %6d  %s" % (width, name, int(m.sum()), cell(m)))


def against_oracle(solver, oracle, cs, ref, dev, sel, what, form=0, bar=None, exits=True):
    """Asserts, on the cases `sel`, the oracle's exit increments (where the solver reports any) and the bar (the solver's, or
    bar(dev, (ref.states, ref.out)) -> per-case mask); returns the per-case absolute errors of the state rows."""
    everyone = np.arange(cs.n)
    if exits and solver.exits is not None:
        want = solver.exits(ref.info)
        bad = np.nonzero(sel & (dev[2] != want).reshape(cs.n, -1).any(axis=1))[0]
        assert bad.size == 0, (what, "exit increments", int(bad.size), where(solver, cs, ref, everyone, bad[0], form), dev[2][bad[0]].tolist(), want[bad[0]].tolist())
    ok = solver.bar(oracle, dev, (ref.states, ref.out)) if bar is None else bar(dev, (ref.states, ref.out))
    bad = np.nonzero(sel & ~ok)[0]
    assert bad.size == 0, (what, "state-row bar", int(bad.size), where(solver, cs, ref, everyone, bad[0], form), (dev[0][bad[0]] - ref.states[bad[0]]).tolist(),
                           ref.states[bad[0]].tolist())
    return errors(dev, ref)


def chain(solver, call, oracle, rate, idx, steps, what, pairwise=False, after=None):
    """The cases `idx` taken `steps` steps on, each side -- the oracle, its perturbed variants, every held form -- fed its own output
    state, the other arguments as in the first step unless after(step, oracle's results, alive, arguments) returns new ones.  Form
    `against` -- where there is none, every held form -- is held to the single step's bar and exits at every step; the other held
    forms have to return form `against`'s bits, state rows, output and increments.  A
    case drops out at the step at which a perturbed oracle, chained the same way, changes a decision or leaves the bar of the
    unperturbed one, or at which the state resets or stops being finite; pairwise: its partner drops with it.  At most MAX_ILL_SHARE
    may drop.  Returns the mask of the cases still alive."""
    cs, ref = solver.mod.corpus(oracle)[rate], solver.mod.references(oracle)[rate]
    state, *rest = solver.args(cs, idx)
    dev = {form: state.copy() for form in solver.held}
    cpu = state.copy(); cpu_p = [state.copy() for _ in solver.variants]
    alive = np.ones(idx.size, dtype=bool)
    for step in range(steps):
        res = solver.oracle(oracle, rate, cpu, *rest)
        cpu = res[0]
        for k, variant in enumerate(solver.variants):
            res_p = solver.oracle(oracle, rate, cpu_p[k], *rest, **variant)
            cpu_p[k] = res_p[0]
            alive &= solver.bar(oracle, res_p, res) & (res_p[2][:, solver.decisions] == res[2][:, solver.decisions]).all(axis=1)
        alive &= np.isfinite(cpu).all(axis=1)
        if solver.reset is not None:
            alive &= res[2][:, solver.reset] == 0
        if pairwise:
            alive = np.repeat(alive.reshape(-1, 2).all(axis=1), 2)
        want = None if solver.exits is None else solver.exits(res[2])
        for form in solver.held:
            got = solver.step(call, form, rate, dev[form], *rest)
            dev[form] = got[0]
            if solver.against not in (None, form):          # form `against` came first and has been held to the bar: this one claims its bits
                if any(a.tobytes() != b.tobytes() for a, b in zip(got, first)):
                    bad = np.nonzero(solver.differ(got, first))[0]
                    raise AssertionError((what, step, "the bits of " + solver.forms[solver.against], where(solver, cs, ref, idx, bad[0], form)))
                continue
            first = got
            ok = solver.bar(oracle, got, res)
            if want is not None:
                ok &= (got[2] == want).reshape(idx.size, -1).all(axis=1)
            bad = np.nonzero(alive & ~ok)[0]
            assert bad.size == 0, (what, step, int(bad.size), where(solver, cs, ref, idx, bad[0], form), (got[0][bad[0]] - cpu[bad[0]]).tolist(), cpu[bad[0]].tolist(),
                                   [a[bad[0]].tolist() for a in got[2:]], None if want is None else want[bad[0]].tolist())
        if after is not None:
            rest = after(step, res, alive, rest) or rest
    assert (~alive).sum() <= solver.mod.MAX_ILL_SHARE * alive.size, (what, int((~alive).sum()), alive.size)
    return alive
