"""What the single-step corpora of the three Newton solvers share (tests/dk_step_cases.py, tests/trem_step_cases.py,
tests/mel_step_cases.py): the case table, the bisection of a state row across one of a step's decisions, the 1e-5-relative-plus-floor
bar, the per-process caches, and the coverage a corpus has to reach before any kernel is measured against it.  A solver module keeps
what is its own: rates, families, kick tables, _build_rate with its seeds and order, and the Reference class (class masks, the
definition of `comparable`, the perturbed variants, the decision columns)."""
import ctypes as C
import math

import numpy as np


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Cases:
    """One chain rate's cases: rows are appended, freeze() turns them into contiguous parallel arrays -- states [n][width], family [n]
    (index into FAMILIES), side [n] (edge families: 0 = the base's side of the decision, 1 = the other side; -1 elsewhere) and one
    float array per name in COLUMNS."""
    FAMILIES = ()
    COLUMNS = ()

    def __init__(self, rate):
        self.rate = rate
        self._rows = []         # (state, family, side, *columns)

    def add(self, state, family, side=-1, **columns):
        self._rows.append((np.array(state, dtype=np.float64), self.FAMILIES.index(family), side) + tuple([float(columns[c]) for c in self.COLUMNS]))

    def freeze(self):
        rows = self._rows
        del self._rows
        self.states = np.ascontiguousarray(np.stack([r[0] for r in rows]))
        self.family = np.array([r[1] for r in rows], dtype=np.int32)
        self.side = np.array([r[2] for r in rows], dtype=np.int32)
        for k, name in enumerate(self.COLUMNS):
            setattr(self, name, np.array([r[3 + k] for r in rows]))
        self.n = self.states.shape[0]
        return self


def bisect_edges(count, bases, rows, mags_hi):
    """States on either side of one of a step's decisions.  count(states [m][width]) -> the info column that counts the decision.  One
    row of a base state is moved, and the moved value is bisected between the base's own (the column as the base has it) and one at
    which the column is larger, down to NEIGHBOURING doubles of the state row; those two and the next three doubles on either side are
    yielded as (state, side), side 0 first.  Every (base, row, sign, starting magnitude) is tried; the ones whose ends differ are kept."""
    trials = [(b, r, s * m) for b in bases for r in rows for s in (1.0, -1.0) for m in mags_hi]
    st0 = np.stack([t[0] for t in trials]); row = np.array([t[1] for t in trials]); idx = np.arange(len(trials))
    lo = st0[idx, row].copy(); hi = lo + np.array([t[2] for t in trials])

    def column(x):
        st = st0.copy(); st[idx, row] = x
        return count(st)
    c0 = column(lo)

    def f(x):
        return column(x) > c0
    ok = f(hi)
    for _ in range(1100):
        mid = 0.5 * (lo + hi)
        stop = (mid == lo) | (mid == hi)
        if stop.all():
            break
        t = f(mid)
        lo = np.where(~t & ~stop, mid, lo); hi = np.where(t & ~stop, mid, hi)
    for i in np.nonzero(ok)[0]:
        for side, (x0, away) in enumerate(((lo[i], -math.inf if hi[i] > lo[i] else math.inf), (hi[i], math.inf if hi[i] > lo[i] else -math.inf))):
            x = x0
            for _ in range(4):
                st = st0[i].copy(); st[row[i]] = x
                yield st, side
                x = math.nextafter(x, away)


def within_bar(a, o, groups):
    """Per case: |a - o| <= 1e-5 |o| + floor on every row of every group; groups = ((rows, floor), ...), rows indexing the second axis of
    a and o ([n][width]), or None for per-case values ([n])."""
    ok = np.ones(a.shape[0], dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, floor in groups:
            x, y = (a, o) if rows is None else (a[:, rows], o[:, rows])
            ok &= (np.abs(x - y) <= 1e-5 * np.abs(y) + floor).reshape(ok.size, -1).all(axis=1)
    return ok


def floor_governed(a, o, groups):
    """Per group: the largest |a - o| over the finite rows whose tolerance in within_bar is governed by the floor rather than by the
    relative term (1e-5 |o| < floor) -- what a floor has to cover."""
    worst = []
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, floor in groups:
            x, y = (a, o) if rows is None else (a[:, rows], o[:, rows])
            g = np.isfinite(x) & np.isfinite(y) & (1e-5 * np.abs(y) < floor)
            worst.append(float(np.abs(x - y)[g].max()) if g.any() else 0.0)
    return tuple(worst)


def cached(build):
    """build(ob), computed once per process and never changed."""
    box = []

    def get(ob):
        if not box:
            box.append(build(ob))
        return box[0]
    return get


def coverage(refs, class_names):
    """Per exit class over all rates: (name, cases, comparable among them); the finite cases and the non-comparable ones among them."""
    rows = []
    for c, name in enumerate(class_names):
        n = sum(int(r.classes[:, c].sum()) for r in refs.values())
        comp = sum(int((r.classes[:, c] & r.comparable).sum()) for r in refs.values())
        rows.append((name, n, comp))
    fin = sum(int(r.finite.sum()) for r in refs.values())
    return {"classes": rows, "finite": fin, "ill": fin - sum(int(r.comparable.sum()) for r in refs.values()),
            "cases": sum(r.finite.size for r in refs.values())}


def check_coverage(mod, ob, empty=(), ill_per_class=False):
    """What every corpus has to reach (mod: a solver's corpus module).  Every class holds MIN_CLASS cases of which MIN_COMPARABLE are
    comparable -- but the classes in `empty`, which a solver documents as unreachable and which must then BE empty; at most MAX_ILL_SHARE
    of the finite cases (ill_per_class: of each class) are not comparable; every family is present at every rate; no non-finite case
    is comparable; and for each family of EDGE_COLUMN both sides of the bisected decision are present, the boundary pairs (the first
    case of each side) differ in the decision's info column, in exactly one state row, and there by neighbouring doubles."""
    cov = coverage(mod.references(ob), mod.CLASS_NAMES)
    for name, n, comp in cov["classes"]:
        if name in empty:
            assert n == 0, "%s exists: give the class its minimum" % name
            continue
        assert n >= mod.MIN_CLASS, (name, n)
        assert comp >= mod.MIN_COMPARABLE, (name, comp)
        assert not ill_per_class or n - comp <= mod.MAX_ILL_SHARE * n, (name, n, n - comp)
    assert ill_per_class or cov["ill"] <= mod.MAX_ILL_SHARE * cov["finite"], cov
    refs = mod.references(ob)
    assert set(refs) == set(mod.RATES)
    for rate, cs in mod.corpus(ob).items():
        r = refs[rate]
        assert set(np.unique(cs.family)) == set(range(len(mod.FAMILIES))), (rate, np.unique(cs.family))
        assert not r.comparable[~r.finite].any()
        for fam, col in getattr(mod, "EDGE_COLUMN", {}).items():
            m = cs.family == mod.FAMILIES.index(fam)
            lo = np.nonzero(m & (cs.side == 0))[0][0::4]; hi = np.nonzero(m & (cs.side == 1))[0][0::4]
            assert lo.size >= 4 and lo.size == hi.size, (rate, fam, lo.size, hi.size)
            assert (r.info[hi, col] > r.info[lo, col]).all(), (rate, fam)
            d = np.abs(cs.states[hi] - cs.states[lo])
            assert ((d > 0).sum(axis=1) == 1).all() and (np.nextafter(cs.states[lo], cs.states[hi]) == cs.states[hi]).all(), (rate, fam)


def cases_of(units, unit):
    """The case indices of the units `units` of `unit` consecutive cases each (2: (main, shadow) pairs), in that order."""
    return (unit * np.asarray(units)[:, None] + np.arange(unit)[None, :]).reshape(-1)


def whole_units(mask, unit):
    """The units all of whose cases are in `mask`."""
    return np.nonzero(mask.reshape(-1, unit).all(axis=1))[0]


def arrangements(sort_keys, n, unit, seeds, ragged_cut):
    """Orders of n cases, as case indices, units kept together: wavefronts uniform in their exits (units sorted by sort_keys,
    np.lexsort's order: last key first), wavefronts that mix everything (a fixed shuffle, seeds[0]), and a ragged tail (another
    shuffle, seeds[1], cut to ragged_cut cases: last wavefronts partly filled)."""
    units = n // unit
    return {"uniform": cases_of(np.lexsort((np.arange(units),) + tuple(sort_keys)), unit),
            "mixed": cases_of(np.random.default_rng(seeds[0]).permutation(units), unit),
            "ragged": cases_of(np.random.default_rng(seeds[1]).permutation(units), unit)[:ragged_cut]}
