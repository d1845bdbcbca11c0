"""The single-step corpus of tests/mel_step_cases.py, checked on the CPU oracle alone before any kernel is measured against it: it has to
reach every way the melange preamp's set_runtime_R; process_sample can go, often enough, and the reference algorithm itself has to pin
the results there (the oracle with pnjlim's logarithm or the rebuilt resistance one double away, either way, keeps its fallback, reset
and cooldown decisions and stays within the state-row bar of the unperturbed one).  tests/test_gpu_mel_step.py compares the kernels on
exactly the cases this file accepts."""
import math

import numpy as np

import oracle_binding as ob
import mel_step_cases as mc
import step_cases as sc


def test_step_entry_is_the_solvers_own_step():
    """owo_melange_step_cases pushes a state row through set_runtime_r_ldr; process_sample: fed the successive states of a running solver
    state it reproduces that run bit for bit, row and return value -- an overdriven run and a depth-1 tremolo run whose resistance moves
    on every sample, at a rebuilt rate and at the codegen rate (baked tables until the first resistance arrives) -- and main minus shadow
    is owo_melange_run's output; the two knobs are off outside the call that sets them."""
    for rate in (96000.0, mc.CODEGEN_RATE):
        n = 1500
        x = 1.5 * np.sin(2.0 * math.pi * 1000.0 * np.arange(n) / rate)
        r = np.zeros(n)
        ob.lib().owo_tremolo_run(ob.C.c_double(1.0), ob.C.c_double(96000.0), ob._p(r), ob.C.c_size_t(n))
        for rr in (None, r):
            y_run = np.zeros(n)
            ob.lib().owo_melange_run(ob.C.c_double(rate), ob._p(x), None if rr is None else ob._p(rr), ob._p(y_run), ob.C.c_size_t(n))
            outs = []
            for xx in (x, None):
                run, y = ob.melange_harvest(rate, n, 1, x=xx, r=rr)
                r_case = run[:-1, 19] if rr is None else rr[:-1]
                got, out, info = ob.melange_step_cases(rate, run[:-1], np.zeros(n - 1) if xx is None else xx[:-1], r_case)
                assert got.tobytes() == run[1:].tobytes(), (rate, rr is None, xx is None)
                assert out.tobytes() == y[:-1].tobytes()
                assert (info[:, 11] == (0 if rr is None else 1)).all() and (info[:, 10] == 0).all()
                outs.append(y)
            assert np.array_equal(outs[0] - outs[1], y_run), rate
    cs = mc.corpus(ob)[96000.0]
    a = ob.melange_step_cases(96000.0, cs.states, cs.x, cs.r)
    ob.melange_step_cases(96000.0, cs.states, cs.x, cs.r, log_ulp=1, r_ulp=1)
    b = ob.melange_step_cases(96000.0, cs.states, cs.x, cs.r)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    # the knobs do reach the step: a logarithm one double away moves some case, and so does a resistance far enough away to survive
    # the addition into G[6][6] (one double of a resistance does not: see test_oracle_sensitivity.py::test_melange_step_floors)
    c = ob.melange_step_cases(96000.0, cs.states, cs.x, cs.r, log_ulp=1)
    d = ob.melange_step_cases(96000.0, cs.states, cs.x, cs.r, r_ulp=4096)
    assert c[0].tobytes() != a[0].tobytes() and d[0].tobytes() != a[0].tobytes()


def test_corpus_is_deterministic_and_paired():
    a = mc.corpus(ob)
    b = mc._build_rate(ob, 96000.0)
    cs = a[96000.0]
    assert b.states.tobytes() == cs.states.tobytes() and np.array_equal(b.family, cs.family)
    assert b.x.tobytes() == cs.x.tobytes() and b.r.tobytes() == cs.r.tobytes()
    for cs in a.values():
        # case 2k+1 has input 0 and case 2k's resistance and pot: what one engine's two solver states can be
        assert cs.n % 2 == 0 and (cs.x[1::2] == 0.0).all()
        assert cs.r[1::2].tobytes() == cs.r[0::2].tobytes() and cs.states[1::2, 19].tobytes() == cs.states[0::2, 19].tobytes()
        assert set(np.unique(cs.states[:, 20])) >= set(float(c) for c in mc.COOLDOWNS)     # (harvested states carry their run's counts too)


def test_corpus_reaches_every_exit_and_the_reference_pins_it():
    """Class sizes and comparable counts of the corpus, measured on the oracle (printed; DESIGN.md section 4.1 carries them).  Every
    class holds at least 256 cases of which at least 64 are comparable; at most 10 % of the finite cases are not comparable; every family
    of the generator is present at every rate, the codegen rate and rebuilt rates among them; the bisected decisions are really straddled.

    The SINGULAR SWEEP class cannot reach its minimum: it is empty.  A sweep is singular when a pivot of I - J K falls below 1e-15 in
    absolute value.  J's entries are >= 0 (IS/nVt * exp), K's diagonal is negative at every rate and resistance (a junction current
    lowers its own junction voltage), so the diagonal of I - J K is >= 1 and partial pivoting starts from a pivot >= 1; a later pivot
    below 1e-15 needs the elimination to cancel to 50 bits, which no state was found to produce.  Searched (singular_search below):
    40 000 random multi-row kicks of 1 mV .. 30 V / 1 uA .. 30 mA per rate at random resistances on top of the corpus.  No case was
    invented; the test fails if one turns up, so that it is then added."""
    cov = sc.coverage(mc.references(ob), mc.CLASS_NAMES)
    print()
    print("mel_step corpus: %d cases (%s per rate), %d finite, %d of them not comparable (%.3f %%)" % (
        cov["cases"], ", ".join("%d" % cs.n for cs in mc.corpus(ob).values()), cov["finite"], cov["ill"], 100.0 * cov["ill"] / cov["finite"]))
    for name, n, comp in cov["classes"]:
        print("  %-30s %6d cases  comparable %6d" % (name, n, comp))
    print("  floors (oracle_binding): %.1e V, %.1e A" % (ob.ABS_FLOOR_MELANGE_STEP_V, ob.ABS_FLOOR_MELANGE_STEP_I))
    sc.check_coverage(mc, ob, empty=(mc.CLASS_NAMES[mc.SINGULAR],))
    refs = mc.references(ob)
    assert mc.CODEGEN_RATE in refs and len(refs) >= 4
    sweeps = set()
    for rate, cs in mc.corpus(ob).items():
        r = refs[rate]
        sweeps |= set(r.info[r.info[:, 1] == 0, 0].tolist())
        # non-finite voltages, currents and input_prev all end in the reset (an infinite pot is a conductance of zero: the step goes
        # through); non-finite inputs and resistances never do on their own
        ext = cs.family == mc.FAMILIES.index("extreme")
        assert r.nan_reset[ext & ~np.isfinite(cs.states[:, :19]).all(axis=1)].all()
        guarded = (cs.family == mc.FAMILIES.index("input")) | ((cs.family == mc.FAMILIES.index("resistance")) & ~np.isfinite(cs.r))
        assert r.finite[guarded].all() and not r.nan_reset[guarded].any()
        # the cooldown counts down by one where nothing re-arms it and is re-armed to 64 by ringing or exhaustion
        cd_in = cs.states[:, 20]; cd_out = r.states[:, 20]; arm = (r.info[:, 3] > 0) | (r.info[:, 4] > 0)
        ok = r.finite & ~r.nan_reset
        assert (cd_out[ok & arm] == 64.0).all() and (cd_out[ok & ~arm] == np.maximum(cd_in[ok & ~arm] - 1.0, 0.0)).all()
        assert (r.info[ok, 5] == (cd_in[ok] > 0)).all()
        # the hysteresis: a resistance within 1e-12 of pot leaves pot and the matrices alone, one beyond it replaces pot
        res = ok & (cs.family == mc.FAMILIES.index("resistance"))
        assert (r.states[res & r.classes[:, 15], 19] == cs.states[res & r.classes[:, 15], 19]).all()
        assert (r.info[res & r.classes[:, 15], 11] == 0).all() and (r.info[res & ~r.classes[:, 15], 11] == 1).all()
        moved = res & ~r.classes[:, 15]
        assert (r.states[moved, 19] == np.clip(cs.r[moved], 1000.0, 1000000.0)).all()
        assert (res & r.classes[:, 15] & (cs.r != cs.states[:, 19]) & np.isfinite(cs.r)).sum() >= 16      # really within, not equal
    assert len(sweeps & set(range(1, 266))) >= 100, sorted(sweeps)     # a wide spread of sweep counts occurs


def singular_search(rate, n=40000):
    rng = np.random.default_rng(4343 + int(rate))
    cs = mc.corpus(ob)[rate]
    base = cs.states[cs.family == mc.FAMILIES.index("base")]
    st = base[rng.integers(base.shape[0], size=n)].copy()
    scale = 10.0 ** rng.uniform(-3.0, 1.5, size=(n, 1))
    st[:, :12] += scale * rng.standard_normal((n, 12)) * (rng.random((n, 12)) < 0.5)
    st[:, 12:18] += 1e-3 * scale * rng.standard_normal((n, 6)) * (rng.random((n, 6)) < 0.4)
    r = 10.0 ** rng.uniform(3.0, 6.0, size=n)
    return int((ob.melange_step_cases(rate, st, np.zeros(n), r)[2][:, 8] > 0).sum())


def test_singular_sweep_search():
    found = {rate: singular_search(rate) for rate in mc.RATES}
    in_corpus = sum(int(r.classes[:, mc.SINGULAR].sum()) for r in mc.references(ob).values())
    print("\nsingular-sweep search: %s, in the corpus: %d" % (found, in_corpus))
    assert all(v == 0 for v in found.values()) and in_corpus == 0, "a singular sweep exists: add it to the corpus (mel_step_cases.py) and to its classes"
