"""The single-step corpus of tests/trem_step_cases.py, checked on the CPU oracle alone before any kernel is measured against it: it has
to reach every way TremCircuit::process_sample's solver can go, often enough, and the reference algorithm itself has to pin the results
there (the oracle with pnjlim's logarithm one double away, either way, keeps its exits and stays within the state-row bar of the
unperturbed one).  tests/test_gpu_trem_step.py compares the kernels on exactly the cases this file accepts."""
import numpy as np

import oracle_binding as ob
import step_cases as sc
import trem_step_cases as tc


def test_step_entry_is_the_circuits_own_step():
    """owo_trem_step_cases pushes a state through TremCircuit::process_sample(0.0): fed the states of a running oscillator one after the
    other it reproduces that run bit for bit, output included (owo_tremolo_osc: the circuit after Tremolo::new's settle), at a rebuilt rate
    and at the codegen rate; and the log_ulp knob is off outside the call that sets it."""
    for rate in (96000.0, tc.CODEGEN_RATE):
        run = ob.trem_harvest(rate, 400, 1)
        got, out, info = ob.trem_step_cases(rate, run[:-1])
        assert got.tobytes() == run[1:].tobytes()
        assert np.array_equal(out, got[:, 0]) and (info[:, 3] == 1).all() and (info[:, 1] == 0).all()
        n = int(2.0 * rate)
        osc = np.zeros(8)
        host = rate if rate >= 88200.0 else rate      # (Tremolo::init takes the chain rate itself)
        ob.lib().owo_tremolo_osc(ob.C.c_double(host), ob._p(osc), ob.C.c_size_t(8))
        st = ob.trem_harvest(rate, n + 1, n)[1:2]
        for k in range(8):
            st, o, _ = ob.trem_step_cases(rate, st)
            assert o[0] == osc[k], (rate, k)
    cs = tc.corpus(ob)[96000.0]
    a = ob.trem_step_cases(96000.0, cs.states)
    ob.trem_step_cases(96000.0, cs.states, log_ulp=1)
    b = ob.trem_step_cases(96000.0, cs.states)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


def test_corpus_is_deterministic():
    a = tc.corpus(ob)
    b = tc._build_rate(ob, 96000.0)
    assert b.states.tobytes() == a[96000.0].states.tobytes() and np.array_equal(b.family, a[96000.0].family)


def test_corpus_reaches_every_exit_and_the_reference_pins_it():
    """Class sizes and comparable counts of the corpus, measured on the oracle (printed; DESIGN.md section 4.1 carries them).  Every
    class -- converged at sweep 0, 1-5, 6-49, retry converged, retry exhausted, a pivot exchange, pnjlim's logarithm, the 3.5 V cap, the
    NaN reset -- holds at least 256 cases of which at least 64 are comparable; at most 10 % of the finite cases are not comparable; every
    family of the generator is present at every rate, the codegen rate and rebuilt rates among them; the bisected decisions are really
    straddled.

    The SINGULAR SWEEP class cannot reach its minimum: it is empty.  A sweep is singular when a pivot of I - J K falls below 1e-15 in
    absolute value; the entries of J K are 0 (junctions off: the matrix is I) or up to 1e8 (exponentials at fast_exp's clamp), and the
    unit diagonal leaves pivots of order 1 or rounding noise of order 1e-8 where K's rank deficiency (its fourth port is the difference
    of two others) cancels the rest: below 1e-15 needs a cancellation to 50 bits that no state was found to produce.  Searched
    (singular_search below): 60 000 random multi-row kicks of 1 mV .. 30 V / 1 uA .. 30 mA per rate on top of the corpus.  No case was
    invented; the test fails if one turns up, so that it is then added."""
    cov = sc.coverage(tc.references(ob), tc.CLASS_NAMES)
    print()
    print("trem_step corpus: %d cases (%s per rate), %d finite, %d of them not comparable (%.3f %%)" % (
        cov["cases"], ", ".join("%d" % cs.n for cs in tc.corpus(ob).values()), cov["finite"], cov["ill"], 100.0 * cov["ill"] / cov["finite"]))
    for name, n, comp in cov["classes"]:
        print("  %-26s %6d cases  comparable %6d" % (name, n, comp))
    print("  floors (oracle_binding): %.1e V, %.1e A" % (ob.ABS_FLOOR_TREM_STEP_V, ob.ABS_FLOOR_TREM_STEP_I))
    sc.check_coverage(tc, ob, empty=("singular sweep",))
    refs = tc.references(ob)
    assert tc.CODEGEN_RATE in refs and len(refs) >= 4
    iters = set()
    for rate, cs in tc.corpus(ob).items():
        r = refs[rate]
        iters |= set(r.info[(r.info[:, 1] == 0), 0].tolist())
        # the non-finite kicks all end in the reset
        ext = cs.family == tc.FAMILIES.index("extreme")
        assert r.nan_reset[ext & ~np.isfinite(cs.states).all(axis=1)].all()
    assert len(iters & set(range(50))) >= 40, sorted(iters)     # (almost) every iteration count occurs


def singular_search(rate, n=60000):
    rng = np.random.default_rng(4242 + int(rate))
    cs = tc.corpus(ob)[rate]
    base = cs.states[cs.family == tc.FAMILIES.index("settled")]
    st = base[rng.integers(base.shape[0], size=n)].copy()
    scale = 10.0 ** rng.uniform(-3.0, 1.5, size=(n, 1))
    st[:, :7] += scale * rng.standard_normal((n, 7)) * (rng.random((n, 7)) < 0.6)
    st[:, 7:] += 1e-3 * scale * rng.standard_normal((n, 8)) * (rng.random((n, 8)) < 0.4)
    return int((ob.trem_step_cases(rate, st)[2][:, 6] > 0).sum())


def test_singular_sweep_search():
    found = {rate: singular_search(rate) for rate in tc.RATES}
    in_corpus = sum(int(r.classes[:, 6].sum()) for r in tc.references(ob).values())
    print("\nsingular-sweep search: %s, in the corpus: %d" % (found, in_corpus))
    assert all(v == 0 for v in found.values()) and in_corpus == 0, "a singular sweep exists: add it to the corpus (trem_step_cases.py) and to its classes"
