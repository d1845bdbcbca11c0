"""The single-step corpus of tests/dk_step_cases.py, checked on the CPU oracle alone before any kernel is measured against it: it has to
reach every way DkPreamp::dk_step's Newton loop can end, often enough, and the reference algorithm itself has to pin the results there
(one-ulp-exp oracle within the state-row bar of the unperturbed one).  tests/test_gpu_dk_step.py compares the kernels on exactly the
cases this file accepts."""
import numpy as np

import dk_step_cases as dk
import oracle_binding as ob
import step_cases as sc


def test_step_entry_is_the_engines_own_step():
    """owo_dk_step_cases pushes a state through DkPreamp::dk_step: fed an engine's solver states, its g_ldr and the input that state saw,
    it returns what the engine's next sample makes of them -- checked on the shadow state, whose input is 0.0 by construction, at depth 0
    after the cell's R has come to rest (no set_ldr_resistance change between two samples)."""
    e = ob.OracleEngine(48000.0)
    e.set_sample_rate(48000.0)
    e.set_tremolo_depth(0.0)
    e.note_on(60, 0.8)
    e.render(4096)
    for _ in range(3):
        s0, ldr0 = e.preamp_state(True)[:14].copy(), e.preamp_ldr()
        e.render(1)                                              # two chain-rate steps
        s2, ldr2 = e.preamp_state(True)[:14], e.preamp_ldr()
        assert ldr0[1] == ldr0[2] == ldr2[1], (ldr0, ldr2)       # R at rest: g_ldr == g_ldr_prev throughout
        g = np.array([ldr0[1]])
        s1 = ob.dk_step_cases(96000.0, s0[None, :], np.zeros(1), g, g)[0]
        got, out, info = ob.dk_step_cases(96000.0, s1, np.zeros(1), g, g)
        assert got[0].tobytes() == s2.tobytes()
        assert out[0] == got[0][2 + 6] and 0 <= info[0][0] <= 6
    e.close()


def test_corpus_is_deterministic():
    a = dk.corpus(ob)
    b = {rate: dk._build_rate(ob, rate) for rate in (96000.0,)}
    for rate, cs in b.items():
        assert cs.states.tobytes() == a[rate].states.tobytes() and cs.inputs.tobytes() == a[rate].inputs.tobytes()
        assert cs.g.tobytes() == a[rate].g.tobytes() and cs.gp.tobytes() == a[rate].gp.tobytes()


def test_corpus_reaches_every_exit_and_the_reference_pins_it():
    """Class sizes and ill-conditioned shares of the corpus, measured on the oracle (printed; DESIGN.md section 4.1 carries them):
    every exit class -- 0 .. 5 updates then converged, six updates unconverged, a junction evaluation clamped at 0.85 V, at -1 V -- holds at
    least 256 cases, at most 10 % of a class are ill-conditioned (the one-ulp-exp oracle leaves the state-row bar) and at least 230 of it
    are comparable; at least 256 (main, shadow) pairs differ in their update counts, in at least 64 the shadow needs more; every family of
    the generator is present at every rate; non-finite results are kept, labelled, and sit in no class.

    The singular exit (|det| < 1e-30) was searched for and NOT found -- no case was invented.  The search (singular_search below): at each
    rate and at g_ldr in {1e-6, 7.6e-5, 1e-3} S, every pair of junction voltages on a 600 x 600 grid over [-1.05 V, 0.9 V] (i_nl consistent)
    and 300 000 random pairs, as the opening state of a step (the first sweep's 2x2 is formed at exactly those voltages), plus every case
    of the corpus.  det = (1 - k00 gm0)(1 - k11 gm1) - k01 k10 gm0 gm1 is 1 when both junctions are off and a sum of O(1) .. O(1e9) terms
    otherwise; |det| < 1e-30 would need them to cancel to 100 bits."""
    refs = dk.references(ob)
    cov = sc.coverage(refs, dk.CLASS_NAMES)
    differ, shadow_more, singular = dk.pair_statistics(refs)
    print()
    print("dk_step corpus: %d cases (%s per rate)" % (cov["cases"], ", ".join("%d" % cs.n for cs in dk.corpus(ob).values())))
    for name, n, comp in cov["classes"]:
        print("  %-26s %6d cases  ill-conditioned %5d (%.2f %%)  comparable %6d" % (name, n, n - comp, 100.0 * (n - comp) / max(n, 1), comp))
    print("  pairs whose update counts differ: %d, shadow needs more: %d; singular exits: %d; non-finite results: %d"
          % (differ, shadow_more, singular, cov["cases"] - cov["finite"]))
    sc.check_coverage(dk, ob, ill_per_class=True)
    assert differ >= 256 and shadow_more >= 64, (differ, shadow_more)
    assert cov["cases"] - cov["finite"] >= 1
    for rate, cs in dk.corpus(ob).items():
        r = refs[rate]
        assert not (r.classes[~r.finite]).any()
        # the clamp edges and the tolerance edge are really straddled
        edge = cs.family == dk.FAMILIES.index("junction edge")
        vn = cs.states[edge][:, 12:14]
        for lim in (-1.0, dk.VBE_MAX):
            assert (vn == lim).any() and (vn == np.nextafter(lim, np.inf)).any() and (vn == np.nextafter(lim, -np.inf)).any()
        tol = cs.family == dk.FAMILIES.index("tolerance edge")
        assert (r.info[tol, 0] == 0).sum() >= 8 and (r.info[tol, 0] == 1).sum() >= 8, (rate, np.bincount(r.info[tol, 0]))


def singular_search(rate, n_grid=600, n_random=300000):
    """Number of steps that leave through |det| < 1e-30 among grid and random junction-voltage pairs (see the test's docstring)."""
    rng = np.random.default_rng(99)
    base = dk.corpus(ob)[rate].states[0]
    ax = np.linspace(-1.05, 0.9, n_grid)
    v0, v1 = np.meshgrid(ax, ax, indexing="ij")
    vn = np.concatenate([np.stack([v0.ravel(), v1.ravel()], axis=1), rng.uniform(-1.05, 0.9, (n_random, 2))])
    st = np.tile(base, (vn.shape[0], 1))
    st[:, 12:14] = vn
    st[:, 10:12] = dk.IS * (np.exp(np.clip(vn, -1.0, dk.VBE_MAX) / dk.VT) - 1.0)
    found = 0
    for g in (1e-6, 7.6e-5, 1e-3):
        gg = np.full(vn.shape[0], g)
        info = ob.dk_step_cases(rate, st, np.zeros(vn.shape[0]), gg, gg)[2]
        found += int((info[:, 1] == ob.DK_EXIT_SINGULAR).sum())
    return found


def test_singular_exit_search():
    found = {rate: singular_search(rate) for rate in dk.RATES}
    in_corpus = sum(int(r.singular.sum()) for r in dk.references(ob).values())
    print("\nsingular-determinant search: %s, in the corpus: %d" % (found, in_corpus))
    assert all(v == 0 for v in found.values()) and in_corpus == 0, "a singular exit exists: add it to the corpus (dk_step_cases.py) and to its classes"
