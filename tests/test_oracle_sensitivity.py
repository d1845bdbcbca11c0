"""Measures the reference ALGORITHM's own indeterminacy on the CPU oracle: the legacy preamp's Newton loop stops at
|f| < 1e-9 V (dk_preamp_legacy.rs:500), and the shadow solver's warm start "sticks" until its residual crosses that
threshold.  A libm whose exp() differs in the last bit therefore moves the output by a few 1e-10 -- independent of
signal level.  This is the absolute floor the GPU parity tests add to the 1e-5 relative bar."""
import numpy as np


def _run(oracle, perturbed):
    e = oracle.OracleEngine(48000.0, perturbed=perturbed)
    e.set_volume(0.5); e.set_tremolo_depth(0.5); e.set_speaker_character(0.0); e.set_mlp_enabled(True)
    for n in (45, 60, 64, 79):
        e.note_on(n, 0.8)
    outs, pres = [], []
    for _ in range(16):
        o, _, p, _ = e.render_taps(256)
        outs.append(o.astype(np.float64)); pres.append(p)
    e.close()
    return np.concatenate(outs), np.concatenate(pres)


def test_one_ulp_exp_moves_the_reference_by_less_than_the_floor(oracle):
    o0, p0 = _run(oracle, False)
    o1, p1 = _run(oracle, True)
    d_out = np.max(np.abs(o1 - o0))
    d_pre = np.max(np.abs(p1 - p0))
    assert d_pre > 1e-12          # the effect exists (it is not rounding noise of ~1e-16 * 8 V)
    assert d_pre < oracle.ABS_FLOOR_PREAMP, d_pre
    assert d_out < oracle.ABS_FLOOR_OUTPUT, d_out
    # and it is tiny against the 1e-5 relative bar at musical level
    assert d_out / np.max(np.abs(o0)) < 1e-5 * 1e-1


def test_output_and_preamp_floor_governing_measurement(oracle):
    """The four-note scenario of the parity tests over 0.5 s (96 blocks of 256; the 16 blocks above are the shortest tests) at tremolo
    depths 0.5 and 0.8: on the samples the 2e-9 floors govern, the reference algorithm itself moves by 4.5-5e-9 at the output and
    3.2-5e-9 at the preamp node when exp() is off by one ulp -- the floors are TIGHTER than that (0.4 of it): the GPU passes them because
    its junction exponential is the library's, bit for bit, not a one-ulp neighbour.  Row 1 and 2 of DESIGN.md's floor table."""
    worst_out, worst_pre = 0.0, 0.0
    for depth in (0.5, 0.8):
        res = []
        for pert in (False, True):
            e = oracle.OracleEngine(48000.0, perturbed=pert)
            e.set_volume(0.5); e.set_tremolo_depth(depth); e.set_speaker_character(0.0); e.set_mlp_enabled(True)
            for n in (45, 60, 64, 79):
                e.note_on(n, 0.8)
            outs, pres = [], []
            for _ in range(96):
                o, _, p, _ = e.render_taps(256)
                outs.append(o.astype(np.float64)); pres.append(p)
            e.close()
            res.append((np.concatenate(outs), np.concatenate(pres)))
        worst_out = max(worst_out, oracle.floor_governed_delta(res[0][0], res[1][0], oracle.ABS_FLOOR_OUTPUT))
        worst_pre = max(worst_pre, oracle.floor_governed_delta(res[0][1], res[1][1], oracle.ABS_FLOOR_PREAMP))
    print(f"\n[floor table] ABS_FLOOR_OUTPUT {oracle.ABS_FLOOR_OUTPUT:.1e}: one-ulp {worst_out:.2e} (ratio {oracle.ABS_FLOOR_OUTPUT / worst_out:.2f}); "
          f"ABS_FLOOR_PREAMP {oracle.ABS_FLOOR_PREAMP:.1e}: one-ulp {worst_pre:.2e} (ratio {oracle.ABS_FLOOR_PREAMP / worst_pre:.2f})")
    assert oracle.ABS_FLOOR_OUTPUT <= oracle.FLOOR_RULE * worst_out and worst_out < 2e-8, worst_out
    assert oracle.ABS_FLOOR_PREAMP <= oracle.FLOOR_RULE * worst_pre and worst_pre < 2e-8, worst_pre


def test_batch_job_floor(oracle):
    worst, worst_any = 0.0, 0.0
    for note, vel in ((96, 50), (60, 127), (33, 50), (84, 127)):
        a = oracle.batch_render_job(note, vel, 0.75, 44100.0)
        b = oracle.batch_render_job(note, vel, 0.75, 44100.0, perturbed=True)
        worst = max(worst, oracle.floor_governed_delta(a, b, oracle.ABS_FLOOR_BATCH))
        worst_any = max(worst_any, float(np.max(np.abs(a - b))))
        assert np.max(np.abs(a - b)) / np.max(np.abs(a)) < 1e-5 * 0.2     # far inside the 1e-5 bar relative to peak
    # the treble end of the 16-job subset at config 4's own length and rate (tests/test_gpu_parity.py::test_batch_render_jobs[48000.0]): a
    # short decay, 4 s of tail at the level the floor governs -- the reference moves by 2.6e-8 there, and that is where the GPU's own
    # worst batch error (2.5e-8) sits
    a = oracle.batch_render_job(96, 50, 5.0, 48000.0)
    b = oracle.batch_render_job(96, 50, 5.0, 48000.0, perturbed=True)
    worst = max(worst, oracle.floor_governed_delta(a, b, oracle.ABS_FLOOR_BATCH))
    print(f"\n[floor table] ABS_FLOOR_BATCH {oracle.ABS_FLOOR_BATCH:.1e}: one-ulp {worst:.2e} on the samples it governs ({worst_any:.2e} anywhere), ratio {oracle.ABS_FLOOR_BATCH / worst:.2f}")
    assert 1e-10 < worst < oracle.ABS_FLOOR_BATCH, worst
    assert oracle.ABS_FLOOR_BATCH <= oracle.FLOOR_RULE * worst, worst


def test_melange_floor(oracle):
    """Melange 12-node preamp: response of the literal-LU oracle to R_ldr moving by one ulp."""
    def run(perturbed):
        e = oracle.OracleEngine(48000.0, perturbed=perturbed, preamp_kind=1)
        e.set_tremolo_depth(0.5)
        for n in (48, 60, 67):
            e.note_on(n, 0.8)
        outs, pres = [], []
        for _ in range(12):
            o, _, p, _ = e.render_taps(512)
            outs.append(o.astype(np.float64)); pres.append(p)
        e.close()
        return np.concatenate(outs), np.concatenate(pres)
    o0, p0 = run(False)
    o1, p1 = run(True)
    assert np.max(np.abs(p1 - p0)) < 5e-9 < oracle.ABS_FLOOR_MELANGE_PREAMP
    assert np.max(np.abs(o1 - o0)) < 2e-8          # f32 rounding flips at |x| ~ 0.1 are 7.5e-9


def test_melange_floor_with_r_ldr_off_by_one_ulp(oracle):
    """The melange preamp re-inverts its 12x12 system whenever R_ldr moved; the rounding noise of that LU inverse (eps * cond(A)) is a
    chaotic function of R's bits.  R comes out of exp() / powf() (tremolo.rs:140-141), so two builds of the REFERENCE with libms that
    differ in the last place hear different noise.  Measured here on the oracle alone: the tremolo's R stream at depth 1.0, then the
    same stream with every value moved to its neighbouring double.  This is the floor the GPU (whose device library is such a
    different libm) can be held to at the preamp node: 5e-8 V covers it with margin; the output floor follows through the chain gain."""
    import ctypes as C
    L = oracle.lib()
    sr = 96000.0
    n = int(sr * 1.0)
    r = np.zeros(n)
    L.owo_tremolo_run(C.c_double(1.0), C.c_double(sr), r.ctypes.data_as(C.c_void_p), C.c_size_t(n))
    x = 0.01 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)

    def run(rr):
        y = np.zeros(n)
        L.owo_melange_run(C.c_double(sr), x.ctypes.data_as(C.c_void_p), rr.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_size_t(n))
        return y
    y0 = run(r)
    y1 = run(np.nextafter(r, np.inf))
    d = float(np.max(np.abs(y1 - y0)))
    assert 1e-9 < d < oracle.ABS_FLOOR_MELANGE_LIT_PREAMP, d          # measured 1.4e-8 V on a 71 mV signal
    # a fast sweep of R (what a depth-knob ramp does to the shunt): same experiment
    rs = 19e3 + (1e6 - 19e3) * (0.5 + 0.5 * np.sin(2 * np.pi * 40.0 * np.arange(n) / sr))
    d2 = float(np.max(np.abs(run(np.nextafter(rs, np.inf)) - run(rs))))
    assert d2 < oracle.ABS_FLOOR_MELANGE_LIT_PREAMP, d2
    dm = max(d, d2)
    print(f"\n[floor table] ABS_FLOOR_MELANGE_LIT_* {oracle.ABS_FLOOR_MELANGE_LIT_PREAMP:.1e}: R off by one ulp moves the node by {dm:.2e}, ratio {oracle.ABS_FLOOR_MELANGE_LIT_PREAMP / dm:.2f}")
    assert oracle.ABS_FLOOR_MELANGE_LIT_PREAMP <= oracle.FLOOR_RULE * dm and oracle.ABS_FLOOR_MELANGE_LIT_OUTPUT <= oracle.FLOOR_RULE * dm, dm


def test_alias_audit_stimulus_floor(oracle):
    """The audit stimulus (alias_audit.rs:135-160) under the same one-ulp exp() experiment: quiet samples move by up to 2.5e-9,
    and the audit's dB figures (harmonics 70-110 dB below H1) by up to a few 1e-3 dB -- the tolerances of tests/test_gpu_alias_audit.py."""
    worst_quiet, worst_db = 0.0, 0.0
    for note in (72, 84, 91):
        a = oracle.alias_audit_render_stimulus(note, 120)
        b = oracle.alias_audit_render_stimulus(note, 120, perturbed=True)
        quiet = np.abs(a) < 1e-3 * np.max(np.abs(a))
        worst_quiet = max(worst_quiet, float(np.max(np.abs(a - b)[quiet])))
        ra = oracle.alias_audit_analyze(a, 44100.0, 440.0 * 2 ** ((note - 69) / 12))
        rb = oracle.alias_audit_analyze(b, 44100.0, 440.0 * 2 ** ((note - 69) / 12))
        assert ra.f0_hz == rb.f0_hz
        worst_db = max(worst_db, max(abs(x - y) for x, y in zip(ra.harmonic_db, rb.harmonic_db)), abs(ra.hf_band_dbc - rb.hf_band_dbc))
    assert 1e-10 < worst_quiet < oracle.ABS_FLOOR_AUDIT, worst_quiet
    assert worst_db < 2e-2, worst_db
    print(f"\n[floor table] ABS_FLOOR_AUDIT {oracle.ABS_FLOOR_AUDIT:.1e}: one-ulp {worst_quiet:.2e}, ratio {oracle.ABS_FLOOR_AUDIT / worst_quiet:.2f}")
    assert oracle.ABS_FLOOR_AUDIT <= oracle.FLOOR_RULE * worst_quiet, worst_quiet


def test_dense_play_floor(oracle):
    """The script of tools/soak_parity.py (random dense play, volume up to 0.65, tremolo depth 0.75) under the one-ulp experiment: the
    floor of the 4-note scenario (2e-9) is too tight here, the reference algorithm itself moves by up to ~3e-9 on quiet samples."""
    sr, length, n = 48000.0, 512, 4
    a = [oracle.OracleEngine(sr) for _ in range(n)]
    b = [oracle.OracleEngine(sr, perturbed=True) for _ in range(n)]
    for e in a + b:
        e.set_sample_rate(sr)
    rng = np.random.default_rng(99)
    for k in range(n):
        for e in (a[k], b[k]):
            e.set_tremolo_depth(0.25 * k); e.set_volume(0.35 + 0.1 * k); e.set_speaker_character(0.3 * (k % 3))
    held = [[] for _ in range(n)]
    worst_quiet = 0.0
    for _ in range(int(9.0 * sr / length)):
        for k in range(n):
            if rng.random() < 0.08 + 0.03 * k:
                note, vel = int(rng.integers(33, 97)), float(rng.uniform(0.2, 1.0))
                for e in (a[k], b[k]):
                    e.note_on(note, vel)
                held[k].append(note)
            if held[k] and rng.random() < 0.07:
                note = held[k].pop(int(rng.integers(0, len(held[k]))))
                for e in (a[k], b[k]):
                    e.note_off(note)
            if rng.random() < 0.01:
                on = bool(rng.integers(0, 2))
                for e in (a[k], b[k]):
                    e.set_sustain(on)
            if rng.random() < 0.002:
                d = float(rng.uniform(0.0, 1.0))
                for e in (a[k], b[k]):
                    e.set_tremolo_depth(d)
        for k in range(n):
            x = a[k].render(length).astype(np.float64); y = b[k].render(length).astype(np.float64)
            d = oracle.floor_governed_delta(x, y, oracle.ABS_FLOOR_DENSE)     # (per block, as the soak compares: the block's own peak sets the relative bar)
            if d == d:
                worst_quiet = max(worst_quiet, d)
    assert 2e-10 < worst_quiet < oracle.ABS_FLOOR_DENSE, worst_quiet
    print(f"\n[floor table] ABS_FLOOR_DENSE {oracle.ABS_FLOOR_DENSE:.1e}: one-ulp {worst_quiet:.2e}, ratio {oracle.ABS_FLOOR_DENSE / worst_quiet:.2f}")
    assert oracle.ABS_FLOOR_DENSE <= oracle.FLOOR_RULE * worst_quiet, worst_quiet


def test_melange_power_amp_guard_timing_is_not_one_ulp_stable(oracle):
    """The melange power amp under dense play: its divergence guard (power_amp.rs:375-407: Newton exhausted / non-finite / a node past
    100 V -> reset to the settled state, hold the last good sample) fires dozens of times per second and per engine on this script,
    and WHEN it fires depends on the last bit of the amp's input: the oracle and its own one-ulp-exp build (a 1e-10 V difference at
    the preamp output) agree to ~1e-10 until a borderline Newton sweep ends at 68 iterations on one side and 69 on the other -- one
    resets, the other does not, and from there the two are different signals (3e-3 apart).  This is a property of the reference
    algorithm (it documents "intermittent divergence under polyphonic input"), so sample-for-sample parity of an engine with this amp
    exists only up to the first such event; what CAN be held bit for bit is the amp on identical input (tests/test_gpu_power_amp.py:
    outputs, iteration counts and guard resets identical on every sample)."""
    sr, length, n = 48000.0, 512, 4
    a = [oracle.OracleEngine(sr, power_amp_kind=1) for _ in range(n)]
    b = [oracle.OracleEngine(sr, power_amp_kind=1, perturbed=True) for _ in range(n)]
    for e in a + b:
        e.set_sample_rate(sr)
    rng = np.random.default_rng(99)
    for k in range(n):
        for e in (a[k], b[k]):
            e.set_tremolo_depth(0.25 * k); e.set_volume(0.35 + 0.1 * k); e.set_speaker_character(0.3 * (k % 3))
    held = [[] for _ in range(n)]
    parted = None
    before = 0.0
    for blk in range(int(3.0 * sr / length)):
        for k in range(n):
            if rng.random() < 0.08 + 0.03 * k:
                note, vel = int(rng.integers(33, 97)), float(rng.uniform(0.2, 1.0))
                for e in (a[k], b[k]):
                    e.note_on(note, vel)
                held[k].append(note)
            if held[k] and rng.random() < 0.07:
                note = held[k].pop(int(rng.integers(0, len(held[k]))))
                for e in (a[k], b[k]):
                    e.note_off(note)
            if rng.random() < 0.01:
                on = bool(rng.integers(0, 2))
                for e in (a[k], b[k]):
                    e.set_sustain(on)
            if rng.random() < 0.002:
                d = float(rng.uniform(0.0, 1.0))
                for e in (a[k], b[k]):
                    e.set_tremolo_depth(d)
        for k in range(n):
            _, pa = a[k].render_pa_tap(length)
            _, pb = b[k].render_pa_tap(length)
            d = float(np.max(np.abs(pa - pb)))
            ga, gb = a[k].power_amp_diag()[3], b[k].power_amp_diag()[3]
            if d > 1e-6 or ga != gb:
                parted = (blk, k, d, ga, gb)
                break
            before = max(before, d)
        if parted:
            break
    assert parted is not None, "the two builds never parted within 3 s: the guard has become stable, tighten the GPU soak"
    blk, k, d, ga, gb = parted
    assert before < 1e-8, before                       # until then they are the same signal to the preamp floor
    assert ga != gb and d > 1e-4, parted               # and they part at a guard event, by a visible amount
    assert min(ga, gb) >= 5, parted                    # after a number of guard resets that both sides took at the same samples


def test_full_depth_tremolo_floor(oracle):
    """Tremolo depth 1.0 (the LDR divider at its largest gain swing): one note after a reset, volume 0.5.  The one-ulp experiment moves quiet
    samples of the reference algorithm by 1.9e-9 -- 0.93 of the 2e-9 floor the four-note scenarios use -- so parity tests of engines at
    full depth (tests/test_gpu_tremolo_groups.py) take the dense-play floor (5e-9), like every scenario whose depth reaches 1."""
    sr = 48000.0
    a, b = oracle.OracleEngine(sr), oracle.OracleEngine(sr, perturbed=True)
    for e in (a, b):
        e.set_sample_rate(sr); e.set_tremolo_depth(1.0); e.set_volume(0.5); e.note_on(45, 0.85)
    for _ in range(12):
        a.render(512); b.render(512)
    for e in (a, b):
        e.reset(); e.note_on(60, 0.8)
    worst = 0.0
    for _ in range(40):
        x = a.render(512).astype(np.float64); y = b.render(512).astype(np.float64)
        q = np.abs(x) < 2e-4
        if q.any():
            worst = max(worst, float(np.max(np.abs(x - y)[q])))
    assert 1e-9 < worst < oracle.ABS_FLOOR_DENSE, worst
    a.close(); b.close()


def test_soak_floor_governing_measurement(oracle):
    """The soak's floor (ABS_FLOOR_SOAK, tools/soak_parity.py, tests/test_gpu_soak.py): the first 8 s of the soak script under seed 5 -- six
    engines scripted, engine 0 (tremolo depth 0, volume 0.35) rendered -- carry the spot where the reference algorithm itself moves most
    over the eight seeds x 120 s of profiles/r06_soak.md: at block 691 a quiet sample of the oracle's one-ulp build lies 3.4e-8 from the
    oracle's.  The GPU's own worst sample of those 16 minutes sits in the same block of the same engine, at 1.5e-8."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import soak_parity
    r = soak_parity.soak(8.0, 6, seed=5, ulp=True, only=[0], verbose=False, floor=oracle.ABS_FLOOR_SOAK)
    assert r["branch"] == "floor" and r["block"] == 691 and r["engine"] == 0, r
    moved = r["worst"] * oracle.ABS_FLOOR_SOAK
    print(f"\n[floor table] ABS_FLOOR_SOAK {oracle.ABS_FLOOR_SOAK:.1e}: one-ulp {moved:.2e} (seed 5, block 691, engine 0), ratio {oracle.ABS_FLOOR_SOAK / moved:.2f}")
    assert 2e-8 < moved < 6e-8, moved
    assert oracle.ABS_FLOOR_SOAK <= oracle.FLOOR_RULE * moved


def test_soak_floor_legacy_tremolo_governing_measurement(oracle):
    """The soak of the `legacy-tremolo` configuration (tremolo_kind 1: the sine LFO in place of the Twin-T) has a floor of its own.  Its R
    stream comes out of sin(), pow() and exp(), where the device library and glibc differ in the last places; the experiment that stands for
    that is the oracle against itself with every r_ldr moved to the neighbouring double.  On the first 8 s of the soak script under seed 5
    (engine 0) the reference moves a quiet sample of block 691 -- the spot where it is touchiest to everything, see the test above -- by
    1.06e-7 with the LFO and by 4.3e-8 with the Twin-T (which the soak's general floor of 2e-8 therefore covers with the usual margin)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import soak_parity
    r = soak_parity.soak(8.0, 6, tk=1, seed=5, ulp="r:1", only=[0], verbose=False, floor=oracle.ABS_FLOOR_SOAK_LFO, stop_on_mismatch=False)
    assert r["branch"] == "floor" and r["block"] == 691 and r["engine"] == 0, r
    moved = r["worst"] * oracle.ABS_FLOOR_SOAK_LFO
    t = soak_parity.soak(8.0, 6, tk=0, seed=5, ulp="r:1", only=[0], verbose=False, floor=oracle.ABS_FLOOR_SOAK, stop_on_mismatch=False)
    moved_t = t["worst"] * oracle.ABS_FLOOR_SOAK
    print(f"\n[floor table] ABS_FLOOR_SOAK_LFO {oracle.ABS_FLOOR_SOAK_LFO:.1e}: R off by one ulp moves the LFO configuration by {moved:.2e} (seed 5, block 691, engine 0), "
          f"ratio {oracle.ABS_FLOOR_SOAK_LFO / moved:.2f}; the Twin-T configuration by {moved_t:.2e} (block {t['block']}), ABS_FLOOR_SOAK / that = {oracle.ABS_FLOOR_SOAK / moved_t:.2f}")
    assert 6e-8 < moved < 2e-7, moved
    assert oracle.ABS_FLOOR_SOAK_LFO <= oracle.FLOOR_RULE * moved
    assert oracle.ABS_FLOOR_SOAK <= oracle.FLOOR_RULE * moved_t and t["block"] == 691


def test_preamp_state_holds_the_evaluation_its_next_step_opens_with(oracle):
    """dk_preamp_legacy.rs: the Newton loop of a step opens with bjt_ic_gm(state.v_nl) (:508-509); state.i_nl is bjt_ic(state.v_nl)
    by construction (at_dc :247, step 9 :548-549) and bjt_ic is the ic half of bjt_ic_gm (:663-666, :686-690).  The product's dk_step
    carries that evaluation from one step into the next instead of repeating it: this pins the invariant on the
    reference's restatement -- at creation, block by block through notes, a depth ramp, a release and a reset, main and shadow."""
    e = oracle.OracleEngine(48000.0)
    e.set_volume(0.5); e.set_tremolo_depth(0.5); e.set_speaker_character(0.0); e.set_mlp_enabled(True)

    def check(tag):
        for shadow in (False, True):
            st = e.preamp_state(shadow)
            assert st[10].tobytes() == st[14].tobytes() and st[11].tobytes() == st[15].tobytes(), (tag, shadow, st[10:16])
    check("new")
    for n in (40, 52, 60, 67, 76, 88):
        e.note_on(n, 0.9)
    for b in range(40):
        e.render(97 if b % 3 else 512)
        if b == 10: e.set_tremolo_depth(1.0)
        if b == 20:
            for n in (40, 60): e.note_off(n)
        if b == 30: e.reset()
        check(b)
    e.close()


def test_trem_step_floors(oracle):
    """ABS_FLOOR_TREM_STEP_V / _I (single steps of the Twin-T oscillator, tests/trem_step_cases.py): the oracle's own movement with pnjlim's
    logarithm -- the step's only operation that is not IEEE arithmetic -- one double away, either way, on the rows where a floor and not the
    relative term has to be the tolerance: the rows that move by more than 1e-5 of their value, in the finite cases that keep their exits
    under the experiment (retry taken or not, converged or exhausted, reset; a case that changes its exit is a different step, not a
    rounding difference, and is what the corpus counts as not comparable).  No volt row needs a floor; junction currents do."""
    import trem_step_cases as tc
    worst_v = worst_i = 0.0
    for rate, ref in tc.references(oracle).items():
        for sp, op, fp in ref.perturbed:
            keep = ref.finite & (fp[:, [1, 3, 4]] == ref.info[:, [1, 3, 4]]).all(axis=1)
            d = np.abs(sp[keep] - ref.states[keep])
            d = np.where(d > 1e-5 * np.abs(ref.states[keep]), d, 0.0)
            worst_v, worst_i = max(worst_v, float(d[:, :7].max())), max(worst_i, float(d[:, 7:].max()))
    print(f"\n[floor table] ABS_FLOOR_TREM_STEP_V {oracle.ABS_FLOOR_TREM_STEP_V:.1e}: one-ulp-log {worst_v:.2e}; "
          f"ABS_FLOOR_TREM_STEP_I {oracle.ABS_FLOOR_TREM_STEP_I:.1e}: one-ulp-log {worst_i:.2e} (ratio {oracle.ABS_FLOOR_TREM_STEP_I / worst_i:.2f})")
    assert worst_v == 0.0 and 1e-12 < worst_i < 1e-10, (worst_v, worst_i)
    assert oracle.ABS_FLOOR_TREM_STEP_V <= oracle.FLOOR_RULE * worst_v, worst_v
    assert oracle.ABS_FLOOR_TREM_STEP_I <= oracle.FLOOR_RULE * worst_i, worst_i


def test_melange_step_floors(oracle):
    """ABS_FLOOR_MELANGE_STEP_V / _I (single steps of the melange preamp solver, tests/mel_step_cases.py): the oracle's own movement with
    pnjlim's logarithm one double away and with the resistance its rebuilds see one double away, either way, on the rows where a floor and
    not the relative term would have to be the tolerance: the rows that move by more than 1e-5 of their value, in the finite cases that
    keep their fallback, reset and cooldown decisions under the experiment.  There is none, in volts or amps: both floors are 0.  The
    largest relative movement is printed; the resistance knob is checked to be what it looks like -- absorbed by the addition into
    g_eff[6][6] -- and not a knob that is not connected."""
    import mel_step_cases as mc
    worst_v = worst_i = worst_rel = 0.0
    moved = [0, 0, 0, 0]
    for rate, ref in mc.references(oracle).items():
        for k, (sp, op, fp) in enumerate(ref.perturbed[:4]):         # the four one-double moves (the fifth variant swaps whole tables)
            keep = ref.finite & (fp[:, mc.DECISIONS] == ref.info[:, mc.DECISIONS]).all(axis=1)
            assert keep[ref.finite].all()                            # no decision changes under any of them
            d = np.abs(sp[keep][:, :18] - ref.states[keep][:, :18])
            a = np.abs(ref.states[keep][:, :18])
            moved[k] += int((d > 0).any(axis=1).sum())
            worst_rel = max(worst_rel, float((d / np.maximum(a, 1e-300)).max()))
            d = np.where(d > 1e-5 * a, d, 0.0)
            worst_v, worst_i = max(worst_v, float(d[:, :12].max())), max(worst_i, float(d[:, 12:].max()))
    print(f"\n[floor table] ABS_FLOOR_MELANGE_STEP_V {oracle.ABS_FLOOR_MELANGE_STEP_V:.1e}: one-ulp {worst_v:.2e}; ABS_FLOOR_MELANGE_STEP_I "
          f"{oracle.ABS_FLOOR_MELANGE_STEP_I:.1e}: one-ulp {worst_i:.2e}; largest relative movement of a row {worst_rel:.2e}; cases moved by "
          f"log +1 / -1, R +1 / -1: {moved}")
    assert worst_v == 0.0 and worst_i == 0.0 and 1e-9 < worst_rel < 1e-5, (worst_v, worst_i, worst_rel)
    assert moved[0] > 100 and moved[1] > 100 and moved[2] == 0 and moved[3] == 0, moved
    assert oracle.ABS_FLOOR_MELANGE_STEP_V <= oracle.FLOOR_RULE * worst_v and oracle.ABS_FLOOR_MELANGE_STEP_I <= oracle.FLOOR_RULE * worst_i
