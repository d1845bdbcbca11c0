"""GPU parity of the note audits `preamp-bench intermod-audit --render` and `overshoot` (tools/preamp-bench/src/main.rs:675-903,
2137-2247) through ow_dft_magnitudes, ow_intermod_audit and ow_overshoot, against the CPU restatement tests/c/note_audit_ref.cpp.

Analysis alone (k_dft_probes on given rows against dft_magnitude on the same rows): the device adds a thread's terms in ascending order
and the 256 partial sums through a fixed tree where the reference adds serially, and its sin / cos are its own; the bar is
note_audit_ref.ANALYSIS_REL relative to the scale (2 / n) sum |x_i| -- at most 10 x the worst difference measured here, never above
(n + 4) 2^-52.  Each case prints its worst.

End to end: the voice row by the bar of the Voice::render_note parity tests, every dB figure within its own derived bar
(note_audit_ref's docstring), verdicts and the report text exactly -- tests/test_note_audit_host.py checks on the CPU that the chosen jobs
allow that.
"""
import math

import numpy as np
import pytest

import note_audit_ref as ref

pytestmark = pytest.mark.gpu

SR = 44100.0


def _rows(n_rows, stride, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(stride) / SR
    sig = np.zeros((n_rows, stride))
    for r in range(n_rows):
        for _ in range(3):
            sig[r] += rng.uniform(0.05, 0.5) * np.sin(2.0 * np.pi * rng.uniform(80.0, 9000.0) * t + rng.uniform(0.0, 6.28))
        sig[r] += 1e-3 * rng.standard_normal(stride)
    return sig


# window lengths shorter than a wavefront, shorter than a workgroup, no multiple of either, and the end-to-end tests' 4 410
@pytest.mark.parametrize("n", [1, 63, 64, 257, 4410])
def test_dft_magnitudes_synthetic(hiplib, n):
    from openwurli_amd import intermod_audit as ia
    start = 37                                                      # start > 0: the phase index counts from the window start
    end = start + n
    stride = (end + 29 + 63) // 64 * 64                             # stride > end
    sig = _rows(3, stride, seed=n)
    sig[:, :start] = 1e3                                            # outside the window: never read
    sig[:, end:] = -1e3
    nan = float("nan")
    freqs = np.array([[0.0, SR / 2.0, 21000.0, nan, 440.0, 660.0],              # three rows, three probe tables
                      [nan, 55.0, 82.5, 21000.0, 0.0, nan],
                      [1234.5, 4321.0, nan, SR / 2.0, 8000.25, 21000.0]])
    want = ref.dft_magnitudes(sig, start, end, SR, freqs)
    got = ia.dft_magnitudes(sig, start, end, freqs, SR)
    assert got.shape == want.shape
    assert np.all(got[np.isnan(freqs)] == 0.0) and np.all(want[np.isnan(freqs)] == 0.0)
    scale = (2.0 / n) * np.sum(np.abs(sig[:, start:end]), axis=1, keepdims=True)
    worst = float(np.max(np.abs(got - want) / scale))
    bar = ref.analysis_rel(n)
    print(f"\n[dft magnitudes n={n}] worst difference / scale {worst:.3e} (bar {bar:.3e}, cap {ref.analysis_cap(n):.3e})")
    assert float(np.max(want)) > 1e-3                               # the probes see signal
    assert worst <= bar <= ref.analysis_cap(n)
    if n == 1:                                                      # one sample: 2 |x| at every frequency, exactly where cos = 1
        assert got[0, 0] == 2.0 * abs(sig[0, start])


# 220 samples: the first peak window is clamped by the length, every other window is empty; 6 615: the early RMS window is clamped;
# 52 920: the late RMS window is clamped
@pytest.mark.parametrize("duration", [0.005, 0.15, 1.2])
def test_window_stats_against_numpy(hiplib, duration):
    from openwurli_amd import overshoot as ov
    from openwurli_amd.intermod_audit import note_jobs
    rows, au = ov.run_jobs(note_jobs([40, 77], [127, 50]), duration, audio=True)
    n = au.shape[1]
    assert n == ref.samples(duration)
    e = [min(x, n) for x in ref.overshoot_edges()]
    for r, x in zip(rows, au):
        assert r["peak_0_10"] == np.max(np.abs(x[:e[0]]), initial=0.0) and r["peak_0_50"] == np.max(np.abs(x[:e[1]]), initial=0.0)    # exact
        for f, (s, t) in (("rms_100_200", (e[2], e[3])), ("rms_1000_1500", (e[4], e[5]))):
            if t <= s:
                assert r[f] == 0.0                                  # an empty window
                continue
            want = float(np.sum(x[s:t].astype(np.longdouble) ** 2))
            got = float(r[f]) ** 2 * (t - s)                        # the sum of squares back from the RMS the row holds
            assert abs(got - want) <= (t - s) * 2.0 ** -52 * want, (f, got, want)
    if duration == 0.005:
        assert e[0] == 220 and np.all(rows["rms_100_200"] == 0.0) and np.all(np.isnan(rows["overshoot_db"])) and np.all(rows["peak_0_10"] > 0.0)
    if duration == 1.2:
        assert e[4:] == [44100, 52920] and np.all(rows["rms_1000_1500"] > 0.0)


def test_rows_do_not_depend_on_the_call(hiplib, monkeypatch):
    """A job alone, among others, and with one job per chunk: the same bits."""
    from openwurli_amd import intermod_audit as ia, overshoot as ov
    jobs = ia.note_jobs([33, 60, 96, 72], [127, 64])
    monkeypatch.delenv("OW_NOTE_AUDIT_CHUNK", raising=False)
    ri, ai = ia.run_jobs(jobs, 0.6, audio=True)
    ro, ao = ov.run_jobs(jobs, 0.25, audio=True)
    for k in (0, 5):
        r1, a1 = ia.run_jobs(jobs[k:k + 1], 0.6, audio=True)
        assert r1.tobytes() == ri[k:k + 1].tobytes() and a1.tobytes() == ai[k:k + 1].tobytes()
        r1, a1 = ov.run_jobs(jobs[k:k + 1], 0.25, audio=True)
        assert r1.tobytes() == ro[k:k + 1].tobytes() and a1.tobytes() == ao[k:k + 1].tobytes()
    assert ia.run_jobs(jobs, 0.6).tobytes() == ri.tobytes()        # asking for the audio changes no number
    monkeypatch.setenv("OW_NOTE_AUDIT_CHUNK", "1")
    rc, ac = ia.run_jobs(jobs, 0.6, audio=True)
    assert rc.tobytes() == ri.tobytes() and ac.tobytes() == ai.tobytes()
    rc, ac = ov.run_jobs(jobs, 0.25, audio=True)
    assert rc.tobytes() == ro.tobytes() and ac.tobytes() == ao.tobytes()
    monkeypatch.setenv("OW_NOTE_AUDIT_CHUNK", "3")
    assert ia.run_jobs(jobs, 0.6).tobytes() == ri.tobytes()


def _voice_row_ok(oracle, got, want):
    rep = oracle.parity_report(got, want, rel=ref.VOICE_REL, floor_frac=1.0)
    assert rep["n_bad"] == 0 and rep["peak"] > 1e-4, rep


@pytest.fixture(scope="module")
def intermod_results(hiplib):
    """{duration: (jobs, rows, audio)} of the chosen jobs, one call per duration."""
    from openwurli_amd import intermod_audit as ia
    out = {}
    for dur, jobs in ((ref.INTERMOD_SHORT, ref.INTERMOD_JOBS_SHORT), (ref.INTERMOD_LONG, ref.INTERMOD_JOBS_LONG)):
        jb = np.zeros(len(jobs), dtype=ia.NOTE_JOB_DTYPE)
        jb["note"], jb["velocity"] = [j[0] for j in jobs], [j[1] for j in jobs]
        rows, au = ia.run_jobs(jb, dur, audio=True)
        out[dur] = (jobs, rows, au)
    return out


def test_intermod_audit_end_to_end(hiplib, oracle, intermod_results):
    for dur, (jobs, rows, au) in intermod_results.items():
        for (note, vel), r, x in zip(jobs, rows, au):
            want_au = ref.row(note, vel, dur)
            _voice_row_ok(oracle, x, want_au)
            a = ref.intermod_audit(want_au, note)
            h, m, rb, det = ref.intermod_bars(want_au, note)
            assert (r["midi"], r["velocity"], r["too_short"]) == (note, vel, 0)
            assert (r["window_start"], r["window_end"]) == (a.start, a.end) == (22050, 26460 if dur == ref.INTERMOD_SHORT else 88200)
            assert (r["n_harmonics"], r["n_midpoints"]) == (a.n_harmonics, a.n_midpoints)
            print(f"\n[intermod {note}/{vel}/{dur}s] h_db {r['h_db']:.6f} (ref {a.h_db:.6f}, bar {h:.2e})  m_db {r['m_db']:.6f} (ref {a.m_db:.6f}, bar {m:.2e})  "
                  f"ratio_db {r['ratio_db']:.6f} (ref {a.ratio_db:.6f}, bar {rb:.2e})  {ref.VERDICTS[a.verdict]}")
            assert rb < 0.05
            assert abs(r["h_db"] - a.h_db) <= h and abs(r["m_db"] - a.m_db) <= m and abs(r["ratio_db"] - a.ratio_db) <= rb
            assert r["verdict"] == a.verdict
            listed = [p for p in a.products if p.listed]
            assert [bool(p["listed"]) for p in r["products"]] == [p.listed for p in a.products] and len(det) == len(listed)
            k = 0
            for p, c in zip(r["products"], a.products):
                assert (p["mode"], p["nearest_integer"], p["intermod_freq"], p["nearest_freq"], p["risk_score"]) == \
                       (c.mode, c.nearest_integer, c.intermod_freq, c.nearest_freq, c.risk_score)
                if c.listed:
                    assert abs(p["ratio_db"] - c.ratio_db) <= det[k], (note, c.mode, p["ratio_db"], c.ratio_db, det[k])
                    k += 1
                else:
                    assert p["intermod_mag"] == 0.0 and p["nearest_mag"] == 0.0 and p["ratio_db"] == 0.0
    assert {r["n_harmonics"] for r in intermod_results[ref.INTERMOD_SHORT][1]} == {32, 10}


@pytest.fixture(scope="module")
def overshoot_results(hiplib):
    from openwurli_amd import overshoot as ov
    from openwurli_amd.intermod_audit import NOTE_JOB_DTYPE
    out = {}
    for dur in ref.OVERSHOOT_DURATIONS:
        jb = np.zeros(len(ref.OVERSHOOT_JOBS), dtype=NOTE_JOB_DTYPE)
        jb["note"], jb["velocity"] = [j[0] for j in ref.OVERSHOOT_JOBS], [j[1] for j in ref.OVERSHOOT_JOBS]
        out[dur] = ov.run_jobs(jb, dur, audio=True)
    return out


def test_overshoot_end_to_end(hiplib, oracle, overshoot_results):
    for dur, (rows, au) in overshoot_results.items():
        for (note, vel), r, x in zip(ref.OVERSHOOT_JOBS, rows, au):
            want_au = ref.row(note, vel, dur)
            _voice_row_ok(oracle, x, want_au)
            o, bars = ref.overshoot(want_au), ref.overshoot_bars(want_au)
            assert (r["note"], r["velocity"]) == (note, vel)
            for f in ref.Overshoot._fields:
                g, w, b = float(r[f]), getattr(o, f), getattr(bars, f)
                if math.isnan(w) or w == -120.0:
                    assert (math.isnan(g) and math.isnan(w)) or g == w, (note, vel, dur, f, g, w)
                else:
                    assert abs(g - w) <= b, (note, vel, dur, f, g, w, b)
            print(f"\n[overshoot {note}/{vel}/{dur}s] overshoot_db {r['overshoot_db']:.6f} (ref {o.overshoot_db:.6f}, bar {bars.overshoot_db:.2e})  "
                  f"bark_decay_db {r['bark_decay_db']:.6f} (ref {o.bark_decay_db:.6f})")
            if dur < 1.0:
                assert math.isnan(r["bark_decay_db"]) and r["rms2_dbfs"] == -120.0 and r["rms_1000_1500"] == 0.0
            else:
                assert r["rms_1000_1500"] > 0.0 and not math.isnan(r["bark_decay_db"])


def test_report_text_on_the_device(hiplib, intermod_results, overshoot_results):
    from openwurli_amd import intermod_audit as ia, overshoot as ov
    for dur, (jobs, rows, _) in intermod_results.items():
        want = [ref.intermod_record(ref.row(n, v, dur), n, v) for n, v in jobs]
        assert ia.format_render(rows, dur) == ia.format_render(want, dur)
    notes, vels = sorted({j[0] for j in ref.OVERSHOOT_JOBS}), sorted({j[1] for j in ref.OVERSHOOT_JOBS})
    assert [(n, v) for n in notes for v in vels] == list(ref.OVERSHOOT_JOBS)
    for dur, (rows, _) in overshoot_results.items():
        want = [ref.overshoot_record(ref.row(n, v, dur), n, v) for n, v in ref.OVERSHOOT_JOBS]
        text = ov.format_report(notes, vels, rows)
        assert text == ov.format_report(notes, vels, want)
        assert ("NaN" in text) == (dur < 1.0)


def _window_stats(hiplib, sig, windows):
    """ow_debug_window_stats: k_window_stats on host rows; windows = [(start, end, kind)], kind 0 = max |x|, 1 = sum of squares."""
    import ctypes as C
    sig = np.ascontiguousarray(sig, dtype=np.float64)
    st, en, ki = (np.array([w[k] for w in windows], dtype=np.uint32) for k in range(3))
    out = np.full((sig.shape[0], len(windows)), -7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert hiplib.ow_debug_window_stats(p(sig), sig.shape[0], sig.shape[1], p(st), p(en), p(ki), len(windows), 0, p(out)) == 0, hiplib.ow_last_error()
    return out


def test_window_stats_on_synthetic_rows(hiplib):
    """The kernel alone: windows shorter than a wavefront and no multiple of a workgroup, an empty window, NaN samples (the peak ignores
    them as Rust's fold(0.0, f64::max) does; a sum of squares that holds one is NaN, as the reference's is), an all-NaN peak window."""
    stride = 1024
    sig = _rows(3, stride, seed=99)
    sig[1, 5] = np.nan
    sig[1, 300] = np.nan
    sig[2, 700:763] = np.nan
    windows = [(0, 441, 0), (3, 66, 0), (129, 900, 1), (500, 500, 1)]
    got = _window_stats(hiplib, sig, windows)
    for r in range(3):
        for k, (s, e, kind) in enumerate(windows):
            x = sig[r, s:e]
            if kind == 0:
                want = float(np.fmax.reduce(np.abs(x), initial=0.0))           # fmax: the non-NaN operand
                assert got[r, k] == want and not math.isnan(got[r, k]), (r, k)
            elif e <= s:
                assert got[r, k] == 0.0
            elif np.isnan(x).any():
                assert math.isnan(got[r, k]), (r, k)
            else:
                want = float(np.sum(x.astype(np.longdouble) ** 2))
                assert abs(got[r, k] - want) <= (e - s) * 2.0 ** -52 * want, (r, k)
    assert got[1, 0] > 0.0 and math.isnan(got[1, 2]) and not math.isnan(got[0, 2])
    only_nan = _window_stats(hiplib, sig, [(700, 763, 0), (700, 701, 0)])
    assert only_nan[2, 0] == 0.0 and only_nan[2, 1] == 0.0 and only_nan[0, 0] > 0.0


def test_dft_magnitudes_of_rows_in_device_memory(hiplib):
    """signals_is_device: the rows an earlier call left in HBM give bitwise what the same rows give from the host."""
    import ctypes as C
    import openwurli_amd as ow
    jobs = [{"note": n, "velocity": 100, "poweramp": True, "volume": 0.6, "speaker": 1.0} for n in (40, 60, 84)]
    n, stride = 4410, 4416
    freqs = np.array([[82.4, 123.6, float("nan"), 21000.0], [261.6, 392.4, 0.0, float("nan")], [1046.5, 1569.7, 22050.0, 3.0]])
    ptr = hiplib.ow_device_alloc(8 * 3 * stride, 0)
    assert ptr
    try:
        ow.batch_render(jobs, 44100.0, 0.1, out_device_ptr=ptr, stride=stride)
        on_device = np.full(freqs.shape, -7.0)
        assert hiplib.ow_dft_magnitudes(C.c_void_p(ptr), 3, stride, 100, n, 44100.0, freqs.ctypes.data_as(C.c_void_p), freqs.shape[1], 0, 1,
                                        on_device.ctypes.data_as(C.c_void_p)) == 0, hiplib.ow_last_error()
        host = np.zeros((3, stride))
        assert hiplib.ow_test_device_read(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), host.nbytes, 0) == 0
    finally:
        hiplib.ow_device_free(ptr, 0)
    from openwurli_amd import intermod_audit as ia
    from_host = ia.dft_magnitudes(host, 100, n, freqs)
    assert on_device.tobytes() == from_host.tobytes() and np.all(on_device[np.isnan(freqs)] == 0.0) and on_device[0, 0] > 1e-6
    want = ref.dft_magnitudes(host, 100, n, SR, freqs)
    scale = (2.0 / (n - 100)) * np.sum(np.abs(host[:, 100:n]), axis=1, keepdims=True)
    assert float(np.max(np.abs(on_device - want) / scale)) <= ref.analysis_rel(n - 100)


def _mode_shape(beta, xi):
    sigma = (np.cosh(beta) + np.cos(beta)) / (np.sinh(beta) + np.sin(beta))
    bx = beta * xi
    return np.cosh(bx) - np.cos(bx) - sigma * (np.sinh(bx) - np.sin(bx))


def test_note_table_against_the_oracle(hiplib, oracle):
    """The note table k_note_table builds, whose maths the host's risk table now shares: f0, the mode ratios and base amplitude x spatial
    coupling of every note against the oracle's tables.  The ratios are plain arithmetic on the eigenvalue table: bit for bit.  f0 goes
    through pow: 4 ulp.  The coupling is ill-conditioned and its bar is derived: mode_shape subtracts cosh(bx) and sigma sinh(bx), both near
    e^beta / 2 (3.7e8 at mode 7), to a result of order 1, so with library calls good to 2 ulp each, sigma a quotient of two rounded sums
    and three subtractions every evaluation carries an absolute error of up to 16 x 2^-52 x e^beta / 2, and so do the Simpson mean of the
    33 evaluations (weights summing to 1) and the tip value.  kappa_raw = |mean / tip| then moves relatively by that error times
    (1 / |mean| + 1 / |tip|), on both sides (device and host libraries), and the normalisation by mode 1 adds mode 1's own term."""
    import ctypes as C
    nt = np.zeros((34, 64))
    assert hiplib.ow_debug_note_table(nt.ctypes.data_as(C.c_void_p), 0) == 0, hiplib.ow_last_error()
    L = oracle.lib()
    d = C.c_double
    base = (1.0, 0.005, 0.0035, 0.0018, 0.0011, 0.0007, 0.0005)
    worst_f0 = worst_amp = worst_share = 0.0
    for ni in range(64):
        midi = 33 + ni
        f0 = L.owo_midi_to_freq(midi)
        worst_f0 = max(worst_f0, abs(nt[31, ni] - f0) / f0)
        mu, length = L.owo_tip_mass_ratio(midi), L.owo_reed_length_mm(midi)
        r, k, b = (d * 7)(), (d * 7)(), (d * 7)()
        L.owo_mode_ratios(d(mu), r)
        L.owo_spatial_coupling(d(mu), d(length), k)
        L.owo_eigenvalues(d(mu), b)
        assert nt[1:8, ni].tobytes() == np.array(list(r)).tobytes(), midi
        ell = min(max(6.0 / length, 0.0), 1.0)
        xi = 1.0 - ell + np.arange(33) * (ell / 32.0)
        w = np.array([1.0] + [4.0, 2.0] * 15 + [4.0, 1.0]) / 96.0                 # Simpson weights over the plate, as a mean
        rel = []
        for i in range(7):
            err = 16.0 * 2.0 ** -52 * math.exp(b[i]) / 2.0
            mean, tip = abs(float(np.sum(w * _mode_shape(b[i], xi)))), abs(float(_mode_shape(b[i], 1.0)))
            rel.append(2.0 * err * (1.0 / mean + 1.0 / tip))                         # both sides
        for i in range(7):
            want = base[i] * k[i]
            got_rel = abs(nt[8 + i, ni] - want) / want
            bar = rel[i] + rel[0] + 4 * 2.0 ** -52
            worst_amp = max(worst_amp, got_rel)
            worst_share = max(worst_share, got_rel / bar)
            assert got_rel <= bar, (midi, i, got_rel, bar)
    print(f"\n[note table] worst relative difference: f0 {worst_f0:.3e}, amplitudes {worst_amp:.3e} ({worst_share:.2f} of the derived bar)")
    assert worst_f0 <= 4 * 2.0 ** -52
