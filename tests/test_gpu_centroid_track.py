"""GPU parity of `preamp-bench centroid-track` (tools/preamp-bench/src/main.rs:1925-2135) through ow_centroid_analyze and
ow_centroid_track, against the CPU restatement tests/c/centroid_track_ref.cpp.

Analysis alone (k_centroid_frames on given rows against the restatement's analysis of the same rows): the only differences are the
device's sin / cos against the host's, so the bar is centroid_track_ref.ANALYSIS_REL relative to c -- at most 10 x the worst difference
measured over these rows, never above 1e-9 (each case prints its worst; DESIGN.md has the measurement).  A wrong bin range, order of
summation or window form moves c by parts in 1e3.

End to end (centroid_track_ref.JOBS): the audio by oracle.parity_report with ABS_FLOOR_BATCH; every frame within its own derived bar
(1.5 x the first-order bound from the sample bars plus the analysis bar); the frames chosen for 10 ms and 300 ms exactly; the statuses
wherever the restatement's value is further than its bar from both edges of the interval.
"""
import ctypes as C

import numpy as np
import pytest

import centroid_track_ref as ref

pytestmark = pytest.mark.gpu


def _rows(n_rows, length, seed):
    """Rows with a few partials and a little noise each, different per row; stride = length rounded up to 64."""
    rng = np.random.default_rng(seed)
    stride = (length + 63) // 64 * 64
    t = np.arange(stride) / 44100.0
    sig = np.zeros((n_rows, stride))
    for r in range(n_rows):
        for _ in range(3):
            sig[r] += rng.uniform(0.05, 0.5) * np.sin(2.0 * np.pi * rng.uniform(80.0, 9000.0) * t + rng.uniform(0.0, 6.28)) * np.exp(-t * rng.uniform(0.0, 40.0))
        sig[r] += 1e-3 * rng.standard_normal(stride)
    return sig


def _worst_rel(got, want):
    m = want != 0.0
    assert np.array_equal(got[~m], want[~m])                       # 0.0 where the reference's power_sum > 0.0 fails
    return float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m]))) if m.any() else 0.0


# window, hop, end, len, rows: bin counts 11 / 55 / 549 (below, near and above a wavefront and a workgroup, all odd), windows that are
# no multiple of 64, 1 / 63 / 64 / 65 rows, a hop larger than the window, end_sample as the limit, a single frame ending exactly at len
CASES = {
    "w44_1row": (44, 22, 10 ** 6, 300, 1),
    "w220_63rows": (220, 110, 10 ** 6, 1500, 63),
    "w220_hop_gt_window_64rows": (220, 300, 10 ** 6, 1500, 64),
    "w220_end_limits_65rows": (220, 110, 700, 1500, 65),
    "w2205_3rows": (2205, 441, 10 ** 6, 4000, 3),
    "single_frame_ending_at_len": (220, 110, 10 ** 6, 220, 2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_analysis_against_the_restatement(hiplib, name):
    from openwurli_amd import centroid_track as ct
    window, hop, end, length, n_rows = CASES[name]
    sig = _rows(n_rows, length, seed=len(name) * 1000 + window)
    sig[:, length:] = 1e3                                          # behind `len`: never read
    if n_rows >= 63:
        sig[5, :length] = 0.0                                      # an all-zero row: 0.0 everywhere
        sig[7, 500] = np.nan                                       # one NaN: the frames that hold it take the else branch, the others are unaffected
    want = ref.analyze_rows(sig, window, hop, end, length)
    got = ct.analyze(sig, window, hop, end, length)
    assert got.shape == want.shape == (n_rows, len(ct.frame_positions(length, window, hop, end))) and got.shape[1] >= 1
    assert ct.bin_range(window)[1] - ct.bin_range(window)[0] + 1 == {44: 11, 220: 55, 2205: 549}[window]
    if name == "single_frame_ending_at_len":
        assert got.shape[1] == 1
    if n_rows >= 63:
        assert not got[5].any() and not want[5].any()
        holds = np.array([p <= 500 < p + window for p in ct.frame_positions(length, window, hop, end)])
        assert (got[7][holds] == 0.0).all() and (got[7][~holds] > 0.0).all() and not np.isnan(got).any()
    worst = _worst_rel(got, want)
    print(f"\n[centroid analysis {name}] worst relative difference of c {worst:.3e} (bar {ref.ANALYSIS_REL:.1e})")
    assert (want[0] > 50.0).all() and worst <= ref.ANALYSIS_REL <= ref.ANALYSIS_REL_CAP


def test_analysis_with_no_frame_leaves_the_output_untouched(hiplib):
    from openwurli_amd import centroid_track as ct
    sig = _rows(2, 219, seed=1)
    out = np.full((2, 4), -7.0)
    assert ct.analyze(sig, 220, 110, 10 ** 6, 219, out=out).shape == (2, 0) and (out == -7.0).all()      # one sample short of a frame
    assert ct.analyze(sig, 220, 110, 10 ** 6, 220, out=out).shape == (2, 1) and (out[:, 1:] == -7.0).all() and (out[:, 0] > 0.0).all()


def test_analysis_of_rows_left_in_device_memory(hiplib):
    """signals_is_device: rows that ow_batch_render left in HBM give bitwise what the same rows give from the host."""
    import openwurli_amd as ow
    from openwurli_amd import centroid_track as ct
    jobs = [{"note": n, "velocity": 100, "poweramp": True, "volume": 0.6, "speaker": 1.0} for n in (40, 60, 84)]
    n, stride = 4410, 4416
    ptr = hiplib.ow_device_alloc(8 * 3 * stride, 0)
    assert ptr
    try:
        ow.batch_render(jobs, 44100.0, 0.1, out_device_ptr=ptr, stride=stride)
        on_device = ct.analyze_device(ptr, 3, stride, n, 220, 110, 10 ** 6)
        host = np.zeros((3, stride))
        assert hiplib.ow_test_device_read(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), host.nbytes, 0) == 0
    finally:
        hiplib.ow_device_free(ptr, 0)
    from_host = ct.analyze(host, 220, 110, 10 ** 6, n)
    assert on_device.shape == (3, 39) and on_device.tobytes() == from_host.tobytes() and (on_device > 50.0).all()
    assert _worst_rel(on_device, ref.analyze_rows(host, 220, 110, 10 ** 6, n)) <= ref.ANALYSIS_REL


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _dev_job(j):
    return (j.note, j.velocity, j.volume, j.speaker, j.ldr, j.no_preamp, j.no_poweramp, j.displacement_scale)


@pytest.fixture(scope="module")
def parity():
    """{name: (device row, device frames, device audio, restatement)}: all jobs in ONE call."""
    from openwurli_amd import centroid_track as ct
    names = list(ref.JOBS)
    refs = ref.track_many([ref.JOBS[k] for k in names], duration=ref.DURATION, end_ms=ref.END_MS)
    rows, frames, audio = ct.run_jobs([_dev_job(ref.JOBS[k]) for k in names], ref.DURATION, end_ms=ref.END_MS, audio=True)
    return {k: (rows[i], frames[i], audio[i], refs[i]) for i, k in enumerate(names)}


@pytest.mark.parametrize("name", list(ref.JOBS))
def test_track_against_the_restatement(oracle, parity, name):
    from openwurli_amd import centroid_track as ct
    row, frames, audio, r = parity[name]
    job = ref.JOBS[name]
    assert audio.size == r.audio.size == ct.samples(ref.DURATION) == 15434 and frames.size == r.frames.size == 128
    rep = oracle.parity_report(audio, r.audio, abs_floor=oracle.ABS_FLOOR_BATCH)
    bars = ref.frame_bars(r, oracle.ABS_FLOOR_BATCH)
    err = np.abs(frames - r.frames)
    i = int(np.argmax(err / bars))
    print(f"\n[centroid-track {name}] audio {rep}\n  frames: worst at {i}: err {err[i]:.3e} Hz bar {bars[i]:.3e} Hz (ratio {err[i] / bars[i]:.3g}); max err {err.max():.3e} Hz")
    assert rep["peak"] > 1e-3 and rep["n_bad"] == 0, rep
    assert (err <= bars).all(), (i, err[i], bars[i])
    # the analysis stage of the call is the analysis stage alone on the call's own audio
    assert ct.analyze(audio, r.window, r.hop, r.end).tobytes() == frames.tobytes()
    # the frames chosen for 10 ms and 300 ms, and the row against the module's restatement of the summary on the device's own frames
    times = ct.frame_times(ref.DURATION, 5.0, 2.5, ref.END_MS)
    assert np.array_equal(times, r.times)
    own = ct.summarise(job.note, frames, times)
    assert row.tobytes() == own.tobytes()
    want = ct.summarise(job.note, r.frames, times)
    assert (row["has_c10"], row["has_c300"], row["frame10"], row["frame300"]) == (1, 1, want["frame10"], want["frame300"]) == (1, 1, 4, 120)
    assert row["c10"] == frames[4] and row["c300"] == frames[120] and row["drift"] == frames[120] - frames[4]
    assert tuple(row[k] for k in ("attack_lo", "attack_hi", "sustain_lo", "sustain_hi", "drift_lo", "drift_hi")) == ct.targets(job.note)
    # the statuses, where the bar allows it
    assert ref.one_hz_share(r, oracle.ABS_FLOOR_BATCH) >= ref.ONE_HZ_SHARE
    checked = 0
    for key, value, bar, lo, hi in (("attack_status", want["c10"], bars[4], want["attack_lo"], want["attack_hi"]),
                                    ("sustain_status", want["c300"], bars[120], want["sustain_lo"], want["sustain_hi"]),
                                    ("drift_status", want["drift"], bars[4] + bars[120], want["drift_lo"], want["drift_hi"])):
        if ref.clear_of_edges(float(value), float(bar), float(lo), float(hi)):
            assert row[key] == want[key], key
            checked += 1
    print(f"  c10 {row['c10']:.3f} ({r.frames[4]:.3f}) c300 {row['c300']:.3f} ({r.frames[120]:.3f}); statuses asserted: {checked} of 3")
    assert checked == 3                                            # every job of the list stands clear of its interval edges


def test_dc_solve_runs_at_the_jobs_ldr(oracle, parity):
    """set_ldr_resistance BEFORE reset(): at 19 kohm the audio matches the restatement (above) and differs from the same job through
    ow_batch_render, which resets first."""
    import openwurli_amd as ow
    j = ref.JOBS["ldr_19k"]
    audio = parity["ldr_19k"][2]
    batch = ow.batch_render([{"note": j.note, "velocity": j.velocity, "mlp": False, "poweramp": True, "volume": j.volume, "speaker": j.speaker, "r_ldr": j.ldr}],
                            44100.0, ref.DURATION)[0]
    rep = oracle.parity_report(audio, batch, abs_floor=oracle.ABS_FLOOR_BATCH)
    assert rep["n_bad"] > 1000 and rep["max_err_rel_peak"] > 1e-2, rep
    # ... while at 1 Mohm the two entry points give the same samples
    j = ref.JOBS["default"]
    batch = ow.batch_render([{"note": j.note, "velocity": j.velocity, "mlp": False, "poweramp": True, "volume": j.volume, "speaker": j.speaker, "r_ldr": j.ldr}],
                            44100.0, ref.DURATION)[0]
    assert oracle.parity_report(parity["default"][2], batch, abs_floor=oracle.ABS_FLOOR_BATCH)["n_bad"] == 0


def _decimal_boundary_within(x, decimals, bar):
    """True when x is within `bar` of a value at which its {:.decimals} print changes."""
    s = abs(float(x)) * 10 ** decimals
    return abs((s - int(s)) - 0.5) <= bar * 10 ** decimals


def test_report_and_csv_of_one_job(oracle, parity, tmp_path):
    """stdout and CSV of the command's default note equal the module run on the restatement's frames, except for digits inside a
    frame's bar."""
    from openwurli_amd import centroid_track as ct
    row, frames, audio, r = parity["default"]
    j = ref.JOBS["default"]
    path = str(tmp_path / "c.csv")
    got = ct.centroid_track(j.note, j.velocity, ref.DURATION, end_ms=ref.END_MS, csv=path)
    assert got["row"].tobytes() == row.tobytes() and got["frames"].tobytes() == frames.tobytes() and got["audio"].tobytes() == audio.tobytes()
    assert open(path).read() == got["csv"]
    bars = ref.frame_bars(r, oracle.ABS_FLOOR_BATCH)
    want_report = ct.format_report(j.note, j.velocity, 5.0, r.frames, r.times, csv_path=path).splitlines()
    want_csv = ct.format_csv(r.frames, r.times).splitlines()
    gl = got["report"].splitlines()
    assert len(gl) == len(want_report) == 3 + 128 + 4 + 2 and gl[0] == "Centroid tracking: C4 (MIDI 60) vel=100, 5ms Hann windows" and gl[-1] == f"  CSV written to {path}"
    for k in range(128):
        assert gl[3 + k] == want_report[3 + k] or _decimal_boundary_within(r.frames[k], 0, bars[k]), (k, gl[3 + k], want_report[3 + k])
        assert got["csv"].splitlines()[1 + k] == want_csv[1 + k] or _decimal_boundary_within(r.frames[k], 1, bars[k]), k
    for line, value, bar in ((132, r.frames[4], bars[4]), (133, r.frames[120], bars[120]), (134, r.frames[120] - r.frames[4], bars[4] + bars[120])):
        assert gl[line] == want_report[line] or _decimal_boundary_within(value, 0, bar), (gl[line], want_report[line])
    assert gl[2] == "   Time (ms)   Centroid (Hz)" and gl[132].startswith("  Attack centroid (10ms):") and gl[134].startswith("  Drift:")


# ---- independence ---------------------------------------------------------------------------------------------------------------------
def test_bit_independence(monkeypatch):
    """A job's numbers are bitwise the same alone, in a call of 65, and under OW_CENTROID_CHUNK=2; audio_out NULL or not changes none."""
    from openwurli_amd import centroid_track as ct
    dur, end = 0.06, 50.0
    probe = ct.make_job(52, 96, 0.7, 0.8, 60_000.0)
    a_rows, a_frames, a_audio = ct.run_jobs(probe, dur, end_ms=end, audio=True)
    assert a_frames.shape == (1, 20) and (a_frames > 0.0).all()
    rng = np.random.default_rng(99)
    grid = ct.make_jobs([(int(rng.integers(33, 97)), int(rng.integers(20, 128)), float(rng.uniform(0.2, 1.0)), float(rng.uniform(0.0, 1.0)),
                          float(np.exp(rng.uniform(np.log(5e3), np.log(1e6)))), bool(i % 5 == 4), bool(i % 4 == 3), 0.3 if i % 7 == 6 else None)
                         for i in range(65)])
    whole = None
    for pos in (0, 33, 64):
        g = grid.copy()
        g[pos] = probe[0]
        rows, frames, audio = ct.run_jobs(g, dur, end_ms=end, audio=True)
        assert rows[pos:pos + 1].tobytes() == a_rows.tobytes() and frames[pos].tobytes() == a_frames.tobytes() and audio[pos].tobytes() == a_audio.tobytes(), pos
        whole = (g, rows, frames, audio)
    g, rows, frames, audio = whole
    r2, f2 = ct.run_jobs(g, dur, end_ms=end)                            # audio_out NULL
    assert r2.tobytes() == rows.tobytes() and f2.tobytes() == frames.tobytes()
    monkeypatch.setenv("OW_CENTROID_CHUNK", "2")                        # 65 jobs in 33 chunks
    r3, f3, a3 = ct.run_jobs(g, dur, end_ms=end, audio=True)
    assert r3.tobytes() == rows.tobytes() and f3.tobytes() == frames.tobytes() and a3.tobytes() == audio.tobytes()


def test_refusals_through_the_c_abi_on_the_device(hiplib):
    from openwurli_amd import binding, centroid_track as ct
    with pytest.raises(binding.OwError, match="note 97"):
        ct.run_jobs([(97, 100)], 0.05, end_ms=40.0)
    with pytest.raises(binding.OwError, match="OW_PREAMP_MELANGE12"):
        ct.run_jobs([(60, 100)], 0.05, end_ms=40.0, preamp_kind=1)
    rows, frames = ct.run_jobs([(60, 100)], 0.05, end_ms=40.0)         # the library still works after a refusal
    assert frames.shape == (1, 16) and (frames > 0.0).all() and rows["has_c10"][0] == 1 and rows["has_c300"][0] == 0
