"""`preamp-bench centroid-track` (tools/preamp-bench/src/main.rs:1925-2135), host side: no GPU needed.

The frame and bin arithmetic against a table (Python mirror, ow_centroid_frame_count, the restatement); the report text and CSV against
strings built by hand; every refusal with its message (all come before any device work); the CPU restatement
(tests/c/centroid_track_ref.cpp) on a signal with a known answer and against the existing oracle's batch job where the two commands
coincide; the status bytes against include/openwurli_hip.h (the structs' layouts: tests/test_abi_layout.py); and the condition under which
the GPU test asserts summary statuses.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import centroid_track_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# window ms, hop ms, end ms -> window samples, hop samples, (k_min, k_max), frames of a 1 s signal
TABLE = [
    (5.0, 2.5, 500.0, 220, 110, (1, 55), 200),
    (10.0, 5.0, 500.0, 441, 220, (1, 110), 100),
    (20.0, 2.5, 500.0, 882, 110, (1, 220), 197),
    (50.0, 10.0, 500.0, 2205, 441, (3, 551), 48),
    (1.0, 0.5, 20.0, 44, 22, (1, 11), 40),
    (3.0, 1.0, 40.0, 132, 44, (1, 33), 39),
]


# ---- frame and bin arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_ms,hop_ms,end_ms,window,hop,bins,frames", TABLE)
def test_frame_and_bin_arithmetic(hiplib_host, window_ms, hop_ms, end_ms, window, hop, bins, frames):
    from openwurli_amd import centroid_track as ct
    assert (ct.ms_to_samples(window_ms), ct.ms_to_samples(hop_ms)) == (window, hop)
    assert ct.bin_range(window) == bins
    pos = ct.frame_positions(ct.samples(1.0), window, hop, ct.ms_to_samples(end_ms))
    assert len(pos) == frames and pos[:2] == [0, hop]
    assert ct.frame_times(1.0, window_ms, hop_ms, end_ms).size == frames
    # the library (host only) ...
    assert ct.frame_count(1.0, window_ms, hop_ms, end_ms) == frames
    # ... and the restatement
    assert (ref.ms_to_samples(window_ms), ref.ms_to_samples(hop_ms), ref.bins(window)) == (window, hop, bins)
    assert ref.analyze(np.zeros(44100), window, hop, ref.ms_to_samples(end_ms)).size == frames


def test_integer_half_in_the_loop_and_float_half_in_the_time():
    """An odd window: the loop condition uses window / 2 as an integer, center_ms as a float."""
    from openwurli_amd import centroid_track as ct
    assert ct.center_ms(0, 441) == 220.5 / 44100.0 * 1000.0 and ct.center_ms(0, 441) != 220 / 44100.0 * 1000.0
    # end_sample 220: pos 0 passes with the integer half (0 + 220 <= 220); a float half (220.5) would not
    assert ct.frame_positions(44100, 441, 220, 220) == [0]
    assert ct.frame_positions(44100, 441, 220, 219) == []
    assert ct.frame_positions(440, 441, 220, 10000) == [] and ct.frame_positions(441, 441, 220, 10000) == [0]
    assert ref.analyze(np.zeros(44100), 441, 220, 220).size == 1 and ref.analyze(np.zeros(44100), 441, 220, 219).size == 0
    with pytest.raises(ValueError):
        ct.frame_positions(44100, 220, 0, 22050)
    # 5 ms frames at 2.5 ms hops: the frame that PRINTS as 10.0 ms is centred at 9.977 ms, so the attack frame is the next one
    t = ct.frame_times()
    assert "%.1f" % t[3] == "10.0" and t[3] < 10.0 <= t[4]


# ---- report text and CSV ------------------------------------------------------------------------------------------------------------
def test_report_with_a_silent_attack_frame_and_a_short_render():
    """The first frame centred at or after 10 ms is taken even when its centroid is 0: MISS, not "no data".  Frames whose centroid is 0
    are neither printed nor written to the CSV.  {:.0} / {:.1} round half to even."""
    from openwurli_amd import centroid_track as ct
    times = ct.frame_times(0.016, 5.0, 2.5, 500.0)
    assert times.size == 5
    frames = [812.5, 0.0, 650.5, 700.25, 0.0]
    text = ct.format_report(60, 100, 5.0, frames, times)
    assert text == ("Centroid tracking: C4 (MIDI 60) vel=100, 5ms Hann windows\n"
                    "\n"
                    "   Time (ms)   Centroid (Hz)\n"
                    "         2.5             812\n"
                    "         7.5             650\n"
                    "        10.0             700\n"
                    "\n"
                    "  Attack centroid (10ms):        0 Hz   (target: 600-1200)  MISS\n"
                    "  Sustain centroid (300ms): (no data — signal too short)\n")
    assert ct.format_csv(frames, times) == "time_ms,centroid_hz\n2.5,812.5\n7.5,650.5\n10.0,700.2\n"
    row = ct.summarise(60, frames, times)
    assert (row["has_c10"], row["frame10"], row["c10"], row["attack_status"]) == (1, 4, 0.0, ct.CENTROID_MISS)
    assert (row["has_c300"], row["frame300"], row["sustain_status"], row["drift_status"]) == (0, -1, ct.CENTROID_NO_DATA, ct.CENTROID_NO_DATA)
    # a render too short to reach 10 ms: both "no data" lines, no drift line
    short = ct.format_report(33, 1, 5.0, [500.0], times[:1])
    assert short == ("Centroid tracking: A1 (MIDI 33) vel=1, 5ms Hann windows\n"
                     "\n"
                     "   Time (ms)   Centroid (Hz)\n"
                     "         2.5             500\n"
                     "\n"
                     "  Attack centroid (10ms):   (no data — signal too short or silent)\n"
                     "  Sustain centroid (300ms): (no data — signal too short)\n")
    assert ct.format_report(33, 1, 5.0, [], []).splitlines()[2:] == ["   Time (ms)   Centroid (Hz)", "", "  Attack centroid (10ms):   (no data — signal too short or silent)",
                                                                     "  Sustain centroid (300ms): (no data — signal too short)"]
    assert ct.format_csv([], []) == "time_ms,centroid_hz\n"


def test_report_with_all_three_summary_lines():
    from openwurli_amd import centroid_track as ct
    text = ct.format_report(84, 127, 2.5, [900.4, 1000.5, 799.5], [5.0, 10.0, 300.0], no_preamp=True, no_poweramp=True, csv_path="out.csv")
    assert text == ("Centroid tracking: C6 (MIDI 84) vel=127, 2.5ms Hann windows\n"
                    "  Preamp: BYPASSED\n"
                    "  Power amp: BYPASSED\n"
                    "\n"
                    "   Time (ms)   Centroid (Hz)\n"
                    "         5.0             900\n"
                    "        10.0            1000\n"
                    "       300.0             800\n"
                    "\n"
                    "  Attack centroid (10ms):     1000 Hz   (target: 800-1600)  OK\n"
                    "  Sustain centroid (300ms):    800 Hz   (target: 800-1400)  MISS\n"      # 799.5 prints as 800 and is below 800
                    "  Drift:                     -201 Hz   (target: -250 to -30) OK\n"
                    "\n"
                    "  CSV written to out.csv\n")
    up = ct.format_report(40, 64, 50.0, [700.0, 790.0], [10.0, 300.0]).splitlines()
    assert up[-3:] == ["  Attack centroid (10ms):      700 Hz   (target: 600-1000)  OK", "  Sustain centroid (300ms):    790 Hz   (target: 500-800)  OK",
                       "  Drift:                      +90 Hz   (target: -200 to -50) MISS"]
    assert up[0] == "Centroid tracking: E2 (MIDI 40) vel=64, 50ms Hann windows"
    nan = ct.format_report(60, 100, 5.0, [math.nan, math.nan], [10.0, 300.0]).splitlines()      # NaN > 0.0 is false: not printed; the summary shows it
    assert nan[3] == "" and nan[4] == "  Attack centroid (10ms):      NaN Hz   (target: 600-1200)  MISS" and nan[6].endswith("(target: -240 to -30) MISS")


def test_targets_by_register_and_display_of_the_window():
    from openwurli_amd import centroid_track as ct
    assert ct.targets(48) == (600.0, 1000.0, 500.0, 800.0, -200.0, -50.0) and ct.targets(33) == ct.targets(48)
    assert ct.targets(49) == (600.0, 1200.0, 600.0, 1000.0, -240.0, -30.0) and ct.targets(72) == ct.targets(49)
    assert ct.targets(73) == (800.0, 1600.0, 800.0, 1400.0, -250.0, -30.0) and ct.targets(96) == ct.targets(73)
    assert [ct.rust_display(x) for x in (5.0, 2.5, 0.1, 100.0, 1e-5, 1e16, -0.5)] == ["5", "2.5", "0.1", "100", "0.00001", "10000000000000000", "-0.5"]
    # interval edges are inside
    r = ct.summarise(60, [600.0, 1000.0], [10.0, 300.0])
    assert (r["attack_status"], r["sustain_status"], r["drift"], r["drift_status"]) == (ct.CENTROID_OK, ct.CENTROID_OK, 400.0, ct.CENTROID_MISS)
    g = ct.grid_jobs()
    assert g.size == 512 and (g["note"][0], g["velocity"][0], g["note"][-1], g["velocity"][-1]) == (33, 20, 96, 127) and (g["volume"] == 0.60).all()
    rows = np.zeros(2, dtype=ct.ROW_DTYPE)
    rows[0] = ct.summarise(33, [700.04, 650.0], [10.0, 300.0])
    rows[1] = ct.summarise(33, [0.0], [10.0])
    assert ct.format_grid_csv(g[:2], rows) == ("note,velocity,c10,c300,drift,attack_status,sustain_status,drift_status\n"
                                               "33,20,700.0,650.0,-50.0,OK,OK,OK\n33,35,0.0,,,MISS,,\n")


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------
def test_status_bytes_are_the_headers_enum_line():
    from openwurli_amd import binding
    hdr = open(os.path.join(ROOT, "include", "openwurli_hip.h")).read()
    assert re.search(r"OW_CENTROID_NO_DATA = 0, OW_CENTROID_OK = 1, OW_CENTROID_MISS = 2", hdr)
    assert (binding.CENTROID_NO_DATA, binding.CENTROID_OK, binding.CENTROID_MISS) == (0, 1, 2)


def _track(lib, jobs, cfg, frames_stride=4096, audio=None, audio_stride=0):
    from openwurli_amd import centroid_track as ct
    rows = np.zeros(max(jobs.size, 1), dtype=ct.ROW_DTYPE)
    frames = np.zeros((max(jobs.size, 1), max(frames_stride, 1)))
    return lib.ow_centroid_track(jobs.ctypes.data_as(C.c_void_p), jobs.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p), frames.ctypes.data_as(C.c_void_p),
                                 frames_stride, audio.ctypes.data_as(C.c_void_p) if audio is not None else None, audio_stride)


def _refused(lib, call, prefix, *needles):
    from openwurli_amd import binding
    lib.ow_clear_error()
    assert call() < 0
    msg = binding.take_error(lib)
    assert msg.startswith(prefix + ": ") and all(s in msg for s in needles), msg


def test_bad_configurations_are_refused_before_device_work(hiplib):
    from openwurli_amd import binding, centroid_track as ct
    job = ct.make_job()
    Cfg = binding.OwCentroidCfg
    cases = [
        (Cfg(hop_ms=0.01), ("hop_samples is 0", "never end")),
        (Cfg(hop_ms=0.0), ("hop_samples is 0",)),
        (Cfg(hop_ms=math.nan), ("hop_samples is 0",)),
        (Cfg(window_ms=0.03), ("no bin in range", "k_min 1 > k_max 0")),         # one sample
        (Cfg(window_ms=0.0), ("window_samples is 0",)),
        (Cfg(window_ms=-5.0), ("window_samples is 0",)),
        (Cfg(window_ms=100.0), ("4410 samples", "OW_CENTROID_MAX_WINDOW = 4096")),
        (Cfg(preamp_kind=1), ("OW_PREAMP_MELANGE12", "--ldr")),
        (Cfg(power_amp_kind=1), ("OW_POWER_AMP_MELANGE", "own launch")),
        (Cfg(preamp_kind=7), ("unknown preamp_kind",)),
        (Cfg(power_amp_kind=7), ("unknown power_amp_kind",)),
        (Cfg(duration_s=1e9), ("duration_s", "2^31")),
        (Cfg(duration_s=math.nan), ("duration_s",)),
    ]
    for field, bad in (("struct_size", C.sizeof(Cfg) - 4), ("job_size", C.sizeof(binding.OwCentroidJob) + 8)):
        cfg = Cfg()
        setattr(cfg, field, bad)
        cases.append((cfg, ("ABI mismatch", "OW_ABI_VERSION 8")))
    for cfg, needles in cases:
        _refused(hiplib, lambda: hiplib.ow_centroid_frame_count(C.byref(cfg)), "ow_centroid_frame_count", *needles)
        _refused(hiplib, lambda: _track(hiplib, job, cfg), "ow_centroid_track", *needles)
    # the largest window that is accepted, and strides
    assert hiplib.ow_centroid_frame_count(C.byref(Cfg(window_ms=92.88))) > 0 and ct.ms_to_samples(92.88) == 4096
    _refused(hiplib, lambda: _track(hiplib, job, Cfg(), frames_stride=199), "ow_centroid_track", "frames_stride", "200 frames")
    _refused(hiplib, lambda: _track(hiplib, job, Cfg(), audio=np.zeros(44099), audio_stride=44099), "ow_centroid_track", "audio_stride", "44100 samples")
    with pytest.raises(binding.OwError, match="ow_centroid_track: hop_samples is 0"):
        ct.run_jobs(job, hop_ms=0.0)
    with pytest.raises(binding.OwError, match="ow_centroid_frame_count: window of 4410 samples"):
        ct.frame_count(window_ms=100.0)


def test_bad_jobs_are_refused_before_device_work(hiplib):
    from openwurli_amd import binding, centroid_track as ct
    good = ct.make_jobs([(60, 100), (40, 127)])
    cfg = binding.OwCentroidCfg()

    def bad(field, value):
        j = good.copy()
        j[field][1] = value
        return j
    call = lambda j: (lambda: _track(hiplib, j, cfg))
    _refused(hiplib, call(bad("note", 32)), "ow_centroid_track", "job 1", "note 32", "33..96")
    _refused(hiplib, call(bad("note", 97)), "ow_centroid_track", "job 1", "note 97")
    _refused(hiplib, call(bad("velocity", 128)), "ow_centroid_track", "job 1", "velocity 128", "127")
    for v in (0.0, -1.0, math.nan, math.inf):
        _refused(hiplib, call(bad("r_ldr", v)), "ow_centroid_track", "job 1", "r_ldr", "finite positive")
    for f in ("volume", "speaker"):
        for v in (math.nan, math.inf, -math.inf):
            _refused(hiplib, call(bad(f, v)), "ow_centroid_track", "job 1", f, "finite")
    for v in (math.nan, math.inf):
        j = bad("displacement_scale", v)
        j["has_displacement_scale"][1] = 1
        _refused(hiplib, call(j), "ow_centroid_track", "job 1", "displacement_scale", "finite")
    # an empty call returns the frame count; a zero-length render has no frame and no data
    assert _track(hiplib, np.zeros(0, dtype=ct.JOB_DTYPE), cfg) == 200
    rows, frames = ct.run_jobs(good, duration=0.0)
    assert frames.shape == (2, 0) and not rows["has_c10"].any() and not rows["has_c300"].any() and (rows["frame10"] == -1).all()
    assert list(rows["attack_hi"]) == [1200.0, 1000.0]


def test_analyze_refusals_before_device_work(hiplib):
    sig = np.zeros((2, 1000))
    out = np.zeros((2, 64))

    def call(stride=1000, length=1000, window=220, hop=110, end=1000, frames_stride=64):
        return lambda: hiplib.ow_centroid_analyze(sig.ctypes.data_as(C.c_void_p), 2, stride, length, window, hop, end, 0, 0, out.ctypes.data_as(C.c_void_p), frames_stride)
    _refused(hiplib, call(hop=0), "ow_centroid_analyze", "hop_samples is 0")
    _refused(hiplib, call(window=1), "ow_centroid_analyze", "no bin in range")
    _refused(hiplib, call(window=0), "ow_centroid_analyze", "window_samples is 0")
    _refused(hiplib, call(window=4097), "ow_centroid_analyze", "4097 samples", "OW_CENTROID_MAX_WINDOW")
    _refused(hiplib, call(length=1001), "ow_centroid_analyze", "stride", "1001 samples")
    _refused(hiplib, call(frames_stride=7), "ow_centroid_analyze", "frames_stride", "8 frames")
    # no frame: nothing to do, nothing written, no device needed
    out[:] = -7.0
    assert call(length=219)() == 0 and call(end=109)() == 0 and (out == -7.0).all()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,k", [(220, 7), (441, 30), (2205, 100)])
def test_restatement_on_a_sine_at_an_exact_bin_frequency(window, k):
    """A sine at bin k of the frame: the periodic Hann window spreads it over the bins k - 1, k, k + 1 alone (weights 1/4, 1/2, 1/4 in
    amplitude, symmetric), so the centroid is the bin frequency itself -- far inside the main lobe's half width of two bins."""
    f = k * 44100.0 / window
    sig = np.sin(2.0 * np.pi * f * np.arange(3 * window) / 44100.0 + 0.3)
    fr, sp = ref.analyze(sig, window, window // 2, 10 ** 9, spectra=True)
    assert fr.size == 5
    assert np.abs(fr - f).max() < 1e-6 * f, (fr, f)
    k_min, k_max = ref.bins(window)
    mag = np.hypot(sp[..., 0], sp[..., 1])
    assert sp.shape == (5, k_max - k_min + 1, 2) and (np.argmax(mag, axis=1) == k - k_min).all()
    # the analysis alone agrees with a direct evaluation of the definition
    hw = ref.hann(window)
    ks = np.arange(k_min, k_max + 1)
    X = (sig[:window] * hw) @ np.exp(-2j * np.pi * np.outer(np.arange(window), ks) / window)
    P = np.abs(X) ** 2
    assert abs(fr[0] - float(np.sum(ks * (44100.0 / window) * P) / np.sum(P))) < 1e-9 * f
    assert ref.analyze(np.zeros(1000), 220, 110, 1000).tolist() == [0.0] * 8
    nanrow = np.ones(1000); nanrow[500] = np.nan
    got = ref.analyze(nanrow, 220, 110, 1000)
    assert [x == 0.0 for x in got] == [False, False, False, True, True, False, False, False]      # the frames that hold sample 500


@pytest.mark.parametrize("poweramp", [True, False])
def test_one_note_job_at_1_mohm_equals_the_oracles_batch_job_bit_for_bit(oracle, poweramp):
    """At 1 Mohm set_ldr_resistance moves nothing and the order of reset() is immaterial: the chain of centroid-track is the chain of
    `render` with --no-mlp."""
    job = ref.Job(57, 90, no_poweramp=not poweramp)
    a = ref.render(job, 0.5)
    b = oracle.batch_render_job_ex(57, 90, 0.5, 44100.0, 0.60, 1.0, 1e6, mlp=False, poweramp=poweramp)
    assert a.size == b.size == 22050 and a.tobytes() == b.tobytes()
    ds = ref.render(ref.Job(57, 90, displacement_scale=0.30, no_preamp=True), 0.25)
    assert ds.tobytes() == oracle.batch_render_job_ex(57, 90, 0.25, 44100.0, 0.60, 1.0, 1e6, mlp=False, displacement_scale=0.30, no_preamp=True).tobytes()


def test_reset_order_matters_at_19k(oracle):
    """set_ldr_resistance BEFORE reset(): the DC solve runs at --ldr.  `render` resets first: more than the parity bar apart."""
    a = ref.render(ref.JOBS["ldr_19k"], ref.DURATION)
    j = ref.JOBS["ldr_19k"]
    b = oracle.batch_render_job_ex(j.note, j.velocity, ref.DURATION, 44100.0, j.volume, j.speaker, j.ldr, mlp=False)
    rep = oracle.parity_report(a, b, abs_floor=oracle.ABS_FLOOR_BATCH)
    assert rep["n_bad"] > 1000 and rep["max_err_rel_peak"] > 1e-2, rep


# ---- the bars of the GPU test -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job_refs():
    names = list(ref.JOBS)
    kw = dict(duration=ref.DURATION, end_ms=ref.END_MS)
    a = ref.track_many([ref.JOBS[k] for k in names], **kw)
    b = ref.track_many([ref.JOBS[k] for k in names], perturbed=True, **kw)
    return {k: (x, y) for k, x, y in zip(names, a, b)}


def test_one_hz_condition_holds_for_every_job_of_the_gpu_list(oracle, job_refs):
    """For every job the GPU test runs, at least 90 % of the frames up to end_ms have a derived bound below 1 Hz, the resolution the
    command prints: only then are summary statuses asserted.  The one-ulp-exp build's own movement of c is printed beside the bound."""
    assert ref.ANALYSIS_REL <= ref.ANALYSIS_REL_CAP == 1e-9 and ref.SECOND_ORDER == 1.5 and ref.ONE_HZ_SHARE == 0.90
    for k, (a, p) in job_refs.items():
        assert a.frames.size == 128 and (a.frames > 0.0).all(), k
        bound = ref.frame_bounds(a, oracle.ABS_FLOOR_BATCH)
        moved = np.abs(a.frames - p.frames)
        print(f"\n[centroid bars] {k}: bound max {bound.max():.3g} Hz median {np.median(bound):.3g}; share below 1 Hz {ref.one_hz_share(a, oracle.ABS_FLOOR_BATCH):.3f}; "
              f"one-ulp exp moves c by at most {moved.max():.3g} Hz ({np.max(moved / bound):.2g} of its frame's bound)")
        assert ref.one_hz_share(a, oracle.ABS_FLOOR_BATCH) >= ref.ONE_HZ_SHARE, k
        assert (moved <= bound).all(), k            # the reference's own sensitivity stays inside the first-order bound
        assert np.array_equal(ref.frame_bars(a, oracle.ABS_FLOOR_BATCH), 1.5 * bound + ref.ANALYSIS_REL * a.frames)
    # ... which is a real condition: a very quiet render sits on the absolute floor and fails it
    quiet = ref.track(ref.Job(60, 5, volume=0.05), duration=0.1, end_ms=90.0)
    assert ref.one_hz_share(quiet, oracle.ABS_FLOOR_BATCH) < ref.ONE_HZ_SHARE


def test_bound_covers_a_sample_perturbation_inside_the_bars(oracle, job_refs):
    """The derivation, tried: moving every sample by its full bar with the sign that pushes c upward moves c by less than 1.5 x the bound."""
    a, _ = job_refs["default"]
    bar = ref.sample_bar(a.audio, oracle.ABS_FLOOR_BATCH)
    rng = np.random.default_rng(7)
    bound = ref.frame_bounds(a, oracle.ABS_FLOOR_BATCH)
    for _ in range(3):
        moved = ref.analyze(a.audio + bar * rng.choice([-1.0, 1.0], a.audio.size), a.window, a.hop, a.end)
        assert (np.abs(moved - a.frames) <= bound).all()
    assert ref.clear_of_edges(700.0, 1.0, 600.0, 1200.0) and not ref.clear_of_edges(600.5, 1.0, 600.0, 1200.0) and not ref.clear_of_edges(1199.5, 1.0, 600.0, 1200.0)
