"""The note audits (`preamp-bench intermod-audit` / `overshoot`) without a device: the static risk table against the CPU restatement,
every refusal, the paths that need no device, the probe lists, the commands' text and the tools' flags.  The restatement
itself is pinned by tables.rs's own three intermod tests (test_intermod_risk_below_threshold, test_intermod_risk_known_values,
test_perceptual_beat_weight_shape), restated assertion for assertion."""
import ctypes as C
import io
import math
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import note_audit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PRODUCT_FIELDS = ("mode", "nearest_integer", "mode_ratio", "fractional_offset", "beat_hz", "effective_amplitude", "perceptual_weight", "risk_score")


# ---- the restatement against tables.rs's own three intermod tests, restated assertion for assertion ---------------------------------
def test_restated_intermod_risk_below_threshold():
    """tables.rs:898-939 test_intermod_risk_below_threshold, the regression guard: 1.25 x the worst max_risk over MIDI_LO..=MIDI_HI is
    below 0.15, and every note's max_risk is below that threshold."""
    worst_risk, worst_midi = 0.0, 0
    for midi in range(33, 97):
        report = ref.intermod_risk(midi)
        if report.max_risk > worst_risk:
            worst_risk, worst_midi = report.max_risk, midi
    threshold = worst_risk * 1.25
    assert threshold < 0.15, (worst_midi, worst_risk, threshold)
    for midi in range(33, 97):
        report = ref.intermod_risk(midi)
        assert report.max_risk < threshold, (midi, report.fundamental_hz, report.max_risk, threshold)


def test_restated_intermod_risk_known_values():
    """tables.rs:941-966 test_intermod_risk_known_values: A1 (MIDI 33), mu = 0.10, mode 2 at ratio ~7.13."""
    report = ref.intermod_risk(33)
    m2 = report.products[0]                                     # mode 2 is first in the products
    assert m2.mode == 2
    assert abs(m2.mode_ratio - 7.13) < 0.1, m2.mode_ratio
    assert m2.nearest_integer == 7
    assert 3.0 < m2.beat_hz < 12.0, m2.beat_hz                  # A1 = 55 Hz, offset ~0.13
    assert m2.perceptual_weight > 0.8, m2.perceptual_weight     # the 5-10 Hz zone


def test_restated_perceptual_beat_weight_shape():
    """tables.rs:968-976 test_perceptual_beat_weight_shape."""
    assert ref.perceptual_beat_weight(0.3) < 0.01
    assert ref.perceptual_beat_weight(7.0) > 0.9
    assert ref.perceptual_beat_weight(50.0) < 0.2


# ---- further checks of the restatement, this project's own (not from tables.rs) ----------------------------------------------------------
def test_restatement_beat_weight_branches():
    """Every branch of perceptual_beat_weight (tables.rs:703-725) and its edges, from the function's text."""
    w = ref.perceptual_beat_weight
    assert w(0.0) == 0.0 and w(0.49) == 0.0 and w(0.5) == 0.0
    assert 0.0 < w(1.0) < 0.5
    assert abs(w(2.0) - 0.5) < 1e-12 and w(3.5) == 0.75
    assert abs(w(5.0) - 1.0) < 1e-12 and w(7.5) == 1.0 and w(10.0) == 1.0
    assert 0.1 < w(25.0) < 1.0 and abs(w(40.0) - 0.1) < 1e-12
    assert w(41.0) == 0.1 and w(1000.0) == 0.1


def test_restatement_reports_are_consistent():
    """Every note of the range: six products, modes 2..7, finite figures, max_risk and total_risk are what the products give."""
    for midi in range(33, 97):
        r = ref.intermod_risk(midi)
        assert len(r.products) == 6 and [p.mode for p in r.products] == [2, 3, 4, 5, 6, 7]
        for p in r.products:
            assert all(math.isfinite(getattr(p, f)) for f in PRODUCT_FIELDS)
            assert p.risk_score >= 0.0 and 0.0 <= p.fractional_offset <= 0.5 and p.nearest_integer >= 1
            assert p.beat_hz == p.fractional_offset * r.fundamental_hz and p.risk_score == p.effective_amplitude * p.perceptual_weight
        assert r.max_risk == max(p.risk_score for p in r.products)
        assert abs(r.total_risk - sum(p.risk_score for p in r.products)) <= 1e-15
    r = ref.intermod_risk(57)                                   # mu = 0 between MIDI 52 and 62: the bare beam's ratios (tables.rs:91-93)
    assert r.mu == 0.0 and abs(r.products[0].mode_ratio - (4.6941 / 1.8751) ** 2) < 1e-12 and r.products[0].nearest_integer == 6


# ---- ow_intermod_risk ----------------------------------------------------------------------------------------------------------------
def test_intermod_risk_matches_restatement_bit_for_bit(hiplib):
    from openwurli_amd import intermod_audit as ia
    for midi in range(256):
        g, c = ia.risk(midi), ref.intermod_risk(midi)
        assert int(g["midi"]) == midi
        got = [g["fundamental_hz"], g["mu"], g["max_risk"], g["total_risk"]] + [float(p[f]) for p in g["products"] for f in PRODUCT_FIELDS]
        want = [c.fundamental_hz, c.mu, c.max_risk, c.total_risk] + [float(getattr(p, f)) for p in c.products for f in PRODUCT_FIELDS]
        assert np.array(got).tobytes() == np.array(want).tobytes(), midi
    assert hiplib.ow_intermod_risk(60, None) < 0 and b"null argument" in hiplib.ow_last_error()
    hiplib.ow_clear_error()


def test_probe_lists_match_restatement(hiplib):
    from openwurli_amd import intermod_audit as ia
    want_h = {33: (32, 31), 60: (32, 31), 96: (10, 9)}          # H = min(floor(22050 / f0), 32): 400 -> 32, 84 -> 32, 10
    for midi in list(want_h) + [45, 72, 84, 90]:
        f, nh, nm = ia.probes(midi)
        cf, ch, cm = ref.probes(midi)
        assert (nh, nm) == (ch, cm) and f.tobytes() == cf.tobytes()
        assert f.size <= 75 and np.all(f[:nh + nm] < 22050.0)
        if midi in want_h:
            assert (nh, nm) == want_h[midi]
        listed = sum(1 for p in ref.intermod_risk(midi).products if p.risk_score >= 0.001)
        assert f.size == nh + nm + 2 * listed
    for bad in (32, 97):
        with pytest.raises(ia.OwError, match="outside 33..96"):
            ia.probes(bad)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _call(hiplib, fn, jobs, cfg, rows, audio=None, stride=0, n_jobs=None):
    hiplib.ow_clear_error()
    rc = getattr(hiplib, fn)(None if jobs is None else jobs.ctypes.data_as(C.c_void_p), len(jobs) if n_jobs is None else n_jobs, cfg,
                             None if rows is None else rows.ctypes.data_as(C.c_void_p), None if audio is None else audio.ctypes.data_as(C.c_void_p), stride)
    msg = hiplib.ow_last_error().decode()
    hiplib.ow_clear_error()
    return rc, msg


@pytest.mark.parametrize("fn", ["ow_intermod_audit", "ow_overshoot"])
def test_refusals(hiplib, fn):
    from openwurli_amd import binding as b, intermod_audit as ia, overshoot as ov
    Cfg, dt = (b.OwIntermodCfg, ia.ROW_DTYPE) if fn == "ow_intermod_audit" else (b.OwOvershootCfg, ov.ROW_DTYPE)
    name = "ow_intermod_cfg" if fn == "ow_intermod_audit" else "ow_overshoot_cfg"
    jobs, rows = ia.note_jobs([60], [100]), np.zeros(1, dtype=dt)
    for field, bad in (("struct_size", 16), ("job_size", 4)):
        cfg = Cfg(1.0)
        setattr(cfg, field, bad)
        rc, msg = _call(hiplib, fn, jobs, C.byref(cfg), rows)
        assert rc < 0 and msg == f"{fn}: ABI mismatch: {name}.struct_size / job_size do not match this library's openwurli_hip.h (OW_ABI_VERSION 8)"
    rc, msg = _call(hiplib, fn, jobs, None, rows)
    assert rc < 0 and msg == f"{fn}: null argument"
    for note, text in ((32, "job 1: note 32 outside 33..96 (the tables' range)"), (97, "job 1: note 97 outside 33..96 (the tables' range)")):
        rc, msg = _call(hiplib, fn, ia.note_jobs([60, note], [100]), C.byref(Cfg(1.0)), np.zeros(2, dtype=dt))
        assert rc < 0 and msg == f"{fn}: {text}"
    rc, msg = _call(hiplib, fn, ia.note_jobs([60], [128]), C.byref(Cfg(1.0)), rows)
    assert rc < 0 and msg == f"{fn}: job 0: velocity 128 above 127 (a MIDI velocity byte)"
    for dur in (2.0 ** 31 / 44100.0 + 1.0, float("inf"), float("nan")):
        rc, msg = _call(hiplib, fn, jobs, C.byref(Cfg(dur)), rows)
        assert rc < 0 and msg == f"{fn}: duration_s must give fewer than 2^31 samples"
    rc, msg = _call(hiplib, fn, jobs, C.byref(Cfg(0.01)), rows, np.zeros(440), 440)
    assert rc < 0 and msg == f"{fn}: audio_stride smaller than the 441 samples of a job"
    rc, msg = _call(hiplib, fn, None, C.byref(Cfg(0.01)), rows, n_jobs=1)
    assert rc < 0 and msg == f"{fn}: null argument"
    rc, msg = _call(hiplib, fn, jobs, C.byref(Cfg(0.01)), None)
    assert rc < 0 and msg == f"{fn}: null argument"
    # n_jobs == 0 returns the sample count and touches nothing, whatever the other pointers are
    rc, msg = _call(hiplib, fn, None, C.byref(Cfg(0.6)), None, n_jobs=0)
    assert rc == 26460 and msg == ""


def test_dft_magnitudes_refusals(hiplib):
    x, f, out = np.zeros(64), np.zeros(2), np.zeros(2)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    def call(sig, stride, start, end, sr, fr, dst):
        hiplib.ow_clear_error()
        rc = hiplib.ow_dft_magnitudes(p(sig), 1, stride, start, end, sr, p(fr), 2, 0, 0, p(dst))
        msg = hiplib.ow_last_error().decode()
        hiplib.ow_clear_error()
        return rc, msg
    assert call(x, 64, 0, 65, 44100.0, f, out) == (-1, "ow_dft_magnitudes: window end 65 beyond the stride of 64 samples")
    assert call(x, 64, 8, 8, 44100.0, f, out) == (-1, "ow_dft_magnitudes: empty window: end 8 <= start 8")
    assert call(x, 64, 9, 8, 44100.0, f, out) == (-1, "ow_dft_magnitudes: empty window: end 8 <= start 9")
    for sr in (0.0, -1.0, float("nan"), float("inf")):
        assert call(x, 64, 0, 64, sr, f, out) == (-1, "ow_dft_magnitudes: sample_rate is not a finite positive number")
    for args in ((None, f, out), (x, None, out), (x, f, None)):
        assert call(args[0], 64, 0, 64, 44100.0, args[1], args[2]) == (-1, "ow_dft_magnitudes: null argument")


# ---- the paths that need no device -----------------------------------------------------------------------------------------------------
def test_too_short_needs_no_device(hiplib):
    """duration 0.5 s: end = 22 050 = start."""
    from openwurli_amd import intermod_audit as ia
    rows = ia.run_jobs(ia.note_jobs([33, 60], [127, 64]), 0.5)
    assert rows.size == 4 and np.all(rows["too_short"] == 1) and np.all(rows["window_start"] == 22050) and np.all(rows["window_end"] == 22050)
    assert list(rows["midi"]) == [33, 33, 60, 60] and list(rows["velocity"]) == [127, 64, 127, 64]
    assert np.all(rows["h_db"] == 0.0) and np.all(rows["ratio_db"] == 0.0)
    a = ref.intermod_audit(np.zeros(22050), 60)
    assert a.too_short and (a.start, a.end) == (22050, 22050)
    r = rows[2]
    assert r["fundamental_hz"] == ref.intermod_risk(60).fundamental_hz and (r["n_harmonics"], r["n_midpoints"]) == (32, 31)
    rep = ref.intermod_risk(60)
    for p, c in zip(r["products"], rep.products):               # the static part of the detail is there all the same
        assert (p["mode"], p["nearest_integer"], bool(p["listed"]), p["intermod_freq"], p["nearest_freq"], p["risk_score"], p["intermod_mag"]) == \
               (c.mode, c.nearest_integer, c.risk_score >= 0.001, c.mode_ratio * rep.fundamental_hz, c.nearest_integer * rep.fundamental_hz, c.risk_score, 0.0)
    assert "(signal too short)" in "\n".join(ia.format_render(rows))


def test_overshoot_of_no_samples_needs_no_device(hiplib):
    from openwurli_amd import overshoot as ov
    rows = ov.audit([60], [64], duration=0.0)
    c = ref.overshoot(np.zeros(0))
    for f in ref.Overshoot._fields:
        g, w = float(rows[0][f]), getattr(c, f)
        assert (math.isnan(g) and math.isnan(w)) or g == w, f
    assert math.isnan(rows[0]["overshoot_db"]) and rows[0]["pk_dbfs"] == -120.0
    assert ref.overshoot_edges() == [441, 2205, 4410, 8820, 44100, 66150]


# ---- the commands' text ----------------------------------------------------------------------------------------------------------------
def _prod(mode, risk, ratio=6.25, nearest=6, off=0.25, beat=12.5, amp=0.0031, w=0.925):
    return {"mode": mode, "nearest_integer": nearest, "mode_ratio": ratio, "fractional_offset": off, "beat_hz": beat, "effective_amplitude": amp,
            "perceptual_weight": w, "risk_score": risk}


def _report(midi, mu, risks):
    return {"midi": midi, "mu": mu, "max_risk": max(risks), "total_risk": sum(risks), "fundamental_hz": 0.0,
            "products": [_prod(k + 2, r, ratio=6.25 + k) for k, r in enumerate(risks)]}


def test_static_table_text_by_hand():
    """"{:>6} {:>4} {:>6.4}  {:>5} {:>6.3} {:>8.5} {:>8.2} {:>7.4} {:>7.3} {:>8.5}{}" (main.rs:762): widths, precision, the *** flag, the
    max_by tie (Rust returns the LAST of equal maxima: mode 5 below, not mode 3) and the flagged block."""
    from openwurli_amd import intermod_audit as ia
    reps = [_report(33, 0.1, [0.05, 0.08, 0.01, 0.08, 0.0, 0.0]), _report(61, 0.0, [0.002, 0.001, 0.0, 0.0, 0.0, 0.0]),
            _report(96, 0.01, [0.07, 0.0, 0.0, 0.0, 0.0, 0.0])]
    lines, flagged = ia.format_static([33, 61, 96], 0.07, reps)
    assert lines == [
        "=== INTERMOD RISK AUDIT ===",
        "Threshold: 0.0700",
        "",
        "  Note MIDI     mu   Mode  Ratio   Offset  Beat Hz Eff Amp  Weight     Risk",
        "-" * 82,
        "    A1   33 0.1000      5  9.250  0.25000    12.50  0.0031   0.925  0.08000 ***",
        "   C#4   61 0.0000      2  6.250  0.25000    12.50  0.0031   0.925  0.00200",
        "    C7   96 0.0100      2  6.250  0.25000    12.50  0.0031   0.925  0.07000 ***",
        "",
        "Flagged notes (risk >= 0.0700): 2",
        "  A1 (33), C7 (96)",
    ]
    assert flagged == [33, 96]
    lines, flagged = ia.format_static([61], 0.07, reps[1:2])
    assert lines[-2:] == ["", "Flagged notes (risk >= 0.0700): 0"] and flagged == []


def test_static_table_from_restatement_numbers(hiplib):
    from openwurli_amd import intermod_audit as ia
    notes = [33, 60, 96]
    lines, _ = ia.format_static(notes, 0.07, [ref.risk_record(m) for m in notes])
    assert lines[5:8] == ["    A1   33 0.1000      2  7.138  0.13755     7.57  0.0034   1.000  0.00338",
                          "    C4   60 0.0000      2  6.267  0.26694    69.84  0.0032   0.100  0.00032",
                          "    C7   96 0.0100      2  6.355  0.35510   743.22  0.0022   0.100  0.00022"]
    assert ia.format_static(notes, 0.07)[0] == lines              # the library's table prints the same


def _row(midi, h, m, verdict, too_short=False, prods=()):
    return {"midi": midi, "velocity": 127, "too_short": too_short, "h_db": h, "m_db": m, "ratio_db": h - m, "verdict": verdict, "products": list(prods)}


def test_render_table_text_by_hand():
    """"{:>6} {:>4}  {:>10.1} {:>10.1} {:>10.1}  {:>8}" (main.rs:856) and the per-product lines (:883), which only rows at ratio_db <= 30.0
    get, and of them only the listed products."""
    from openwurli_amd import intermod_audit as ia
    d = lambda mode, listed, r: {"mode": mode, "nearest_integer": 6, "listed": listed, "intermod_freq": 392.584, "nearest_freq": 330.0, "ratio_db": r,
                                 "risk_score": 0.00338, "intermod_mag": 0.0, "nearest_mag": 0.0}
    rows = [_row(33, -12.34, -60.0, 3, prods=[d(2, True, -3.0)]), _row(60, -20.0, -55.04, 2), _row(61, -20.0, -50.0, 1, prods=[d(2, True, -41.25), d(3, False, 0.0), d(4, True, 0.0)]),
            _row(62, -20.0, -120.0, 3), _row(96, 0.0, 0.0, 0, too_short=True), _row(72, -30.0, -11.0, 0, prods=[])]
    assert ia.format_render(rows, 3.0) == [
        "",
        "=== RENDER ANALYSIS (sustain spectral grass) ===",
        "Duration: 3.0s, analysis window: 0.5-2.0s",
        "",
        "  Note MIDI   Harm (dB)   Mid (dB) Ratio (dB)   Verdict",
        "-" * 64,
        "    A1   33       -12.3      -60.0       47.7     CLEAN",
        "    C4   60       -20.0      -55.0       35.0        OK",
        "   C#4   61       -20.0      -50.0       30.0  MARGINAL",
        "  Per-product detail:",
        "    Mode 2: 392.6 Hz (near H6 @ 330.0 Hz) intermod/harmonic = -41.2 dB, risk=0.00338",
        "    Mode 4: 392.6 Hz (near H6 @ 330.0 Hz) intermod/harmonic = 0.0 dB, risk=0.00338",
        "    D4   62       -20.0     -120.0      100.0     CLEAN",
        "    C7   96  (signal too short)",
        "    C5   72       -30.0      -11.0      -19.0     DIRTY",
        "  Per-product detail:",
    ]
    assert ia.format_render([], 0.55)[2] == "Duration: 0.6s, analysis window: 0.5-2.0s"          # {:.1} of 0.55 (binary 0.55000000000000004)


def test_report_branches(hiplib):
    """Without --notes only flagged notes are rendered; with --notes all given notes; without --render the hint; nothing to render: all clear."""
    from openwurli_amd import intermod_audit as ia
    seen = []
    def run(notes, duration):
        seen.append((list(notes), duration))
        return [_row(m, -10.0, -52.0, 3) for m in notes]
    top = max(float(ia.risk(m)["max_risk"]) for m in range(33, 97))
    text = ia.report(threshold=top, render=True, duration=1.5, run=run)                         # exactly the riskiest notes are flagged (>=)
    flagged = [m for m in range(33, 97) if float(ia.risk(m)["max_risk"]) >= top]
    assert seen == [(flagged, 1.5)] and flagged
    assert text.count(" ***\n") == len(flagged) and "Flagged notes (risk >= %.4f): %d\n" % (top, len(flagged)) in text
    assert text.endswith("%6s %4d  %10.1f %10.1f %10.1f  %8s\n" % (ia.midi_note_name(flagged[-1]), flagged[-1], -10.0, -52.0, 42.0, "CLEAN"))
    assert len(text.split("\n")) == 5 + 64 + 3 + 6 + len(flagged) + 1
    text = ia.report(threshold=top, render=False)
    assert text.endswith("\n\nRun with --render to analyze flagged notes spectrally.\n")
    text = ia.report(threshold=top * 2, render=False)
    assert text.endswith("Flagged notes (risk >= %.4f): 0\n" % (top * 2))
    del seen[:]
    text = ia.report(threshold=top * 2, render=True, run=run)
    assert text.endswith("Flagged notes (risk >= %.4f): 0\n\nNo notes to render-analyze. All clear!\n" % (top * 2)) and not seen
    text = ia.report(threshold=top * 2, render=True, notes=[60, 61], run=run)                   # --notes: rendered though not flagged
    assert seen == [([60, 61], 3.0)] and text.count("CLEAN") == 2
    text = ia.report(threshold=top * 2, render=True, notes=[], run=run)                         # --notes with nothing that parses
    assert text.endswith("No notes to render-analyze. All clear!\n") and len(seen) == 1


def test_overshoot_text_by_hand():
    """"{:>6} {:>4}  {:>7.1} {:>7.1} {:>7.1}  {:>9.1} {:>9.1}" (main.rs:2218): NaN as Rust prints it, a blank line after each note."""
    from openwurli_amd import overshoot as ov
    r = lambda pk, r1, r2, o, b: {"pk_dbfs": pk, "rms1_dbfs": r1, "rms2_dbfs": r2, "overshoot_db": o, "bark_decay_db": b}
    nan = float("nan")
    text = ov.format_report([36, 84], [64, 127], [r(-20.04, -25.06, -120.0, 5.02, nan), r(-10.0, -13.25, -31.0, 3.25, 21.0), r(-120.0, -120.0, -120.0, nan, nan),
                                                  r(-3.0, -9.0, -40.0, 6.0, 37.0)])
    assert text.split("\n") == [
        "=== OVERSHOOT AUDIT ===",
        "Spec metric:  0-10ms peak vs 100-200ms RMS (calibration-and-evaluation.md §10.1)",
        "Bark decay:   0-50ms peak vs 1000-1500ms RMS (perceptual bark fade, NOT overshoot)",
        "",
        "  Note  Vel  Pk(0-10) RMS(sus) RMS(late)   Overshoot  BarkDecay",
        "                 dBFS     dBFS     dBFS          dB         dB",
        "-" * 76,
        "    C2   64    -20.0   -25.1  -120.0        5.0       NaN",
        "    C2  127    -10.0   -13.2   -31.0        3.2      21.0",
        "",
        "    C6   64   -120.0  -120.0  -120.0        NaN       NaN",
        "    C6  127     -3.0    -9.0   -40.0        6.0      37.0",
        "",
        "Targets (from calibration-and-evaluation.md §4.1 & §10.1):",
        "  Overshoot at mf (v64):   2-5 dB   (from modal superposition)",
        "  Overshoot at ff (v127):  5-10 dB  (from modal superposition)",
        "  Bark decay:              no target (physics-correct bark fade, not a defect)",
        "",
    ]


def test_grid_csv():
    from openwurli_amd import intermod_audit as ia
    rows = [dict(_row(60, -20.0, -55.044, 2), velocity=20), dict(_row(96, 0.0, 0.0, 0, too_short=True), velocity=127)]
    assert ia.format_grid_csv(rows) == "note,velocity,h_db,m_db,ratio_db,verdict\n60,20,-20.00,-55.04,35.04,OK\n96,127,,,,\n"


# ---- the tools' flags ------------------------------------------------------------------------------------------------------------------
def test_tool_flags(hiplib, monkeypatch):
    import intermod_audit as tool_ia
    import overshoot as tool_ov
    from openwurli_amd import intermod_audit as ia, overshoot as ov
    from openwurli_amd._rust_text import parse_csv_u8
    assert parse_csv_u8("36, 48,x,256,-1,60,,+7, 1.0") == [36, 48, 60, 7]          # entries that are no u8 are dropped silently
    a = tool_ia.parse_args([])
    assert (a.command, a.threshold, a.render, a.duration, a.notes) == ("audit", 0.07, False, 3.0, None)
    a = tool_ia.parse_args(["--threshold", "0.002", "--render", "--duration", "0.8", "--notes", "40,zz,41"])
    assert (a.threshold, a.render, a.duration, a.notes) == (0.002, True, 0.8, "40,zz,41")
    assert tool_ia.parse_note_range("40..43") == [40, 41, 42, 43] and tool_ia.parse_note_range("40,x,42") == [40, 42]
    a = tool_ov.parse_args([])
    assert (a.notes, a.velocities) == ("36,48,60,72,84", "64,127")
    seen = {}
    monkeypatch.setattr(ia, "report", lambda *args: seen.setdefault("ia", args) and "" or "")
    monkeypatch.setattr(ov, "report", lambda *args, **kw: seen.setdefault("ov", (args, kw)) and "" or "")
    with redirect_stdout(io.StringIO()):
        tool_ia.main(["--notes", "40,zz,41", "--render"])
        tool_ov.main(["--notes", "36,bad", "--velocities", "300,64"])
    assert seen["ia"] == (0.07, True, 3.0, [40, 41], 0) and seen["ov"] == (([36], [64]), {"device": 0})
    monkeypatch.setattr(ia, "audit", lambda notes, vels, dur, dev: seen.setdefault("grid", (notes, vels, dur)) and [] or [])
    buf = io.StringIO()
    with redirect_stdout(buf):
        tool_ia.main(["grid", "--notes", "60..61", "--velocities", "20,127"])
    assert seen["grid"] == ([60, 61], [20, 127], 3.0) and buf.getvalue() == "note,velocity,h_db,m_db,ratio_db,verdict\n"


# ---- the conditions of the GPU tests' jobs, on the CPU -----------------------------------------------------------------------------
def test_gpu_jobs_meet_their_conditions():
    """Every intermod-audit job of the GPU tests: the derived bar of ratio_db is below 0.05 dB (what the command prints), ratio_db lies
    further from 20 / 30 / 40 than its bar, and no printed figure lies within its bar of a rounding boundary -- for the restatement and for
    its sibling whose voice library calls are off by one ulp, whose own figures must lie within the bars."""
    for note, vel, dur in ref.intermod_jobs():
        base = None
        for perturbed in (False, True):
            au = ref.row(note, vel, dur, perturbed)
            a = ref.intermod_audit(au, note)
            h, m, r, det = ref.intermod_bars(au, note)
            assert not a.too_short and (a.start, a.end) == (22050, min(88200, au.size))
            assert r < 0.05, (note, vel, dur, r)
            for edge in (20.0, 30.0, 40.0):
                assert abs(a.ratio_db - edge) > r, (note, vel, dur, a.ratio_db, r)
            assert ref.clear_of_rounding(a.h_db, h, 1) and ref.clear_of_rounding(a.m_db, m, 1) and ref.clear_of_rounding(a.ratio_db, r, 1)
            listed = [p for p in a.products if p.listed]
            if a.ratio_db <= 30.0:
                for p, bar in zip(listed, det):
                    assert ref.clear_of_rounding(p.ratio_db, bar, 1), (note, p)
            if base is None:
                base = a
            else:
                assert abs(a.ratio_db - base.ratio_db) <= r and abs(a.h_db - base.h_db) <= h and abs(a.m_db - base.m_db) <= m
    for dur in ref.OVERSHOOT_DURATIONS:
        for note, vel in ref.OVERSHOOT_JOBS:
            au = ref.row(note, vel, dur)
            o, bars = ref.overshoot(au), ref.overshoot_bars(au)
            for f in ("pk_dbfs", "rms1_dbfs", "rms2_dbfs", "overshoot_db", "bark_decay_db"):
                assert ref.clear_of_rounding(getattr(o, f), getattr(bars, f), 1), (note, vel, dur, f)
            assert math.isnan(o.bark_decay_db) == (dur < 1.0) and (o.rms2_dbfs == -120.0) == (dur < 1.0)
