"""`preamp-bench bark-audit` without a device: the binding's struct sizes and the restatement's field names, every refusal of ow_bark_audit with its message, the
returns that need no device, the report's text against a hand-written block, the CSV header, the tool's flags -- and, on the CPU
restatement (tests/c/bark_audit_ref.cpp), the conditions under which tests/test_gpu_bark_audit.py compares report text exactly.
"""
import ctypes as C
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import bark_audit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "ow_bark_audit"


# ---- the binding's sizes, the restatement's fields, the package's export (against the header: tests/test_abi_layout.py) ------------------------
def test_struct_layouts_header_binding_numpy():
    import openwurli_amd
    from openwurli_amd import binding as b, bark_audit as ba
    assert [32, 104, 8] == [C.sizeof(b.OwBarkCfg), C.sizeof(b.OwBarkRow), C.sizeof(b.OwNoteJob)] and ba.ROW_DTYPE.itemsize == 104
    assert tuple(ref.FIELDS) == tuple(b.BARK_ROW_FIELDS)
    assert openwurli_amd.bark_audit is ba and "bark_audit" in openwurli_amd.__all__


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _call(hiplib, jobs, cfg, rows, taps=None, stride=0, n_jobs=None):
    hiplib.ow_clear_error()
    rc = hiplib.ow_bark_audit(None if jobs is None else jobs.ctypes.data_as(C.c_void_p), len(jobs) if n_jobs is None else n_jobs, cfg,
                              None if rows is None else rows.ctypes.data_as(C.c_void_p), None if taps is None else taps.ctypes.data_as(C.c_void_p), stride)
    msg = hiplib.ow_last_error().decode()
    hiplib.ow_clear_error()
    return rc, msg


def test_refusals(hiplib):
    from openwurli_amd import binding as b, bark_audit as ba
    from openwurli_amd.intermod_audit import note_jobs
    Cfg = b.OwBarkCfg
    jobs, rows = note_jobs([60], [100]), np.zeros(1, dtype=ba.ROW_DTYPE)
    for field, bad in (("struct_size", 24), ("job_size", 4)):
        cfg = Cfg()
        setattr(cfg, field, bad)
        assert _call(hiplib, jobs, C.byref(cfg), rows) == \
               (-1, f"{FN}: ABI mismatch: ow_bark_cfg.struct_size / job_size do not match this library's openwurli_hip.h (OW_ABI_VERSION 8)")
    assert _call(hiplib, jobs, None, rows) == (-1, f"{FN}: null argument")
    assert _call(hiplib, None, C.byref(Cfg()), rows, n_jobs=1) == (-1, f"{FN}: null argument")
    assert _call(hiplib, jobs, C.byref(Cfg()), None) == (-1, f"{FN}: null argument")
    for note in (32, 97):
        assert _call(hiplib, note_jobs([60, note], [100]), C.byref(Cfg()), np.zeros(2, dtype=ba.ROW_DTYPE)) == \
               (-1, f"{FN}: job 1: note {note} outside 33..96 (the tables' range)")
    assert _call(hiplib, note_jobs([60], [128]), C.byref(Cfg()), rows) == (-1, f"{FN}: job 0: velocity 128 above 127 (a MIDI velocity byte)")
    for kind in (-1, 2):
        assert _call(hiplib, jobs, C.byref(Cfg(preamp_kind=kind)), rows) == (-1, f"{FN}: unknown preamp_kind")
    for dur in (-0.5, float("inf"), float("nan")):
        assert _call(hiplib, jobs, C.byref(Cfg(dur, 0.0)), rows) == (-1, f"{FN}: duration_s is not a finite non-negative number")
    for start in (-0.25, float("inf"), float("nan")):
        assert _call(hiplib, jobs, C.byref(Cfg(0.5, start)), rows) == (-1, f"{FN}: measure_start_s is not a finite non-negative number")
    assert _call(hiplib, jobs, C.byref(Cfg(2.0 ** 31 / 44100.0 + 1.0, 0.0)), rows) == (-1, f"{FN}: duration_s must give fewer than 2^31 samples")
    for start, m0 in ((0.5, 22050), (0.75, 33075)):                  # the reference's slice would panic
        assert _call(hiplib, jobs, C.byref(Cfg(0.5, start)), rows) == \
               (-1, f"{FN}: measure_start_s leaves no sample to measure: the window starts at {m0} of 22050 samples")
    assert _call(hiplib, jobs, C.byref(Cfg(0.01, 0.0)), rows, np.zeros(3 * 440), 440) == (-1, f"{FN}: tap_stride smaller than the 441 samples of a job")
    # the refusals come before any job is looked at, and before n_jobs == 0 returns
    assert _call(hiplib, None, C.byref(Cfg(0.5, 0.5)), None, n_jobs=0)[0] == -1


def test_returns_that_need_no_device(hiplib):
    from openwurli_amd import binding as b, bark_audit as ba
    # n_jobs == 0 returns the sample count and touches nothing, whatever the other pointers are
    assert _call(hiplib, None, C.byref(b.OwBarkCfg()), None, n_jobs=0) == (22050, "")
    assert _call(hiplib, None, C.byref(b.OwBarkCfg(0.05, 0.025)), None, n_jobs=0) == (2205, "")
    assert (ref.samples(0.5), ref.samples(0.25), ref.samples(0.05), ref.samples(0.025)) == (22050, 11025, 2205, 1102)
    # no samples: every figure is 0, the static columns are there
    rows = ba.bark_audit([33, 60], [40, 127], duration=0.0, measure_start=0.0)
    assert rows.size == 4 and list(rows["note"]) == [33, 33, 60, 60] and list(rows["velocity"]) == [40, 127, 40, 127]
    for f in ("reed_peak", "y_peak", "pu_peak", "pu_h1", "pu_h2", "pu_h2_h1", "pre_h1", "pre_h2", "pre_h2_h1"):
        assert np.all(rows[f] == 0.0), f
    assert np.all(rows["window_start"] == 0) and np.all(rows["window_end"] == 0)
    want = ref.run(60, 127, ref.SHORT_SIZE).row
    assert rows[2]["fundamental_hz"] == want.fundamental_hz
    assert abs(rows[2]["displacement_scale"] - want.displacement_scale) <= 1e-12 * want.displacement_scale


# ---- the command's text ----------------------------------------------------------------------------------------------------------------
def _row(note, vel, reed_peak, y_peak, pu, pk, pre):
    return {"note": note, "velocity": vel, "reed_peak": reed_peak, "y_peak": y_peak, "pu_h2_h1": pu, "pu_peak": pk, "pre_h2_h1": pre}


def test_report_text_by_hand():
    """main.rs:568-663 character for character: {:>6} {:>4}  {:>10.4} {:>10.4} {:>9.1}% {:>10.2} {:>9.1}%, a blank line behind each note."""
    from openwurli_amd import bark_audit as ba
    rows = [_row(36, 40, 0.374921, 0.0512349, 0.382858, 0.0211337, 0.398500), _row(36, 127, 0.96969, 0.13251, 1.220216, 0.8145725, 1.257315),
            _row(61, 40, 0.12029, 0.00005, 0.0, 0.0182904, 0.00049), _row(61, 127, 12.5, 1.0, 0.09996, 1.0, 0.10004)]
    want = "\n".join([
        "=== BARK AUDIT: H2/H1 at each signal chain stage ===",
        "",
        "  Note  Vel     Reed pk     y_peak   PU H2/H1  PU pk(mV)  Pre H2/H1",
        "-" * 76,
        "    C2   40      0.3749     0.0512      38.3%      21.13      39.9%",
        "    C2  127      0.9697     0.1325     122.0%     814.57     125.7%",
        "",
        "   C#4   40      0.1203     0.0001       0.0%      18.29       0.0%",
        "   C#4  127     12.5000     1.0000      10.0%    1000.00      10.0%",
        "",
        "Legend:",
        "  Reed pk   = peak reed displacement (model units)",
        "  y_peak    = physical displacement fraction (y = reed_pk * DS), DS = per-note from tables",
        "  PU H2/H1  = H2/H1 after time-varying RC pickup (coupled NL + HPF at 2312 Hz)",
        "  PU pk(mV) = peak signal after pickup (millivolts, feeds preamp)",
        "  Pre H2/H1 = H2/H1 after preamp (2x gain, no tremolo)",
        "",
        "SPICE targets: y=0.10 → H2/H1 ≈ 8.7%, pickup HPF boosts H2 ~1.9x relative to H1",
    ]) + "\n"
    assert ba.format_report(rows) == want == ba.format_report(rows, 2, 2)
    # one velocity per note: a blank line behind every row; the same note twice in a row is two blocks when the caller says so
    two = ba.format_report([rows[0], rows[1]], 1, 2).splitlines()
    assert two[4].startswith("    C2   40") and two[5] == "" and two[6].startswith("    C2  127") and two[7] == "" and two[8] == "Legend:"
    # no velocities: the command prints its blank line per note all the same
    none = ba.format_report([], 0, 3).splitlines()
    assert none[3] == "-" * 76 and none[4:7] == ["", "", ""] and none[7] == "Legend:"
    assert ba.format_report([]).splitlines()[4] == "Legend:"


def test_midi_note_name():
    from openwurli_amd import bark_audit as ba
    assert [ba.midi_note_name(n) for n in (33, 36, 48, 60, 61, 72, 84, 95, 96)] == ["A1", "C2", "C3", "C4", "C#4", "C5", "C6", "B6", "C7"]
    assert ba.midi_note_name(0) == "C-1" and ba.midi_note_name(127) == "G9"


def test_grid_csv_and_tool_flags(monkeypatch):
    from openwurli_amd import bark_audit as ba
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bark_audit as tool
    assert ba.GRID_HEADER == "note,velocity,model,reed_peak,y_peak,pu_h2_h1_pct,pu_peak_mv,pre_h2_h1_pct"
    rows = np.zeros(1, dtype=ba.ROW_DTYPE)
    rows["note"], rows["velocity"], rows["reed_peak"], rows["y_peak"], rows["pu_h2_h1"], rows["pu_peak"], rows["pre_h2_h1"] = 60, 80, 0.41, 0.05, 0.342967, 0.0820049, 0.344168
    assert ba.format_grid_csv([(0, rows), (1, rows)]) == ba.GRID_HEADER + "\n60,80,legacy,0.410000,0.050000,34.297,82.0049,34.417\n" \
                                                                          "60,80,melange,0.410000,0.050000,34.297,82.0049,34.417\n"
    seen = {}

    def fake_audit(notes, velocities, preamp_kind=0, duration=0.5, measure_start=0.25, device=0, taps=False):
        seen.setdefault("calls", []).append((list(notes), list(velocities), preamp_kind, duration, measure_start, device))
        return np.zeros(0, dtype=ba.ROW_DTYPE)
    monkeypatch.setattr(ba, "bark_audit", fake_audit)
    buf = io.StringIO()
    with redirect_stdout(buf):
        tool.main([])
    assert seen["calls"] == [([36, 48, 60, 72, 84], [40, 80, 100, 127], 0, 0.5, 0.25, 0)]       # main.rs:562-566
    assert buf.getvalue().startswith("=== BARK AUDIT: H2/H1 at each signal chain stage ===\n\n  Note  Vel")
    for argv, kind in ((["--model", "dk", "--preamp", "melange"], 1), (["--model", "dk-legacy", "--preamp", "melange"], 0), (["--preamp", "legacy"], 0)):
        seen["calls"] = []
        with redirect_stdout(io.StringIO()):
            tool.main(argv + ["--notes", "60, 61,x,300", "--velocities", "127", "--device", "2"])
        assert seen["calls"] == [([60, 61], [127], kind, 0.5, 0.25, 2)]
    seen["calls"] = []
    buf = io.StringIO()
    with redirect_stdout(buf):
        tool.main(["grid", "--notes", "60..61", "--velocities", "20,127"])
    assert [c[:3] for c in seen["calls"]] == [([60, 61], [20, 127], 0), ([60, 61], [20, 127], 1)] and buf.getvalue() == ba.GRID_HEADER + "\n"


# ---- the conditions of the GPU tests' jobs, on the CPU -----------------------------------------------------------------------------
def test_gpu_text_jobs_are_clear_of_rounding(oracle):
    """Every job whose report text the GPU test compares exactly (legacy preamp): no printed figure lies within its derived bar of a
    rounding boundary -- for the restatement and for its sibling whose voice library calls are off by one ulp, whose own figures must lie
    within the bars and print the same text."""
    from openwurli_amd import bark_audit as ba
    floors = ref.stage_floors(oracle, 0)
    for size, jobs in ref.TEXT_JOBS.items():
        runs = ref.run_many(jobs, size, 0)
        for (note, vel), r in zip(jobs, runs):
            assert (r.n, r.m0) == (ref.samples(size[0]), ref.samples(size[1]))
            b = ref.bars(r, floors)
            assert ref.text_is_clear(r, b), (size, note, vel, r.row, b)
            p = ref.run(note, vel, size, 0, perturbed=True)
            for f in ref.FIELDS:
                assert abs(getattr(p.row, f) - getattr(r.row, f)) <= getattr(b, f), (size, note, vel, f)
            assert ba.format_report([ref.record(note, vel, p)]) == ba.format_report([ref.record(note, vel, r)])


def test_restatement_stages(oracle):
    """The restatement against itself: the figures are those of its own taps, the stages are the ones the calibration sweep's restatement
    runs (same reed and pickup code: T1 / T2 of a point whose config gives the table's displacement scale)."""
    import calibrate_ref
    from openwurli_amd import calibrate as cal
    r = ref.run(60, 127, ref.DEFAULT_SIZE)
    w = slice(r.m0, r.n)
    assert r.row.reed_peak == np.max(np.abs(r.taps[0][w])) and r.row.pu_peak == np.max(np.abs(r.taps[1][w]))
    assert r.row.y_peak == r.row.reed_peak * r.row.displacement_scale
    assert r.row.pu_h1 == ref.dft_magnitude(r.taps[1][w], r.row.fundamental_hz) and r.row.pre_h2 == ref.dft_magnitude(r.taps[2][w], 2.0 * r.row.fundamental_hz)
    assert r.row.pre_h2_h1 == r.row.pre_h2 / r.row.pre_h1
    _, taps = calibrate_ref.run_point(60, 127, cal.CalibrationConfig(), 0.40, 1.0, taps=True)     # Default: the in-tree constants
    assert np.array_equal(taps[0], r.taps[0]) and np.array_equal(taps[1], r.taps[1])
