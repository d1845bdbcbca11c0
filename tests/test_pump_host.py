"""The pump measurements without a device: the CPU restatement (tests/pump_ref.py) against what the reference's pump commands are known to
show, its own one-ulp sensitivity at every shape the GPU tests use, the row's field tuples, every refusal of ow_pump_measure, the
commands' text from fixed numbers, and the points each command builds."""
import ctypes as C
import math

import numpy as np
import pytest

import pump_ref as ref
from openwurli_amd import binding, pump
from openwurli_amd._rust_text import _e


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_restatement_shows_the_47k5_spike_at_48k_only():
    """main.rs:2543-2568: sigma jumps from ~3e-2 V to ~8e-1 V at that one point -- at 48 kHz; 88.2 kHz has no spike."""
    for sr, spike in ((48_000.0, True), (88_200.0, False)):
        rows, _ = ref.run_points(pump.static_points(sr, [30_000.0, 47_500.0, 70_000.0], 2048, 256), trace=False)
        print(sr, rows["raw_std"])
        assert rows["raw_std"][0] < 0.1 and rows["raw_std"][2] < 0.1
        assert (rows["raw_std"][1] > 0.1) == spike


def test_restatement_low_resistance_runs_on_the_fallback_alone():
    """At 1 k and 5 kOhm every sample exhausts the trapezoidal solve and takes the backward-Euler fallback, whose tables are never
    rebuilt: the output does not depend on the rate or on which of the two resistances it is."""
    pts = np.concatenate([pump.static_points(sr, [1_000.0, 5_000.0], 512, 1792) for sr in (44_100.0, 48_000.0, 88_200.0)])
    rows, traces = ref.run_points(pts)
    for t in traces[1:]:
        assert np.array_equal(t.view(np.uint64), traces[0].view(np.uint64))
    assert np.all(rows["be_fallbacks"] == 512 + 1792) and np.all(rows["nan_resets"] == 0)
    assert np.all(rows["nr_exhausted"] >= 512 + 1792)


def test_sensitivity_variant_stays_tame():
    """The restatement itself, with every non-zero entry of the rebuilt s, k, s_ni one ulp off (both polarities), at every GPU test
    shape: within 2.5 x the committed figures, the same fallback and reset counts.  Measured (x86-64, g++ -O2 -ffp-contract=off):
    static 1.098e-7 V (88.2 kHz, 100 kOhm), schedules 7.251e-7 V (log-cosine, two cycles)."""
    for name, pts, bar in (("static", ref.static_test_points(), ref.ULP_MOVE_STATIC), ("schedule", ref.schedule_test_points(), ref.ULP_MOVE_SCHEDULE)):
        r0, t0 = ref.run_points(pts)
        worst = 0.0
        for pol in (1, -1):
            r1, t1 = ref.run_points(pts, pol)
            for i in range(pts.size):
                worst = max(worst, float(np.max(np.abs(t0[i] - t1[i]))), abs(float(r0[i]["extra"]) - float(r1[i]["extra"])))
            assert np.array_equal(r0["be_fallbacks"], r1["be_fallbacks"]) and np.array_equal(r0["nan_resets"], r1["nan_resets"])
            assert np.array_equal(r0["nr_exhausted"], r1["nr_exhausted"])
        print(name, "largest movement %.3e V" % worst)
        assert worst <= 2.5 * bar
    assert ref.PUMP_REL <= 1e-5


def test_restatement_row_is_the_reduction_of_its_trace():
    p = pump.make_point(48_000.0, 30_000.0, 64, 33, in_amp=0.005, in_freq=1000.0, extra_sample=1, schedule=pump.RAMP, r_to=70_000.0)
    row, y = ref.run_point(p[0])
    assert row["sum"] == np.cumsum(y)[-1] and row["min"] == y.min() and row["max"] == y.max()
    assert row["max_step"] == np.max(np.abs(np.diff(np.concatenate([[row["extra"]], y]))))
    assert row["mean"] == row["sum"] / 33


# ---- the row's field tuples (the structs' layouts: tests/test_abi_layout.py) -------------------------------------------------------------------
def test_row_field_tuples_are_the_rows_fields():
    assert pump.ROW_FIELDS + pump.ROW_COUNTERS == pump.ROW_DTYPE.names == tuple(f for f, _ in binding.OwPumpRow._fields_)
    assert all(pump.ROW_DTYPE[f] == np.float64 for f in pump.ROW_FIELDS) and all(pump.ROW_DTYPE[f] == np.uint64 for f in pump.ROW_COUNTERS)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _call(hiplib_host, pts, cfg=None, rows=True, trace_stride=None):
    pts = np.ascontiguousarray(pts, dtype=pump.POINT_DTYPE)
    out = np.zeros(max(pts.size, 1), dtype=pump.ROW_DTYPE)
    cfg = binding.OwPumpCfg(0) if cfg is None else cfg
    tr = np.zeros(4) if trace_stride is not None else None
    rc = hiplib_host.ow_pump_measure(pts.ctypes.data_as(C.c_void_p) if pts.size else None, pts.size, C.byref(cfg) if cfg is not False else None,
                                     out.ctypes.data_as(C.c_void_p) if rows else None, tr.ctypes.data_as(C.c_void_p) if tr is not None else None,
                                     trace_stride or 0)
    return rc, binding.take_error(hiplib_host)


def test_refusals(hiplib_host):
    good = pump.make_point(48_000.0, 19_000.0, 4, 4)

    def bad(**kw):
        p = good.copy()
        for k, v in kw.items():
            p[k] = v
        return p
    cases = [(bad(sample_rate=0.0), "sample_rate is not a finite positive number"), (bad(sample_rate=math.nan), "sample_rate is not a finite positive number"),
             (bad(sample_rate=-48_000.0), "sample_rate is not a finite positive number"), (bad(r_settle=0.0), "r_settle is not a finite positive number"),
             (bad(r_settle=math.inf), "r_settle is not a finite positive number"), (bad(in_amp=math.nan), "in_amp is not finite"),
             (bad(in_freq=math.inf), "in_freq is not finite"), (bad(capture=0), "capture is 0"), (bad(extra_sample=2), "extra_sample is neither 0 nor 1"),
             (bad(schedule=4), "unknown schedule"), (bad(schedule=pump.STEP, r_to=0.0), "r_to is not a finite positive number"),
             (bad(schedule=pump.RAMP, r_to=math.nan), "r_to is not a finite positive number"),
             (bad(schedule=pump.RAMP, r_to=70_000.0, capture=1), "capture below 2 with OW_PUMP_RAMP"),
             (bad(schedule=pump.LOGCOS, ln_mid=math.nan), "ln_mid is not finite"), (bad(schedule=pump.LOGCOS, ln_amp=math.inf), "ln_amp is not finite"),
             (bad(schedule=pump.LOGCOS, sched_freq=math.nan), "sched_freq is not finite"), (bad(settle=1 << 40), "a run of 2^40 samples or more")]
    for p, text in cases:
        rc, err = _call(hiplib_host, p)
        assert rc < 0 and err.startswith("ow_pump_measure: point 0: ") and text in err, (text, err)
    two = np.concatenate([good, bad(capture=0)])
    rc, err = _call(hiplib_host, two)
    assert rc < 0 and "point 1: capture is 0" in err
    rc, err = _call(hiplib_host, good, trace_stride=3)
    assert rc < 0 and "trace_stride smaller than the largest capture (4)" in err
    rc, err = _call(hiplib_host, good, rows=False)
    assert rc < 0 and "null argument" in err
    rc, err = _call(hiplib_host, good, cfg=False)
    assert rc < 0 and "null argument" in err
    cfg = binding.OwPumpCfg(0)
    cfg.point_size += 8
    rc, err = _call(hiplib_host, good, cfg=cfg)
    assert rc < 0 and "ABI mismatch" in err
    cfg = binding.OwPumpCfg(0)
    cfg.struct_size -= 4
    rc, err = _call(hiplib_host, good, cfg=cfg)
    assert rc < 0 and "ABI mismatch" in err
    assert _call(hiplib_host, good[:0]) == (0, "")                 # nothing to do: no device needed


# ---- text ----------------------------------------------------------------------------------------------------------------------------
def test_rust_exponent_form():
    assert _e(1000.0, 6) == "1.000000e3" and _e(8.540762973, 9) == "8.540762973e0" and _e(2.5e-7, 2) == "2.50e-7"
    assert _e(12345.678, 6, True) == "+1.234568e4" and _e(-0.5, 6, True) == "-5.000000e-1" and _e(0.0, 2) == "0.00e0"
    assert _e(1e100, 3) == "1.000e100" and _e(math.nan, 6) == "NaN" and _e(math.inf, 6) == "inf" and _e(-math.inf, 6) == "-inf"
    assert _e(9.99999996, 6) == "1.000000e1"                     # the rounding carries into the exponent


def _rows(n, **cols):
    r = np.zeros(n, dtype=pump.ROW_DTYPE)
    for k, v in cols.items():
        r[k] = v
    return r


def test_sweep_text():
    rows = _rows(2, mean=[8.540762973, 6.5], std=[0.0, 0.031], min=[8.5, 6.25], max=[8.75, 6.75])
    assert pump.format_sweep_csv([1000.0, 1_000_000.0], rows) == ("r_ldr,pump_v,pump_std,pump_min,pump_max\n"
                                                                  "1.000000e3,8.540762973e0,0.000000e0,8.500000000e0,8.750000000e0\n"
                                                                  "1.000000e6,6.500000000e0,3.100000e-2,6.250000000e0,6.750000000e0\n")
    assert pump.format_sweep_report([1000.0, 1_000_000.0], rows, 1000.0, 1_000_000.0, 60000, 4096, 48000.0, 1.26, "/x/p.csv") == (
        "pump-sweep: 2 points from 1000 Ω to 1000000 Ω (log), settle=60000, avg=4096, SR=48000 Hz\n"
        "  [  0/2] R_ldr =       1000 Ω  pump = +8.540763e0 V  (σ = 0.00e0, span = 2.50e-1)\n"
        "  [  1/2] R_ldr =    1000000 Ω  pump = +6.500000e0 V  (σ = 3.10e-2, span = 5.00e-1)\n"
        "pump-sweep: done in 1.3s → /x/p.csv\n")
    many = _rows(70, mean=1.0)
    rep = pump.format_sweep_report([1000.0 + i for i in range(70)], many, 1000.0, 1069.0, 1, 2, 88200.0, 0.0, "c")
    assert [ln.split("]")[0] for ln in rep.splitlines()[1:-1]] == ["  [  0/70", "  [ 32/70", "  [ 64/70", "  [ 69/70"]


def test_trace_text_and_figures():
    y = np.array([8.0, 8.5, 7.5, 8.25, 8.0, 7.75, 8.125, 8.0])
    st = pump.trace_stats(y)
    cpu = ref.trace_stats(y)
    assert st["mean"] == cpu["mean"] and st["std"] == cpu["std"] and st["min"] == 7.5 and st["max"] == 8.5 and st["band_rms"] == cpu["band_rms"]
    assert pump.format_trace_csv(y[:2]) == "sample,pump_v\n0,8.000000000e0\n1,8.500000000e0\n"
    rep = pump.format_trace_report(1_000_000.0, 400000, 131072, {"mean": 6.5, "std": 0.25, "min": 6.0, "max": 7.0, "band_rms": [0.5, 0.25, 0.125, 0.0625, 0.03125]},
                                   12.34, "/x/t.csv")
    assert rep == ("pump-trace: R_ldr = 1000000 Ω, settle = 400000, samples = 131072 (2.731 s @ 48 kHz)\n"
                   "  mean   = +6.500000000e0 V\n"
                   "  std    = 2.500000e-1 V\n"
                   "  span   = 1.000000e0 V  (min +6.000000e0, max +7.000000e0)\n"
                   "  HPF RMS above:\n"
                   "        0.1 Hz : 5.000000e-1 V\n"
                   "        1.0 Hz : 2.500000e-1 V\n"
                   "       10.0 Hz : 1.250000e-1 V\n"
                   "      100.0 Hz : 6.250000e-2 V\n"
                   "     1000.0 Hz : 3.125000e-2 V\n"
                   "pump-trace: done in 12.3s → /x/t.csv\n")


def test_step_text_and_figures():
    rng = np.random.default_rng(7)
    for n in (20, 21, 23, 40):
        y = 8.0 + rng.standard_normal(n)
        a, b = pump.step_tail(y), ref.step_tail(y)
        assert all(a[k] == b[k] for k in b), n
    y = np.array([1.0, 2.0, 4.0])
    assert pump.format_step_csv(y, 1_000_000.0, 19_000.0, 88200.0, 6.5) == (
        "# pump-step  r_from=1.000000e6  r_to=1.900000e4  sr=88200  settled_at_from=6.500000000e0\n"
        "sample,pump_v,pump_avg2\n"
        "0,1.000000000e0,1.500000000e0\n1,2.000000000e0,1.500000000e0\n2,4.000000000e0,4.000000000e0\n")
    rep = pump.format_step_report(1_000_000.0, 19_000.0, 88200.0, 750000, 720000, 6.5, {"initial": 6.25, "tail_mean": 13.5, "tail_std": 0.00125, "total_swing": 7.25},
                                  3.96, "/x/s.csv")
    assert rep == ("pump-step: R_from=1000000 Ω → R_to=19000 Ω  SR=88200 Hz  settle=750000  samples=720000 (8.163 s)\n"
                   "  settled value at R_from: +6.500000 V\n"
                   "  initial (pair-mean after step):  +6.250000 V\n"
                   "  tail (last 10% pair-mean):       mean=+13.500000 V  std=1.250e-3 V\n"
                   "  total swing:                     +7.250000 V  (720000 samples = 8.163 s of capture)\n"
                   "pump-step: done in 4.0s → /x/s.csv\n")


def test_sinusoid_text_and_figures():
    rng = np.random.default_rng(9)
    for n in (2, 7, 8, 31):
        y = 8.0 + 0.2 * rng.standard_normal(n)
        assert pump.sinusoid_bifurcations(y) == ref.sinusoid_bifurcations(y), n
    assert pump.sinusoid_bifurcations([0.0, 0.0, 1.0, 1.0, 1.0]) == 1
    y = [1.0, 2.0, 4.0]
    assert pump.format_sinusoid_csv([1_000_000.0, 500_000.0, 19_000.0], y, 19_000.0, 1_000_000.0, 5.6, 88200.0, 10.0) == (
        "# pump-sinusoid  ldr_min=1.900000e4  ldr_max=1.000000e6  freq=5.600000  sr=88200  cycles=10\n"
        "sample,r_ldr,pump_v,pump_avg2\n"
        "0,1.000000e6,1.000000000e0,1.500000000e0\n1,5.000000e5,2.000000000e0,1.500000000e0\n2,1.900000e4,4.000000000e0,3.000000000e0\n")
    p = pump.sinusoid_points()[0]
    rep = pump.format_sinusoid_report(p, 19_000.0, 1_000_000.0, 5.6, 10.0, [1_000_000.0, 999_000.5, 998_000.0], [6.5, 6.75, 6.25], 0.5, 7.77, "/x/q.csv")
    assert rep == ("pump-sinusoid: R = exp(11.834 + 1.982·cos(2π·5.6·t))  R ∈ [19000, 1000000] Ω\n"
                   "  SR=88200 Hz  cycles=10  samples=157500 (1.786 s)  settle=750000\n"
                   "  pump range: [6.250, 6.750] V (span 0.500 V)\n"
                   "  max sample-to-sample step:  dR=1000.50 Ω  dY=0.5000 V\n"
                   "  bifurcation events (pair-step > 0.1 V): 1  (expect 0 for slewed-R)\n"
                   "pump-sinusoid: done in 7.8s → /x/q.csv\n")


def test_spike_text():
    pts = pump.spike_points(1024, 64)
    rows = _rows(pts.size, pair_mean=8.5, pair_std=0.001, raw_std=0.0125)
    rows["raw_std"][3] = 0.84                                     # one width candidate
    rows["raw_std"][256 + 64 + 10] = 0.5                          # one hit at 48 kHz
    rows["raw_std"][512 + 2 * 64 + 1] = 0.25                      # one hit at amp 0.005
    slew = np.array([8.0, 8.25, 8.125])
    csvs, rep = pump.format_spike(pts, rows, slew, {"max_step": 1.1}, "/tmp/pump_spike")
    assert sorted(csvs) == ["audio", "samplerate", "slew", "width"]
    w = csvs["width"].splitlines()
    assert w[0] == "r_ldr,pump_v,pair_std,raw_std" and len(w) == 257 and w[1] == "4.650000e4,8.500000000e0,1.000000e-3,1.250000e-2"
    s = csvs["samplerate"].splitlines()
    assert s[0] == "sample_rate,r_ldr,pump_v,raw_std" and len(s) == 257 and s[1] == "44100,3.000000e4,8.500000000e0,1.250000e-2" and s[-1].startswith("96000,7.000000e4,")
    a = csvs["audio"].splitlines()
    assert a[0] == "input_amp,r_ldr,pump_v,raw_std" and len(a) == 321 and a[65].startswith("1.000000e-3,3.000000e4,") and a[-1].startswith("1.000000e-1,7.000000e4,")
    assert csvs["slew"] == "sample,r_ldr,pump_v\n0,3.000000e4,8.000000000e0\n1,5.000000e4,8.250000000e0\n2,7.000000e4,8.125000000e0\n"
    lines = rep.splitlines()
    r3 = float(pts["r_settle"][3])
    assert lines[:4] == ["[1/4] WIDTH: 256 points in [46500, 48500] Ω …", "  → 1 points with raw_std > 0.1 V (spike candidates):",
                         "      R=%.1f Ω  pump=+8.5000 V  raw_std=0.8400 V" % r3, "  CSV: /tmp/pump_spike_width.csv"]
    assert lines[4:6] == ["[2/4] SR=44100 Hz: 64 points in [30000, 70000] Ω …", "  → NO SPIKE at SR=44100"]
    assert lines[6] == "[2/4] SR=48000 Hz: 64 points in [30000, 70000] Ω …" and lines[7] == "  → spike: R=%.1f Ω  pump=+8.5000 V  raw_std=0.5000 V" % float(pts["r_settle"][330])
    assert "[3/4] AUDIO amp=0.0050 V @1 kHz: 64 points in [30000, 70000] Ω …" in lines and "  → NO SPIKE at amp=0.1000" in lines
    assert lines[-5:] == ["  CSV: /tmp/pump_spike_audio.csv", "[4/4] SLEW: R ramps 30000 → 70000 Ω over 1 s (3 samples) …",
                          "  → max sample-to-sample step during slew: 1.1000 V (compare to ~0.5 V static-R spike)", "  CSV: /tmp/pump_spike_slew.csv",
                          "pump-spike: all 4 tests complete."]


# ---- the points each command builds -----------------------------------------------------------------------------------------------------
def test_points_of_each_command():
    g = pump.log_grid(1_000.0, 1_000_000.0, 256)
    step = (math.log(1_000_000.0) - math.log(1_000.0)) / 255
    assert g == [math.exp(math.log(1_000.0) + step * i) for i in range(256)] and abs(g[0] - 1000.0) < 1e-9
    p = pump.sweep_points()
    assert p.size == 256 and np.all(p["sample_rate"] == 48_000.0) and np.all(p["settle"] == 60_000) and np.all(p["capture"] == 4_096)
    assert list(p["r_settle"]) == g and np.all(p["schedule"] == pump.STATIC) and np.all(p["extra_sample"] == 0) and np.all(p["in_amp"] == 0.0)
    with pytest.raises(ValueError):
        pump.sweep_points(points=1)
    with pytest.raises(ValueError):
        pump.sweep_points(ldr_min=5.0, ldr_max=5.0)

    t = pump.trace_points()
    assert t.size == 1 and t[0]["sample_rate"] == 48_000.0 and t[0]["r_settle"] == 1_000_000.0 and (t[0]["settle"], t[0]["capture"]) == (400_000, 131_072)

    s = pump.spike_points()
    assert s.size == 256 + 4 * 64 + 5 * 64
    assert list(s["r_settle"][:256]) == pump.log_grid(46_500.0, 48_500.0, 256) and np.all(s["settle"][:256] == 400_000) and np.all(s["capture"] == 8_192)
    grid = pump.log_grid(30_000.0, 70_000.0, 64)
    for k, sr in enumerate((44_100.0, 48_000.0, 88_200.0, 96_000.0)):
        q = s[256 + 64 * k:256 + 64 * (k + 1)]
        assert np.all(q["sample_rate"] == sr) and list(q["r_settle"]) == grid and np.all(q["settle"] == int(400_000.0 * sr / 48_000.0)) and np.all(q["in_amp"] == 0.0)
    assert int(400_000.0 * 44_100.0 / 48_000.0) == 367_500
    for k, amp in enumerate((0.0, 0.001, 0.005, 0.020, 0.100)):
        q = s[512 + 64 * k:512 + 64 * (k + 1)]
        assert np.all(q["sample_rate"] == 48_000.0) and np.all(q["in_amp"] == amp) and np.all(q["in_freq"] == 1000.0) and np.all(q["settle"] == 400_000)
    with pytest.raises(ValueError):
        pump.spike_points(avg=7)
    sl = pump.slew_point()[0]
    assert (sl["sample_rate"], sl["r_settle"], sl["r_to"], sl["capture"], sl["extra_sample"], sl["schedule"]) == (48_000.0, 30_000.0, 70_000.0, 48_000, 1, pump.RAMP)
    rs = pump.slew_resistances(48_000)
    assert rs[0] == 30_000.0 and rs[-1] == 70_000.0 and rs[1] == 30_000.0 + 40_000.0 * (1 / 47_999)

    st = pump.step_points()[0]
    assert (st["sample_rate"], st["r_settle"], st["r_to"], st["settle"], st["capture"], st["extra_sample"], st["schedule"]) == (
        88_200.0, 1_000_000.0, 19_000.0, 750_000, 720_000, 1, pump.STEP)

    assert pump.sinusoid_samples(10.0, 88_200.0, 5.6) == int(10.0 * 88_200.0 / 5.6) == 157_500
    assert pump.sinusoid_samples(1.0, 88_200.0, 88_200.0 / 2048.0) == 2048 and pump.sinusoid_samples(2.5, 48_000.0, 7.0) == 17_142
    si = pump.sinusoid_points()[0]
    assert si["ln_mid"] == 0.5 * (math.log(1_000_000.0) + math.log(19_000.0)) and si["ln_amp"] == 0.5 * (math.log(1_000_000.0) - math.log(19_000.0))
    assert (si["r_settle"], si["capture"], si["sched_freq"], si["extra_sample"], si["schedule"]) == (1_000_000.0, 157_500, 5.6, 1, pump.LOGCOS)
    rr = pump.sinusoid_resistances(si)
    assert len(rr) == 157_500 and abs(rr[0] - 1_000_000.0) < 1e-6 and rr[1] == math.exp(si["ln_mid"] + si["ln_amp"] * math.cos((2.0 * math.pi * 5.6) * (1 * (1.0 / 88_200.0))))
    # ... and the restatement builds the same schedule from the point's fields (its capture runs under these resistances)
    assert pump.temp_default("pump_sweep.csv").endswith("pump_sweep.csv")
