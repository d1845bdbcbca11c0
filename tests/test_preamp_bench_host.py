"""Preamp measurements (`preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep`), host side: no GPU needed.

The CPU restatement (tests/c/preamp_bench_ref.cpp) against the per-point model the device runs (r_reset), the reference's own gain
assertions and published figures on the restatement, the Python point builders and text formats against main.rs, and
ow_preamp_measure's input guards (which refuse before any device work).  The structs' layouts: tests/test_abi_layout.py.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import preamp_bench_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def trem_seq():
    """The default tremolo-sweep on ONE preamp object (the reference's reset() chain), both kinds: {kind: met [20][9]}."""
    from openwurli_amd import preamp_bench as pb
    p = pb.tremolo_sweep_points()
    return {k: ref.measure_seq(k, p["freq_hz"], p["amplitude"], p["r_ldr"])[0] for k in (0, 1)}


@pytest.mark.parametrize("kind", [0, 1])
def test_reset_chain_equals_independent_points_bit_for_bit(kind, trem_seq):
    """measure_gain_at's reset() chain on one object == independent points with r_reset = the previous point's resistance."""
    from openwurli_amd import preamp_bench as pb
    p = pb.tremolo_sweep_points()
    ind = np.array([ref.point(kind, *q)[0] for q in p.tolist()])
    assert ind.tobytes() == trem_seq[kind].tobytes()
    if kind == 0:      # the quirk is real for the legacy preamp: a DC solve at 1 Mohm instead moves the gain of later points
        no_chain = np.array([ref.point(kind, q[0], q[1], q[2], 1e6)[0] for q in p.tolist()])
        assert np.abs(no_chain[1:, 1] - trem_seq[0][1:, 1]).max() > 1e-3
        assert no_chain[0].tobytes() == trem_seq[0][0].tobytes()


def test_non_default_tremolo_sweep_chain_and_harmonics_start():
    """A descending sweep with a sub-1-kohm step (clamped) and a repeated R (within the 0.01 ohm hysteresis): the chain still matches;
    cmd_harmonics (new(), no reset()) equals a point with r_reset = 1 Mohm."""
    from openwurli_amd import preamp_bench as pb
    rr = [200_000.0, 500.0, 500.0, 1000.004, 50_000.0]
    chain = pb.reset_chain(rr)
    assert chain == [1e6, 200_000.0, 1000.0, 1000.0, 1000.0]
    seq, _ = ref.measure_seq(0, [700.0] * 5, [0.002] * 5, rr)
    ind = np.array([ref.point(0, 700.0, 0.002, r, q)[0] for r, q in zip(rr, chain)])
    assert ind.tobytes() == seq.tobytes()
    for k in (0, 1):
        assert ref.harmonics(k, 440.0, 0.005, 19_000.0)[0].tobytes() == ref.point(k, 440.0, 0.005, 19_000.0, 1e6)[0].tobytes()


def test_reference_gain_assertions_through_the_oversampled_path(trem_seq):
    """dk_preamp_legacy.rs:949-983 test_gain_no_tremolo / test_gain_increases_with_tremolo and dk_preamp/mod.rs:101-119
    test_melange_vs_legacy_gain_gate, on measure_gain_at's numbers (1 kHz, 1 mV)."""
    for k in (0, 1):
        g_1m, g_19k = trem_seq[k][-1, 0], trem_seq[k][0, 0]
        assert 3.0 < 20.0 * math.log10(g_1m) < 12.0
        assert g_19k > g_1m * 1.2
    for i in (0, -1):
        assert abs(trem_seq[1][i, 1] - trem_seq[0][i, 1]) < 2.0


def test_published_figures(trem_seq):
    """CHANGELOG.md:117-120, dk_preamp/mod.rs:3-8, on the default tremolo-sweep as the CSV prints it: the tremolo range is 6.10 dB for
    both kinds and the endpoints of the two kinds differ by 0.18 dB.  What does not reproduce is pinned as measured: the
    legacy range is 6.1056 dB (6.11 when the difference itself is rounded), the melange one 6.0980 dB, and the offset between the kinds
    runs from 0.1766 dB (1 Mohm end) to 0.1842 dB (19 kohm end), 0.19 dB in one printed cell.  The default `harmonics` THD is 0.0097 % for both kinds, not the
    published 0.79 %."""
    cells = {k: [float("%.2f" % g) for g in trem_seq[k][:, 1]] for k in (0, 1)}
    for k in (0, 1):
        assert "%.2f" % (cells[k][0] - cells[k][-1]) == "6.10"
    assert ["%.2f" % abs(cells[0][i] - cells[1][i]) for i in (0, -1)] == ["0.18", "0.18"]       # the endpoints as printed
    assert "%.2f" % max(abs(a - b) for a, b in zip(cells[0], cells[1])) == "0.19"                # not every cell: a finding
    assert ["%.4f" % (trem_seq[k][0, 1] - trem_seq[k][-1, 1]) for k in (0, 1)] == ["6.1056", "6.0980"]
    off = np.abs(trem_seq[0][:, 1] - trem_seq[1][:, 1])
    assert ("%.4f" % off.min(), "%.4f" % off.max(), "%.4f" % off[-1], "%.4f" % off[0]) == ("0.1766", "0.1842", "0.1766", "0.1842")
    h = {k: ref.harmonics(k, 440.0, 0.005, 1e6)[0] for k in (0, 1)}
    assert ["%.4f" % h[k][7] for k in (0, 1)] == ["0.0097", "0.0097"]     # THD identical to 4 decimals (measured, both kinds)


def test_log_spacing_and_point_builders():
    from openwurli_amd import preamp_bench as pb
    s = pb.sweep_points()
    assert s.size == 50 and s["freq_hz"][0] == math.exp(math.log(20.0)) == 19.999999999999996     # as the reference prints it: 20.0
    a, b = math.log(20.0), math.log(20000.0)
    assert list(s["freq_hz"]) == [math.exp(a + (i / 49) * (b - a)) for i in range(50)]
    assert (s["amplitude"] == 0.001).all() and (s["r_ldr"] == 1e6).all() and (s["r_reset"] == 1e6).all()
    s19 = pb.sweep_points(r_ldr=19_000.0, points=3)
    assert list(s19["r_reset"]) == [1e6, 19_000.0, 19_000.0]
    assert pb.sweep_points(points=1)["freq_hz"].tolist() == [19.999999999999996]          # (points - 1).max(1)
    assert pb.sweep_points(points=0).size == 0
    t = pb.tremolo_sweep_points()
    assert t.size == 20 and (t["freq_hz"] == 1000.0).all() and (t["amplitude"] == 0.001).all()
    assert list(t["r_reset"]) == [1e6] + list(t["r_ldr"][:-1])
    assert abs(t["r_ldr"][0] - 19_000.0) < 1e-8 and t["r_ldr"][-1] == math.exp(math.log(1e6))
    for f in (pb.gain_points(), pb.harmonics_points(r_ldr=19_000.0)):
        assert f["r_reset"].tolist() == [1e6]
    assert pb.harmonics_points()[0].tolist() == (440.0, 0.005, 1e6, 1e6)
    assert pb.gain_points()[0].tolist() == (1000.0, 0.001, 1e6, 1e6)
    sp = pb.surface_points([100.0, 1000.0], [19_000.0, 1e6])
    assert sp["r_ldr"].tolist() == [19_000.0, 19_000.0, 1e6, 1e6] and sp["r_reset"].tolist() == [1e6, 19_000.0, 1e6, 1e6]


def _rows(pts, met):
    from openwurli_amd import preamp_bench as pb
    r = np.zeros(len(pts), dtype=pb.ROW_DTYPE)
    r["freq_hz"], r["amplitude"], r["r_ldr"] = pts["freq_hz"], pts["amplitude"], pts["r_ldr"]
    r["gain"], r["gain_db"], r["h"], r["thd_pct"], r["h2_h3_db"] = met[:, 0], met[:, 1], met[:, 2:7], met[:, 7], met[:, 8]
    return r


def test_text_formats():
    from openwurli_amd import preamp_bench as pb
    p = pb.make_points([19.96, 1000.0], [0.001] * 2, [19_000.4, 1e6], [1e6, 1e6])
    met = np.array([[2.0, 6.0205999, 0, 0, 0, 0, 0, 0, 0], [4.0, -0.005, 0, 0, 0, 0, 0, 0, 0]], dtype=float)
    r = _rows(p, met)
    assert pb.format_sweep_csv(r) == "freq_hz,gain_db\n20.0,6.02\n1000.0,-0.01\n"
    assert pb.format_tremolo_sweep_csv(r) == "ldr_ohm,gain_db\n19000,6.02\n1000000,-0.01\n"
    t = pb.format_sweep(r, 1e6).splitlines()
    assert t[:3] == ["Frequency response sweep (LDR = 1000000 Ω)", " Freq (Hz)   Gain (dB)", "----------  ----------"]
    assert t[3] == "      20.0        6.02"
    tt = pb.format_tremolo_sweep(r).splitlines()
    assert tt[1] == "     LDR (Ω)   Gain (dB)" and tt[3] == "       19000        6.02" and tt[-1] == "  Range:                      6.1 dB"
    g = pb.format_gain(r[0]).splitlines()
    assert g == ["Preamp gain measurement", "  Frequency:   20 Hz", "  Amplitude:   0.001000 V", "  LDR path:    19000 Ω",
                 "  Gain:        2.000x (6.02 dB)", "  SPICE target: 12.1 dB", "  Delta:       -6.08 dB"]
    h = np.zeros(1, dtype=pb.ROW_DTYPE)[0]
    h["freq_hz"], h["amplitude"], h["r_ldr"], h["h"], h["thd_pct"], h["h2_h3_db"] = 440.0, 0.005, 1e6, [0.01, 1e-4, 0.0, 1e-5, 1e-6], 1.005, math.inf
    hl = pb.format_harmonics(h).splitlines()
    assert hl[5] == "  H1 (fund):   0.010000" and hl[6] == "  H2:          0.000100  (-40.0 dB rel)"
    assert hl[7] == "  H3:          0.000000  (-inf dB rel)" and hl[-2] == "  THD:         1.0050%"
    assert hl[-1] == "  H2/H3:       inf dB  (target: H2 > H3, i.e. > 0 dB)"
    assert pb.format_surface_csv([20.0], [19_000.0], np.array([[6.0]])) == "ldr_ohm,freq_hz,gain_db\n19000,20.0,6.00\n"
    assert pb.target_db(500_000.0) == 12.1 and pb.target_db(500_000.5) == 6.0


def test_window_constants_match_the_header():
    from openwurli_amd import binding
    hdr = open(os.path.join(ROOT, "include", "openwurli_hip.h")).read()
    for name, v in (("OW_PBENCH_SAMPLES", binding.PBENCH_SAMPLES), ("OW_PBENCH_GAIN_LO", binding.PBENCH_GAIN_LO),
                    ("OW_PBENCH_HARM_LO", binding.PBENCH_HARM_LO)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == v
    assert (binding.PBENCH_SAMPLES, binding.PBENCH_GAIN_LO, binding.PBENCH_HARM_LO) == (int(44100.0 * 0.5), int(44100.0 * 0.3), 22050 * 3 // 4)


def _call(lib, points, cfg, trace=None, stride=0):
    from openwurli_amd import preamp_bench
    rows = np.zeros(max(points.size, 1), dtype=preamp_bench.ROW_DTYPE)
    return lib.ow_preamp_measure(points.ctypes.data_as(C.c_void_p), points.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p), trace, stride)


def test_struct_size_guards_refuse_before_device_work(hiplib):
    from openwurli_amd import binding, preamp_bench
    pts = preamp_bench.gain_points()
    for field, bad in (("struct_size", C.sizeof(binding.OwPreampMeasureCfg) - 4), ("point_size", C.sizeof(binding.OwPreampPoint) + 8)):
        cfg = binding.OwPreampMeasureCfg()
        setattr(cfg, field, bad)
        hiplib.ow_clear_error()
        assert _call(hiplib, pts, cfg) < 0
        assert "ABI mismatch" in binding.take_error(hiplib)


@pytest.mark.parametrize("field", ["freq_hz", "amplitude", "r_ldr", "r_reset"])
@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan, math.inf])
def test_non_positive_or_non_finite_points_are_refused(hiplib, field, bad):
    from openwurli_amd import binding, preamp_bench
    pts = np.concatenate([preamp_bench.gain_points(), preamp_bench.gain_points()])
    pts[field][1] = bad
    hiplib.ow_clear_error()
    assert _call(hiplib, pts, binding.OwPreampMeasureCfg()) < 0
    msg = binding.take_error(hiplib)
    assert "point 1" in msg and field in msg and "finite positive" in msg


def test_short_trace_stride_and_unknown_kind_are_refused(hiplib):
    from openwurli_amd import binding, preamp_bench
    pts = preamp_bench.gain_points()
    buf = np.zeros(100)
    assert _call(hiplib, pts, binding.OwPreampMeasureCfg(), buf.ctypes.data_as(C.c_void_p), 100) < 0
    assert "trace_stride" in binding.take_error(hiplib)
    assert _call(hiplib, pts, binding.OwPreampMeasureCfg(preamp_kind=7)) < 0
    assert "preamp_kind" in binding.take_error(hiplib)


def test_empty_grid_is_a_no_op(hiplib):
    from openwurli_amd import binding, preamp_bench
    assert _call(hiplib, np.zeros(0, dtype=preamp_bench.POINT_DTYPE), binding.OwPreampMeasureCfg()) == 0
