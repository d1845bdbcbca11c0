"""GPU parity of the preamp measurements (`preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep`,
tools/preamp-bench/src/main.rs:150-369) through ow_preamp_measure, against the CPU restatement tests/c/preamp_bench_ref.cpp.

Bars: gain_db and H1 <= 1e-4 dB (the calibration sweep's bar, 100x finer than the 0.01 dB the CSV prints).  H2..H5 sit near the DFT's
leakage level (~5e-7 against an H1 of ~1e-2), where the chain's absolute sample error matters: each is held to 1e-4 dB or to 2x the
chain's absolute floor (a dft_magnitude bin moves by at most twice the largest sample error), whichever is larger -- the pattern of
test_gpu_calibrate._floor_tols.  Floors: ABS_FLOOR_BATCH for the legacy preamp, ABS_FLOOR_MELANGE_PREAMP for the melange one (the floors of
the batch chain these kernels restate).  Traces: oracle.parity_report (the 8d metric) with the same floors.
"""
import math

import numpy as np
import pytest

import preamp_bench_ref as ref

pytestmark = pytest.mark.gpu

DB_TOL = 1e-4


def _floor(oracle, kind):
    return oracle.ABS_FLOOR_MELANGE_PREAMP if kind else oracle.ABS_FLOOR_BATCH


def _check(rows, met, floor, what=""):
    """rows: ROW_DTYPE from the device; met: [n][9] from the restatement."""
    assert len(rows) == met.shape[0]
    rel = 10.0 ** (DB_TOL / 20.0) - 1.0
    for i, (r, c) in enumerate(zip(rows, met)):
        assert abs(r["gain_db"] - c[1]) <= DB_TOL, (what, i, r["gain_db"], c[1])
        assert abs(r["gain"] - c[0]) <= rel * c[0], (what, i, r["gain"], c[0])
        h = r["h"]
        assert abs(20.0 * np.log10(h[0] / c[2])) <= DB_TOL, (what, i, h[0], c[2])
        for k in range(1, 5):
            bar = max(rel * c[2 + k], 2.0 * floor)
            assert abs(h[k] - c[2 + k]) <= bar, (what, i, k + 1, h[k], c[2 + k], bar)
        # the host's finish is cmd_harmonics' own expression on the device's bins
        h = [float(x) for x in h]
        thd = (math.sqrt(h[1] * h[1] + h[2] * h[2] + h[3] * h[3] + h[4] * h[4]) / h[0]) * 100.0
        assert r["thd_pct"] == thd
        assert r["h2_h3_db"] == (20.0 * math.log10(h[1] / h[2]) if h[2] > 1e-15 else math.inf)
        tol_thd = 100.0 * sum(max(rel * c[2 + k], 2.0 * floor) for k in range(1, 5)) / c[2] + 2 * rel * c[7]
        assert abs(r["thd_pct"] - c[7]) <= tol_thd, (what, i, r["thd_pct"], c[7], tol_thd)


def _ref_points(kind, pts):
    return ref.points(kind, [tuple(q) for q in pts.tolist()])


def _near_boundary(x, decimals, eps=1e-4):
    s = abs(x) * 10 ** decimals
    return abs((s - int(s)) - 0.5) <= eps * 10 ** decimals


@pytest.mark.parametrize("kind", [0, 1])
def test_default_commands_against_the_restatement(oracle, kind):
    from openwurli_amd import preamp_bench as pb
    fl = _floor(oracle, kind)
    g = pb.measure_gain(preamp_kind=kind)
    _check([g], _ref_points(kind, pb.gain_points()), fl, "gain")
    h = pb.harmonics(preamp_kind=kind)
    _check([h], ref.harmonics(kind, 440.0, 0.005, 1e6)[0][None, :], fl, "harmonics")
    for name, pts, rows, csv in (("sweep", pb.sweep_points(), pb.sweep(preamp_kind=kind), pb.format_sweep_csv),
                                 ("tremolo-sweep", pb.tremolo_sweep_points(), pb.tremolo_sweep(preamp_kind=kind), pb.format_tremolo_sweep_csv)):
        met = _ref_points(kind, pts)          # == the sequential run bit for bit (test_preamp_bench_host.py)
        _check(rows, met, fl, name)
        # the CSV cell for cell, except within 1e-4 dB of a rounding boundary of the printed precision
        cr = rows.copy()
        cr["gain_db"] = met[:, 1]
        gl, cl = csv(rows).splitlines(), csv(cr).splitlines()
        assert gl[0] == cl[0]
        for a, b, v in zip(gl[1:], cl[1:], met[:, 1]):
            assert a == b or _near_boundary(v, 2), (name, a, b)


@pytest.mark.parametrize("kind", [0, 1])
def test_trace_rows_against_the_restatement(oracle, kind):
    from openwurli_amd import preamp_bench as pb
    # amplitudes up to 50 mV: driven harder the preamp leaves the domain where a trace is comparable at all (at 0.2 V / 19 kHz one ulp of
    # amplitude moves the restatement's own output by 6.9 V of a 9.1 V peak)
    pts = pb.make_points([30.0, 440.0, 1000.0, 7500.0, 19000.0], [0.001, 0.005, 0.05, 0.001, 0.02], [1e6, 19_000.0, 100_000.0, 50_000.0, 1e6],
                         [1e6, 1e6, 19_000.0, 300_000.0, 2500.0])
    rows, tr = pb.run_points(pts, kind, trace=True)
    for i, q in enumerate(pts.tolist()):
        met, ct = ref.point(kind, *q, trace=True)
        rep = oracle.parity_report(tr[i], ct, abs_floor=_floor(oracle, kind))
        assert rep["n_bad"] == 0, (i, rep)
        _check(rows[i:i + 1], met[None, :], _floor(oracle, kind), "trace point")
    assert rows.tobytes() == pb.run_points(pts, kind).tobytes()        # asking for a trace changes no number


def test_non_default_tremolo_sweep_follows_the_reset_chain(oracle):
    """Legacy, where the previous point's resistance matters: against the restatement's sequential run on ONE object (real reset()s)."""
    from openwurli_amd import preamp_bench as pb
    args = dict(ldr_min=8_000.0, ldr_max=600_000.0, steps=7, freq=3_000.0, amplitude=0.002)
    pts = pb.tremolo_sweep_points(**args)
    rows = pb.tremolo_sweep(**args)
    met, _ = ref.measure_seq(0, pts["freq_hz"], pts["amplitude"], pts["r_ldr"])
    _check(rows, met, oracle.ABS_FLOOR_BATCH, "tremolo-sweep")
    # ... and the chain is what makes it agree: the same points from new()'s 1 Mohm state differ by more than the bar
    flat = pb.run_points(pb.make_points(pts["freq_hz"], pts["amplitude"], pts["r_ldr"], 1e6))
    assert np.abs(flat["gain_db"][1:] - met[1:, 1]).max() > 10 * DB_TOL


def test_row_and_lane_pair_kernels_are_bit_identical(monkeypatch):
    from openwurli_amd import preamp_bench as pb
    pts = np.concatenate([pb.sweep_points(points=23), pb.tremolo_sweep_points(steps=14), pb.harmonics_points(amplitude=0.3)])
    out = {}
    for v in ("0", "1"):
        monkeypatch.setenv("OW_PBENCH_ROW", v)
        out[v] = pb.run_points(pts, trace=True)
    assert out["0"][0].tobytes() == out["1"][0].tobytes()
    assert np.array_equal(out["0"][1], out["1"][1])


@pytest.mark.parametrize("kind", [0, 1])
def test_point_independence(monkeypatch, kind):
    """A point's row and trace bits do not depend on its position, the grid size or the chunking."""
    from openwurli_amd import preamp_bench as pb
    rng = np.random.default_rng(1234)
    probe = pb.make_points([1234.5], [0.004], [60_000.0], [210_000.0])
    alone_r, alone_t = pb.run_points(probe, kind, trace=True)
    for n in (7, 100, 4096):
        other = pb.make_points(np.exp(rng.uniform(np.log(20), np.log(20000), n)), np.exp(rng.uniform(np.log(1e-4), np.log(0.1), n)),
                               np.exp(rng.uniform(np.log(1500), np.log(1e6), n)), np.exp(rng.uniform(np.log(1500), np.log(1e6), n)))
        for pos in sorted({0, n // 2, n - 1}):
            grid = other.copy()
            grid[pos] = probe[0]
            if n <= 100:
                r, t = pb.run_points(grid, kind, trace=True)
                assert np.array_equal(t[pos], alone_t[0]), (n, pos)
            else:
                r = pb.run_points(grid, kind)
            assert r[pos:pos + 1].tobytes() == alone_r.tobytes(), (n, pos)
    grid = other[:100].copy()
    grid[57] = probe[0]
    whole_r, whole_t = pb.run_points(grid, kind, trace=True)
    monkeypatch.setenv("OW_PBENCH_CHUNK", "9")                       # the documented chunk cap: 100 points in 12 launches
    ch_r, ch_t = pb.run_points(grid, kind, trace=True)
    assert ch_r.tobytes() == whole_r.tobytes() and np.array_equal(ch_t, whole_t)
    assert np.array_equal(ch_t[57], alone_t[0])


@pytest.mark.parametrize("kind", [0, 1])
def test_surface_64x64_against_the_restatement(oracle, kind):
    from openwurli_amd import preamp_bench as pb
    freqs = pb.log_spaced(25.0, 18_000.0, 64)
    rs = pb.log_spaced(19_000.0, 1e6, 64)
    g = pb.response_surface(freqs, rs, 0.001, kind)
    assert g.shape == (64, 64) and np.isfinite(g).all()
    pts = pb.surface_points(freqs, rs, 0.001)
    rng = np.random.default_rng(64)
    cells = sorted(set(rng.integers(0, 64 * 64, 24).tolist()) | {0, 1, 64 * 64 - 1})
    met = _ref_points(kind, pts[cells])
    for c, m in zip(cells, met):
        assert abs(g.flat[c] - m[1]) <= DB_TOL, (c, g.flat[c], m[1])
    rows = pb.run_points(pts[cells], kind)                           # a cell alone is the same cell of the surface
    assert np.array_equal(rows["gain_db"], g.flat[cells])


def test_refusals_through_the_c_abi_on_the_device(hiplib):
    import ctypes as C
    from openwurli_amd import binding, preamp_bench as pb
    pts = pb.gain_points()
    rows = np.zeros(1, dtype=pb.ROW_DTYPE)
    bad = binding.OwPreampMeasureCfg()
    bad.point_size = 24
    assert hiplib.ow_preamp_measure(pts.ctypes.data_as(C.c_void_p), 1, C.byref(bad), rows.ctypes.data_as(C.c_void_p), None, 0) < 0
    assert "ABI mismatch" in binding.take_error(hiplib)
    neg = pb.make_points([1000.0], [-0.001], [1e6], [1e6])
    with pytest.raises(binding.OwError, match="amplitude"):
        pb.run_points(neg)
    r = pb.run_points(pts)                                            # the library still works after a refusal
    assert np.isfinite(r["gain_db"]).all() and r["gain_db"][0] > 3.0
