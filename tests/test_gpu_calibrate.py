"""GPU parity of the calibration sweep (`preamp-bench calibrate` / `sensitivity`, tools/preamp-bench/src/main.rs:1069-1395) through
ow_calibrate, against the CPU restatement tests/c/calibrate_ref.cpp (run_calibrate in the reference's statement order over the oracle).

Bars (100x finer than the 0.01 dB the CSV prints): ds_actual / proxy_db / trim_db <= 1e-12 relative (host scalars), y_peak <= 1e-10
relative (the voice parity bar), every dB column <= 1e-4 dB on every grid (measured worst: 5.1e-5 dB, a tanh_compression_db at velocity
40), the -120 floors exactly.  Only the velocity-1 edge points -- T4 peaks near 1e-6, where the batch chain's absolute floor is a few
percent of the signal -- get the T4 / T5 allowance of that floor (ABS_FLOOR_BATCH, the floor of the job chain both columns come out of).
Tap rows: oracle.parity_report with the existing floors of the chain they pass through.
"""
import numpy as np
import pytest

import calibrate_ref

pytestmark = pytest.mark.gpu

F = ("ds_at_c4", "ds_actual", "y_peak", "t2_peak_db", "t2_rms_db", "t2_h2_h1_db", "t3_peak_db", "t3_rms_db", "t4_peak_db", "t4_rms_db",
     "t4_h2_h1_db", "t5_peak_db", "t5_rms_db", "t5_h2_h1_db", "proxy_db", "trim_db", "proxy_error_db", "tanh_compression_db")
DB = [f for f in F if f.endswith("_db")]


def _grid(notes, vels, cfg):
    return [(n, v, cfg) for n in notes for v in vels]


def _floor_tols(c, floor):
    """dB allowance of the T4 / T5 columns of a near-silent point: what an absolute sample error <= `floor` amounts to at the level of
    the value (a peak or RMS moves by <= floor, a dft_magnitude bin by <= 2 floor; H1 of the tone taken as half its peak)."""
    def lvl(db, err):
        return 20.0 * np.log10(1.0 + err / 10.0 ** (db / 20.0))
    t = {}
    for s in ("t4", "t5"):
        t[s + "_peak_db"] = lvl(c[s + "_peak_db"], floor)
        t[s + "_rms_db"] = lvl(c[s + "_rms_db"], floor)
        h1_db = c[s + "_peak_db"] - 20.0 * np.log10(2.0)
        t[s + "_h2_h1_db"] = lvl(h1_db, 2 * floor) + lvl(h1_db + c[s + "_h2_h1_db"], 2 * floor)
    t["tanh_compression_db"] = t["t4_peak_db"] + t["t5_peak_db"]
    return t


def _check_rows(rows, ref, points, db_tol=1e-4, floor_for=None):
    """floor_for: None, or (predicate on the point, absolute floor) -- the points the predicate selects get _floor_tols on their T4 / T5
    columns where that is larger than db_tol."""
    assert len(rows) == len(points) == ref.shape[0]
    for r, c, p in zip(rows, ref, points):
        n, v = p[0], p[1]
        assert (r.midi, r.velocity) == (n, v)
        g = {f: getattr(r, f) for f in F}
        c = dict(zip(F, c))
        assert g["ds_at_c4"] == c["ds_at_c4"]
        for f in ("ds_actual", "proxy_db", "trim_db"):
            assert abs(g[f] - c[f]) <= 1e-12 * abs(c[f]), (n, v, f, g[f], c[f])
        assert abs(g["y_peak"] - c["y_peak"]) <= 1e-10 * abs(c["y_peak"]), (n, v, g["y_peak"], c["y_peak"])
        tol = {}
        if floor_for is not None and floor_for[0](p):
            tol = _floor_tols(c, floor_for[1])
        for f in DB:
            if c[f] == -120.0 or g[f] == -120.0:
                assert g[f] == c[f], (n, v, f, g[f], c[f])      # the floor branches agree exactly
            else:
                bar = max(db_tol, tol.get(f, 0.0))
                assert abs(g[f] - c[f]) <= bar, (n, v, f, g[f], c[f], bar)


def _check_taps(oracle, gt, ct, floors):
    for k in range(5):
        rep = oracle.parity_report(gt[k], ct[k], abs_floor=floors[k])
        assert rep["n_bad"] == 0, (k + 1, rep)


def test_calibrate_default_grid_legacy_and_taps(oracle):
    from openwurli_amd import calibrate as cal
    cfg = cal.calibrate_config()
    pts = _grid(cal.CALIBRATE_NOTES, cal.CALIBRATE_VELOCITIES, cfg)
    tap_idx = (0, 7, 17, 20, 31, 38)
    ref, ref_taps = calibrate_ref.run_points(pts, 0.40, 1.0, taps_for=tap_idx)
    rows, taps = cal.calibrate(taps=True)
    _check_rows(rows, ref, pts)
    for i in tap_idx:
        _check_taps(oracle, taps[i], ref_taps[i], [oracle.ABS_FLOOR_BATCH] * 5)
    assert rows == cal.calibrate()                      # asking for taps changes no number


def test_sensitivity_grid_is_one_call_and_lane_independent():
    from openwurli_amd import calibrate as cal
    rows = cal.sensitivity()
    assert len(rows) == 192
    per_ds = []
    for ds in cal.SENSITIVITY_DS:
        per_ds += cal.run_calibrate(cal.SENSITIVITY_NOTES, cal.SENSITIVITY_VELOCITIES, cal.sensitivity_config(ds), 0.40, 1.0)
    assert rows == per_ds                               # bit for bit: a lane's result does not depend on its neighbours
    assert [r.ds_at_c4 for r in rows] == list(np.repeat(cal.SENSITIVITY_DS, 24))


@pytest.mark.parametrize("mode", ["track", "zero-trim", "freeze"])
def test_sensitivity_scale_modes_against_the_restatement(mode):
    from openwurli_amd import calibrate as cal
    dsv = (0.55, 0.80)
    rows = cal.sensitivity(ds_values=dsv, scale_mode=mode)
    pts = [p for ds in dsv for p in _grid(cal.SENSITIVITY_NOTES, cal.SENSITIVITY_VELOCITIES, cal.sensitivity_config(ds, mode))]
    ref, _ = calibrate_ref.run_points(pts, 0.40, 1.0)
    ref[:, 0] = np.repeat(dsv, 24)                       # the stamped column
    _check_rows(rows, ref, pts)


def test_calibrate_melange_preamp(oracle):
    from openwurli_amd import calibrate as cal
    cfg = cal.calibrate_config(zero_trim=True)           # the configuration register_trim_db was measured with (tables.rs:465-470)
    pts = _grid(cal.CALIBRATE_NOTES, cal.CALIBRATE_VELOCITIES, cfg)
    tap_idx = (1, 12, 26, 38)
    ref, ref_taps = calibrate_ref.run_points(pts, 0.40, 1.0, preamp_kind=1, taps_for=tap_idx)
    rows, taps = cal.calibrate(zero_trim=True, preamp_kind=cal.PREAMP_MELANGE12, taps=True)
    _check_rows(rows, ref, pts)
    floors = [oracle.ABS_FLOOR_BATCH] * 3 + [oracle.ABS_FLOOR_MELANGE_PREAMP, oracle.ABS_FLOOR_MELANGE_OUTPUT]
    for i in tap_idx:
        _check_taps(oracle, taps[i], ref_taps[i], floors)


def test_calibrate_melange_power_amp(oracle):
    from openwurli_amd import calibrate as cal
    cfg = cal.calibrate_config()
    pts = _grid((36, 48, 60, 84), (40, 127), cfg)
    ref, ref_taps = calibrate_ref.run_points(pts, 0.40, 1.0, power_amp_kind=1, taps_for=range(len(pts)))
    rows, taps = cal.run_calibrate((36, 48, 60, 84), (40, 127), cfg, 0.40, 1.0, power_amp_kind=cal.POWER_AMP_MELANGE, taps=True)
    _check_rows(rows, ref, pts)
    for i in range(len(pts)):
        _check_taps(oracle, taps[i], ref_taps[i], [oracle.ABS_FLOOR_BATCH] * 4 + [oracle.ABS_FLOOR_MELANGE_OUTPUT])


def test_edge_points(oracle):
    from openwurli_amd import calibrate as cal
    cfg = cal.calibrate_config()
    notes, vels = (33, 96), (0, 1, 127)
    pts = _grid(notes, vels, cfg)
    ref, _ = calibrate_ref.run_points(pts, 0.40, 1.0)
    rows = cal.run_calibrate(notes, vels, cfg, 0.40, 1.0)
    _check_rows(rows, ref, pts, floor_for=(lambda p: p[1] == 1, oracle.ABS_FLOOR_BATCH))
    silent = [r for r in rows if r.velocity == 0]
    assert silent and all(getattr(r, f) == -120.0 for r in silent for f in DB if f[:2] in ("t2", "t3", "t4", "t5"))   # to_dbfs / rms_db / h2_h1 floors


def test_chunked_grid_equals_unchunked(monkeypatch):
    from openwurli_amd import calibrate as cal
    cfgs = [cal.calibrate_config(), cal.CalibrationConfig(ds_at_c4=0.6, zero_trim=True)]
    nn, vv, cc = [], [], []
    for c in cfgs:
        for n in (33, 41, 58, 60, 73, 90, 96):
            for v in (0, 64, 100):
                nn.append(n); vv.append(v); cc.append(c)
    pts = cal.make_points(nn, vv, cc)
    whole, wt = cal.run_points(pts, 0.40, 1.0, taps=True)
    monkeypatch.setenv("OW_CALIB_CHUNK", "5")               # the documented chunk cap: 42 points in 9 chunks
    chunked, ct = cal.run_points(pts, 0.40, 1.0, taps=True)
    assert whole.tobytes() == chunked.tobytes()
    assert np.array_equal(wt, ct)
