"""Calibration sweep (`preamp-bench calibrate` / `sensitivity`), host side: no GPU needed.

The CPU restatement's table functions against the oracle, the Python configs and CSV writer against the reference's text, and
ow_calibrate's input guards (which refuse before any device work).  The structs' layouts: tests/test_abi_layout.py.
"""
import ctypes as C

import numpy as np
import pytest

import calibrate_ref


def test_restated_table_functions_equal_the_oracle_bit_for_bit(oracle):
    from openwurli_amd.calibrate import CalibrationConfig
    L = calibrate_ref.lib()
    cfg = calibrate_ref.cfg6(CalibrationConfig())
    ol = oracle.lib()
    for m in range(33, 97):
        assert L.ocal_pickup_displacement_scale(m, cfg, 0) == ol.owo_pickup_displacement_scale(m)
        for v in range(128):
            assert L.ocal_output_scale(m, v / 127.0, cfg, 0) == ol.owo_output_scale(m, C.c_double(v / 127.0)), (m, v)


def test_calibration_config_defaults_match_tables_rs():
    from openwurli_amd.calibrate import CalibrationConfig, calibrate_config
    c = CalibrationConfig()                                    # tables.rs:249-277
    assert (c.ds_at_c4, c.ds_exponent, c.ds_clamp, c.target_db, c.voicing_slope, c.zero_trim) == (0.85, 0.75, (0.02, 0.95), -35.0, -0.04, False)
    k = calibrate_config()                                     # main.rs:1072-1091: the command's own defaults
    assert (k.ds_at_c4, k.ds_clamp, k.zero_trim) == (0.75, (0.02, 0.82), False)
    assert (k.ds_exponent, k.target_db, k.voicing_slope) == (0.75, -35.0, -0.04)
    assert calibrate_config(0.8, 0.9, True) == CalibrationConfig(ds_at_c4=0.8, ds_clamp=(0.02, 0.9), zero_trim=True)


def test_sensitivity_scale_modes_and_stamped_column(monkeypatch):
    from openwurli_amd import calibrate as cal
    seen = {}

    def fake_run_points(points, volume, speaker_char, preamp_kind=0, power_amp_kind=0, device=0, taps=False):
        seen["points"] = points.copy()
        seen["args"] = (volume, speaker_char, preamp_kind, power_amp_kind)
        r = np.zeros(points.size, dtype=cal.ROW_DTYPE)
        r["midi"] = points["note"]; r["velocity"] = points["velocity"]; r["ds_at_c4"] = points["ds_at_c4"]
        return r

    monkeypatch.setattr(cal, "run_points", fake_run_points)
    rows = cal.sensitivity()
    p = seen["points"]
    assert len(rows) == p.size == 192 and seen["args"] == (0.40, 1.0, 0, 0)
    ds = np.repeat(cal.SENSITIVITY_DS, 24)
    assert np.array_equal(p["ds_at_c4"], ds) and not p["zero_trim"].any()
    assert np.array_equal(p["note"], np.tile(np.repeat(cal.SENSITIVITY_NOTES, 3), 8))
    assert np.array_equal(p["velocity"], np.tile(cal.SENSITIVITY_VELOCITIES, 64))
    assert (p["ds_clamp_lo"] == 0.02).all() and (p["ds_clamp_hi"] == 0.95).all()           # CalibrationConfig::default()'s clamp
    assert [r.ds_at_c4 for r in rows] == list(ds)
    for mode, zt in (("zero-trim", True), ("track", False)):
        rows = cal.sensitivity(ds_values=(0.6, 0.7), scale_mode=mode)
        assert np.array_equal(seen["points"]["ds_at_c4"], np.repeat([0.6, 0.7], 24)) and (seen["points"]["zero_trim"] == zt).all()
    cal.sensitivity(ds_values=(0.6,), zero_trim=True)                                         # --zero-trim is shorthand for the mode
    assert seen["points"]["zero_trim"].all()
    rows = cal.sensitivity(ds_values=(0.6, 0.7), scale_mode="freeze")
    assert (seen["points"]["ds_at_c4"] == 0.85).all() and not seen["points"]["zero_trim"].any()   # every sweep value renders at 0.85
    assert [r.ds_at_c4 for r in rows] == [0.6] * 24 + [0.7] * 24                                # ... and is stamped with its own value


def test_midi_note_names():
    from openwurli_amd.calibrate import midi_note_name
    names = [midi_note_name(m) for m in range(33, 97)]
    assert names[:4] == ["A1", "A#1", "B1", "C2"]
    assert midi_note_name(60) == "C4" and midi_note_name(61) == "C#4" and midi_note_name(69) == "A4" and midi_note_name(96) == "C7"
    octave = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
    assert names == [f"{octave[m % 12]}{m // 12 - 1}" for m in range(33, 97)]


def test_write_calibrate_csv_format(tmp_path):
    from openwurli_amd.calibrate import CalibrateRow, write_calibrate_csv
    rows = [CalibrateRow(60, 127, 0.75, 0.75, 0.7146231440535268, -7.143101704191829, -15.495925720177766, -2.6764108437227456,
                         -42.14310170419183, -50.49592572017774, -35.168237510277095, -43.79499874276853, -2.655949329066676,
                         -28.328598184913176, -37.400548073687716, -2.6589354322721395, -35.0, 0.0, -15.495925720177738, -6.839639325363919),
            CalibrateRow(33, 0, 0.5, 0.88, 0.0, -120.0, -120.0, -120.0, -120.0, -120.0, -120.0, -120.0, -120.0, -120.0, -120.0, -120.0,
                         -35.0, -1.3, -85.0, 0.0),
            CalibrateRow(96, 1, 0.85, 0.2412345, 1e-5, -0.0, -0.004, 12.345678, 0.005, 99.994999, -1e-9, 3.0, 0.0, 1.0, 2.0, 3.0,
                         -0.0, 3.6, 0.125, -0.001)]
    p = tmp_path / "c.csv"
    write_calibrate_csv(str(p), rows)
    assert p.read_bytes().decode() == (
        "midi,note_name,velocity,ds_at_c4,ds_actual,y_peak,t2_peak_db,t2_rms_db,t2_h2_h1_db,t3_peak_db,t3_rms_db,"
        "t4_peak_db,t4_rms_db,t4_h2_h1_db,t5_peak_db,t5_rms_db,t5_h2_h1_db,proxy_db,trim_db,proxy_error_db,tanh_compression_db\n"
        "60,C4,127,0.7500,0.7500,0.7146,-7.14,-15.50,-2.68,-42.14,-50.50,-35.17,-43.79,-2.66,-28.33,-37.40,-2.66,-35.00,0.00,-15.50,-6.84\n"
        "33,A1,0,0.5000,0.8800,0.0000,-120.00,-120.00,-120.00,-120.00,-120.00,-120.00,-120.00,-120.00,-120.00,-120.00,-120.00,"
        "-35.00,-1.30,-85.00,0.00\n"
        "96,C7,1,0.8500,0.2412,0.0000,-0.00,-0.00,12.35,0.01,99.99,-0.00,3.00,0.00,1.00,2.00,3.00,-0.00,3.60,0.12,-0.00\n")


def _call(lib, points, cfg, taps=None, stride=0):
    from openwurli_amd import calibrate
    rows = np.zeros(max(points.size, 1), dtype=calibrate.ROW_DTYPE)
    rc = lib.ow_calibrate(points.ctypes.data_as(C.c_void_p), points.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p), taps, stride)
    return rc


def test_struct_size_guards_refuse_before_device_work(hiplib):
    from openwurli_amd import binding, calibrate
    pts = calibrate.make_points([60], [100], [calibrate.CalibrationConfig()])
    for field, bad in (("struct_size", C.sizeof(binding.OwCalibrateCfg) - 8), ("point_size", C.sizeof(binding.OwCalibPoint) + 8)):
        cfg = binding.OwCalibrateCfg()
        setattr(cfg, field, bad)
        hiplib.ow_clear_error()
        assert _call(hiplib, pts, cfg) < 0
        assert "ABI mismatch" in binding.take_error(hiplib)


@pytest.mark.parametrize("note", [0, 32, 97, 127])
def test_notes_outside_the_tables_are_refused(hiplib, note):
    from openwurli_amd import binding, calibrate
    pts = calibrate.make_points([60, 60], [100, 100], [calibrate.CalibrationConfig()] * 2)
    pts["note"][1] = note                                        # past make_points' own check: the library guard
    hiplib.ow_clear_error()
    assert _call(hiplib, pts, binding.OwCalibrateCfg()) < 0
    assert "outside 33..96" in binding.take_error(hiplib)


def test_inverted_clamp_and_short_tap_stride_are_refused(hiplib):
    from openwurli_amd import binding, calibrate
    pts = calibrate.make_points([60], [100], [calibrate.CalibrationConfig(ds_clamp=(0.9, 0.1))])
    assert _call(hiplib, pts, binding.OwCalibrateCfg()) < 0
    assert "ds_clamp" in binding.take_error(hiplib)
    pts = calibrate.make_points([60], [100], [calibrate.CalibrationConfig()])
    buf = np.zeros(5 * 100)
    assert _call(hiplib, pts, binding.OwCalibrateCfg(), buf.ctypes.data_as(C.c_void_p), 100) < 0
    assert "taps_stride" in binding.take_error(hiplib)


def test_velocity_above_127_is_refused(hiplib):
    from openwurli_amd import binding, calibrate
    pts = calibrate.make_points([60], [100], [calibrate.CalibrationConfig()])
    pts["velocity"] = 128                                        # past make_points' own check: the library refuses it as well
    hiplib.ow_clear_error()
    assert _call(hiplib, pts, binding.OwCalibrateCfg()) < 0
    assert "above 127" in binding.take_error(hiplib)


@pytest.mark.parametrize("notes,vels", [([300], [100]), ([-1], [100]), ([32], [100]), ([97], [100]), ([60], [128]), ([60], [-1])])
def test_make_points_refuses_out_of_range_values_instead_of_wrapping(notes, vels):
    from openwurli_amd import calibrate
    with pytest.raises(ValueError):
        calibrate.make_points(notes, vels, [calibrate.CalibrationConfig()])
