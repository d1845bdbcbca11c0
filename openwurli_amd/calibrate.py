"""Calibration sweeps on the device: host mirror of ``preamp-bench calibrate`` and ``preamp-bench sensitivity``
(tools/preamp-bench/src/main.rs:1069-1395) over the C-ABI (``ow_calibrate``).  Same names as the reference: ``CalibrationConfig``
(tables.rs:254-277), ``run_calibrate``, ``write_calibrate_csv``, ``midi_note_name``; every grid point of a call -- a whole sensitivity
sweep included -- renders lane-parallel in one library call.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from .binding import (CALIB_SAMPLES, CALIBRATE_ROW_FIELDS, OwCalibPoint, OwCalibrateCfg, OwCalibrateRow, OwError, check,
                      load_library, take_error)  # noqa: F401

from ._rust_text import BASE_SR, midi_note_name  # noqa: F401
MIDI_LO, MIDI_HI = 33, 96                                   # tables.rs:6-7
PREAMP_LEGACY8, PREAMP_MELANGE12 = 0, 1
POWER_AMP_BEHAVIORAL, POWER_AMP_MELANGE = 0, 1

CALIBRATE_NOTES = (36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84)     # main.rs:1070
CALIBRATE_VELOCITIES = (40, 80, 127)                                        # main.rs:1071
SENSITIVITY_NOTES = (36, 48, 54, 60, 66, 72, 78, 84)                        # main.rs:1322
SENSITIVITY_VELOCITIES = (40, 80, 127)                                      # main.rs:1323
SENSITIVITY_DS = (0.50, 0.55, 0.60, 0.65, 0.70, 0.75, 0.80, 0.85)           # main.rs:1324-1328
SCALE_MODES = ("track", "zero-trim", "freeze")                              # main.rs:1331-1377
FREEZE_DS_AT_C4 = 0.85                                                      # main.rs:1352-1356


@dataclass
class CalibrationConfig:                                    # tables.rs:254-277 (Default = the in-tree constants)
    ds_at_c4: float = 0.85
    ds_exponent: float = 0.75
    ds_clamp: Tuple[float, float] = (0.02, 0.95)
    target_db: float = -35.0
    voicing_slope: float = -0.04
    zero_trim: bool = False


@dataclass
class CalibrateRow:                                         # main.rs:1099-1121
    midi: int
    velocity: int
    ds_at_c4: float
    ds_actual: float
    y_peak: float
    t2_peak_db: float
    t2_rms_db: float
    t2_h2_h1_db: float
    t3_peak_db: float
    t3_rms_db: float
    t4_peak_db: float
    t4_rms_db: float
    t4_h2_h1_db: float
    t5_peak_db: float
    t5_rms_db: float
    t5_h2_h1_db: float
    proxy_db: float
    trim_db: float
    proxy_error_db: float
    tanh_compression_db: float


# numpy views of the C structs (include/openwurli_hip.h ow_calib_point / ow_calibrate_row), for grids of 10^4..10^5 points
POINT_DTYPE = np.dtype(OwCalibPoint)
ROW_DTYPE = np.dtype(OwCalibrateRow)


def make_points(notes: Sequence[int], velocities: Sequence[int], cfgs: Sequence[CalibrationConfig]) -> np.ndarray:
    """One ow_calib_point per (note, velocity, config) triple (three equal-length sequences)."""
    n = len(notes)
    if len(velocities) != n or len(cfgs) != n:
        raise ValueError("notes, velocities and configs must have equal length")
    nn = np.asarray(notes, dtype=np.int64).reshape(n)
    vv = np.asarray(velocities, dtype=np.int64).reshape(n)
    if n and (nn.min() < MIDI_LO or nn.max() > MIDI_HI):    # checked before the u8 fields could wrap a 300 into range
        raise ValueError(f"notes must lie in {MIDI_LO}..{MIDI_HI} (the tables' range)")
    if n and (vv.min() < 0 or vv.max() > 127):
        raise ValueError("velocities must lie in 0..127 (MIDI velocity bytes)")
    p = np.zeros(n, dtype=POINT_DTYPE)
    p["note"] = nn
    p["velocity"] = vv
    p["zero_trim"] = [1 if c.zero_trim else 0 for c in cfgs]
    p["ds_at_c4"] = [c.ds_at_c4 for c in cfgs]
    p["ds_exponent"] = [c.ds_exponent for c in cfgs]
    p["ds_clamp_lo"] = [c.ds_clamp[0] for c in cfgs]
    p["ds_clamp_hi"] = [c.ds_clamp[1] for c in cfgs]
    p["target_db"] = [c.target_db for c in cfgs]
    p["voicing_slope"] = [c.voicing_slope for c in cfgs]
    return p


def run_points(points: np.ndarray, volume: float, speaker_char: float, preamp_kind=PREAMP_LEGACY8, power_amp_kind=POWER_AMP_BEHAVIORAL,
               device=0, taps=False):
    """``ow_calibrate`` on a POINT_DTYPE array: a ROW_DTYPE array (and, with taps, the f64 [n][5][22050] T1..T5 renders)."""
    L = load_library()
    pts = np.ascontiguousarray(points, dtype=POINT_DTYPE)
    rows = np.zeros(pts.size, dtype=ROW_DTYPE)
    tp = np.zeros((pts.size, 5, CALIB_SAMPLES)) if taps else None
    cfg = OwCalibrateCfg(float(volume), float(speaker_char), int(device), int(preamp_kind), int(power_amp_kind))
    check(L, L.ow_calibrate(pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p),
                            tp.ctypes.data_as(C.c_void_p) if tp is not None else None, CALIB_SAMPLES))
    return (rows, tp) if taps else rows


def rows_from_array(a: np.ndarray) -> List[CalibrateRow]:
    cols = [a[f].tolist() for f in CALIBRATE_ROW_FIELDS]
    mid, vel = a["midi"].tolist(), a["velocity"].tolist()
    return [CalibrateRow(mid[i], vel[i], *(c[i] for c in cols)) for i in range(a.size)]


def run_calibrate(notes: Sequence[int], velocities: Sequence[int], cfg: CalibrationConfig, volume: float, speaker_char: float,
                  preamp_kind=PREAMP_LEGACY8, power_amp_kind=POWER_AMP_BEHAVIORAL, device=0, taps=False):
    """run_calibrate (main.rs:1128-1262): one row per (note, velocity), notes outer.  taps=True also returns T1..T5 [n][5][22050]."""
    nn = [int(n) for n in notes for _ in velocities]
    vv = [int(v) for _ in notes for v in velocities]
    res = run_points(make_points(nn, vv, [cfg] * len(nn)), volume, speaker_char, preamp_kind, power_amp_kind, device, taps)
    if taps:
        return rows_from_array(res[0]), res[1]
    return rows_from_array(res)


def calibrate(notes=CALIBRATE_NOTES, velocities=CALIBRATE_VELOCITIES, ds_at_c4=0.75, ds_clamp_max=0.82, volume=0.40, speaker=1.0,
              zero_trim=False, preamp_kind=PREAMP_LEGACY8, power_amp_kind=POWER_AMP_BEHAVIORAL, device=0, taps=False):
    """cmd_calibrate (main.rs:1069-1096) with its CLI defaults.  The 0.82 clamp is the command's own default (not tables.rs's 0.95)."""
    cfg = calibrate_config(ds_at_c4, ds_clamp_max, zero_trim)
    return run_calibrate(notes, velocities, cfg, volume, speaker, preamp_kind, power_amp_kind, device, taps)


def calibrate_config(ds_at_c4=0.75, ds_clamp_max=0.82, zero_trim=False) -> CalibrationConfig:   # main.rs:1086-1091
    return CalibrationConfig(ds_at_c4=ds_at_c4, ds_clamp=(0.02, ds_clamp_max), zero_trim=zero_trim)


def sensitivity_config(ds: float, scale_mode="track") -> CalibrationConfig:                      # main.rs:1348-1371
    if scale_mode == "freeze":
        return CalibrationConfig(ds_at_c4=FREEZE_DS_AT_C4, zero_trim=False)
    if scale_mode == "zero-trim":
        return CalibrationConfig(ds_at_c4=ds, zero_trim=True)
    return CalibrationConfig(ds_at_c4=ds, zero_trim=False)       # "track" (and, as in the reference, any other name)


def sensitivity(notes=SENSITIVITY_NOTES, velocities=SENSITIVITY_VELOCITIES, ds_values=SENSITIVITY_DS, scale_mode="track", zero_trim=False,
                volume=0.40, speaker=1.0, preamp_kind=PREAMP_LEGACY8, power_amp_kind=POWER_AMP_BEHAVIORAL, device=0) -> List[CalibrateRow]:
    """cmd_sensitivity (main.rs:1318-1389): DS values outer, then notes, then velocities; the whole grid is ONE ow_calibrate call and
    every row's ds_at_c4 column carries its sweep value.  zero_trim=True is --zero-trim (shorthand for scale_mode="zero-trim")."""
    if zero_trim:
        scale_mode = "zero-trim"
    nn, vv, cc, stamp = [], [], [], []
    for ds in ds_values:
        cfg = sensitivity_config(ds, scale_mode)
        for n in notes:
            for v in velocities:
                nn.append(int(n)); vv.append(int(v)); cc.append(cfg); stamp.append(float(ds))
    rows = run_points(make_points(nn, vv, cc), volume, speaker, preamp_kind, power_amp_kind, device)
    rows["ds_at_c4"] = stamp                                     # main.rs:1375-1378
    return rows_from_array(rows)


_HEADER = ("midi,note_name,velocity,ds_at_c4,ds_actual,y_peak,t2_peak_db,t2_rms_db,t2_h2_h1_db,t3_peak_db,t3_rms_db,"
           "t4_peak_db,t4_rms_db,t4_h2_h1_db,t5_peak_db,t5_rms_db,t5_h2_h1_db,proxy_db,trim_db,proxy_error_db,tanh_compression_db")


def format_calibrate_csv(rows: Sequence[CalibrateRow]) -> str:
    """write_calibrate_csv's text (main.rs:1265-1310): {:.4} for ds_at_c4 / ds_actual / y_peak, {:.2} for every dB column."""
    out = [_HEADER]
    for r in rows:
        v = [getattr(r, f) for f in CALIBRATE_ROW_FIELDS]
        out.append(",".join([str(int(r.midi)), midi_note_name(int(r.midi)), str(int(r.velocity))] + ["%.4f" % x for x in v[:3]]
                            + ["%.2f" % x for x in v[3:]]))
    return "\n".join(out) + "\n"


def write_calibrate_csv(path, rows: Sequence[CalibrateRow]):
    with open(path, "w", newline="") as f:
        f.write(format_calibrate_csv(rows))


__all__ = ["CalibrationConfig", "CalibrateRow", "run_calibrate", "calibrate", "sensitivity", "calibrate_config", "sensitivity_config",
           "write_calibrate_csv", "format_calibrate_csv", "midi_note_name", "make_points", "run_points", "rows_from_array"]
