"""Spectral centroid over time on the device: host mirror of ``preamp-bench centroid-track`` (tools/preamp-bench/src/main.rs:1925-2135)
over the C-ABI (``ow_centroid_track`` / ``ow_centroid_analyze`` / ``ow_centroid_frame_count``).

The command renders one note through the whole offline chain, follows the spectral centroid of the output in short periodic-Hann frames
(a brute-force DFT over the bins from 50 Hz to a quarter of the sample rate) and compares the attack centroid (first frame centred at or
after 10 ms), the sustain centroid (300 ms) and their drift with per-register targets.  On the device every note of a call runs at once:
``run_jobs`` returns one summary row and one row of frames per job, ``centroid_track`` is the command itself (stdout, CSV), ``grid_jobs`` /
``format_grid_csv`` the keyboard x velocity-layer map this project adds, ``analyze`` the analysis stage alone on given rows.
"""
import ctypes as C
import math
from decimal import Decimal
from typing import Optional

import numpy as np

from .binding import (CENTROID_MAX_WINDOW, CENTROID_MISS, CENTROID_NO_DATA, CENTROID_OK, OwCentroidCfg, OwCentroidJob, OwCentroidRow, OwError,
                      check, load_library, take_error)
from ._rust_text import BASE_SR, _f, as_usize as _as_usize, midi_note_name, samples  # noqa: F401

ML_VELOCITIES = (20, 35, 50, 65, 80, 95, 110, 127)          # the ML pipeline's velocity layers (ml/render_model_notes.py:26)
STATUS = {CENTROID_NO_DATA: "", CENTROID_OK: "OK", CENTROID_MISS: "MISS"}

# numpy views of include/openwurli_hip.h ow_centroid_job / ow_centroid_row
JOB_DTYPE = np.dtype(OwCentroidJob)
ROW_DTYPE = np.dtype(OwCentroidRow)


def make_job(note=60, velocity=100, volume=0.60, speaker=1.0, ldr=1_000_000.0, no_preamp=False, no_poweramp=False,
             displacement_scale: Optional[float] = None) -> np.ndarray:
    """One JOB_DTYPE record; the defaults are the command's (main.rs:1961-1977)."""
    j = np.zeros(1, dtype=JOB_DTYPE)
    j["note"], j["velocity"], j["volume"], j["speaker"], j["r_ldr"] = int(note), int(velocity), volume, speaker, ldr
    j["no_preamp"], j["no_poweramp"] = 1 if no_preamp else 0, 1 if no_poweramp else 0
    if displacement_scale is not None:
        j["has_displacement_scale"], j["displacement_scale"] = 1, displacement_scale
    return j


def make_jobs(jobs) -> np.ndarray:
    """JOB_DTYPE array from JOB_DTYPE records, dicts (make_job's keywords) or tuples (make_job's positional arguments)."""
    if isinstance(jobs, np.ndarray) and jobs.dtype == JOB_DTYPE:
        return np.ascontiguousarray(jobs).ravel()
    out = [make_job(**j) if isinstance(j, dict) else (j.reshape(1) if isinstance(j, (np.ndarray, np.void)) else make_job(*j)) for j in jobs]
    return np.concatenate(out) if out else np.zeros(0, dtype=JOB_DTYPE)


def ms_to_samples(ms: float) -> int:
    """((ms / 1000.0) * BASE_SR) as usize (main.rs:2012-2014): 5 ms -> 220."""
    return _as_usize((float(ms) / 1000.0) * BASE_SR)


def bin_range(window_samples: int):
    """(k_min, k_max) of spectral_centroid (main.rs:1933-1935) for a frame of window_samples at BASE_SR, 50 Hz .. BASE_SR / 4, in f64."""
    n = int(window_samples)
    freq_resolution = BASE_SR / float(n)
    return int(math.ceil(50.0 / freq_resolution)), min(int(math.floor((BASE_SR / 4.0) / freq_resolution)), n // 2)


def frame_positions(length: int, window_samples: int, hop_samples: int, end_sample: int) -> list:
    """The `pos` values of the command's while loop (main.rs:2045-2072): integer half in the condition."""
    if hop_samples <= 0:
        raise ValueError("hop_samples is 0: the reference's frame loop would never end")
    out, pos = [], 0
    while pos + window_samples <= length and pos + window_samples // 2 <= end_sample:
        out.append(pos)
        pos += hop_samples
    return out


def center_ms(pos: int, window_samples: int) -> float:
    """main.rs:2047: float half."""
    return (float(pos) + float(window_samples) / 2.0) / BASE_SR * 1000.0


def frame_times(duration=1.0, window_ms=5.0, hop_ms=2.5, end_ms=500.0) -> np.ndarray:
    """center_ms of every frame of a call."""
    w = ms_to_samples(window_ms)
    return np.array([center_ms(p, w) for p in frame_positions(samples(duration), w, ms_to_samples(hop_ms), ms_to_samples(end_ms))])


def frame_count(duration=1.0, window_ms=5.0, hop_ms=2.5, end_ms=500.0, preamp_kind=0, power_amp_kind=0) -> int:
    """``ow_centroid_frame_count`` (host only): raises OwError where the library refuses the configuration."""
    L = load_library()
    cfg = OwCentroidCfg(float(duration), float(window_ms), float(hop_ms), float(end_ms), 0, int(preamp_kind), int(power_amp_kind))
    return int(check(L, L.ow_centroid_frame_count(C.byref(cfg))))


def run_jobs(jobs, duration=1.0, window_ms=5.0, hop_ms=2.5, end_ms=500.0, device=0, audio=False, preamp_kind=0, power_amp_kind=0):
    """``ow_centroid_track``: (rows ROW_DTYPE [n], frames f64 [n][frames]); with audio=True also final_output f64 [n][samples]."""
    L = load_library()
    jb = make_jobs(jobs)
    cfg = OwCentroidCfg(float(duration), float(window_ms), float(hop_ms), float(end_ms), int(device), int(preamp_kind), int(power_amp_kind))
    nf = L.ow_centroid_frame_count(C.byref(cfg))
    if nf < 0:
        raise OwError(take_error(L).replace("ow_centroid_frame_count", "ow_centroid_track", 1))
    rows = np.zeros(jb.size, dtype=ROW_DTYPE)
    frames = np.zeros((jb.size, nf))
    n = samples(duration)
    au = np.zeros((jb.size, n)) if audio else None
    rc = check(L, L.ow_centroid_track(jb.ctypes.data_as(C.c_void_p), jb.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p), frames.ctypes.data_as(C.c_void_p),
                                      nf, au.ctypes.data_as(C.c_void_p) if audio else None, n))
    assert rc == nf
    return (rows, frames, au) if audio else (rows, frames)


def analyze(signals, window_samples, hop_samples, end_sample, length=None, device=0, out=None) -> np.ndarray:
    """``ow_centroid_analyze`` on host rows: signals f64 [n_rows][stride], the first `length` (default: all) samples of a row analysed.
    Returns f64 [n_rows][frames]; `out` ([n_rows][>= frames]) is filled in place instead when given (columns past the frames untouched)."""
    sig = np.ascontiguousarray(np.atleast_2d(signals), dtype=np.float64)
    length = sig.shape[1] if length is None else int(length)
    return _analyze(sig.ctypes.data_as(C.c_void_p), sig.shape[0], sig.shape[1], length, window_samples, hop_samples, end_sample, device, 0, out)


def analyze_device(ptr, n_rows, stride, length, window_samples, hop_samples, end_sample, device=0, out=None) -> np.ndarray:
    """``ow_centroid_analyze`` on rows that lie in device memory (e.g. what ``ow_batch_render`` left there): `ptr` a device address."""
    return _analyze(C.c_void_p(int(ptr)), n_rows, stride, length, window_samples, hop_samples, end_sample, device, 1, out)


def _analyze(ptr, n_rows, stride, length, window_samples, hop_samples, end_sample, device, is_device, out):
    L = load_library()
    if out is None:
        try:
            nf = len(frame_positions(min(int(length), int(stride)), int(window_samples), int(hop_samples), int(end_sample)))
        except ValueError:
            nf = 0                                           # the library refuses with its own message below
        out = np.zeros((int(n_rows), nf))
        whole = True
    else:
        assert out.dtype == np.float64 and out.ndim == 2 and out.shape[0] == n_rows and out.flags.c_contiguous
        whole = False
    rc = check(L, L.ow_centroid_analyze(ptr, int(n_rows), int(stride), int(length), int(window_samples), int(hop_samples), int(end_sample), int(device),
                                        int(is_device), out.ctypes.data_as(C.c_void_p), out.shape[1]))
    return out if whole else out[:, :rc]


def targets(note: int):
    """(attack_lo, attack_hi, sustain_lo, sustain_hi, drift_lo, drift_hi) by register (main.rs:2079-2088)."""
    if note <= 48:
        return (600.0, 1000.0, 500.0, 800.0, -200.0, -50.0)
    if note <= 72:
        return (600.0, 1200.0, 600.0, 1000.0, -240.0, -30.0)
    return (800.0, 1600.0, 800.0, 1400.0, -250.0, -30.0)


def summarise(note: int, frames, times) -> np.void:
    """The command's summary (main.rs:2042-2069, 2090-2129) of one job's frames as a ROW_DTYPE record -- what ow_centroid_track puts into
    rows_out, restated here so that frames from anywhere (a CSV, another renderer) get the same verdicts."""
    r = np.zeros(1, dtype=ROW_DTYPE)[0]
    t = targets(int(note))
    for k, v in zip(("attack_lo", "attack_hi", "sustain_lo", "sustain_hi", "drift_lo", "drift_hi"), t):
        r[k] = v
    r["frame10"] = r["frame300"] = -1
    for j, (c, ms) in enumerate(zip(frames, times)):
        if r["frame10"] < 0 and ms >= 10.0:
            r["frame10"], r["c10"], r["has_c10"] = j, c, 1
        if r["frame300"] < 0 and ms >= 300.0:
            r["frame300"], r["c300"], r["has_c300"] = j, c, 1
    ok = lambda x, lo, hi: CENTROID_OK if (x >= lo and x <= hi) else CENTROID_MISS
    if r["has_c10"]:
        r["attack_status"] = ok(r["c10"], t[0], t[1])
    if r["has_c300"]:
        r["sustain_status"] = ok(r["c300"], t[2], t[3])
    if r["has_c10"] and r["has_c300"]:
        r["drift"] = r["c300"] - r["c10"]
        r["drift_status"] = ok(r["drift"], t[4], t[5])
    return r


def rust_display(x: float) -> str:
    """Rust's `{}` of an f64: the shortest digits that round-trip, never an exponent, no trailing ".0" (5.0 -> "5", 2.5 -> "2.5")."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(x)), "f")
    return s[:-2] if s.endswith(".0") else s


def _fw(x, spec, width):
    return _f(x, spec).rjust(width)


def format_csv(frames, times) -> str:
    """The command's CSV (main.rs:2039-2061, 2131-2133): only the frames whose centroid is > 0."""
    lines = ["time_ms,centroid_hz"]
    for c, ms in zip(frames, times):
        if c > 0.0:
            lines.append("%s,%s" % (_f(ms, ".1f"), _f(c, ".1f")))
    return "\n".join(lines) + "\n"


def format_report(note, velocity, window_ms, frames, times, row=None, no_preamp=False, no_poweramp=False, csv_path="") -> str:
    """The command's stdout (main.rs:2025-2134).  `row`: the job's ROW_DTYPE record (default: summarise(note, frames, times)).  Rust's
    {:.0} / {:.1} round the exact binary value half to even, as Python's %-format does."""
    note = int(note)
    row = summarise(note, frames, times) if row is None else row
    out = ["Centroid tracking: %s (MIDI %d) vel=%d, %sms Hann windows" % (midi_note_name(note), note, int(velocity), rust_display(window_ms))]
    if no_preamp:
        out.append("  Preamp: BYPASSED")
    if no_poweramp:
        out.append("  Power amp: BYPASSED")
    out += ["", "  %10s  %14s" % ("Time (ms)", "Centroid (Hz)")]
    for c, ms in zip(frames, times):
        if c > 0.0:
            out.append("  %s  %s" % (_fw(ms, ".1f", 10), _fw(c, ".0f", 14)))
    out.append("")
    if row["has_c10"]:
        out.append("  Attack centroid (10ms):   %s Hz   (target: %s-%s)  %s" % (_fw(row["c10"], ".0f", 6), _f(row["attack_lo"], ".0f"),
                                                                                _f(row["attack_hi"], ".0f"), STATUS[int(row["attack_status"])]))
    else:
        out.append("  Attack centroid (10ms):   (no data — signal too short or silent)")
    if row["has_c300"]:
        out.append("  Sustain centroid (300ms): %s Hz   (target: %s-%s)  %s" % (_fw(row["c300"], ".0f", 6), _f(row["sustain_lo"], ".0f"),
                                                                                _f(row["sustain_hi"], ".0f"), STATUS[int(row["sustain_status"])]))
    else:
        out.append("  Sustain centroid (300ms): (no data — signal too short)")
    if row["has_c10"] and row["has_c300"]:
        out.append("  Drift:                   %s Hz   (target: %s to %s) %s" % (_fw(row["drift"], "+.0f", 6), _f(row["drift_lo"], ".0f"),
                                                                                _f(row["drift_hi"], ".0f"), STATUS[int(row["drift_status"])]))
    if csv_path:
        out += ["", "  CSV written to %s" % csv_path]
    return "\n".join(out) + "\n"


def centroid_track(note=60, velocity=100, duration=1.0, window_ms=5.0, hop_ms=2.5, end_ms=500.0, ldr=1_000_000.0, volume=0.60, speaker=1.0,
                   no_poweramp=False, no_preamp=False, csv: str = "", displacement_scale: Optional[float] = None, device=0) -> dict:
    """cmd_centroid_track for one note: {"row", "frames", "times", "audio", "report", "csv"}; with `csv` set the CSV file is written."""
    rows, frames, audio = run_jobs(make_job(note, velocity, volume, speaker, ldr, no_preamp, no_poweramp, displacement_scale), duration, window_ms,
                                   hop_ms, end_ms, device, audio=True)
    times = frame_times(duration, window_ms, hop_ms, end_ms)
    text = format_csv(frames[0], times)
    if csv:
        with open(csv, "w", newline="") as f:
            f.write(text)
    return {"row": rows[0], "frames": frames[0], "times": times, "audio": audio[0], "csv": text,
            "report": format_report(note, velocity, window_ms, frames[0], times, rows[0], no_preamp, no_poweramp, csv)}


def grid_jobs(notes=range(33, 97), velocities=ML_VELOCITIES, volume=0.60, speaker=1.0, ldr=1_000_000.0, no_preamp=False, no_poweramp=False,
              displacement_scale: Optional[float] = None) -> np.ndarray:
    """notes x velocities, note outer: JOB_DTYPE array (default: the keyboard x the ML pipeline's eight velocity layers, 512 jobs)."""
    return make_jobs([(n, v, volume, speaker, ldr, no_preamp, no_poweramp, displacement_scale) for n in notes for v in velocities])


def format_grid_csv(jobs: np.ndarray, rows: np.ndarray) -> str:
    """The `grid` command's CSV (this project's addition): one row per (note, velocity); a figure the command would not print is empty."""
    out = ["note,velocity,c10,c300,drift,attack_status,sustain_status,drift_status"]
    for j, r in zip(jobs, rows):
        both = r["has_c10"] and r["has_c300"]
        out.append("%d,%d,%s,%s,%s,%s,%s,%s" % (j["note"], j["velocity"], _f(r["c10"], ".1f") if r["has_c10"] else "",
                                                _f(r["c300"], ".1f") if r["has_c300"] else "", _f(r["drift"], ".1f") if both else "",
                                                STATUS[int(r["attack_status"])], STATUS[int(r["sustain_status"])], STATUS[int(r["drift_status"])]))
    return "\n".join(out) + "\n"


__all__ = ["JOB_DTYPE", "ROW_DTYPE", "ML_VELOCITIES", "STATUS", "CENTROID_MAX_WINDOW", "make_job", "make_jobs", "ms_to_samples", "samples", "bin_range",
           "frame_positions", "center_ms", "frame_times", "frame_count", "run_jobs", "analyze", "analyze_device", "targets", "summarise",
           "rust_display", "format_csv", "format_report", "centroid_track", "grid_jobs", "format_grid_csv"]
