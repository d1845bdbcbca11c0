"""Overshoot audit on the device: host mirror of ``preamp-bench overshoot`` (tools/preamp-bench/src/main.rs:2137-2247) over the C-ABI
(``ow_overshoot``).

The command renders a note with one voice and no chain and compares the attack peak with the sustain level: the spec metric (0-10 ms peak
against the 100-200 ms RMS) and the "bark decay" (0-50 ms peak against the 1000-1500 ms RMS).  On the device every (note, velocity) job of
a call runs at once: ``audit`` returns one row per job, ``report`` is the command's stdout.
"""
import ctypes as C

import numpy as np

from .binding import OVERSHOOT_ROW_FIELDS, OwError, OwOvershootCfg, OwOvershootRow, check, load_library, take_error  # noqa: F401
from .intermod_audit import NOTE_JOB_DTYPE, note_jobs
from ._rust_text import _f, midi_note_name, parse_csv_u8, samples  # noqa: F401

DEFAULT_NOTES = (36, 48, 60, 72, 84)                        # main.rs:2148
DEFAULT_VELOCITIES = (64, 127)                              # main.rs:2149
DURATION = 2.0                                              # main.rs:2151

# numpy view of include/openwurli_hip.h ow_overshoot_row
ROW_DTYPE = np.dtype(OwOvershootRow)


def run_jobs(jobs, duration=DURATION, device=0, audio=False):
    """``ow_overshoot``: rows ROW_DTYPE [n]; with audio=True also the voice rows f64 [n][samples]."""
    L = load_library()
    jb = np.ascontiguousarray(jobs, dtype=NOTE_JOB_DTYPE).ravel()
    cfg = OwOvershootCfg(float(duration), int(device))
    rows = np.zeros(jb.size, dtype=ROW_DTYPE)
    n = samples(duration)
    au = np.zeros((jb.size, n)) if audio else None
    check(L, L.ow_overshoot(jb.ctypes.data_as(C.c_void_p), jb.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p),
                            au.ctypes.data_as(C.c_void_p) if audio else None, n))
    return (rows, au) if audio else rows


def audit(notes=DEFAULT_NOTES, velocities=DEFAULT_VELOCITIES, duration=DURATION, device=0) -> np.ndarray:
    """notes x velocities (note outer) in one call: ROW_DTYPE [len(notes) * len(velocities)]."""
    return run_jobs(note_jobs(list(notes), list(velocities)), duration, device)


def format_report(notes, velocities, rows) -> str:
    """cmd_overshoot's stdout (main.rs:2153-2228) from rows in note-outer order (ROW_DTYPE, or anything indexable by the same names)."""
    out = ["=== OVERSHOOT AUDIT ===",
           "Spec metric:  0-10ms peak vs 100-200ms RMS (calibration-and-evaluation.md §10.1)",
           "Bark decay:   0-50ms peak vs 1000-1500ms RMS (perceptual bark fade, NOT overshoot)",
           "",
           "%6s %4s  %8s %8s %8s  %10s %10s" % ("Note", "Vel", "Pk(0-10)", "RMS(sus)", "RMS(late)", "Overshoot", "BarkDecay"),
           "%6s %4s  %8s %8s %8s  %10s %10s" % ("", "", "dBFS", "dBFS", "dBFS", "dB", "dB"),
           "-" * 76]
    k = 0
    for note in notes:
        for vel in velocities:
            r = rows[k]
            k += 1
            out.append("%6s %4d  %s %s %s  %s %s" % (midi_note_name(int(note)), int(vel), _f(r["pk_dbfs"], "7.1f"), _f(r["rms1_dbfs"], "7.1f"),
                                                     _f(r["rms2_dbfs"], "7.1f"), _f(r["overshoot_db"], "9.1f"), _f(r["bark_decay_db"], "9.1f")))
        out.append("")
    out += ["Targets (from calibration-and-evaluation.md §4.1 & §10.1):",
            "  Overshoot at mf (v64):   2-5 dB   (from modal superposition)",
            "  Overshoot at ff (v127):  5-10 dB  (from modal superposition)",
            "  Bark decay:              no target (physics-correct bark fade, not a defect)"]
    return "\n".join(out) + "\n"


def report(notes=DEFAULT_NOTES, velocities=DEFAULT_VELOCITIES, duration=DURATION, device=0) -> str:
    notes, velocities = [int(n) for n in notes], [int(v) for v in velocities]
    rows = audit(notes, velocities, duration, device) if notes and velocities else np.zeros(0, dtype=ROW_DTYPE)
    return format_report(notes, velocities, rows)


__all__ = ["DEFAULT_NOTES", "DEFAULT_VELOCITIES", "DURATION", "ROW_DTYPE", "run_jobs", "audit", "format_report", "report", "parse_csv_u8"]
