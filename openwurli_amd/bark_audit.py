"""Bark audit on the device: host mirror of ``preamp-bench bark-audit`` (tools/preamp-bench/src/main.rs:551-664) over the C-ABI
(``ow_bark_audit``).

For each (note, velocity) the command reports how much second harmonic the reed carries into the pickup and out of the preamp, stage by
stage: the raw reed (no onset ramp, no attack noise), the pickup at the note's own displacement scale, a fresh preamp at a static 1 Mohm.
On the device every job of a call runs at once: ``bark_audit`` returns one row per job (optionally the three stage rows too),
``format_report`` is the command's stdout, ``grid`` the keyboard x velocity-layer x preamp-model map this project adds.
"""
import ctypes as C

import numpy as np

from .binding import BARK_ROW_FIELDS, OwBarkCfg, OwBarkRow, OwError, check, load_library, take_error  # noqa: F401
from .intermod_audit import NOTE_JOB_DTYPE, note_jobs
from ._rust_text import _f, midi_note_name, parse_csv_u8, samples  # noqa: F401

DEFAULT_NOTES = (36, 48, 60, 72, 84)                        # main.rs:562
DEFAULT_VELOCITIES = (40, 80, 100, 127)                     # main.rs:563
DURATION = 0.5                                              # main.rs:565
MEASURE_START = 0.25                                        # main.rs:566
PREAMP_LEGACY8, PREAMP_MELANGE12 = 0, 1
KIND_NAMES = ("legacy", "melange")
ML_VELOCITIES = (20, 35, 50, 65, 80, 95, 110, 127)          # the velocity layers of the other grids

# numpy view of include/openwurli_hip.h ow_bark_row
ROW_DTYPE = np.dtype(OwBarkRow)


def run_jobs(jobs, preamp_kind=PREAMP_LEGACY8, duration=DURATION, measure_start=MEASURE_START, device=0, taps=False):
    """``ow_bark_audit``: rows ROW_DTYPE [n]; with taps=True also the stage rows f64 [n][3][samples] (reed, pickup, preamp)."""
    L = load_library()
    jb = np.ascontiguousarray(jobs, dtype=NOTE_JOB_DTYPE).ravel()
    cfg = OwBarkCfg(float(duration), float(measure_start), int(device), int(preamp_kind))
    rows = np.zeros(jb.size, dtype=ROW_DTYPE)
    n = samples(duration)
    tp = np.zeros((jb.size, 3, n)) if taps else None
    check(L, L.ow_bark_audit(jb.ctypes.data_as(C.c_void_p), jb.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p),
                             tp.ctypes.data_as(C.c_void_p) if taps else None, n))
    return (rows, tp) if taps else rows


def bark_audit(notes=DEFAULT_NOTES, velocities=DEFAULT_VELOCITIES, preamp_kind=PREAMP_LEGACY8, duration=DURATION, measure_start=MEASURE_START,
               device=0, taps=False):
    """notes x velocities (note outer) in one call: ROW_DTYPE [len(notes) * len(velocities)], with taps=True also the stage rows."""
    return run_jobs(note_jobs(list(notes), list(velocities)), preamp_kind, duration, measure_start, device, taps)


def format_report(rows, per_note=None, n_notes=None) -> str:
    """cmd_bark_audit's stdout (main.rs:568-663) from rows in note-outer order (ROW_DTYPE, or anything indexable by the same names).  The
    command prints a blank line behind each note's velocities: behind every `per_note` rows (`n_notes` blocks in all; default: wherever the
    note changes)."""
    out = ["=== BARK AUDIT: H2/H1 at each signal chain stage ===",
           "",
           "%6s %4s  %10s %10s %10s %10s %10s" % ("Note", "Vel", "Reed pk", "y_peak", "PU H2/H1", "PU pk(mV)", "Pre H2/H1"),
           "-" * 76]
    n = len(rows)
    for k, r in enumerate(rows):
        out.append("%6s %4d  %s %s %s%% %s %s%%" % (midi_note_name(int(r["note"])), int(r["velocity"]), _f(r["reed_peak"], "10.4f"), _f(r["y_peak"], "10.4f"),
                                                   _f(r["pu_h2_h1"] * 100.0, "9.1f"), _f(r["pu_peak"] * 1000.0, "10.2f"),
                                                   _f(r["pre_h2_h1"] * 100.0, "9.1f")))
        last = (k + 1) % per_note == 0 if per_note else (k + 1 == n or int(rows[k + 1]["note"]) != int(r["note"]))
        if last:
            out.append("")
    if per_note == 0 and n_notes:
        out += [""] * int(n_notes)                           # notes without velocities: the blank lines alone
    out += ["Legend:",
            "  Reed pk   = peak reed displacement (model units)",
            "  y_peak    = physical displacement fraction (y = reed_pk * DS), DS = per-note from tables",
            "  PU H2/H1  = H2/H1 after time-varying RC pickup (coupled NL + HPF at 2312 Hz)",
            "  PU pk(mV) = peak signal after pickup (millivolts, feeds preamp)",
            "  Pre H2/H1 = H2/H1 after preamp (2x gain, no tremolo)",
            "",
            "SPICE targets: y=0.10 → H2/H1 ≈ 8.7%, pickup HPF boosts H2 ~1.9x relative to H1"]
    return "\n".join(out) + "\n"


def report(notes=DEFAULT_NOTES, velocities=DEFAULT_VELOCITIES, preamp_kind=PREAMP_LEGACY8, device=0) -> str:
    """The command's stdout for notes x velocities."""
    notes, velocities = [int(n) for n in notes], [int(v) for v in velocities]
    rows = bark_audit(notes, velocities, preamp_kind, device=device) if notes and velocities else np.zeros(0, dtype=ROW_DTYPE)
    return format_report(rows, len(velocities), len(notes))


GRID_HEADER = "note,velocity,model,reed_peak,y_peak,pu_h2_h1_pct,pu_peak_mv,pre_h2_h1_pct"


def format_grid_csv(rows_by_kind) -> str:
    """The `grid` command's CSV (this project's addition): one row per (note, velocity layer, model), model outer."""
    out = [GRID_HEADER]
    for kind, rows in rows_by_kind:
        for r in rows:
            out.append("%d,%d,%s,%s,%s,%s,%s,%s" % (r["note"], r["velocity"], KIND_NAMES[int(kind)], _f(r["reed_peak"], ".6f"), _f(r["y_peak"], ".6f"),
                                                    _f(r["pu_h2_h1"] * 100.0, ".3f"), _f(r["pu_peak"] * 1000.0, ".4f"),
                                                    _f(r["pre_h2_h1"] * 100.0, ".3f")))
    return "\n".join(out) + "\n"


def grid(notes=range(33, 97), velocities=ML_VELOCITIES, kinds=(PREAMP_LEGACY8, PREAMP_MELANGE12), device=0):
    """Every (note, velocity layer, model): ([(kind, rows)], the CSV text); one device call per model."""
    by_kind = [(int(k), bark_audit(list(notes), list(velocities), int(k), device=device)) for k in kinds]
    return by_kind, format_grid_csv(by_kind)


__all__ = ["DEFAULT_NOTES", "DEFAULT_VELOCITIES", "DURATION", "MEASURE_START", "PREAMP_LEGACY8", "PREAMP_MELANGE12", "KIND_NAMES", "ML_VELOCITIES",
           "ROW_DTYPE", "run_jobs", "bark_audit", "format_report", "report", "GRID_HEADER", "format_grid_csv", "grid", "parse_csv_u8",
           "midi_note_name"]
