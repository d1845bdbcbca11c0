"""Intermodulation audit on the device: host mirror of ``preamp-bench intermod-audit`` (tools/preamp-bench/src/main.rs:675-903) over the
C-ABI (``ow_intermod_risk`` / ``ow_intermod_probes`` / ``ow_intermod_audit`` / ``ow_dft_magnitudes``).

The command has two halves.  The static table (tables::intermod_risk, host only) says for every note how close the ratio of each reed mode
lies to an integer harmonic and how audible the resulting beat would be.  The render analysis (``--render``) renders the flagged notes
with one voice and no chain, takes the sustain window 0.5-2.0 s and compares the energy at the harmonics with the energy at the midpoints
between them ("spectral grass"), by brute-force DFT.  On the device every (note, velocity) job of a call runs at once: ``audit`` returns one
row per job, ``report`` is the command's stdout, ``format_grid_csv`` the keyboard x velocity-layer map this project adds.
"""
import ctypes as C

import numpy as np

from .binding import (INTERMOD_MAX_PROBES, OwError, OwIntermodCfg, OwIntermodDetail, OwIntermodProduct, OwIntermodReport, OwIntermodRow, OwNoteJob, check,
                      load_library, take_error)  # noqa: F401
from ._rust_text import _f, midi_note_name, parse_csv_u8, samples  # noqa: F401

MIDI_LO, MIDI_HI = 33, 96                                    # tables.rs:6-7
VERDICTS = ("DIRTY", "MARGINAL", "OK", "CLEAN")              # ow_intermod_row.verdict

# numpy views of include/openwurli_hip.h ow_note_job / ow_intermod_report / ow_intermod_row
NOTE_JOB_DTYPE = np.dtype(OwNoteJob)
PRODUCT_DTYPE = np.dtype(OwIntermodProduct)
REPORT_DTYPE = np.dtype(OwIntermodReport)
DETAIL_DTYPE = np.dtype(OwIntermodDetail)
ROW_DTYPE = np.dtype(OwIntermodRow)


def note_jobs(notes, velocities=(127,)) -> np.ndarray:
    """notes x velocities, note outer: NOTE_JOB_DTYPE array."""
    j = np.zeros(len(notes) * len(velocities), dtype=NOTE_JOB_DTYPE)
    j["note"] = np.repeat(np.asarray(notes, dtype=np.int64), len(velocities))
    j["velocity"] = np.tile(np.asarray(velocities, dtype=np.int64), len(notes))
    return j


def risk(midi: int) -> np.void:
    """``ow_intermod_risk`` (host only): the REPORT_DTYPE record of any MIDI byte."""
    L = load_library()
    r = np.zeros(1, dtype=REPORT_DTYPE)
    check(L, L.ow_intermod_risk(int(midi), C.cast(r.ctypes.data, C.POINTER(OwIntermodReport))))
    return r[0]


def probes(midi: int):
    """``ow_intermod_probes`` (host only): (frequencies f64 [count], n_harmonics, n_midpoints) of the render analysis of one note."""
    L = load_library()
    f = np.zeros(INTERMOD_MAX_PROBES)
    nh, nm = C.c_uint32(0), C.c_uint32(0)
    c = check(L, L.ow_intermod_probes(int(midi), f.ctypes.data_as(C.c_void_p), C.byref(nh), C.byref(nm)))
    return f[:c].copy(), int(nh.value), int(nm.value)


def dft_magnitudes(signals, start, end, freqs, sample_rate=44100.0, device=0) -> np.ndarray:
    """``ow_dft_magnitudes`` on host rows: dft_magnitude of signals[r][start:end] at freqs[r][k]; NaN in freqs: no probe, 0.0."""
    L = load_library()
    sig = np.ascontiguousarray(np.atleast_2d(signals), dtype=np.float64)
    fr = np.ascontiguousarray(np.atleast_2d(freqs), dtype=np.float64)
    assert fr.shape[0] == sig.shape[0]
    out = np.zeros(fr.shape)
    check(L, L.ow_dft_magnitudes(sig.ctypes.data_as(C.c_void_p), sig.shape[0], sig.shape[1], int(start), int(end), float(sample_rate),
                                 fr.ctypes.data_as(C.c_void_p), fr.shape[1], int(device), 0, out.ctypes.data_as(C.c_void_p)))
    return out


def run_jobs(jobs, duration=3.0, device=0, audio=False):
    """``ow_intermod_audit``: rows ROW_DTYPE [n]; with audio=True also the voice rows f64 [n][samples]."""
    L = load_library()
    jb = np.ascontiguousarray(jobs, dtype=NOTE_JOB_DTYPE).ravel()
    cfg = OwIntermodCfg(float(duration), int(device))
    rows = np.zeros(jb.size, dtype=ROW_DTYPE)
    n = samples(duration)
    au = np.zeros((jb.size, n)) if audio else None
    check(L, L.ow_intermod_audit(jb.ctypes.data_as(C.c_void_p), jb.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p),
                                 au.ctypes.data_as(C.c_void_p) if audio else None, n))
    return (rows, au) if audio else rows


def audit(notes, velocities=(127,), duration=3.0, device=0) -> np.ndarray:
    """The render analysis of notes x velocities (note outer) in one call: ROW_DTYPE [len(notes) * len(velocities)]."""
    return run_jobs(note_jobs(list(notes), list(velocities)), duration, device)


def worst_product(rep):
    """`products.iter().max_by(risk_score)`: Rust's max_by returns the LAST of equal maxima."""
    best = rep["products"][0]
    for p in rep["products"][1:]:
        if p["risk_score"] >= best["risk_score"]:
            best = p
    return best


def format_static(notes, threshold=0.07, reports=None):
    """The static half of the command's stdout (main.rs:733-789) as lines, and the flagged notes."""
    reports = [risk(m) for m in notes] if reports is None else reports
    out = ["=== INTERMOD RISK AUDIT ===", "Threshold: %s" % _f(threshold, ".4f"), "",
           "%6s %4s %6s  %5s %6s %8s %8s %7s %7s %8s" % ("Note", "MIDI", "mu", "Mode", "Ratio", "Offset", "Beat Hz", "Eff Amp", "Weight", "Risk"),
           "-" * 82]
    flagged = []
    for midi, rep in zip(notes, reports):
        is_flagged = rep["max_risk"] >= threshold
        if is_flagged:
            flagged.append(int(midi))
        w = worst_product(rep)
        out.append("%6s %4d %s  %5d %s %s %s %s %s %s%s" % (
            midi_note_name(int(midi)), int(midi), _f(rep["mu"], "6.4f"), int(w["mode"]), _f(w["mode_ratio"], "6.3f"), _f(w["fractional_offset"], "8.5f"),
            _f(w["beat_hz"], "8.2f"), _f(w["effective_amplitude"], "7.4f"), _f(w["perceptual_weight"], "7.3f"), _f(w["risk_score"], "8.5f"),
            " ***" if is_flagged else ""))
    out += ["", "Flagged notes (risk >= %s): %d" % (_f(threshold, ".4f"), len(flagged))]
    if flagged:
        out.append("  " + ", ".join("%s (%d)" % (midi_note_name(m), m) for m in flagged))
    return out, flagged


def format_render(rows, duration=3.0):
    """The render half (main.rs:812-888) as lines, from ROW_DTYPE rows (or anything indexable by the same names)."""
    out = ["", "=== RENDER ANALYSIS (sustain spectral grass) ===", "Duration: %ss, analysis window: 0.5-2.0s" % _f(duration, ".1f"), "",
           "%6s %4s  %10s %10s %10s  %8s" % ("Note", "MIDI", "Harm (dB)", "Mid (dB)", "Ratio (dB)", "Verdict"), "-" * 64]
    for r in rows:
        midi = int(r["midi"])
        if r["too_short"]:
            out.append("%6s %4d  (signal too short)" % (midi_note_name(midi), midi))
            continue
        out.append("%6s %4d  %s %s %s  %8s" % (midi_note_name(midi), midi, _f(r["h_db"], "10.1f"), _f(r["m_db"], "10.1f"), _f(r["ratio_db"], "10.1f"),
                                               VERDICTS[int(r["verdict"])]))
        if r["ratio_db"] <= 30.0:
            out.append("  Per-product detail:")
            for p in r["products"]:
                if not p["listed"]:
                    continue
                out.append("    Mode %d: %s Hz (near H%d @ %s Hz) intermod/harmonic = %s dB, risk=%s" % (
                    int(p["mode"]), _f(p["intermod_freq"], ".1f"), int(p["nearest_integer"]), _f(p["nearest_freq"], ".1f"), _f(p["ratio_db"], ".1f"),
                    _f(p["risk_score"], ".5f")))
    return out


def report(threshold=0.07, render=False, duration=3.0, notes=None, device=0, run=None) -> str:
    """cmd_intermod_audit's stdout.  notes=None: MIDI_LO..=MIDI_HI and only the flagged notes are rendered; a list (``--notes``): all of it
    is rendered.  `run`: what renders and analyses, run(notes, duration) -> rows (default: the device, every note at velocity 127)."""
    given = notes is not None
    notes = list(range(MIDI_LO, MIDI_HI + 1)) if notes is None else [int(m) for m in notes]
    out, flagged = format_static(notes, threshold)
    if not render:
        if flagged:
            out += ["", "Run with --render to analyze flagged notes spectrally."]
        return "\n".join(out) + "\n"
    render_notes = notes if given else flagged
    if not render_notes:
        out += ["", "No notes to render-analyze. All clear!"]
        return "\n".join(out) + "\n"
    rows = (run or (lambda ns, d: audit(ns, (127,), d, device)))(render_notes, duration)
    return "\n".join(out + format_render(rows, duration)) + "\n"


def format_grid_csv(rows) -> str:
    """The `grid` command's CSV (this project's addition): one row per (note, velocity); no figures where the signal is too short."""
    out = ["note,velocity,h_db,m_db,ratio_db,verdict"]
    for r in rows:
        if r["too_short"]:
            out.append("%d,%d,,,," % (r["midi"], r["velocity"]))
        else:
            out.append("%d,%d,%s,%s,%s,%s" % (r["midi"], r["velocity"], _f(r["h_db"], ".2f"), _f(r["m_db"], ".2f"), _f(r["ratio_db"], ".2f"),
                                              VERDICTS[int(r["verdict"])]))
    return "\n".join(out) + "\n"


__all__ = ["MIDI_LO", "MIDI_HI", "VERDICTS", "NOTE_JOB_DTYPE", "PRODUCT_DTYPE", "REPORT_DTYPE", "DETAIL_DTYPE", "ROW_DTYPE", "note_jobs", "risk", "probes",
           "dft_magnitudes", "run_jobs", "audit", "worst_product", "format_static", "format_render", "report", "format_grid_csv", "parse_csv_u8",
           "midi_note_name"]
