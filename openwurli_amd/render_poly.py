"""Chord intermodulation on the device: host mirror of ``preamp-bench render-poly`` (tools/preamp-bench/src/main.rs:1397-1592) over the
C-ABI (``ow_render_poly``).

The command renders a chord's voices, sends their sum through ONE chain and every voice through a chain of its OWN, and reports the
residual "shared - sum of separate" as the intermodulation level.  On the device every chord of a call -- all dyads of the keyboard, a
chord across volume, velocity and LDR -- runs at once: ``run_chords`` returns one row per chord, ``render_poly`` is the command itself
(report text, WAV files), ``dyad_grid`` / ``format_grid_csv`` the map of ``intermod_ratio_db`` this project adds.
"""
import ctypes as C
import math
import os
import tempfile
from typing import Optional, Sequence

import numpy as np

from .binding import POLY_MAX_NOTES, WAV_ROUND, OwError, OwPolyCfg, OwPolyChord, OwPolyRow, check, load_library, take_error  # noqa: F401

from ._rust_text import BASE_SR, _f, midi_note_name, parse_csv_u8, samples, to_dbfs  # noqa: F401
WIN_LO, WIN_HI = 8820, 88200                                # (0.2 * BASE_SR) / (2.0 * BASE_SR) as usize, main.rs:1516-1517
DEFAULT_NOTES, DEFAULT_VELOCITIES = (38, 59, 62, 66), (45, 40, 40, 40)      # main.rs:1398-1399

# numpy views of include/openwurli_hip.h ow_poly_chord / ow_poly_row
CHORD_DTYPE = np.dtype(OwPolyChord)
ROW_DTYPE = np.dtype(OwPolyRow)


def pad_velocities(notes: Sequence[int], velocities_raw: Sequence[int]) -> list:
    """main.rs:1410-1420: one velocity per note; missing ones repeat the last given, 80 when none was given; extra ones are dropped."""
    raw = list(velocities_raw)
    return [raw[i] if i < len(raw) else (raw[-1] if raw else 80) for i in range(len(notes))]


def make_chord(notes, velocities=(), volume=0.60, speaker=1.0, ldr=1_000_000.0, no_poweramp=False) -> np.ndarray:
    """One CHORD_DTYPE record; the velocities are padded to the notes by the command's rule."""
    notes = [int(x) for x in notes]
    if not 1 <= len(notes) <= POLY_MAX_NOTES:
        raise ValueError("a chord has 1..%d notes, got %d" % (POLY_MAX_NOTES, len(notes)))
    c = np.zeros(1, dtype=CHORD_DTYPE)
    c["n_notes"], c["no_poweramp"] = len(notes), 1 if no_poweramp else 0
    c["notes"][0, :len(notes)] = notes
    c["velocities"][0, :len(notes)] = pad_velocities(notes, [int(v) for v in velocities])
    c["volume"], c["speaker"], c["r_ldr"] = volume, speaker, ldr
    return c


def make_chords(chords) -> np.ndarray:
    """CHORD_DTYPE array from CHORD_DTYPE records, dicts (make_chord's keywords) or (notes, velocities[, volume, speaker, ldr, no_poweramp])."""
    if isinstance(chords, np.ndarray) and chords.dtype == CHORD_DTYPE:
        return np.ascontiguousarray(chords).ravel()
    out = [make_chord(**c) if isinstance(c, dict) else (c.reshape(1) if isinstance(c, (np.ndarray, np.void)) else make_chord(*c)) for c in chords]
    return np.concatenate(out) if out else np.zeros(0, dtype=CHORD_DTYPE)


def run_chords(chords, duration=3.0, device=0, final=False, separate_sum=False, residual=False, preamp_kind=0, power_amp_kind=0):
    """``ow_render_poly``: a ROW_DTYPE array, one row per chord.  With any of final / separate_sum / residual set, returns
    (rows, {"final": f64 [n_chords][n], ...}) with the audio that was asked for."""
    L = load_library()
    ch = make_chords(chords)
    rows = np.zeros(ch.size, dtype=ROW_DTYPE)
    n = samples(duration)
    want = (("final", final), ("separate_sum", separate_sum), ("residual", residual))
    audio = {k: np.zeros((ch.size, n)) for k, w in want if w}
    ptr = lambda k: audio[k].ctypes.data_as(C.c_void_p) if k in audio else None
    cfg = OwPolyCfg(float(duration), int(device), int(preamp_kind), int(power_amp_kind))
    check(L, L.ow_render_poly(ch.ctypes.data_as(C.c_void_p), ch.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p), ptr("final"), ptr("separate_sum"),
                              ptr("residual"), n))
    return (rows, audio) if audio else rows


def wav_scales(peak: float, residual_peak: float, normalize: bool):
    """The two factors write_wav_24bit gets (main.rs:1533-1549): --normalize brings a peak above 0.7 down to 0.7; the residual is always
    brought to 0.5 (unless it is below 1e-10)."""
    scale = (0.7 / peak if peak > 0.7 else 1.0) if normalize else 1.0
    return scale, (0.5 / residual_peak if residual_peak > 1e-10 else 1.0)


def residual_path(output: str) -> str:
    """main.rs:1542: output_path.replace(".wav", "_residual.wav") -- every occurrence, as str::replace does."""
    return output.replace(".wav", "_residual.wav")


def default_output() -> str:
    """temp_default("preamp_render_poly.wav"), main.rs:123-128, 1406."""
    return os.path.join(tempfile.gettempdir(), "preamp_render_poly.wav")


def verdict(ratio_db: float) -> str:
    """main.rs:1579-1587."""
    if ratio_db > 60.0:
        return "CLEAN — intermod negligible"
    if ratio_db > 40.0:
        return "OK — intermod present but likely inaudible"
    if ratio_db > 20.0:
        return "MARGINAL — intermod may be audible on revealing systems"
    return "DIRTY — intermod clearly audible"


def format_report(notes, velocities, duration, volume, speaker, row, output, residual_output=None) -> str:
    """The command's stdout (main.rs:1552-1591).  `velocities` as given on the command line (padded here); `row` a ROW_DTYPE row.
    Rust's {:.N} rounds the exact binary value half to even, as Python's %-format does; {:?} of a Vec<String> quotes each item."""
    notes = [int(n) for n in notes]
    vel = pad_velocities(notes, [int(v) for v in velocities])
    pk, rms = [float(x) for x in row["peak_db"]], [float(x) for x in row["rms_db"]]
    ratio = rms[0] - rms[2]
    res_out = residual_path(output) if residual_output is None else residual_output
    return "\n".join([
        "Polyphonic render complete",
        "  Notes:     [%s]" % ", ".join('"%s (%d)"' % (midi_note_name(n), n) for n in notes),
        "  Velocities: [%s]" % ", ".join(str(v) for v in vel),
        f"  Duration:  {_f(duration, '.1f')}s",
        f"  Volume:    {_f(volume, '.3f')} (audio taper: {_f(float(volume) * float(volume), '.3f')})",
        f"  Speaker:   {_f(speaker, '.1f')}",
        f"  Peak:      {_f(to_dbfs(float(row['peak'])), '.1f')} dBFS",
        "",
        "  === INTERMOD ANALYSIS (0.2-2.0s window) ===",
        f"  Shared chain (poly):  peak={_f(pk[0], '.1f')} dBFS  rms={_f(rms[0], '.1f')} dBFS",
        f"  Separate chains (sum): peak={_f(pk[1], '.1f')} dBFS  rms={_f(rms[1], '.1f')} dBFS",
        f"  Residual (intermod):  peak={_f(pk[2], '.1f')} dBFS  rms={_f(rms[2], '.1f')} dBFS",
        f"  Intermod ratio:       {_f(ratio, '.1f')} dB below signal",
        "",
        f"  Verdict: {verdict(ratio)}",
        "",
        f"  Output:    {output}",
        f"  Residual:  {res_out} (normalized for listening)",
    ]) + "\n"


def write_wavs(output: str, final, residual, peak: float, residual_peak: float, normalize: bool):
    """X.wav and X_residual.wav as the command writes them (24-bit mono, write_wav_24bit's rounding), through ow_wav24_write."""
    L = load_library()
    scale, res_scale = wav_scales(float(peak), float(residual_peak), normalize)
    for path, sig, sc in ((output, final, scale), (residual_path(output), residual, res_scale)):
        sig = np.ascontiguousarray(sig, dtype=np.float64)
        check(L, L.ow_wav24_write(path.encode(), sig.ctypes.data_as(C.c_void_p), sig.size, int(BASE_SR), float(sc), WAV_ROUND))
    return scale, res_scale


def render_poly(notes=DEFAULT_NOTES, velocities=DEFAULT_VELOCITIES, duration=3.0, volume=0.60, speaker=1.0, ldr=1_000_000.0, no_poweramp=False,
                normalize=False, output: Optional[str] = None, device=0) -> dict:
    """cmd_render_poly for one chord: {"row", "final", "separate_sum", "residual", "report", "output", "residual_output"}.  With `output`
    set the two WAV files are written; the report names `output` (or the command's default path when none is written)."""
    rows, audio = run_chords(make_chord(notes, velocities, volume, speaker, ldr, no_poweramp), duration, device, True, True, True)
    row = rows[0]
    out = {"row": row, "final": audio["final"][0], "separate_sum": audio["separate_sum"][0], "residual": audio["residual"][0],
           "output": output, "residual_output": residual_path(output) if output else None}
    if output:
        write_wavs(output, out["final"], out["residual"], row["peak"], row["residual_peak"], normalize)
    out["report"] = format_report(notes, velocities, duration, volume, speaker, row, output or default_output())
    return out


def dyad_grid(lo=33, hi=96, velocities=(80, 80), volume=0.60, speaker=1.0, ldr=1_000_000.0, no_poweramp=False) -> np.ndarray:
    """Every dyad (a < b) of the notes lo..hi at the given velocity pair: CHORD_DTYPE array, a outer."""
    pairs = [(a, b) for a in range(int(lo), int(hi) + 1) for b in range(a + 1, int(hi) + 1)]
    return make_chords([((a, b), velocities, volume, speaker, ldr, no_poweramp) for a, b in pairs])


def format_grid_csv(chords: np.ndarray, rows: np.ndarray) -> str:
    """The `grid` command's CSV (this project's addition): note_a,note_b,vel_a,vel_b,intermod_ratio_db with {:.2} for the ratio."""
    out = ["note_a,note_b,vel_a,vel_b,intermod_ratio_db"]
    for c, r in zip(chords, rows):
        out.append("%d,%d,%d,%d,%s" % (c["notes"][0], c["notes"][1], c["velocities"][0], c["velocities"][1], _f(r["intermod_ratio_db"], ".2f")))
    return "\n".join(out) + "\n"


__all__ = ["CHORD_DTYPE", "ROW_DTYPE", "pad_velocities", "parse_csv_u8", "midi_note_name", "make_chord", "make_chords", "samples", "run_chords",
           "wav_scales", "residual_path", "default_output", "to_dbfs", "verdict", "format_report", "write_wavs", "render_poly", "dyad_grid",
           "format_grid_csv"]
