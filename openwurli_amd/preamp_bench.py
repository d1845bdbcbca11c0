"""Preamp measurements on the device: host mirror of ``preamp-bench gain`` / ``sweep`` / ``harmonics`` / ``tremolo-sweep``
(tools/preamp-bench/src/main.rs:150-369) over the C-ABI (``ow_preamp_measure``).  Every point of a call -- a whole sweep, or a
frequency x LDR response surface -- runs in one library call.

Each command builds exactly the point sequence its CLI command runs.  ``sweep`` and ``tremolo-sweep`` reuse ONE preamp object and
``reset()`` it per point, and the legacy preamp's reset() solves DC at the previous point's resistance (dk_preamp_legacy.rs:628-640): the
``r_reset`` of a point carries that, so the points are independent on the device and still give the reference's numbers.
"""
import ctypes as C
import math
from typing import List, Sequence

import numpy as np

from .binding import PBENCH_SAMPLES, OwError, OwPreampMeasureCfg, OwPreampMeasureRow, OwPreampPoint, check, load_library, take_error  # noqa: F401

from ._rust_text import BASE_SR, _f  # noqa: F401
PREAMP_LEGACY8, PREAMP_MELANGE12 = 0, 1
R_NEW = 1_000_000.0                                         # the r_ldr DkPreamp::new() solves DC at (dk_preamp_legacy.rs:269-366)

# numpy views of include/openwurli_hip.h ow_preamp_point / ow_preamp_measure_row
POINT_DTYPE = np.dtype(OwPreampPoint)
ROW_DTYPE = np.dtype(OwPreampMeasureRow)


def log_spaced(lo: float, hi: float, n: int) -> List[float]:
    """cmd_sweep / cmd_tremolo_sweep's spacing (main.rs:229-235, 342-344), in the reference's order of operations:
    exp(ln(lo) + frac * (ln(hi) - ln(lo))), frac = i / max(n - 1, 1)."""
    a, b = math.log(lo), math.log(hi)
    return [math.exp(a + (i / max(n - 1, 1)) * (b - a)) for i in range(n)]


def reset_chain(r_ldrs: Sequence[float], r_start: float = R_NEW) -> List[float]:
    """r_reset of each point of ONE preamp object that measure_gain_at visits in order: reset() solves DC at the r_ldr the object holds,
    which set_ldr_resistance moved to max(r, 1 kohm) unless that is within 0.01 ohm of it (dk_preamp_legacy.rs:620-626).  The object
    starts from new(), i.e. 1 Mohm."""
    out, state = [], float(r_start)
    for r in r_ldrs:
        out.append(state)
        new_r = max(float(r), 1000.0)
        if abs(new_r - state) > 0.01:
            state = new_r
    return out


def make_points(freqs, amplitudes, r_ldrs, r_resets) -> np.ndarray:
    """One ow_preamp_point per (freq, amplitude, r_ldr, r_reset) (four sequences of equal length, or scalars)."""
    f, a, r, q = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (freqs, amplitudes, r_ldrs, r_resets)))
    p = np.zeros(f.size, dtype=POINT_DTYPE)
    p["freq_hz"], p["amplitude"], p["r_ldr"], p["r_reset"] = f.ravel(), a.ravel(), r.ravel(), q.ravel()
    return p


def gain_points(freq=1000.0, amplitude=0.001, r_ldr=1_000_000.0) -> np.ndarray:
    """cmd_gain (main.rs:192-215): a fresh preamp, reset(), set_ldr_resistance -- the DC solve runs at new()'s 1 Mohm."""
    return make_points([freq], [amplitude], [r_ldr], [R_NEW])


def sweep_points(start=20.0, end=20000.0, points=50, r_ldr=1_000_000.0, amplitude=0.001) -> np.ndarray:
    """cmd_sweep (main.rs:217-254): log-spaced frequencies on one preamp object."""
    fr = log_spaced(start, end, int(points))
    rr = [float(r_ldr)] * len(fr)
    return make_points(fr, [amplitude] * len(fr), rr, reset_chain(rr))


def harmonics_points(freq=440.0, amplitude=0.005, r_ldr=1_000_000.0) -> np.ndarray:
    """cmd_harmonics (main.rs:256-323): a fresh preamp, set_ldr_resistance, no reset() -- new()'s state, the DC solve at 1 Mohm."""
    return make_points([freq], [amplitude], [r_ldr], [R_NEW])


def tremolo_sweep_points(ldr_min=19_000.0, ldr_max=1_000_000.0, steps=20, freq=1000.0, amplitude=0.001) -> np.ndarray:
    """cmd_tremolo_sweep (main.rs:325-368): log-spaced LDR resistances on one preamp object, so point i starts from the DC state of
    point i-1's resistance."""
    rr = log_spaced(ldr_min, ldr_max, int(steps))
    return make_points([freq] * len(rr), [amplitude] * len(rr), rr, reset_chain(rr))


def surface_points(freqs: Sequence[float], r_ldrs: Sequence[float], amplitude=0.001) -> np.ndarray:
    """response_surface's grid, R outer: row k is `sweep --ldr r_ldrs[k]` over `freqs` (its own preamp object, its own reset chain)."""
    out = []
    for r in r_ldrs:
        rr = [float(r)] * len(freqs)
        out.append(make_points(list(freqs), [amplitude] * len(rr), rr, reset_chain(rr)))
    return np.concatenate(out) if out else np.zeros(0, dtype=POINT_DTYPE)


def run_points(points: np.ndarray, preamp_kind=PREAMP_LEGACY8, device=0, trace=False):
    """``ow_preamp_measure`` on a POINT_DTYPE array: a ROW_DTYPE array (and, with trace, the f64 [n][22050] base-rate preamp output)."""
    L = load_library()
    pts = np.ascontiguousarray(points, dtype=POINT_DTYPE)
    rows = np.zeros(pts.size, dtype=ROW_DTYPE)
    tr = np.zeros((pts.size, PBENCH_SAMPLES)) if trace else None
    cfg = OwPreampMeasureCfg(int(device), int(preamp_kind))
    check(L, L.ow_preamp_measure(pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p),
                                 tr.ctypes.data_as(C.c_void_p) if tr is not None else None, PBENCH_SAMPLES))
    return (rows, tr) if trace else rows


def measure_gain(freq=1000.0, amplitude=0.001, r_ldr=1_000_000.0, preamp_kind=PREAMP_LEGACY8, device=0):
    """cmd_gain: one ROW_DTYPE row."""
    return run_points(gain_points(freq, amplitude, r_ldr), preamp_kind, device)[0]


def sweep(start=20.0, end=20000.0, points=50, r_ldr=1_000_000.0, amplitude=0.001, preamp_kind=PREAMP_LEGACY8, device=0):
    """cmd_sweep: ROW_DTYPE rows (freq_hz, gain_db are the CSV's columns)."""
    return run_points(sweep_points(start, end, points, r_ldr, amplitude), preamp_kind, device)


def harmonics(freq=440.0, amplitude=0.005, r_ldr=1_000_000.0, preamp_kind=PREAMP_LEGACY8, device=0):
    """cmd_harmonics: one ROW_DTYPE row (h, thd_pct, h2_h3_db)."""
    return run_points(harmonics_points(freq, amplitude, r_ldr), preamp_kind, device)[0]


def tremolo_sweep(ldr_min=19_000.0, ldr_max=1_000_000.0, steps=20, freq=1000.0, amplitude=0.001, preamp_kind=PREAMP_LEGACY8, device=0):
    """cmd_tremolo_sweep: ROW_DTYPE rows (r_ldr, gain_db are the CSV's columns)."""
    return run_points(tremolo_sweep_points(ldr_min, ldr_max, steps, freq, amplitude), preamp_kind, device)


def response_surface(freqs: Sequence[float], r_ldrs: Sequence[float], amplitude=0.001, preamp_kind=PREAMP_LEGACY8, device=0) -> np.ndarray:
    """Gain in dB over the frequency x LDR plane, [len(r_ldrs)][len(freqs)], in ONE device call.

    Row k is by definition what ``preamp-bench sweep --ldr r_ldrs[k]`` would return over these frequencies (in this order): one preamp
    object per row, reset() per point, so with the legacy preamp the first point of a row starts from new()'s 1 Mohm DC state and the
    others from that of r_ldrs[k].  Every cell can thus be checked against the reference's own command."""
    rows = run_points(surface_points(freqs, r_ldrs, amplitude), preamp_kind, device)
    return rows["gain_db"].reshape(len(r_ldrs), len(freqs))


# ---- the reference's text (main.rs:192-368), numbers through _f
def target_db(r_ldr: float) -> float:                       # main.rs:201
    return 6.0 if r_ldr > 500_000.0 else 12.1


def format_gain(row) -> str:
    """cmd_gain's report (main.rs:198-214)."""
    freq, amp, r, gain, gdb = (float(row[k]) for k in ("freq_hz", "amplitude", "r_ldr", "gain", "gain_db"))
    t = target_db(r)
    return ("Preamp gain measurement\n"
            f"  Frequency:   {_f(freq, '.0f')} Hz\n"
            f"  Amplitude:   {_f(amp, '.6f')} V\n"
            f"  LDR path:    {_f(r, '.0f')} Ω\n"
            f"  Gain:        {_f(gain, '.3f')}x ({_f(gdb, '.2f')} dB)\n"
            f"  SPICE target: {_f(t, '.1f')} dB\n"
            f"  Delta:       {_f(gdb - t, '+.2f')} dB\n")


def format_sweep_csv(rows) -> str:
    """cmd_sweep's CSV (main.rs:227, 241, 245): freq_hz,gain_db with {:.1},{:.2}."""
    return "\n".join(["freq_hz,gain_db"] + [f"{_f(float(f), '.1f')},{_f(float(g), '.2f')}" for f, g in zip(rows["freq_hz"], rows["gain_db"])]) + "\n"


def format_sweep(rows, r_ldr=1_000_000.0) -> str:
    """cmd_sweep's table (main.rs:229-242)."""
    out = [f"Frequency response sweep (LDR = {_f(float(r_ldr), '.0f')} Ω)", "%10s  %10s" % ("Freq (Hz)", "Gain (dB)"), "-" * 10 + "  " + "-" * 10]
    out += [f"{_f(float(f), '10.1f')}  {_f(float(g), '10.2f')}" for f, g in zip(rows["freq_hz"], rows["gain_db"])]
    return "\n".join(out) + "\n"


def format_tremolo_sweep_csv(rows) -> str:
    """cmd_tremolo_sweep's CSV (main.rs:338, 354, 364): ldr_ohm,gain_db with {:.0},{:.2}."""
    return "\n".join(["ldr_ohm,gain_db"] + [f"{_f(float(r), '.0f')},{_f(float(g), '.2f')}" for r, g in zip(rows["r_ldr"], rows["gain_db"])]) + "\n"


def format_tremolo_sweep(rows) -> str:
    """cmd_tremolo_sweep's table and its SPICE-target footer (main.rs:340-362)."""
    out = ["Tremolo sweep (gain vs LDR path resistance)", "%12s  %10s" % ("LDR (Ω)", "Gain (dB)"), "-" * 12 + "  " + "-" * 10]
    out += [f"{_f(float(r), '12.0f')}  {_f(float(g), '10.2f')}" for r, g in zip(rows["r_ldr"], rows["gain_db"])]
    out += ["", "SPICE targets:", "  R_ldr = 1M  (no trem):     6.0 dB", "  R_ldr = 19K (trem bright): 12.1 dB", "  Range:                      6.1 dB"]
    return "\n".join(out) + "\n"


def format_surface_csv(freqs, r_ldrs, gain_db) -> str:
    """The `surface` command's CSV (this project's addition): ldr_ohm,freq_hz,gain_db with {:.0},{:.1},{:.2}, R outer."""
    out = ["ldr_ohm,freq_hz,gain_db"]
    for k, r in enumerate(r_ldrs):
        out += [f"{_f(float(r), '.0f')},{_f(float(f), '.1f')},{_f(float(g), '.2f')}" for f, g in zip(freqs, gain_db[k])]
    return "\n".join(out) + "\n"


def format_harmonics(row) -> str:
    """cmd_harmonics' report (main.rs:300-322)."""
    freq, amp, r = float(row["freq_hz"]), float(row["amplitude"]), float(row["r_ldr"])
    h = [float(x) for x in row["h"]]
    with np.errstate(all="ignore"):                         # IEEE results, as the reference's f64 arithmetic gives them
        rel = [float(20.0 * np.log10(np.float64(x) / np.float64(h[0]))) for x in h]
    out = ["Harmonic analysis", f"  Frequency:   {_f(freq, '.0f')} Hz", f"  Amplitude:   {_f(amp, '.6f')} V", f"  LDR path:    {_f(r, '.0f')} Ω", "",
           f"  H1 (fund):   {_f(h[0], '.6f')}"]
    for k in range(1, 5):
        out.append(f"  H{k + 1}:          {_f(h[k], '.6f')}  ({_f(rel[k], '.1f')} dB rel)")
    out += ["", f"  THD:         {_f(float(row['thd_pct']), '.4f')}%",
            f"  H2/H3:       {_f(float(row['h2_h3_db']), '.1f')} dB  (target: H2 > H3, i.e. > 0 dB)"]
    return "\n".join(out) + "\n"


__all__ = ["POINT_DTYPE", "ROW_DTYPE", "log_spaced", "reset_chain", "make_points", "gain_points", "sweep_points", "harmonics_points",
           "tremolo_sweep_points", "surface_points", "run_points", "measure_gain", "sweep", "harmonics", "tremolo_sweep", "response_surface",
           "target_db", "format_gain", "format_sweep", "format_sweep_csv", "format_tremolo_sweep", "format_tremolo_sweep_csv",
           "format_harmonics", "format_surface_csv"]
