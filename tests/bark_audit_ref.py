"""ctypes loader of the CPU restatement of `preamp-bench bark-audit` (tests/c/bark_audit_ref.cpp, over the oracle's headers).
tests/native.py has oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that source.  A
second build with -DOW_ORACLE_VOICE_PERTURB (the voice's library calls off by one ulp, oracle/ow_voice.hpp) is the sensitivity variant.

Also here, because the host and the GPU tests share them: the jobs the GPU tests run, the bars, and the report's text built from the
restatement's numbers.

The bars are derived, not chosen.  A stage's row is known to +- tol_i per sample, the tolerance oracle.parity_report applies to it
(max(1e-5 x max(|x_i|, 1e-3 x peak), the stage's absolute floor)).  A peak then moves by at most max tol_i over the window;
dft_magnitude = (2 / n) |sum x_i e^(-j phase_i)| by at most B = (2 / n) sum tol_i -- it is linear in the samples, the triangle
inequality is the whole bound; a ratio h2 / h1 by ratio x (B / h1 + B / h2) to first order, SECOND_ORDER x that as the bar.  The analysis
(the device's lane-strided sums and its sin / cos against the serial host loop) adds B_a = analysis_cap(n) x (2 / n) sum |x_i|, the
a-priori bound of an n-term sum: a magnitude's bar is B + B_a, a ratio's gains ratio x (B_a / h1 + B_a / h2).
"""
import ctypes as C
import math
import threading
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native
from note_audit_ref import analysis_cap, clear_of_rounding  # noqa: F401  (one definition of each for the audits)

BASE_SR = 44100.0
SECOND_ORDER = 1.5
PARITY_REL, PARITY_FLOOR_FRAC = 1e-5, 1e-3      # oracle_binding.parity_report's defaults
_LOCK = threading.Lock()
_WARM = set()
_VP = C.c_void_p

FIELDS = ("fundamental_hz", "displacement_scale", "reed_peak", "y_peak", "pu_peak", "pu_h1", "pu_h2", "pu_h2_h1", "pre_h1", "pre_h2", "pre_h2_h1")
Row = namedtuple("Row", FIELDS)
Run = namedtuple("Run", "row taps n m0")
STAGES = ("reed", "pickup", "preamp")

# The sizes of the GPU tests: the command's own, and a tenth of it -- 2 205 samples, a remainder against every chunk size of the kernels
# (16, 24, 64), a window of 1 103
DEFAULT_SIZE = (0.5, 0.25)
SHORT_SIZE = (0.05, 0.025)
# taps: the keyboard's ends and middle at ff, one soft note
TAP_JOBS = ((33, 127), (60, 127), (96, 127), (72, 40))
# report text: jobs whose printed figures lie clear of a rounding boundary by their bars (tests/test_bark_audit_host.py asserts it on the
# CPU for the legacy preamp; a job that does not is swapped for a neighbouring note or velocity, the bar is never loosened)
# (at ff the pickup peak reaches hundreds of mV: its bar of 1e-5 x peak is then as wide as the 0.01 mV the command prints, and no such job
# can be clear -- hence the softer velocities in the loud registers)
TEXT_JOBS = {DEFAULT_SIZE: ((33, 127), (48, 100), (60, 40), (72, 127), (84, 80), (96, 127)),
             SHORT_SIZE: ((33, 100), (48, 40), (60, 100), (72, 80), (84, 100), (96, 100))}


def lib(perturbed=False):
    return native.load("bark_audit_ref", "voice_perturbed" if perturbed else "")


def samples(seconds):
    return lib().obr_samples(float(seconds))


def dft_magnitude(signal, freq, sr=BASE_SR):
    s = np.ascontiguousarray(signal, dtype=np.float64)
    return lib().obr_dft_magnitude(s.ctypes.data_as(_VP), s.size, float(freq), float(sr))


# ---- the restatement's runs, computed once per process and shared by the tests (never modified) -----------------------------------
_RUNS = {}


def run(note, velocity, size=DEFAULT_SIZE, kind=0, perturbed=False):
    """One (note, velocity) of the command: Run(row, taps [3][n] read-only, n, m0)."""
    key = (int(note), int(velocity), float(size[0]), float(size[1]), int(kind), bool(perturbed))
    with _LOCK:
        got = _RUNS.get(key)
    if got is None:
        L = lib(perturbed)
        n, m0 = L.obr_samples(float(size[0])), L.obr_samples(float(size[1]))
        assert 0 <= m0 < n
        row, taps = np.zeros(11), np.zeros((3, n))
        assert L.obr_run(key[0], key[1], key[2], key[3], key[4], row.ctypes.data_as(_VP), taps.ctypes.data_as(_VP)) == n
        taps.setflags(write=False)
        got = Run(Row(*[float(v) for v in row]), taps, n, m0)
        with _LOCK:
            _RUNS[key] = got
    return got


def run_many(jobs, size=DEFAULT_SIZE, kind=0, threads=16):
    """[Run] of (note, velocity) jobs on `threads` host threads (ctypes drops the GIL); the first run of a solver kind goes alone, so the
    oracle's lazily settled states are built once."""
    jobs = list(jobs)
    if kind not in _WARM and jobs:
        run(jobs[0][0], jobs[0][1], size, kind)
        _WARM.add(kind)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(lambda j: run(j[0], j[1], size, kind), jobs))


# ---- bars ---------------------------------------------------------------------------------------------------------------------------
def sample_tol(cpu_row, abs_floor):
    """oracle.parity_report's tolerance of every sample of a row."""
    cpu = np.abs(np.asarray(cpu_row, dtype=np.float64))
    peak = float(cpu.max()) if cpu.size else 0.0
    return np.maximum(PARITY_REL * np.maximum(cpu, PARITY_FLOOR_FRAC * peak), abs_floor)


def stage_floors(oracle, kind):
    """The absolute floors tests/test_gpu_calibrate.py applies to the same stages: reed, pickup, preamp."""
    return (oracle.ABS_FLOOR_BATCH, oracle.ABS_FLOOR_BATCH, oracle.ABS_FLOOR_MELANGE_PREAMP if kind else oracle.ABS_FLOOR_BATCH)


def magnitude_bars(window, tol_window):
    """(B, B_a) of a dft_magnitude over `window` whose samples are known to +- tol_window."""
    n = window.size
    return 2.0 / n * float(np.sum(tol_window)), analysis_cap(n) * 2.0 / n * float(np.sum(np.abs(window)))


def ratio_bar(ratio, h1, h2, B, Ba):
    if not (h1 > 1e-15 and h2 > 0.0):
        return math.inf
    return SECOND_ORDER * ratio * (B / h1 + B / h2) + ratio * (Ba / h1 + Ba / h2)


def bars(r, floors):
    """Row of bars for a Run: peaks by max tol_i, magnitudes by B + B_a, ratios by ratio_bar.  fundamental_hz and
    displacement_scale are host scalars (1e-12 relative, as the calibration sweep's)."""
    w = slice(r.m0, r.n)
    tol = [sample_tol(r.taps[k], floors[k])[w] for k in range(3)]
    reed_b = float(tol[0].max())
    ds = r.row.displacement_scale
    Bp, Bap = magnitude_bars(r.taps[1][w], tol[1])
    Bq, Baq = magnitude_bars(r.taps[2][w], tol[2])
    return Row(1e-12 * r.row.fundamental_hz, 1e-12 * ds, reed_b, reed_b * ds + 1e-12 * abs(r.row.y_peak), float(tol[1].max()),
               Bp + Bap, Bp + Bap, ratio_bar(r.row.pu_h2_h1, r.row.pu_h1, r.row.pu_h2, Bp, Bap),
               Bq + Baq, Bq + Baq, ratio_bar(r.row.pre_h2_h1, r.row.pre_h1, r.row.pre_h2, Bq, Baq))


# the figures the command prints: (row field, factor, decimals)
PRINTED = (("reed_peak", 1.0, 4), ("y_peak", 1.0, 4), ("pu_h2_h1", 100.0, 1), ("pu_peak", 1000.0, 2), ("pre_h2_h1", 100.0, 1))


def text_is_clear(r, b):
    """Every printed figure of the Run lies further than its bar from the nearest rounding boundary of its format."""
    return all(clear_of_rounding(getattr(r.row, f) * k, getattr(b, f) * k, d) for f, k, d in PRINTED)


def record(note, velocity, r):
    """The restatement's row as the package's formatter reads it."""
    d = r.row._asdict()
    d.update(note=note, velocity=velocity)
    return d
