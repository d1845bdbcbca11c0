"""ctypes loader of the CPU restatement of `preamp-bench gain` / `sweep` / `harmonics` / `tremolo-sweep` (tests/c/preamp_bench_ref.cpp,
over the oracle's headers).

tests/native.py has oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that source.  Every
function returns per point the nine values the restatement computes: gain, gain_db, H1..H5, THD %, H2/H3 dB (MET fields).
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native

N_SAMPLES = 22050
MET = ("gain", "gain_db", "h1", "h2", "h3", "h4", "h5", "thd_pct", "h2_h3_db")
_WARM = set()
_VP = C.c_void_p


def lib():
    return native.load("preamp_bench_ref")


def _p(a):
    return a.ctypes.data_as(_VP) if a is not None else None


def _warm(kind):
    """The oracle builds the melange preamp's settled state lazily in a static: the first call of a kind runs alone."""
    if kind not in _WARM:
        point(kind, 1000.0, 0.001, 1e6, 1e6)
        _WARM.add(kind)


def measure_seq(kind, freqs, amps, r_ldrs, trace=False):
    """cmd_sweep / cmd_tremolo_sweep: measure_gain_at on ONE preamp object, point after point (reset() per point).
    Returns (met [n][9], traces [n][22050] or None)."""
    f = np.ascontiguousarray(freqs, dtype=np.float64)
    a = np.ascontiguousarray(amps, dtype=np.float64)
    r = np.ascontiguousarray(r_ldrs, dtype=np.float64)
    n = f.size
    met = np.zeros((n, 9))
    tr = np.zeros((n, N_SAMPLES)) if trace else None
    _warm(kind)
    lib().opb_measure_seq(int(kind), n, _p(f), _p(a), _p(r), _p(met), _p(tr))
    return met, tr


def harmonics(kind, freq, amp, r_ldr, trace=False):
    """cmd_harmonics: a fresh preamp, set_ldr_resistance, no reset().  Returns (met [9], trace or None)."""
    met = np.zeros(9)
    tr = np.zeros(N_SAMPLES) if trace else None
    _warm(kind)
    lib().opb_harmonics(int(kind), float(freq), float(amp), float(r_ldr), _p(met), _p(tr))
    return met, tr


def point(kind, freq, amp, r_ldr, r_reset, trace=False):
    """One independent point of the device's model (reset() at r_reset, then set_ldr_resistance(r_ldr))."""
    met = np.zeros(9)
    tr = np.zeros(N_SAMPLES) if trace else None
    lib().opb_point(int(kind), float(freq), float(amp), float(r_ldr), float(r_reset), _p(met), _p(tr))
    return met, tr


def points(kind, pts, threads=16):
    """Independent points [(freq, amp, r_ldr, r_reset)] on `threads` host threads (ctypes drops the GIL).  Returns met [n][9]."""
    pts = list(pts)
    met = np.zeros((len(pts), 9))
    _warm(kind)

    def one(i):
        met[i] = point(kind, *pts[i])[0]

    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, range(len(pts))))
    return met
