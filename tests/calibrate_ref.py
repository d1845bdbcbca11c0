"""ctypes loader of the CPU restatement of `preamp-bench calibrate` (tests/c/calibrate_ref.cpp, over the oracle's headers).

tests/native.py has oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that source.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native

N_SAMPLES = 22050
_WARM = set()


def lib():
    return native.load("calibrate_ref")


def cfg6(cfg):
    return (C.c_double * 6)(cfg.ds_at_c4, cfg.ds_exponent, cfg.ds_clamp[0], cfg.ds_clamp[1], cfg.target_db, cfg.voicing_slope)


def run_point(note, vel, cfg, volume, speaker, preamp_kind=0, power_amp_kind=0, taps=False):
    """(row18 as a numpy array, taps [5][22050] or None) of one grid point."""
    L = lib()
    row = np.zeros(18)
    tp = np.zeros((5, N_SAMPLES)) if taps else None
    L.ocal_run_point(int(note), int(vel), cfg6(cfg), 1 if cfg.zero_trim else 0, float(volume), float(speaker), int(preamp_kind), int(power_amp_kind),
                     row.ctypes.data_as(C.c_void_p), tp.ctypes.data_as(C.c_void_p) if tp is not None else None)
    return row, tp


def run_points(points, volume, speaker, preamp_kind=0, power_amp_kind=0, taps_for=(), threads=16):
    """points: [(note, velocity, CalibrationConfig)].  Returns (rows [n][18], {index: taps}).  The calls run on `threads` host threads
    (ctypes drops the GIL); the first point of each solver kind runs alone, so the oracle's lazily settled states are built once."""
    lib()
    kind = (preamp_kind, power_amp_kind)
    pts = list(points)
    rows = np.zeros((len(pts), 18))
    taps = {}
    taps_for = set(taps_for)

    def one(i):
        n, v, c = pts[i]
        r, t = run_point(n, v, c, volume, speaker, preamp_kind, power_amp_kind, taps=i in taps_for)
        rows[i] = r
        if t is not None:
            taps[i] = t

    start = 0
    if kind not in _WARM and pts:
        one(0)
        _WARM.add(kind)
        start = 1
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, range(start, len(pts))))
    return rows, taps
