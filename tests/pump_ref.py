"""ctypes loader of the CPU restatement of the pump measurements (tests/c/pump_ref.cpp, over oracle/ow_melange.hpp).  tests/native.py has
oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that source.

Also here, because the host and the GPU tests share them: the points the GPU tests run, the restatement's own one-ulp movement at those
points (measured by tests/test_pump_host.py, which holds the restatement to 2.5 x these figures), and the device's parity bar.
"""
import ctypes as C
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native
from openwurli_amd import pump

_VP = C.c_void_p

# The restatement's own movement when every non-zero entry of the rebuilt s, k, s_ni moves by one ulp (both polarities), largest
# |trace difference| in volts over the GPU test shapes below.  Measured on the CPU (x86-64, g++ -O2 -ffp-contract=off); the host test
# asserts 2.5 x these.
ULP_MOVE_STATIC = 1.3e-7        # measured here 1.098e-7 (88.2 kHz, 100 kOhm)
ULP_MOVE_SCHEDULE = 7.3e-7      # measured here 7.251e-7 (log-cosine, two cycles)
# Device against restatement: every trace sample, the extra sample, mean, min, max within PUMP_REL x max |reference trace|.  10 x the worst
# ratio measured on an MI355X over the shapes below (4.988e-11: 3.25e-10 V on a 6.5 V trace, 48 kHz, 1 MOhm, with the 5 mV sine; every
# point WITHOUT the sine, schedules included, came out bit-identical to the restatement -- the whole difference is the device's sin against
# the host's), far below 1e-5, the project's parity bar.  DESIGN.md, feature row f10.
PUMP_REL = 5e-10

SETTLE, CAPTURE = 2048, 256
R_NOMINAL = 9.99999999999999854e4


def static_test_points() -> np.ndarray:
    """Rates {48 000, 88 200} x R {1 k, 19 k, 47.5 k, 100 k, 1 M} x amplitude {0, 5 mV at 1 kHz}, one 44 100 Hz point at 19 k, and the
    nominal pot at 48 kHz (no rebuild: codegen tables)."""
    parts = []
    for sr in (48_000.0, 88_200.0):
        for amp in (0.0, 0.005):
            parts.append(pump.static_points(sr, [1_000.0, 19_000.0, 47_500.0, 100_000.0, 1_000_000.0], SETTLE, CAPTURE, amp, 1000.0 if amp else 0.0))
    parts.append(pump.static_points(44_100.0, [19_000.0], SETTLE, CAPTURE))
    parts.append(pump.static_points(48_000.0, [R_NOMINAL], SETTLE, CAPTURE))
    return np.concatenate(parts)


def schedule_test_points() -> np.ndarray:
    """Settle 2 048 and the extra sample everywhere: two steps, a ramp, the log-cosine over one and two cycles of 2 048 samples."""
    ln_hi, ln_lo = math.log(1_000_000.0), math.log(19_000.0)
    logcos = dict(extra_sample=1, schedule=pump.LOGCOS, ln_mid=0.5 * (ln_hi + ln_lo), ln_amp=0.5 * (ln_hi - ln_lo), sched_freq=88_200.0 / 2048.0)
    return np.concatenate([
        pump.make_point(88_200.0, 1_000_000.0, SETTLE, 2048, extra_sample=1, schedule=pump.STEP, r_to=19_000.0),
        pump.make_point(48_000.0, 19_000.0, SETTLE, 2048, extra_sample=1, schedule=pump.STEP, r_to=1_000_000.0),
        pump.make_point(48_000.0, 30_000.0, SETTLE, 1024, extra_sample=1, schedule=pump.RAMP, r_to=70_000.0),
        pump.make_point(88_200.0, 1_000_000.0, SETTLE, 2048, **logcos),
        pump.make_point(88_200.0, 1_000_000.0, SETTLE, 4096, **logcos)])


def placement_points() -> np.ndarray:
    """The points of the placement tests: every static and schedule shape above, cut to 256 settle samples and at most 256 captured ones
    (placement is about which lane, wavefront and chunk a point lands in, not about how long it runs)."""
    p = np.concatenate([static_test_points(), schedule_test_points()])
    p["settle"] = 256
    p["capture"] = np.minimum(p["capture"], 256)
    return p


def lib():
    return native.load("pump_ref")


def run_point(point, polarity=0, trace=True):
    """One POINT_DTYPE record through the restatement: (ROW_DTYPE record, trace f64 [capture] or None)."""
    L = lib()
    p = np.ascontiguousarray(np.asarray(point, dtype=pump.POINT_DTYPE).reshape(1))
    row = np.zeros(1, dtype=pump.ROW_DTYPE)
    tr = np.zeros(int(p[0]["capture"])) if trace else None
    rc = L.opr_run(p.ctypes.data_as(_VP), int(polarity), row.ctypes.data_as(_VP), tr.ctypes.data_as(_VP) if trace else None)
    if rc != 0:
        raise ValueError("the restatement refuses this point's shape")
    return row[0], tr


def run_points(points, polarity=0, trace=True, threads=16):
    """Every point on a host thread of its own (ctypes releases the GIL): (ROW_DTYPE [n], list of traces)."""
    pts = np.asarray(points, dtype=pump.POINT_DTYPE).ravel()
    lib()
    with ThreadPoolExecutor(max_workers=max(1, min(int(threads), 16))) as ex:
        res = list(ex.map(lambda q: run_point(q, polarity, trace), pts))
    rows = np.zeros(pts.size, dtype=pump.ROW_DTYPE)
    for i, (r, _) in enumerate(res):
        rows[i] = r
    return rows, [t for _, t in res]


def trace_stats(buf):
    b = np.ascontiguousarray(buf, dtype=np.float64)
    out = np.zeros(9)
    lib().opr_trace_stats(b.ctypes.data_as(_VP), b.size, out.ctypes.data_as(_VP))
    return {"mean": out[0], "std": out[1], "min": out[2], "max": out[3], "band_rms": list(out[4:9])}


def step_tail(buf):
    b = np.ascontiguousarray(buf, dtype=np.float64)
    out = np.zeros(4)
    lib().opr_step_tail(b.ctypes.data_as(_VP), b.size, out.ctypes.data_as(_VP))
    return {"tail_mean": out[0], "tail_std": out[1], "initial": out[2], "total_swing": out[3]}


def sinusoid_bifurcations(buf) -> int:
    b = np.ascontiguousarray(buf, dtype=np.float64)
    return int(lib().opr_sinusoid_bifurcs(b.ctypes.data_as(_VP), b.size))

