"""ctypes loader of the CPU restatement of `preamp-bench render-poly` (tests/c/render_poly_ref.cpp, over the oracle's headers).

tests/native.py has oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that source.  A
second build with -DOW_ORACLE_EXP_PERTURB (the BJT exp() off by one ulp, oracle/ow_chain.hpp) is the sensitivity variant the sample floor is
measured with.  render() returns a Result: the row figures (ROW fields, include/openwurli_hip.h ow_poly_row), final, separate_sum, residual
and the per-voice rows -- the outputs of the voices' OWN chains, i.e. the terms of separate_sum.

Also here, because both the host and the GPU tests use them: the chords the GPU parity test runs (CHORDS), the sample bars of the three
outputs, and the condition that keeps an assertion on intermod_ratio_db honest.
"""
import ctypes as C
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native

ROW = ("peak", "residual_peak", "win_peak", "win_mean_sq", "peak_db", "rms_db", "intermod_ratio_db")
WIN_LO, WIN_HI = 8820, 88200                                                           # main.rs:1516-1517
_VP = C.c_void_p

Result = namedtuple("Result", "row final separate_sum residual voices")
Chord = namedtuple("Chord", "notes velocities duration volume speaker ldr no_poweramp")

# The chords of the GPU parity test (tests/test_gpu_render_poly.py): the command's default chord at its default 3 s, a loud low dyad, a
# chord at the tremolo's bright end (19 kohm: the DC solve at --ldr matters), a --no-poweramp chord and speaker 0 (the speaker's tanh and
# cubic off; quiet, because the power amp's crossover region is where a linear speaker leaves intermodulation).  The shorter ones keep the CPU side of the GPU run short; every window is [8820, min(88200, n)).
CHORDS = {
    "default": Chord((38, 59, 62, 66), (45, 40, 40, 40), 3.0, 0.60, 1.0, 1e6, False),
    "loud_low_dyad": Chord((36, 43), (127, 120), 1.0, 0.90, 1.0, 1e6, False),
    "ldr_19k": Chord((50, 57, 65), (90, 80, 70), 1.0, 0.60, 1.0, 19_000.0, False),
    "no_poweramp": Chord((45, 64, 83), (100, 60, 110), 1.0, 0.60, 1.0, 1e6, True),
    "speaker_0": Chord((40, 52, 71, 90), (80, 80, 80, 80), 1.0, 0.40, 0.0, 120_000.0, False),
}
# The absolute floor F of the sample bars.  The one-ulp-exp experiment on these chords (restatement against its perturbed build,
# oracle_binding.floor_governed_delta of `final`) moves the floor-governed samples by up to 9.3e-9 (the loud low dyad; 5.3e-9 on the
# default chord); ABS_FLOOR_BATCH (3e-8) is above 2.5 x that, so render-poly has its own floor under the project's rule
# F <= FLOOR_RULE x measurement (tests/test_render_poly_host.py asserts it; DESIGN.md section 2 has the row).
ABS_FLOOR_POLY = 2.3e-8


def lib(perturbed=False):
    return native.load("render_poly_ref", "perturbed" if perturbed else "")


def samples(duration):
    return lib().orp_samples(float(duration))


def render(notes, velocities, duration=3.0, volume=0.60, speaker=1.0, ldr=1e6, no_poweramp=False, perturbed=False, audio=True):
    """cmd_render_poly for one chord (velocities already padded to the notes).  audio=False: the row alone (benchmarks)."""
    L = lib(perturbed)
    no = np.ascontiguousarray(notes, dtype=np.uint8)
    ve = np.ascontiguousarray(velocities, dtype=np.uint8)
    assert no.size == ve.size >= 1
    n = L.orp_samples(float(duration))
    row = np.zeros(15)
    fin, sep, res = (np.zeros(n) for _ in range(3)) if audio else (None, None, None)
    vo = np.zeros((no.size, n)) if audio else None
    p = lambda a: a.ctypes.data_as(_VP) if a is not None else None
    got = L.orp_render(int(no.size), p(no), p(ve), float(duration), float(volume), float(speaker), float(ldr), 1 if no_poweramp else 0,
                       p(row), p(fin), p(sep), p(res), p(vo))
    if got == 0:
        raise ValueError("render-poly: %d samples, the measurement window starts at %d (the reference panics)" % (n, WIN_LO))
    d = {"peak": row[0], "residual_peak": row[1], "win_peak": row[2:5].copy(), "win_mean_sq": row[5:8].copy(), "peak_db": row[8:11].copy(),
         "rms_db": row[11:14].copy(), "intermod_ratio_db": row[14]}
    return Result(d, fin, sep, res, vo)


def render_chord(ch, **kw):
    return render(ch.notes, ch.velocities, ch.duration, ch.volume, ch.speaker, ch.ldr, ch.no_poweramp, **kw)


def render_many(chords, threads=16, **kw):
    """Chords on `threads` host threads (ctypes drops the GIL)."""
    chords = list(chords)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(lambda c: render_chord(c, **kw), chords))


# ---- bars (the issue's): final by oracle.parity_report; separate_sum per sample within the SUM over its voices' chains s_k of
# max(1e-5 * max(|s_k|, 1e-3 * peak_k), F) -- errors add; residual within the bar of final plus the bar of separate_sum.
def final_bar(final, floor, rel=1e-5, floor_frac=1e-3):
    final = np.asarray(final)
    return np.maximum(rel * np.maximum(np.abs(final), floor_frac * np.max(np.abs(final))), floor)


def separate_bar(voices, floor, rel=1e-5, floor_frac=1e-3):
    return sum(final_bar(s, floor, rel, floor_frac) for s in np.asarray(voices))


def residual_bar(ref, floor):
    return final_bar(ref.final, floor) + separate_bar(ref.voices, floor)


def window(n):
    return slice(WIN_LO, min(WIN_HI, int(n)))


def ratio_is_assertable(ref, floor, factor=10.0):
    """The restatement's residual RMS over the window is at least `factor` x the RMS of the residual bar there: only then does an
    agreement of intermod_ratio_db say something about the residual and not about the bar."""
    w = window(ref.final.size)
    rms = lambda x: float(np.sqrt(np.mean(np.square(x[w]))))
    return rms(ref.residual) >= factor * rms(residual_bar(ref, floor))
