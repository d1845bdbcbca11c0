"""ctypes loader of the CPU restatement of `preamp-bench centroid-track` (tests/c/centroid_track_ref.cpp, over the oracle's headers).

tests/native.py has oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that source.  A
second build with -DOW_ORACLE_EXP_PERTURB (the BJT exp() off by one ulp, oracle/ow_chain.hpp) is the sensitivity variant.

Also here, because both the host and the GPU tests use them: the jobs the GPU parity test runs (JOBS), and the bars.

The centroid bar is derived, not chosen.  A frame with spectrum X_k (bins k_min..k_max at f_k), power P_k = |X_k|^2 and centroid
c = sum f_k P_k / sum P_k moves, to first order, by  dc = sum (f_k - c) dP_k / sum P_k  with  dP_k = 2 Re(conj(X_k) dX_k)  and
|dX_k| <= sum_i hann_i |dx_i| <= B = sum_i hann_i b_i  when sample i is known to +- b_i.  Hence

    |dc| <= 2 B sum_k |f_k - c| |X_k| / sum_k |X_k|^2                                                       (frame_bounds)

with b_i the batch path's sample bars (oracle.parity_report's, ABS_FLOOR_BATCH).  The end-to-end bar of a frame is 1.5 x that bound (the
factor covers the second-order terms) plus the analysis bar ANALYSIS_REL x c, which covers the device's sin / cos against the host's.
"""
import ctypes as C
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native

BASE_SR = 44100.0
_VP, _Z = C.c_void_p, C.c_size_t

Job = namedtuple("Job", "note velocity volume speaker ldr no_preamp no_poweramp displacement_scale")
Job.__new__.__defaults__ = (0.60, 1.0, 1e6, False, False, None)
Result = namedtuple("Result", "audio frames spectra times window hop end k_min k_max")

# The jobs of the GPU parity test (tests/test_gpu_centroid_track.py), all at DURATION / END_MS so that the serial chain stays short: the
# command's default note at velocity 100, a bass and a treble note at ff (with the default note: the three target registers), a job at
# the tremolo's bright end (19 kohm: the DC solve at --ldr matters), --no-preamp, --no-poweramp with speaker 0, a displacement scale.
DURATION, END_MS = 0.35, 320.0
JOBS = {
    "default": Job(60, 100),
    "bass_ff": Job(40, 127),
    "treble_ff": Job(84, 127),
    "ldr_19k": Job(57, 90, ldr=19_000.0),
    "no_preamp": Job(64, 110, no_preamp=True),
    "no_poweramp_speaker_0": Job(45, 100, speaker=0.0, no_poweramp=True),
    "displacement_scale": Job(72, 110, displacement_scale=0.30),
}
# The analysis bar, relative to c: ow_centroid_analyze against oct_analyze on the SAME rows differs only by the device's sin / cos
# against the host's.  Committed as at most 10 x the worst relative difference measured over the synthetic rows of
# tests/test_gpu_centroid_track.py, and never above ANALYSIS_REL_CAP.  DESIGN.md (feature row f8) has the measurement.
ANALYSIS_REL_CAP = 1e-9
ANALYSIS_REL = 4.8e-15       # measured worst 4.871e-16 (220-sample frames, 65 rows); 2.0e-16 at 2 205 samples
SECOND_ORDER = 1.5
ONE_HZ_SHARE = 0.90          # the condition: at least this share of a job's frames has a bound below 1 Hz, what the command prints


def lib(perturbed=False):
    return native.load("centroid_track_ref", "perturbed" if perturbed else "")


def samples(duration):
    return lib().oct_samples(float(duration))


def ms_to_samples(ms):
    return lib().oct_ms_to_samples(float(ms))


def bins(window_samples):
    """(k_min, k_max) of a frame of window_samples."""
    a, b = _Z(0), _Z(0)
    lib().oct_bins(int(window_samples), C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def render(job, duration=1.0, perturbed=False):
    """final_output of the command for one Job."""
    L = lib(perturbed)
    n = L.oct_samples(float(duration))
    out = np.zeros(max(n, 1))
    ds = job.displacement_scale
    got = L.oct_render(int(job.note), int(job.velocity), float(duration), float(job.volume), float(job.speaker), float(job.ldr), 1 if job.no_preamp else 0,
                       1 if job.no_poweramp else 0, 0 if ds is None else 1, 0.0 if ds is None else float(ds), out.ctypes.data_as(_VP), out.size)
    assert got == n
    return out[:n]


def analyze(signal, window_samples, hop_samples, end_sample, length=None, spectra=False):
    """The command's frame loop on one signal: centroids f64 [frames] (and the bins' (re, im) [frames][bins][2] with spectra=True)."""
    L = lib()
    sig = np.ascontiguousarray(signal, dtype=np.float64)
    length = sig.size if length is None else int(length)
    assert length <= sig.size
    nf = L.oct_analyze(sig.ctypes.data_as(_VP), length, int(window_samples), int(hop_samples), int(end_sample), None, None, 0)
    assert nf != _Z(-1).value, "hop_samples is 0"
    k_min, k_max = bins(window_samples) if window_samples else (0, -1)
    fr = np.zeros(nf)
    sp = np.zeros((nf, max(k_max - k_min + 1, 0), 2)) if spectra else None
    got = L.oct_analyze(sig.ctypes.data_as(_VP), length, int(window_samples), int(hop_samples), int(end_sample), fr.ctypes.data_as(_VP),
                        sp.ctypes.data_as(_VP) if spectra else None, nf)
    assert got == nf
    return (fr, sp) if spectra else fr


def analyze_rows(signals, window_samples, hop_samples, end_sample, length=None, threads=16):
    """analyze() of every row on `threads` host threads (ctypes drops the GIL): f64 [rows][frames]."""
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return np.array(list(ex.map(lambda s: analyze(s, window_samples, hop_samples, end_sample, length), list(signals))))


def track(job, duration=1.0, window_ms=5.0, hop_ms=2.5, end_ms=500.0, perturbed=False, audio=None):
    """cmd_centroid_track for one Job up to its summary: Result(audio, frames, spectra, times, window, hop, end, k_min, k_max)."""
    au = render(job, duration, perturbed) if audio is None else audio
    w, h, e = ms_to_samples(window_ms), ms_to_samples(hop_ms), ms_to_samples(end_ms)
    fr, sp = analyze(au, w, h, e, spectra=True)
    times = np.array([(float(j * h) + float(w) / 2.0) / BASE_SR * 1000.0 for j in range(fr.size)])
    k_min, k_max = bins(w)
    return Result(au, fr, sp, times, w, h, e, k_min, k_max)


def track_many(jobs, threads=16, **kw):
    jobs = list(jobs)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(lambda j: track(j, **kw), jobs))


def hann(window_samples):
    """The command's periodic Hann table."""
    n = int(window_samples)
    return np.array([0.5 * (1.0 - np.cos(2.0 * np.pi * float(i) / float(n))) for i in range(n)])


def sample_bar(audio, floor, rel=1e-5, floor_frac=1e-3):
    """oracle.parity_report's per-sample tolerance."""
    audio = np.asarray(audio)
    return np.maximum(rel * np.maximum(np.abs(audio), floor_frac * np.max(np.abs(audio))), floor)


def frame_bounds(res, floor):
    """The first-order bound on |dc| of every frame of a Result, from its own spectra and the sample bars (module docstring).  inf where
    the frame has no power."""
    b = sample_bar(res.audio, floor)
    hw = hann(res.window)
    f = np.arange(res.k_min, res.k_max + 1) * (BASE_SR / float(res.window))
    out = np.zeros(res.frames.size)
    for j in range(res.frames.size):
        pos = j * res.hop
        B = float(np.sum(hw * b[pos:pos + res.window]))
        mag = np.hypot(res.spectra[j, :, 0], res.spectra[j, :, 1])
        power = float(np.sum(mag * mag))
        out[j] = 2.0 * B * float(np.sum(np.abs(f - res.frames[j]) * mag)) / power if power > 0.0 else np.inf
    return out


def frame_bars(res, floor):
    """The end-to-end bar of every frame: SECOND_ORDER x the bound plus the analysis bar."""
    return SECOND_ORDER * frame_bounds(res, floor) + ANALYSIS_REL * np.abs(res.frames)


def one_hz_share(res, floor):
    """Share of the frames whose bound is below 1 Hz."""
    b = frame_bounds(res, floor)
    return float(np.mean(b < 1.0)) if b.size else 0.0


def clear_of_edges(value, bar, lo, hi):
    """A status may be asserted only when the restatement's value is further than its bar from both edges of the target interval."""
    return abs(value - lo) > bar and abs(value - hi) > bar
