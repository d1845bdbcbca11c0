"""ctypes loader of the CPU restatement of `preamp-bench intermod-audit` and `overshoot` (tests/c/note_audit_ref.cpp, over the oracle's
headers).  tests/native.py has oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that
source.  A second build with -DOW_ORACLE_VOICE_PERTURB (the voice's library calls off by one ulp, oracle/ow_voice.hpp) is the sensitivity
variant of the voice row.

Also here, because the host and the GPU tests share them: the jobs the GPU tests run, the bars, and the reports' text built from the
restatement's numbers.

The bars are derived, not chosen.  The voice row is known to +- b_i, the bar of the existing Voice::render_note parity tests
(tests/test_gpu_parity.py: 1e-10 x the row's peak, on every sample).  dft_magnitude = (2 / n) |sum x_i e^(-j phase_i)| then moves by at most
B = (2 / n) sum b_i; an energy sum of N magnitudes by at most dE = 2 B sum mag_k + N B^2; a dB figure 10 log10 E by 10 / ln 10 x dE / E.
The end-to-end bar of a dB figure is SECOND_ORDER x that plus the analysis bar (ANALYSIS_REL, the device's lane-strided sums and its
sin / cos against the serial host loop), which enters the same way with B_a = ANALYSIS_REL x (2 / n) sum |x_i|.
"""
import ctypes as C
import math
import threading
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native

BASE_SR = 44100.0
MAX_PROBES = 75
_LOCK = threading.Lock()
_VP = C.c_void_p

VOICE_REL = 1e-10            # tests/test_gpu_parity.py test_render_note: |gpu - cpu| <= 1e-10 x peak|cpu| on every sample
SECOND_ORDER = 1.5
# The analysis bar of ow_dft_magnitudes against dft_magnitude on the SAME rows, relative to the scale (2 / n) sum |x_i| (not to the
# magnitude: midpoint probes cancel).  Committed as at most 10 x the worst difference measured in tests/test_gpu_note_audit.py
# test_dft_magnitudes_synthetic, and never above the a-priori bound (n + 4) 2^-52 of an n-term sum with a sin / cos good to 2 ulp on both
# sides.  DESIGN.md (feature row f9) has the measurement.
ANALYSIS_REL = 1.9e-15       # measured worst 1.908e-16 (257 samples); 9.5e-17 at 64, 7.9e-17 at 63, 6.2e-18 at 4 410, 0 at 1


def analysis_cap(n):
    return (n + 4) * 2.0 ** -52


def analysis_rel(n):
    return min(ANALYSIS_REL, analysis_cap(n))


Product = namedtuple("Product", "mode nearest_integer mode_ratio fractional_offset beat_hz effective_amplitude perceptual_weight risk_score")
Report = namedtuple("Report", "midi fundamental_hz mu max_risk total_risk products")
Detail = namedtuple("Detail", "mode nearest_integer listed intermod_freq nearest_freq intermod_mag nearest_mag ratio_db risk_score")
Audit = namedtuple("Audit", "midi too_short h_db m_db ratio_db verdict harmonic_energy midpoint_energy n_harmonics n_midpoints start end products")
Overshoot = namedtuple("Overshoot", "peak_0_10 peak_0_50 rms_100_200 rms_1000_1500 overshoot_db bark_decay_db pk_dbfs rms1_dbfs rms2_dbfs")
VERDICTS = ("DIRTY", "MARGINAL", "OK", "CLEAN")

# The jobs of the GPU tests (tests/test_gpu_note_audit.py).  intermod-audit: note 33 (32 harmonics), 60, 96 (10 harmonics) at ff and one
# job at velocity 64, all at 0.6 s (window 22 050..26 460: the min(len) branch); one job at 2.05 s for the other branch.
INTERMOD_SHORT, INTERMOD_LONG = 0.6, 2.05
INTERMOD_JOBS_SHORT = ((33, 127), (60, 127), (96, 127), (72, 64))
INTERMOD_JOBS_LONG = ((48, 127),)
# overshoot: 0.25 s (the late window is empty: NaN, -120 dBFS) and 1.6 s
OVERSHOOT_DURATIONS = (0.25, 1.6)
OVERSHOOT_JOBS = ((36, 64), (36, 127), (84, 64), (84, 127))


def lib(perturbed=False):
    return native.load("note_audit_ref", "voice_perturbed" if perturbed else "")


def samples(duration):
    return lib().onr_samples(float(duration))


def intermod_risk(midi):
    o = np.zeros(4 + 6 * 8)
    lib().onr_intermod_risk(int(midi), o.ctypes.data_as(_VP))
    prods = tuple(Product(int(p[0]), int(p[1]), *[float(x) for x in p[2:]]) for p in o[4:].reshape(6, 8))
    return Report(int(midi), float(o[0]), float(o[1]), float(o[2]), float(o[3]), prods)


def perceptual_beat_weight(beat_hz):
    return lib().onr_perceptual_beat_weight(float(beat_hz))


def dft_magnitude(signal, freq, sr=BASE_SR):
    s = np.ascontiguousarray(signal, dtype=np.float64)
    return lib().onr_dft_magnitude(s.ctypes.data_as(_VP), s.size, float(freq), float(sr))


def dft_magnitudes(rows, start, end, sr, freqs, threads=16):
    """dft_magnitude of rows[r][start:end] at freqs[r][k] (NaN: 0.0), serial per (row, probe), the pairs spread over host threads."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    freqs = np.atleast_2d(freqs)
    out = np.zeros(freqs.shape)
    todo = [(r, k) for r in range(freqs.shape[0]) for k in range(freqs.shape[1]) if not math.isnan(freqs[r, k])]
    with ThreadPoolExecutor(max_workers=threads) as ex:
        for (r, k), v in zip(todo, ex.map(lambda rk: dft_magnitude(rows[rk[0], start:end], freqs[rk[0], rk[1]], sr), todo)):
            out[r, k] = v
    return out


def render(note, velocity, duration, perturbed=False):
    """Voice::render_note(note, velocity / 127, duration, 44100)."""
    L = lib(perturbed)
    n = L.onr_samples(float(duration))
    out = np.zeros(max(n, 1))
    assert L.onr_render(int(note), int(velocity), float(duration), out.ctypes.data_as(_VP), out.size) == n
    return out[:n]


def probes(midi):
    """(freqs, n_harmonics, n_midpoints) of the render analysis."""
    f = np.zeros(MAX_PROBES)
    nh, nm = C.c_uint32(0), C.c_uint32(0)
    c = lib().onr_probes(int(midi), f.ctypes.data_as(_VP), C.byref(nh), C.byref(nm))
    return f[:c].copy(), int(nh.value), int(nm.value)


def intermod_audit(signal, midi):
    s = np.ascontiguousarray(signal, dtype=np.float64)
    o, d = np.zeros(10), np.zeros((6, 7))
    short = lib().onr_intermod_audit(s.ctypes.data_as(_VP), s.size, int(midi), o.ctypes.data_as(_VP), d.ctypes.data_as(_VP))
    rep = intermod_risk(midi)
    prods = tuple(Detail(p.mode, p.nearest_integer, bool(x[0]), *[float(v) for v in x[1:]]) for p, x in zip(rep.products, d))
    return Audit(int(midi), bool(short), float(o[0]), float(o[1]), float(o[2]), int(o[3]), float(o[4]), float(o[5]), int(o[6]), int(o[7]),
                 int(o[8]), int(o[9]), prods)


def overshoot(signal):
    s = np.ascontiguousarray(signal, dtype=np.float64)
    o = np.zeros(9)
    lib().onr_overshoot(s.ctypes.data_as(_VP), s.size, o.ctypes.data_as(_VP), None)
    return Overshoot(*[float(v) for v in o])


def overshoot_edges():
    s, o, e = np.zeros(1), np.zeros(9), (C.c_size_t * 6)()
    lib().onr_overshoot(s.ctypes.data_as(_VP), 1, o.ctypes.data_as(_VP), e)
    return [int(v) for v in e]


def many(fn, items, threads=16):
    items = list(items)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(fn, items))


# ---- bars ---------------------------------------------------------------------------------------------------------------------------
def voice_bar(audio):
    """b of the voice row: one value for every sample."""
    return VOICE_REL * float(np.max(np.abs(audio)))


def db_bar(mags, B):
    """First-order bound on 10 log10(sum mag^2) when every magnitude moves by at most B."""
    mags = np.asarray(mags, dtype=np.float64)
    E = float(np.sum(mags * mags))
    return math.inf if E <= 0.0 else 10.0 / math.log(10.0) * (2.0 * B * float(np.sum(mags)) + mags.size * B * B) / E


def intermod_bars(audio, midi):
    """(bar of h_db, bar of m_db, bar of ratio_db, [bar of each listed product's ratio_db]) for the restatement's row `audio`."""
    a = intermod_audit(audio, midi)
    win = np.asarray(audio[a.start:a.end])
    n = win.size
    f, nh, nm = probes(midi)
    mags = np.array([dft_magnitude(win, x) for x in f])
    Bv = 2.0 * voice_bar(audio)                                                        # (2 / n) sum b_i with every b_i = b
    Ba = analysis_rel(n) * (2.0 / n) * float(np.sum(np.abs(win)))
    h = SECOND_ORDER * db_bar(mags[:nh], Bv) + db_bar(mags[:nh], Ba)
    m = SECOND_ORDER * db_bar(mags[nh:nh + nm], Bv) + db_bar(mags[nh:nh + nm], Ba)
    det = []
    for p in a.products:
        if p.listed:                                         # 20 log10(a / b): each of the two magnitudes moves by B
            B = SECOND_ORDER * Bv + Ba
            det.append(20.0 / math.log(10.0) * (B / p.intermod_mag + B / p.nearest_mag) if min(p.intermod_mag, p.nearest_mag) > 0 else math.inf)
    return h, m, h + m, det


def overshoot_bars(audio):
    """Bars of the nine figures of Overshoot for the restatement's row: peaks +- b, RMS +- sqrt(mean b^2) = b, dB by the first-order
    rule 20 / ln 10 x (dp / p + dr / r); nan where the figure is NaN or -120."""
    o = overshoot(audio)
    b = voice_bar(audio)
    k = SECOND_ORDER * 20.0 / math.log(10.0)
    rel = lambda x: b / x if x > 1e-15 else math.nan
    return Overshoot(b, b, b, b, k * (rel(o.peak_0_10) + rel(o.rms_100_200)), k * (rel(o.peak_0_50) + rel(o.rms_1000_1500)), k * rel(o.peak_0_10),
                     k * rel(o.rms_100_200), k * rel(o.rms_1000_1500))


def clear_of_rounding(value, bar, decimals):
    """A printed figure may be compared as text only when the value lies further than its bar from the nearest rounding boundary of
    {:.decimals}."""
    if math.isnan(value) or value == -120.0:
        return True
    scaled = value * 10 ** decimals
    return abs(scaled - math.floor(scaled) - 0.5) > bar * 10 ** decimals


# ---- the restatement's rows, rendered once per process and shared by the tests (never modified) -----------------------------------
_ROWS = {}


def row(note, velocity, duration, perturbed=False):
    key = (int(note), int(velocity), float(duration), bool(perturbed))
    with _LOCK:
        got = _ROWS.get(key)
    if got is None:
        got = render(note, velocity, duration, perturbed)
        got.setflags(write=False)
        with _LOCK:
            _ROWS[key] = got
    return got


def intermod_jobs():
    """[(note, velocity, duration)] of the GPU tests' intermod-audit jobs."""
    return [(n, v, INTERMOD_SHORT) for n, v in INTERMOD_JOBS_SHORT] + [(n, v, INTERMOD_LONG) for n, v in INTERMOD_JOBS_LONG]


# ---- the commands' text from the restatement's numbers (dict rows with the names the package's formatters read) --------------------
def risk_record(midi):
    r = intermod_risk(midi)
    return {"midi": r.midi, "fundamental_hz": r.fundamental_hz, "mu": r.mu, "max_risk": r.max_risk, "total_risk": r.total_risk,
            "products": [p._asdict() for p in r.products]}


def intermod_record(audio, midi, velocity=127):
    a = intermod_audit(audio, midi)
    return {"midi": midi, "velocity": velocity, "too_short": a.too_short, "verdict": a.verdict, "h_db": a.h_db, "m_db": a.m_db, "ratio_db": a.ratio_db,
            "n_harmonics": a.n_harmonics, "n_midpoints": a.n_midpoints, "window_start": a.start, "window_end": a.end,
            "harmonic_energy": a.harmonic_energy, "midpoint_energy": a.midpoint_energy, "products": [p._asdict() for p in a.products]}


def overshoot_record(audio, note, velocity):
    d = overshoot(audio)._asdict()
    d.update(note=note, velocity=velocity)
    return d
