"""CPU restatement (numpy) of the recording side of the ML loop.  TEST INFRASTRUCTURE ONLY.

Restates (reference file:line):
  * goertzel_mag / extract_harmonics_goertzel   ml/goertzel_utils.py:34-57, 106-119
  * measure_interharmonic_snr                    ml/compute_residuals.py:59-127
  * detect_anomalous_harmonics, compute_note_residual, assemble_dataset      ml/compute_residuals.py:130-363
Pinned: tests/test_harmonics_host.py and tests/test_residuals_host.py hold it bit for bit to tests/golden/residuals_golden.npz, the
outputs of the reference's own Python (tests/golden/make_residuals_golden.py).

The reference's Goertzel loop is one interpreted recurrence after the other.  Here every recurrence of a call advances together, one
numpy operation per IEEE operation of the loop body ((x + (coeff * s1)) - s2), so the results are the same bits; `plan` may be the
coefficients and bins a library reports instead of numpy's own.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import features_oracle as fo  # noqa: E402

N_OFFSETS = 11
N_HARMONICS = 8
N_FREQ, N_DECAY = 5, 5
N_TARGETS = N_FREQ + N_DECAY + 1
DS_IDX = N_FREQ + N_DECAY
TIER_WEIGHTS = {"gold": 1.0, "silver": 0.6, "bronze": 0.3}
SNR_THRESHOLD_DB = 10.0
MAX_RELIABLE_HARMONIC = 2
VELOCITY_BUCKETS = (20, 35, 50, 65, 80, 95, 110, 127)


# ---- Goertzel ---------------------------------------------------------------------------------------------------------------------------
def goertzel_plan(n, sr, f0, n_harmonics=N_HARMONICS, search_pct=0.01):
    """(coeffs [n_harmonics, 11], bins [n_harmonics, 11]) of one segment of n samples: bin -1 (coefficient 0) where the offset is
    skipped (k <= 0, k >= n // 2) or the harmonic lies at or above sr / 2 - 100."""
    coeffs = np.zeros((n_harmonics, N_OFFSETS))
    bins = np.full((n_harmonics, N_OFFSETS), -1, dtype=np.int32)
    for h in range(n_harmonics):
        fh = f0 * (h + 1)
        if fh >= sr / 2 - 100:
            continue
        for o, offset in enumerate(np.linspace(-search_pct, search_pct, N_OFFSETS)):
            k = int(round(fh * (1.0 + offset) * n / sr))
            if k <= 0 or k >= n // 2:
                continue
            bins[h, o] = k
            coeffs[h, o] = 2.0 * np.cos(2.0 * np.pi * k / n)
    return coeffs, bins


def goertzel_states(signals, coeff_lists):
    """(s1, s2) of every recurrence: signals[i] runs under each coefficient of coeff_lists[i].  All recurrences advance together; a
    signal that has ended drops out (the signals are walked longest first)."""
    order = sorted(range(len(signals)), key=lambda i: -len(signals[i]))
    lens = np.array([len(signals[i]) for i in order])
    width = int(lens[0]) if len(order) else 0
    x = np.zeros((len(order), width))
    for r, i in enumerate(order):
        x[r, :lens[r]] = signals[i]
    owner = np.concatenate([np.full(len(coeff_lists[i]), r, dtype=np.int64) for r, i in enumerate(order)]) if order else np.zeros(0, dtype=np.int64)
    coeff = np.concatenate([np.asarray(coeff_lists[i], dtype=np.float64) for i in order]) if order else np.zeros(0)
    first = np.concatenate([[0], np.cumsum([len(coeff_lists[i]) for i in order])])
    s1 = np.zeros(coeff.size)
    s2 = np.zeros(coeff.size)
    xt = np.ascontiguousarray(x.T)
    for t in range(width):
        live = int(first[int(np.searchsorted(-lens, -t, side="left"))])     # recurrences of signals longer than t: a prefix
        s0 = (xt[t, owner[:live]] + coeff[:live] * s1[:live]) - s2[:live]
        s2[:live] = s1[:live]
        s1[:live] = s0
    out = [None] * len(signals)
    for r, i in enumerate(order):
        out[i] = (s1[first[r]:first[r + 1]].copy(), s2[first[r]:first[r + 1]].copy())
    return out


def goertzel_amps_many(signals, plans):
    """extract_harmonics_goertzel of many signals: plans[i] = (coeffs [nh, 11], bins [nh, 11], past [nh] bool: harmonic at or above
    the Nyquist cut).  Returns a list of amps [nh]."""
    lists = [np.asarray(c)[np.asarray(b) >= 0] for c, b, _ in plans]
    states = goertzel_states(signals, lists)
    out = []
    for x, (coeffs, bins, past), (s1, s2) in zip(signals, plans, states):
        n = len(x)
        amps = np.zeros(len(past))
        r = 0
        for h in range(len(past)):
            best = 0.0
            for o in range(N_OFFSETS):
                if bins[h][o] < 0:
                    continue
                c, a, b = np.float64(coeffs[h][o]), s1[r], s2[r]
                r += 1
                mag = np.sqrt(a * a + b * b - c * a * b) / n * 2.0
                if mag > best:
                    best = mag
            amps[h] = 1e-20 if past[h] else max(best, 1e-20)
        out.append(amps)
    return out


def past_cut(sr, f0, n_harmonics):
    return np.array([f0 * (h + 1) >= sr / 2 - 100 for h in range(n_harmonics)], dtype=bool)


def goertzel_amps(signal, sr, f0, n_harmonics=N_HARMONICS, search_pct=0.01, plan=None):
    """extract_harmonics_goertzel of one signal; plan = (coeffs, bins) to use instead of numpy's own."""
    coeffs, bins = goertzel_plan(len(signal), sr, f0, n_harmonics, search_pct) if plan is None else plan
    return goertzel_amps_many([np.asarray(signal, dtype=np.float64)], [(coeffs[:n_harmonics], bins[:n_harmonics], past_cut(sr, f0, n_harmonics))])[0]


# ---- inter-harmonic noise floor and SNR ---------------------------------------------------------------------------------------------------
def noise_bands(n, sr, f0, n_harmonics=N_HARMONICS):
    """Inclusive bin range of each noise band on the 4n-point axis, or None (past the cut, or no bin)."""
    nfft = 4 * n
    axis = np.fft.rfftfreq(nfft, d=1.0 / sr)
    out = []
    for h in range(n_harmonics):
        nf = (h + 1.5) * f0
        if nf >= sr / 2 - 100:
            out.append(None)
            continue
        idx = np.where((axis >= nf * 0.99) & (axis <= nf * 1.01))[0]
        out.append((int(idx[0]), int(idx[-1])) if idx.size else None)
    return out


def noise_medians(segment, sr, f0, n_harmonics=N_HARMONICS):
    x = np.asarray(segment, dtype=np.float64)
    n = x.size
    spec = np.abs(np.fft.rfft(x * np.hanning(n), n=4 * n)) * 2.0 / n / 0.5
    out = np.zeros(n_harmonics)
    for h, b in enumerate(noise_bands(n, sr, f0, n_harmonics)):
        out[h] = 1e-20 if b is None else max(np.median(spec[b[0]:b[1] + 1]), 1e-20)
    return out


def snr_window(n_audio, sr, onset_s=0.0, window_start=0.05, window_end=0.20):
    """(start, end) of the measuring window, or None where the reference answers all-NaN."""
    a, b = max(int((onset_s + window_start) * sr), 0), min(int((onset_s + window_end) * sr), n_audio)
    return (a, b) if b - a >= 128 else None


def snr_from(h_amps, noise):
    out = np.full(len(h_amps), np.nan)
    for h in range(len(h_amps)):
        if h_amps[h] > 1e-20 and noise[h] > 1e-20:
            out[h] = 20.0 * np.log10(h_amps[h] / noise[h])
    return out


def interharmonic_snr(audio, sr, f0, onset_s=0.0, n_harmonics=N_HARMONICS):
    w = snr_window(len(audio), sr, onset_s)
    if w is None:
        return np.full(n_harmonics, np.nan)
    seg = np.asarray(audio, dtype=np.float64)[w[0]:w[1]]
    return snr_from(fo.extract_harmonics(seg, sr, f0, n_harmonics)[0], noise_medians(seg, sr, f0, n_harmonics))


# ---- residual bookkeeping -----------------------------------------------------------------------------------------------------------------
def bucket_velocity(v):
    return min(VELOCITY_BUCKETS, key=lambda b: abs(b - v))


def anomalous(db):
    """Targets (0 = H2) whose harmonic is louder than the one below it."""
    return {h for h in range(1, min(len(db) - 1, 7)) if db[h + 1] is not None and db[h] is not None and db[h + 1] > db[h]}


def _snr_bad(snr, i, threshold):
    return snr is not None and i < len(snr) and (np.isnan(snr[i]) or snr[i] < threshold)


def note_residual(real, model, snr=None, threshold=SNR_THRESHOLD_DB):
    t = np.full(N_TARGETS, np.nan)
    m = np.zeros(N_TARGETS, dtype=bool)
    rw, mw = real["windows"].get("early_sustain"), model["windows"].get("early_sustain")
    if rw is None or mw is None:
        rw, mw = real["windows"].get("sustain"), model["windows"].get("sustain")
    if rw is None or mw is None:
        return t, m
    odd = anomalous(rw["amps_dB_rel_H1"])
    for h in range(MAX_RELIABLE_HARMONIC):
        rf, mf = rw["freqs_hz"][h + 1], mw["freqs_hz"][h + 1]
        if rf is None or mf is None or rf <= 0 or mf <= 0 or _snr_bad(snr, h + 1, threshold) or h in odd:
            continue
        t[h] = 1200.0 * math.log2(rf / mf)
        m[h] = True
    four = [f["windows"].get(w) for f in (real, model) for w in ("early_sustain", "sustain")]
    if all(w is not None for w in four):
        for h in range(MAX_RELIABLE_HARMONIC):
            re, rs, me, ms = (w["amps_linear"][h + 1] for w in four)
            if any(v is None for v in (re, rs, me, ms)) or not (re > 1e-12 and rs > 1e-12 and me > 1e-12 and ms > 1e-12):
                continue
            if _snr_bad(snr, h + 1, threshold) or h in odd:
                continue
            t[N_FREQ + h] = (rs / re) / (ms / me)
            m[N_FREQ + h] = True
    r2, m2 = rw["amps_dB_rel_H1"][1], mw["amps_dB_rel_H1"][1]
    if r2 is not None and m2 is not None and 0 not in odd and not _snr_bad(snr, 1, threshold):
        t[DS_IDX] = 2.0 ** ((r2 - m2) / 6.0)
        m[DS_IDX] = True
    return t, m


def assemble(real_features, model_features, snr_cache=None):
    rows = []
    for f in real_features:
        vel = f.get("velocity_midi", 80)
        model = model_features.get(f"{f['midi_note']}_{bucket_velocity(vel)}")
        if model is None:
            continue
        t, m = note_residual(f, model, snr_cache.get(f.get("id", "")) if snr_cache else None)
        if m.any():
            rows.append(([(f["midi_note"] - 21) / (108 - 21), vel / 127.0], t, m, TIER_WEIGHTS.get(f.get("isolation_tier", "bronze"), 0.3), f.get("id", "")))
    return (np.array([r[0] for r in rows], dtype=np.float32), np.nan_to_num(np.array([r[1] for r in rows], dtype=np.float32), nan=0.0),
            np.array([r[2] for r in rows], dtype=bool), np.array([r[3] for r in rows], dtype=np.float32), [r[4] for r in rows])
