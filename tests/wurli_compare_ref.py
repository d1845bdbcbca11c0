"""numpy restatement of the analysis of the reference's tools/wurli_compare.py (compute_stft :46-58, harmonic_profile :61-92,
measure_decay :95-119, measure_spectral_centroid :122-127, measure_rms :130-133, measure_attack_time :136-154, compare_note :235-299),
with a `dtype` switch:

  float32   the reference's arithmetic as numpy runs it: float32 samples, a float32 window, a single-precision rfft (numpy 2 keeps
            float32 input in single precision), S and its mean in float32, float32 squares and means for the RMS figures;
  float64   the contract of ow_stft_profile / ow_frame_rms: the same float32 operands (samples rounded to float32, frame * window one
            rounded float32 product), everything after that in float64.

Every function returns UNROUNDED figures; the script's rounding is applied on top by openwurli_amd.wurli_compare.comparison_from_figures,
so that the golden's rounded report can be compared with both forms.  The fixtures' clips are generated here (`golden_clip`), but
travel in the fixture as integers: a libm's last bit must not move a quantised sample.
"""
import numpy as np

SR = 44100


def frames_of(y, n, hop):
    """[n_frames, n]: frame i = y[i * hop : i * hop + n], zero-padded; max(1, (len - n) // hop + 1) frames (Python's floor)."""
    n_frames = max(1, (len(y) - n) // hop + 1)
    need = (n_frames - 1) * hop + n
    if need > len(y):
        y = np.concatenate([y, np.zeros(need - len(y), dtype=y.dtype)])
    idx = (np.arange(n_frames) * hop)[:, None] + np.arange(n)[None, :]
    return y[idx]


def spectrogram(y, n_fft, hop, dtype):
    """S [n_fft / 2 + 1, n_frames] (C order, as the reference fills it column by column) and the frequency axis."""
    y32 = np.asarray(y).astype(np.float32)
    window = np.hanning(n_fft).astype(np.float32)
    prod = frames_of(y32, n_fft, hop) * window                    # float32 x float32, one rounding
    S = np.zeros((n_fft // 2 + 1, prod.shape[0]), dtype=dtype)
    for i in range(prod.shape[0]):                                # one transform per frame, as the reference runs them
        S[:, i] = np.abs(np.fft.rfft(prod[i].astype(dtype)))
    return S, np.fft.rfftfreq(n_fft, 1.0 / SR), prod


def mean_spectrum(y, n_fft=8192, hop=512, dtype=np.float64):
    S, freqs, prod = spectrogram(y, n_fft, hop, dtype)
    return S.mean(axis=1), freqs, prod


def centroid(y, n_fft=4096, hop=512, dtype=np.float64):
    S, freqs, _ = spectrogram(y, n_fft, hop, dtype)
    power = S ** 2
    per_frame = np.sum(freqs[:, None] * power, axis=0) / (np.sum(power, axis=0) + 1e-10)
    return float(np.mean(per_frame))


def harmonic_peaks(s_avg, freqs, f0_hz, n_harmonics=10):
    amps, bins = [], []
    for h in range(1, n_harmonics + 1):
        fh = f0_hz * h
        if fh > SR / 2:
            break
        idx = int(np.argmin(np.abs(freqs - fh)))
        lo, hi = max(0, idx - 4), min(len(s_avg), idx + 5)
        k = lo + int(np.argmax(s_avg[lo:hi]))
        amps.append(float(s_avg[k])); bins.append(k)
    return amps, bins


def rms_envelope(y, frame_len, hop, dtype):
    """The reference fills a float64 array with float32 results (sqrt(mean(frame ** 2)) of a float32 frame stays float32)."""
    f = frames_of(np.asarray(y).astype(np.float32), frame_len, hop).astype(dtype)
    out = np.zeros(f.shape[0])
    for i in range(f.shape[0]):
        out[i] = np.sqrt(np.mean(f[i] ** 2))
    return out


def decay_slope(rms, hop=512):
    a, b = int(0.08 * SR / hop), min(len(rms), int((0.08 + 0.5) * SR / hop))
    if b - a < 5:
        return None
    db = 20 * np.log10(rms[a:b] + 1e-10)
    t = np.arange(len(db)) * hop / SR
    return float(np.polyfit(t, db, 1)[0])


def rms_db(y, dtype):
    v = np.asarray(y).astype(np.float32).astype(dtype)
    r = np.sqrt(np.mean(v ** 2))
    return float(20 * np.log10(r + 1e-10))         # float32: the sum and the logarithm stay in single precision, as in the reference


def attack(rms):
    if len(rms) == 0 or rms.max() < 1e-10:
        return None, None
    k = int(np.argmax(rms))
    return k, float(k * 128 / SR * 1000)


def side_figures(y, sustain, f0_hz, dtype):
    """What openwurli_amd.wurli_compare.analyse_side returns for one clip: the unrounded figures of one side of a pair."""
    s_avg, freqs, _ = mean_spectrum(sustain, 8192, 512, dtype)
    amps, bins = harmonic_peaks(s_avg, freqs, f0_hz)
    k, ms = attack(rms_envelope(y, 1024, 128, dtype))
    return {"amps": amps, "bins": bins, "decay": decay_slope(rms_envelope(y, 2048, 512, dtype)), "centroid": centroid(sustain, 4096, 512, dtype),
            "attack_frame": k, "attack_ms": ms, "rms_db": rms_db(y, dtype)}


def slices(y_real, y_synth):
    skip = int(0.08 * SR)
    dur = min(len(y_real), len(y_synth), int(1.0 * SR))
    return (y_real[skip:skip + dur] if len(y_real) > skip else y_real), (y_synth[skip:skip + dur] if len(y_synth) > skip else y_synth)


def pair_figures(y_real, y_synth, f0_hz, dtype):
    a, b = slices(y_real, y_synth)
    return side_figures(y_real, a, f0_hz, dtype), side_figures(y_synth, b, f0_hz, dtype)


# ---- figure classes: what the float32 -> float64 movement is measured and bounded in --------------------------------------------------
CLASSES = ("ratio", "db", "decay", "centroid", "rms", "attack")


def class_values(fig):
    """class -> the unrounded figures of that class of one side (harmonic ratios and their dB re H1, the rest scalars)."""
    a = fig["amps"]
    ratios = [x / a[0] for x in a] if a and a[0] >= 1e-10 else []
    return {"ratio": ratios, "db": [float(20 * np.log10(r + 1e-10)) for r in ratios], "decay": [] if fig["decay"] is None else [fig["decay"]],
            "centroid": [fig["centroid"]], "rms": [fig["rms_db"]], "attack": [] if fig["attack_ms"] is None else [fig["attack_ms"]]}


def movement(figs_a, figs_b):
    """class -> the largest |a - b| over the sides given (lists of side figures of equal length)."""
    out = {c: 0.0 for c in CLASSES}
    for fa, fb in zip(figs_a, figs_b):
        va, vb = class_values(fa), class_values(fb)
        for c in CLASSES:
            assert len(va[c]) == len(vb[c]), c
            for x, y in zip(va[c], vb[c]):
                out[c] = max(out[c], abs(x - y))
    return out


# ---- the fixtures' clips --------------------------------------------------------------------------------------------------------------
def golden_clip(seed, f0, seconds, level=0.3):
    """A decaying harmonic series with a 10 ms onset ramp and a 1e-4 noise floor."""
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n) / SR
    x = np.zeros(n)
    for h in range(1, 11):
        if f0 * h < SR / 2:
            x += rng.uniform(0.05, 1.0) / h * np.exp(-t * rng.uniform(1.0, 9.0)) * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28))
    x *= np.minimum(1.0, t / 0.010)
    return level * x / max(1.0, np.max(np.abs(x))) + 1e-4 * rng.standard_normal(n)


_GOLDEN = None


def load_golden():
    """(the golden's dictionary, [(recorded clip, render clip, f0)] as the float64 values of the files' integers); read once."""
    global _GOLDEN
    if _GOLDEN is None:
        import json
        import os
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(here, "wurli_compare_golden.json")) as f:
            g = json.load(f)
        z = np.load(os.path.join(here, "wurli_compare_golden.npz"))
        pairs = [(z[f"real{i}"].astype(np.float64) / 32768.0, z[f"synth{i}"].astype(np.float64) / 8388608.0, c["f0_hz"])
                 for i, c in enumerate(g["comparisons"])]
        _GOLDEN = (g, pairs)
    return _GOLDEN


_FIGURES = {}


def golden_figures(dtype):
    """[(recorded side, render side)] of the golden's pairs in one form of the restatement; computed once per form."""
    key = np.dtype(dtype).name
    if key not in _FIGURES:
        _FIGURES[key] = [pair_figures(a, b, f0, dtype) for a, b, f0 in load_golden()[1]]
    return _FIGURES[key]
