"""The pickup-law study on the device: host mirror of the reference's ``ml/h3_analysis_v2.py`` over the C-ABI (``ow_pickup_law``, and
``ow_dft_magnitudes`` for its step 1).

The reference asks whether the pickup's ``y / (1 - y)`` law should change -- to ``y / (1 - y)^alpha``, with a ``(1 + k y)`` factor, or
blended with ``y / (1 - y^2)`` -- by running a small forward model per note (sine, clip, law, one-pole high-pass, DFT probes over the
second half) for every law point in Python loops and comparing H2 / H3 against the recorded harmonics of ``harmonics.json``.  Here every
(carrier, law) pair of a run is one lane of ONE ``ow_pickup_law`` call; include/openwurli_hip.h states the arithmetic.

A carrier is (f0_hz, ds, vel_scale).  The law kinds are plain ints: 0 ``POWER`` (alpha), 1 ``FACTOR`` (k), 2 ``BLEND``.
"""
import csv
import ctypes as C
import io
import json
import os

import numpy as np

from .binding import OwError, check, load_library  # noqa: F401

HPF_FC = 2312.0
SENSITIVITY = 1.8375
DS_AT_C4 = 0.70
CLIP = 0.90
SR = 44100
DUR = 0.5
VEL_MIDI = 80
N_HARMONICS = 8                               # OW_MAX_HARMONICS; the report reads H1..H3
POWER, FACTOR, BLEND = 0, 1, 2                # the law kinds of ow_pickup_law
FAMILIES = ("alpha", "k", "blend")
ALPHAS = np.arange(1.0, 2.51, 0.1)            # the reference's sweep, unrounded (1.1 is 1.1 + 1 ulp of arange's arithmetic)
KS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0)
BLENDS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
FALLBACK_ANOMALOUS = frozenset((54, 66, 70))  # the script's fallback set
RELIABLE_SNR_DB = 10.0
SNR_WINDOW = (0.05, 0.2)                      # early_sustain


# ---- the script's host functions ------------------------------------------------------------------------------------------------------
def midi_to_freq(midi):
    return 440.0 * 2 ** ((midi - 69) / 12.0)


def reed_length_mm(midi):
    n = max(1, min(64, midi - 32))
    inches = 3.0 - n / 20.0 if n <= 20 else 2.0 - (n - 20) / 44.0
    return inches * 25.4


def reed_blank_dims(midi):
    reed = max(1, min(64, midi - 32))
    w = 0.151 if reed <= 14 else 0.127 if reed <= 20 else 0.121 if reed <= 42 else 0.111 if reed <= 50 else 0.098
    t = 0.020 if reed <= 16 else 0.020 + (reed - 16) / 10.0 * 0.011 if reed <= 26 else 0.031
    return w * 25.4, t * 25.4


def reed_compliance(midi):
    length = reed_length_mm(midi)
    w, t = reed_blank_dims(midi)
    return length ** 3 / (w * t ** 3)


def pickup_ds(midi):
    c = reed_compliance(midi)
    c_ref = reed_compliance(60)
    return max(0.02, min(0.80, DS_AT_C4 * (c / c_ref) ** 0.65))


def velocity_exponent(midi):
    m = float(midi)
    t = np.exp(-0.5 * ((m - 62.0) / 15.0) ** 2)
    return 0.75 + t * 0.65


def hpf_coeffs(sr=SR):
    """(b0, a1) of the script's bilinear one-pole high-pass, with numpy's tan as the script takes it."""
    w_d = np.tan(np.pi * HPF_FC / sr)
    return float(1.0 / (1 + w_d)), float((1 - w_d) / (1 + w_d))


def vel_scale_approx(f0, vel_midi=VEL_MIDI):
    """compute_harmonics' scale (:59-61): the exponent of midi_approx = 69 + 12 log2(f0 / 440)."""
    midi_approx = 69 + 12 * np.log2(f0 / 440.0)
    vel = vel_midi / 127.0
    return float(vel ** velocity_exponent(midi_approx))


def vel_scale_midi(midi, vel_midi=VEL_MIDI):
    """The k and blend variants' scale (:292-293, :346-347): the exponent of the integer note."""
    vel = vel_midi / 127.0
    return float(vel ** velocity_exponent(midi))


def carriers(midis, velocities=(VEL_MIDI,), variants=("approx", "midi")):
    """The carrier rows of a run and what each is: (rows f64 [n][3], keys [(midi, vel_midi, variant)]).  Per (note, velocity) one row per
    variant of the script's scale: `approx` (compute_harmonics: y_peak and the alpha sweep) and `midi` (the k and blend lists).  The two
    can differ in the last bits on a host whose log2 leaves midi_approx off the integer, so a run that reproduces the script carries both."""
    scale = {"approx": lambda midi, f0, vel: vel_scale_approx(f0, vel), "midi": lambda midi, f0, vel: vel_scale_midi(midi, vel)}
    rows, keys = [], []
    for midi in midis:
        f0, ds = midi_to_freq(midi), pickup_ds(midi)
        for vel in velocities:
            for variant in variants:
                rows.append((f0, ds, scale[variant](midi, f0, vel)))
                keys.append((int(midi), int(vel), variant))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 3), keys


def script_laws():
    """The script's 29 law points in its order: (kinds i32, params f64)."""
    kinds = [POWER] * len(ALPHAS) + [FACTOR] * len(KS) + [BLEND] * len(BLENDS)
    params = [float(a) for a in ALPHAS] + list(KS) + list(BLENDS)
    return np.asarray(kinds, dtype=np.int32), np.asarray(params, dtype=np.float64)


# ---- the call -------------------------------------------------------------------------------------------------------------------------
def pickup_law(carrier_rows, kinds, params, n_samples=int(SR * DUR), n_harmonics=N_HARMONICS, sample_rate=float(SR), sensitivity=SENSITIVITY,
               clip=CLIP, hpf=None, device=0):
    """``ow_pickup_law``: (amps f64 [n_carriers][n_laws][n_harmonics], y_peak f64 [n_carriers])."""
    L = load_library()
    car = np.ascontiguousarray(np.asarray(carrier_rows, dtype=np.float64).reshape(-1, 3))
    kd = np.ascontiguousarray(np.asarray(kinds, dtype=np.int32).ravel())
    pr = np.ascontiguousarray(np.asarray(params, dtype=np.float64).ravel())
    if kd.size != pr.size:
        raise ValueError(f"{kd.size} law kinds and {pr.size} parameters")
    b0, a1 = hpf_coeffs(sample_rate) if hpf is None else hpf
    amps = np.zeros((car.shape[0], kd.size, max(int(n_harmonics), 0)))
    peak = np.zeros(car.shape[0])
    check(L, L.ow_pickup_law(car.ctypes.data_as(C.c_void_p), car.shape[0], kd.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), kd.size,
                             float(sample_rate), int(n_samples), int(n_harmonics), float(sensitivity), float(clip), float(b0), float(a1), int(device),
                             amps.ctypes.data_as(C.c_void_p), peak.ctypes.data_as(C.c_void_p)))
    return amps, peak


def run_script(midis, device=0):
    """Everything the script's steps 3 to 6 compute for the notes `midis`, in one call: {"midis", "amps" [n][2][29][8], "y_peak" [n][2]};
    axis 1 is the carrier variant (0 approx, 1 midi)."""
    midis = [int(m) for m in midis]
    rows, _ = carriers(midis)
    kinds, params = script_laws()
    amps, peak = pickup_law(rows, kinds, params, device=device)
    return {"midis": midis, "amps": amps.reshape(len(midis), 2, kinds.size, N_HARMONICS), "y_peak": peak.reshape(len(midis), 2)}


# ---- step 1: inter-harmonic SNR of the recorded clips ------------------------------------------------------------------------------------
def read_clip(path):
    """sf.read(path) for PCM WAV: (int / 2^(bits - 1) as f64, the first channel as the script takes it; sample rate)."""
    import wave
    with open(path, "rb") as f:
        raw = bytearray(f.read())
    at = raw.find(b"fmt ")
    if at >= 0 and raw[at + 8:at + 10] == b"\xfe\xff" and raw[at + 32:at + 34] == b"\x01\x00":     # extensible PCM, as harmonics.load_audio
        raw[at + 8:at + 10] = b"\x01\x00"
    try:
        with wave.open(io.BytesIO(bytes(raw)), "rb") as w:
            channels, width, sr, payload = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.readframes(w.getnframes())
    except wave.Error as e:
        raise ValueError(f"{path}: not a PCM WAV file this reader understands ({e}); FLAC and float WAV are out of scope") from None
    if width == 2:
        ints = np.frombuffer(payload, dtype="<i2").astype(np.int64)
    elif width == 3:
        b = np.frombuffer(payload, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        ints = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        ints = ints - ((ints & 0x800000) << 1)
    elif width == 4:
        ints = np.frombuffer(payload, dtype="<i4").astype(np.int64)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples; this reader takes 16-, 24- or 32-bit PCM")
    data = (ints.astype(np.float64) / float(1 << (8 * width - 1))).reshape(-1, channels)
    return data[:, 0].copy(), sr


def snr_window(n, sr):
    """measure_interharmonic_floor's early_sustain window of a clip of n samples: (start, end), or None where the script returns NaN."""
    start, end = int(SNR_WINDOW[0] * sr), int(SNR_WINDOW[1] * sr)
    end = min(end, n)
    return None if start >= end else (start, end)


def snr_from_magnitudes(h_amps, noise_amps):
    snr = np.full(len(h_amps), np.nan)
    for i in range(len(h_amps)):
        if noise_amps[i] > 0 and h_amps[i] > 0:
            snr[i] = 20 * np.log10(h_amps[i] / noise_amps[i])
    return snr


def interharmonic_snr(clips, f0s, sample_rates, n_harmonics=8, device=0):
    """measure_interharmonic_floor (:97-148) of many clips: (h_amps [n][n_harmonics], snr [n][n_harmonics]); NaN rows where the window is
    empty.  Probes h f0 and (h + 0.5) f0 over [int(0.05 sr), min(int(0.2 sr), len)) through ow_dft_magnitudes, one call per distinct
    (window, rate): clips of one recording session share theirs."""
    from .intermod_audit import dft_magnitudes
    n = len(clips)
    h_amps, snr = np.full((n, n_harmonics), np.nan), np.full((n, n_harmonics), np.nan)
    groups = {}
    for i, (clip, sr) in enumerate(zip(clips, sample_rates)):
        w = snr_window(len(clip), sr)
        if w is not None:
            groups.setdefault((w, sr), []).append(i)
    for ((start, end), sr), idx in groups.items():
        rows = np.stack([np.asarray(clips[i], dtype=np.float64)[start:end] for i in idx])
        freqs = np.array([[h * f0s[i] for h in range(1, n_harmonics + 1)] + [(h + 0.5) * f0s[i] for h in range(1, n_harmonics + 1)] for i in idx])
        mags = dft_magnitudes(rows, 0, end - start, freqs, float(sr), device)
        for r, i in enumerate(idx):
            h_amps[i] = mags[r, :n_harmonics]
            snr[i] = snr_from_magnitudes(mags[r, :n_harmonics], mags[r, n_harmonics:])
    return h_amps, snr


# ---- the recorded side ----------------------------------------------------------------------------------------------------------------
def load_obm(path):
    """load_obm: {midi: {f0, db, amps, source_file}} from the early_sustain windows of harmonics.json."""
    with open(path) as f:
        data = json.load(f)
    out = {}
    for e in data:
        es = e["windows"]["early_sustain"]
        out[e["midi_note"]] = {"f0": e["f0"], "db": es["amps_dB_rel_H1"], "amps": es["amps_linear"], "source_file": e.get("source_file", "")}
    return out


def load_model(path):
    """load_model: read as the script reads it (and, like the script, used by nothing after)."""
    with open(path) as f:
        data = json.load(f)
    return {e["midi_note"]: {"f0": e["f0"], "db": e["windows"]["early_sustain"]["amps_dB_rel_H1"]} for e in data.values()}


def measure_snr(obm, device=0):
    """Step 1 for the notes whose source_file exists: {midi: (h2_snr, h3_snr)}, NaN for the others."""
    midis = [m for m in sorted(obm) if obm[m].get("source_file") and os.path.exists(obm[m]["source_file"])]
    read = [read_clip(obm[m]["source_file"]) for m in midis]
    _, snr = interharmonic_snr([c for c, _ in read], [obm[m]["f0"] for m in midis], [sr for _, sr in read], device=device)
    out = {m: (float("nan"), float("nan")) for m in obm}
    for m, row in zip(midis, snr):
        out[m] = (row[1], row[2])
    return out


# ---- the report -----------------------------------------------------------------------------------------------------------------------
def law_errors(obm, numbers, midis, variant, law):
    """The script's (h2e, h3e) lists of one law point over `midis`."""
    h2e, h3e = [], []
    for midi in midis:
        amps = numbers["amps"][numbers["midis"].index(midi)][variant][law]
        h1 = amps[0]
        if h1 > 0:
            h2_db = 20 * np.log10(amps[1] / h1) if amps[1] > 0 else -120
            h3_db = 20 * np.log10(amps[2] / h1) if amps[2] > 0 else -120
            h2e.append(obm[midi]["db"][1] - h2_db)
            h3e.append(obm[midi]["db"][2] - h3_db)
    return h2e, h3e


def report(obm, snr, numbers):
    """The script's stdout up to its SUMMARY banner: sections 1 to 6.  `snr`: {midi: (h2_snr, h3_snr)}; `numbers`: run_script's result for
    every note of `obm`."""
    out = io.StringIO()

    def p(s=""):
        out.write(s + "\n")

    bar = "=" * 95
    p(bar)
    p("H3 DEFICIT ANALYSIS v2 — SNR-Filtered, Outlier-Identified")
    p(bar)
    p("\n--- OBM Inter-Harmonic SNR Analysis (early_sustain) ---")
    p(f"{'MIDI':>4} {'f0':>7} {'H2 dB':>7} {'H3 dB':>7} {'H2 SNR':>7} {'H3 SNR':>7} {'Reliable?':>10}")
    reliable_h3 = {}
    for midi in sorted(obm):
        o = obm[midi]
        h2_snr, h3_snr = snr[midi]
        is_reliable = h3_snr > RELIABLE_SNR_DB if not np.isnan(h3_snr) else False
        reliable_h3[midi] = is_reliable
        tag = "YES" if is_reliable else "NO"
        p(f"{midi:>4} {o['f0']:>7.1f} {o['db'][1]:>7.2f} {o['db'][2]:>7.2f} {h2_snr:>7.1f} {h3_snr:>7.1f} {tag:>10}")

    p("\n--- Harmonic Pattern Analysis ---")
    p("Notes where H3 > H2 or H4 > H3 (anomalous — NOT possible from pure 1/(1-y)):")
    for midi in sorted(obm):
        o = obm[midi]
        db = o["db"]
        anomalies = []
        if db[2] > db[1]:
            anomalies.append(f"H3({db[2]:.1f}) > H2({db[1]:.1f})")
        if len(db) > 3 and db[3] > db[2]:
            anomalies.append(f"H4({db[3]:.1f}) > H3({db[2]:.1f})")
        if len(db) > 4 and db[4] > db[3]:
            anomalies.append(f"H5({db[4]:.1f}) > H4({db[3]:.1f})")
        if anomalies:
            p(f"  MIDI {midi} ({o['f0']:.0f} Hz): {', '.join(anomalies)}")

    p("\n--- Effective y_peak at each note (vel=80) ---")
    p(f"{'MIDI':>4} {'DS':>6} {'y_peak':>7} {'HPF@f0':>7} {'HPF@2f':>7} {'HPF@3f':>7}")
    for midi in sorted(obm):
        f0 = midi_to_freq(midi)
        ds = pickup_ds(midi)
        y_peak = numbers["y_peak"][numbers["midis"].index(midi)][0]
        hpf1 = f0 / np.sqrt(f0 ** 2 + HPF_FC ** 2)
        hpf2 = (2 * f0) / np.sqrt((2 * f0) ** 2 + HPF_FC ** 2)
        hpf3 = (3 * f0) / np.sqrt((3 * f0) ** 2 + HPF_FC ** 2)
        p(f"{midi:>4} {ds:>6.3f} {y_peak:>7.3f} {hpf1:>7.4f} {hpf2:>7.4f} {hpf3:>7.4f}")

    reliable_midis = [m for m in sorted(obm) if reliable_h3.get(m, False)]
    unreliable_midis = [m for m in sorted(obm) if not reliable_h3.get(m, False)]
    p(f"\n--- Reliable H3 notes (n={len(reliable_midis)}): {reliable_midis}")
    p(f"--- Unreliable/anomalous H3: {unreliable_midis}")
    if len(reliable_midis) < 3:
        p("\nToo few reliable notes for alpha optimization.")
        reliable_midis = [m for m in sorted(obm) if m not in FALLBACK_ANOMALOUS]
        p(f"Fallback: excluding known anomalous notes. Using n={len(reliable_midis)}: {reliable_midis}")

    p(f"\n{bar}")
    p("ALPHA SWEEP — Reliable notes only")
    p(bar)
    best = (1.0, 999, 999)
    for law, alpha in enumerate(ALPHAS):
        h2e, h3e = law_errors(obm, numbers, reliable_midis, 0, law)
        h3_rms = np.sqrt(np.mean(np.array(h3e) ** 2))
        combined = np.sqrt(np.mean(np.array(h2e) ** 2 + np.array(h3e) ** 2))
        if combined < best[2]:
            best = (alpha, h3_rms, combined)
        p(f"  alpha={alpha:.1f}  H2: {np.mean(h2e):+6.1f}±{np.std(h2e):.1f}  H3: {np.mean(h3e):+6.1f}±{np.std(h3e):.1f}  "
          f"H3_RMS={h3_rms:.1f}  Total={combined:.1f}")
    p(f"\nBest alpha (min total RMS on reliable): {best[0]:.1f}")

    p(f"\n{bar}")
    p("ALTERNATIVE: polynomial nonlinearity y/(1-y) * (1 + k*y)")
    p("This adds an asymmetric enhancement that boosts H3 relative to H2")
    p(bar)
    for j, k in enumerate(KS):
        h2e, h3e = law_errors(obm, numbers, reliable_midis, 1, len(ALPHAS) + j)
        h2m, h3m = np.mean(h2e), np.mean(h3e)
        h2s, h3s = np.std(h2e), np.std(h3e)
        p(f"  k={k:.1f}  H2: {h2m:+6.1f}±{h2s:.1f}  H3: {h3m:+6.1f}±{h3s:.1f}  "
          f"combined={np.sqrt(np.mean(np.array(h2e) ** 2 + np.array(h3e) ** 2)):.1f}")

    p(f"\n{bar}")
    p("ALTERNATIVE: y/(1-y^2) — symmetric gap modulation")
    p("Models reed that moves BOTH toward and away from plate")
    p(bar)
    for j, blend in enumerate(BLENDS):
        h2e, h3e = law_errors(obm, numbers, reliable_midis, 1, len(ALPHAS) + len(KS) + j)
        p(f"  blend={blend:.1f}  H2: {np.mean(h2e):+6.1f}±{np.std(h2e):.1f}  H3: {np.mean(h3e):+6.1f}±{np.std(h3e):.1f}  "
          f"combined={np.sqrt(np.mean(np.array(h2e) ** 2 + np.array(h3e) ** 2)):.1f}")
    return out.getvalue()


def analyse(harmonics_path, model_path=None, device=0):
    """The default command: the script's report for harmonics.json (model_harmonics.json is read, as the script reads it)."""
    obm = load_obm(harmonics_path)
    if model_path:
        load_model(model_path)
    snr = measure_snr(obm, device)
    return report(obm, snr, run_script(sorted(obm), device))


# ---- grid (ours) ----------------------------------------------------------------------------------------------------------------------
def parse_axis(text):
    """`lo:hi:step` (hi included: np.arange(lo, hi + step / 2, step)) or a comma list; empty: no points."""
    if not text:
        return np.zeros(0)
    if ":" in text:
        lo, hi, step = (float(x) for x in text.split(":"))
        if not step > 0:
            raise ValueError(f"{text!r}: the step must be positive")
        return np.arange(lo, hi + 0.5 * step, step)
    return np.array([float(x) for x in text.split(",")])


def grid_laws(alphas=(), ks=(), blends=()):
    kinds = [POWER] * len(alphas) + [FACTOR] * len(ks) + [BLEND] * len(blends)
    params = [float(x) for x in alphas] + [float(x) for x in ks] + [float(x) for x in blends]
    return np.asarray(kinds, dtype=np.int32), np.asarray(params, dtype=np.float64)


def grid_tables(obm, keys, kinds, params, amps):
    """The grid's two tables from the call's amplitudes [n_carriers][n_laws][>= 3]: (law rows, per-note rows).
    A law row: family, parameter, n, H2 mean / std, H3 mean / std, H3 RMS, total RMS over the (note, velocity) jobs with H1 > 0.
    A per-note row: for each (note, velocity) the law point with the smallest sqrt(h2e^2 + h3e^2), the first of equals."""
    law_rows, best = [], {}
    for law in range(len(kinds)):
        h2e, h3e = [], []
        for c, (midi, vel, _) in enumerate(keys):
            a = amps[c][law]
            if a[0] > 0:
                h2 = obm[midi]["db"][1] - (20 * np.log10(a[1] / a[0]) if a[1] > 0 else -120)
                h3 = obm[midi]["db"][2] - (20 * np.log10(a[2] / a[0]) if a[2] > 0 else -120)
                h2e.append(h2); h3e.append(h3)
                d = float(np.sqrt(h2 ** 2 + h3 ** 2))
                if (midi, vel) not in best or d < best[(midi, vel)][0]:
                    best[(midi, vel)] = (d, law, float(h2), float(h3))
        fam, par = FAMILIES[kinds[law]], float(params[law])
        if h2e:
            a2, a3 = np.array(h2e), np.array(h3e)
            law_rows.append((fam, par, len(h2e), float(np.mean(a2)), float(np.std(a2)), float(np.mean(a3)), float(np.std(a3)),
                             float(np.sqrt(np.mean(a3 ** 2))), float(np.sqrt(np.mean(a2 ** 2 + a3 ** 2)))))
        else:
            law_rows.append((fam, par, 0) + (float("nan"),) * 6)
    note_rows = [(midi, vel, FAMILIES[kinds[b[1]]], float(params[b[1]]), b[2], b[3], b[0]) for (midi, vel), b in sorted(best.items())]
    return law_rows, note_rows


LAW_HEADER = ("family", "parameter", "n", "h2_mean_db", "h2_std_db", "h3_mean_db", "h3_std_db", "h3_rms_db", "total_rms_db")
NOTE_HEADER = ("midi", "velocity", "family", "parameter", "h2_err_db", "h3_err_db", "distance_db")


def table_csv(header, rows):
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator="\n")
    w.writerow(header)
    for r in rows:
        w.writerow([repr(x) if isinstance(x, float) else x for x in r])
    return buf.getvalue()


def grid(obm, alphas=(), ks=(), blends=(), velocities=(VEL_MIDI,), device=0):
    """Every law point x the notes of `obm` x the velocity layers in one call (the integer-note scale): (law csv, per-note csv, amps)."""
    rows, keys = carriers(sorted(obm), velocities, variants=("midi",))
    kinds, params = grid_laws(alphas, ks, blends)
    amps, _ = pickup_law(rows, kinds, params, n_harmonics=3, device=device)
    law_rows, note_rows = grid_tables(obm, keys, kinds, params, amps)
    return table_csv(LAW_HEADER, law_rows), table_csv(NOTE_HEADER, note_rows), amps
