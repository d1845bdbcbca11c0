"""tools/wurli_compare.py of the reference on the GPU: recorded notes against renders of the same notes.

The reference renders one note per `cargo run` and analyses each clip with a Python STFT loop.  Here the renders of a run are batch
renders whose audio stays in HBM, and the analysis of all clips of a side takes four calls: `ow_stft_profile` twice (8192 / 512 over the
sustain slices for the harmonic profile, 4096 / 512 for the centroid) and `ow_frame_rms` twice (2048 / 512 for the decay, 1024 / 128 for
the attack; the first also returns the clip's sum of squares).  What stays on the host is the script's bookkeeping: the +-4-bin peak
pick, ratios and dB, the line fit, argmax, rounding, selection and the report.

Arithmetic: the reference holds float32 (its samples, its window, S); the device states the same algorithm in f64 on the reference's
float32 operands (see openwurli_hip.h, ow_stft_profile).  tests/wurli_compare_ref.py states both forms in numpy.

The recorded clip: the reference re-writes it with soundfile's default subtype (PCM_16) before analysing it, so what it analyses is a
16-bit requantisation.  `pcm16_roundtrip` states that step (lrint(x * 32767) on write, / 32768 on read, from libsndfile's source; no
soundfile is at hand to confirm it by a run); `real_as_is=True` switches it off.
"""
import ctypes as C
import json
import os
import sys
from collections import defaultdict

import numpy as np

from . import binding
from .binding import OwError

SR = 44100                       # the script analyses at 44 100 Hz whatever a file says
_WAV_MODES = {None: binding.WAV_NONE, "round": binding.WAV_ROUND, "truncate": binding.WAV_TRUNCATE}
NOTE_LO, NOTE_HI = 33, 96        # what `preamp-bench render` accepts


# ---- device primitives ---------------------------------------------------------------------------------------------------------------
def hann_f32(n_fft):
    """The script's window: np.hanning(n_fft).astype(float32), widened for the C-ABI."""
    return np.hanning(n_fft).astype(np.float32).astype(np.float64)


def _clip_args(clips, lengths, device_audio):
    """(pointer, n_clips, stride, on_device, lengths u32, keep-alive)."""
    if device_audio is not None:
        ptr, rows, stride = device_audio
        lens = np.ascontiguousarray(lengths, dtype=np.uint32)
        if lens.size != rows:
            raise ValueError(f"lengths: {lens.size} entries for {rows} rows")
        return C.c_void_p(int(ptr)), int(rows), int(stride), 1, lens, None
    arr = np.ascontiguousarray(clips, dtype=np.float64)
    if arr.ndim != 2:
        raise ValueError("clips: a [n_clips, stride] array")
    lens = np.full(arr.shape[0], arr.shape[1], dtype=np.uint32) if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint32)
    if lens.size != arr.shape[0]:
        raise ValueError(f"lengths: {lens.size} entries for {arr.shape[0]} rows")
    return arr.ctypes.data_as(C.c_void_p), arr.shape[0], arr.shape[1], 0, lens, arr


def stft_profile(clips, lengths=None, n_fft=8192, hop=512, sample_rate=SR, wav24=None, device=0, device_audio=None, mean_mag=True,
                 centroid=True, window=None):
    """``ow_stft_profile``: (mean_mag [n, n_fft / 2 + 1] or None, centroid [n] or None) of clips f64 [n, stride] with lengths[c] valid
    samples each; device_audio = (pointer, rows, stride) analyses rows that lie in HBM (`clips` is then ignored)."""
    lib = binding.load_library()
    ptr, n, stride, on_dev, lens, _keep = _clip_args(clips, lengths, device_audio)
    win = hann_f32(n_fft) if window is None else np.ascontiguousarray(window, dtype=np.float64)
    mm = np.zeros((n, n_fft // 2 + 1)) if mean_mag else None
    ce = np.zeros(n) if centroid else None
    rc = lib.ow_stft_profile(ptr, n, stride, lens.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p), int(n_fft), int(hop), float(sample_rate),
                             _WAV_MODES[wav24], int(device), on_dev, None if mm is None else mm.ctypes.data_as(C.c_void_p),
                             None if ce is None else ce.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise OwError(binding.take_error(lib))
    return mm, ce


def frame_count(length, frame_len, hop):
    return max(1, (int(length) - frame_len) // hop + 1)


def frame_rms(clips, lengths=None, frame_len=2048, hop=512, wav24=None, device=0, device_audio=None, sum_sq=True):
    """``ow_frame_rms``: (rms [n, most frames], n_frames [n], sum_sq [n] or None)."""
    lib = binding.load_library()
    ptr, n, stride, on_dev, lens, _keep = _clip_args(clips, lengths, device_audio)
    fs = max([frame_count(x, frame_len, hop) for x in lens] or [1])
    rms = np.zeros((n, fs)); nf = np.zeros(n, dtype=np.uint32); ss = np.zeros(n) if sum_sq else None
    rc = lib.ow_frame_rms(ptr, n, stride, lens.ctypes.data_as(C.c_void_p), int(frame_len), int(hop), _WAV_MODES[wav24], int(device), on_dev,
                          rms.ctypes.data_as(C.c_void_p), fs, nf.ctypes.data_as(C.c_void_p), None if ss is None else ss.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise OwError(binding.take_error(lib))
    return rms, nf, ss


# ---- the script's bookkeeping on what the device returns (unrounded figures first, the script's rounding on top) ----------------------
def harmonic_peaks(s_avg, sr, f0_hz, n_harmonics=10, n_fft=8192):
    """The peak of the mean spectrum within +-4 bins of the bin nearest to h * f0, h = 1.. while h * f0 <= sr / 2: (amplitudes, bins)."""
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    amps, bins = [], []
    for h in range(1, n_harmonics + 1):
        fh = f0_hz * h
        if fh > sr / 2:
            break
        idx = int(np.argmin(np.abs(freqs - fh)))
        lo, hi = max(0, idx - 4), min(len(s_avg), idx + 5)
        k = lo + int(np.argmax(s_avg[lo:hi]))
        amps.append(float(s_avg[k])); bins.append(k)
    return amps, bins


def profile_from_peaks(amps, f0_hz):
    if not amps or amps[0] < 1e-10:
        return None
    ratios = [a / amps[0] for a in amps]
    db = [20 * np.log10(r + 1e-10) for r in ratios]
    return {"n_harmonics": len(amps), "ratios": [round(r, 4) for r in ratios], "db": [round(float(d), 1) for d in db], "f0_hz": f0_hz}


def decay_slope(rms, sr, skip_attack_s=0.08, window_s=0.5, hop=512):
    """dB/s of the line through 20 log10(rms + 1e-10) over the frames after the attack; None with fewer than 5 frames.  Unrounded."""
    a = int(skip_attack_s * sr / hop)
    b = min(len(rms), int((skip_attack_s + window_s) * sr / hop))
    if b - a < 5:
        return None
    y = 20 * np.log10(np.asarray(rms[a:b], dtype=np.float64) + 1e-10)
    t = np.arange(len(y)) * hop / sr
    return float(np.polyfit(t, y, 1)[0])


def attack_frame(rms):
    """The first frame of the largest RMS; None for a silent clip."""
    if len(rms) == 0 or np.max(rms) < 1e-10:
        return None
    return int(np.argmax(rms))


def rms_db_value(sum_sq, n):
    return float(20 * np.log10(np.sqrt(sum_sq / n) + 1e-10)) if n else float("nan")


def _round1(x):
    return None if x is None else round(float(x), 1)


# ---- one clip at a time: the reference's functions ------------------------------------------------------------------------------------
def _one(y):
    return np.ascontiguousarray(y, dtype=np.float64)[None, :]


def harmonic_profile(y, sr, f0_hz, n_harmonics=10, n_fft=8192, device=0):
    mm, _ = stft_profile(_one(y), None, n_fft, 512, sr, device=device, centroid=False)
    return profile_from_peaks(harmonic_peaks(mm[0], sr, f0_hz, n_harmonics, n_fft)[0], f0_hz)


def measure_decay(y, sr, skip_attack_s=0.08, window_s=0.5, device=0):
    rms, nf, _ = frame_rms(_one(y), None, 2048, 512, device=device, sum_sq=False)
    return _round1(decay_slope(rms[0, :nf[0]], sr, skip_attack_s, window_s))


def measure_spectral_centroid(y, sr, n_fft=4096, device=0):
    _, ce = stft_profile(_one(y), None, n_fft, 512, sr, device=device, mean_mag=False)
    return round(float(ce[0]), 1)


def measure_rms(y, device=0):
    y = np.asarray(y)
    _, _, ss = frame_rms(_one(y), None, 2048, 512, device=device)
    return round(rms_db_value(ss[0], y.size), 1)


def measure_attack_time(y, sr, threshold_db=-10, device=0):
    rms, nf, _ = frame_rms(_one(y), None, 1024, 128, device=device, sum_sq=False)
    k = attack_frame(rms[0, :nf[0]])
    return None if k is None else round(float(k * 128 / sr * 1000), 1)


# ---- both sides of many notes ---------------------------------------------------------------------------------------------------------
def pcm16_roundtrip(y):
    """What soundfile's default WAV subtype leaves of a float clip: PCM_16 written as lrint(x * 32767) (clipped), read back as int / 32768."""
    q = np.clip(np.rint(np.asarray(y, dtype=np.float64) * 32767.0), -32768, 32767)
    return q / 32768.0


def _pack(clips):
    lens = np.array([len(c) for c in clips], dtype=np.uint32)
    arr = np.zeros((len(clips), max(int(lens.max(initial=0)), 1)))
    for i, c in enumerate(clips):
        arr[i, :len(c)] = c
    return arr, lens


def analyse_side(lengths, sustain, f0s, clips=None, device_audio=None, wav24=None, sr=SR, device=0):
    """The unrounded figures of one side of every pair.  lengths[c]: the clip's samples; sustain[c] = (start, n): its sustain slice.
    Host clips ([n, stride]) are re-packed for the slices; rows in HBM (device_audio) must share the slice's start."""
    n = len(lengths)
    if n == 0:
        return []
    lengths = np.asarray(lengths, dtype=np.uint32)
    sus_len = np.array([s[1] for s in sustain], dtype=np.uint32)
    if device_audio is not None:
        ptr, rows, stride = device_audio
        starts = {s[0] for s in sustain}
        if len(starts) != 1:
            raise ValueError("rows in device memory: every sustain slice must start at the same sample")
        sus = dict(device_audio=(int(ptr) + 8 * starts.pop(), rows, stride), clips=None)
        whole = dict(device_audio=device_audio, clips=None)
    else:
        sus_arr, _ = _pack([clips[i][s[0]:s[0] + s[1]] for i, s in enumerate(sustain)])
        sus = dict(clips=sus_arr)
        whole = dict(clips=clips)
    mm, _ = stft_profile(lengths=sus_len, n_fft=8192, hop=512, sample_rate=sr, wav24=wav24, device=device, centroid=False, **sus)
    _, ce = stft_profile(lengths=sus_len, n_fft=4096, hop=512, sample_rate=sr, wav24=wav24, device=device, mean_mag=False, **sus)
    r_dec, nf_dec, ss = frame_rms(lengths=lengths, frame_len=2048, hop=512, wav24=wav24, device=device, **whole)
    r_att, nf_att, _ = frame_rms(lengths=lengths, frame_len=1024, hop=128, wav24=wav24, device=device, sum_sq=False, **whole)
    out = []
    for i in range(n):
        amps, bins = harmonic_peaks(mm[i], sr, f0s[i])
        k = attack_frame(r_att[i, :nf_att[i]])
        out.append({"amps": amps, "bins": bins, "decay": decay_slope(r_dec[i, :nf_dec[i]], sr), "centroid": float(ce[i]),
                    "attack_frame": k, "attack_ms": None if k is None else float(k * 128 / sr * 1000), "rms_db": rms_db_value(ss[i], int(lengths[i]))})
    return out


def sustain_slices(len_real, len_synth, sr=SR):
    """compare_note's slices: skip the first 80 ms of a clip that is longer than that, keep min(len_real, len_synth, 1 s) samples."""
    skip = int(0.08 * sr)
    dur = min(len_real, len_synth, int(1.0 * sr))

    def one(n):
        return (skip, max(0, min(dur, n - skip))) if n > skip else (0, n)
    return one(len_real), one(len_synth)


def comparison_from_figures(real, synth, f0_hz):
    """compare_note's dictionary from the two sides' unrounded figures, with the script's rounding and truthiness tests."""
    hp_real, hp_synth = profile_from_peaks(real["amps"], f0_hz), profile_from_peaks(synth["amps"], f0_hz)
    dist = diffs_out = None
    if hp_real and hp_synth:
        n = min(len(hp_real["db"]), len(hp_synth["db"]))
        diffs = [hp_synth["db"][i] - hp_real["db"][i] for i in range(1, n)]
        dist = round(float(np.sqrt(np.mean(np.array(diffs) ** 2))), 1)
        diffs_out = [round(d, 1) for d in diffs]
    d_real, d_synth = _round1(real["decay"]), _round1(synth["decay"])
    c_real, c_synth = round(real["centroid"], 1), round(synth["centroid"], 1)
    return {
        "harmonics_real": hp_real, "harmonics_synth": hp_synth, "harmonic_distance_db": dist, "harmonic_diffs_db": diffs_out,
        "decay_real_db_s": d_real, "decay_synth_db_s": d_synth,
        "decay_diff_db_s": round(d_synth - d_real, 1) if (d_real and d_synth) else None,
        "centroid_real_hz": c_real, "centroid_synth_hz": c_synth,
        "centroid_diff_hz": round(c_synth - c_real, 1) if (c_real and c_synth) else None,
        "attack_real_ms": _round1(real["attack_ms"]), "attack_synth_ms": _round1(synth["attack_ms"]),
        "rms_real_db": round(real["rms_db"], 1), "rms_synth_db": round(synth["rms_db"], 1),
    }


def compare_many(reals, f0s, synths=None, synth_device=None, synth_lengths=None, synth_wav24=None, sr=SR, device=0, figures=None):
    """compare_note for many pairs.  reals: list of 1-D clips as the script analyses them (after `pcm16_roundtrip`, unless as-is);
    the other side: `synths` (list of 1-D clips) or `synth_device` = (pointer, rows, stride) with `synth_lengths`, analysed as the 24-bit
    file of quantiser `synth_wav24`.  Returns the list of comparison dictionaries; `figures` (a list) receives (real, synth) unrounded."""
    n = len(reals)
    if n == 0:
        return []
    real_arr, real_len = _pack(reals)
    if synth_device is None:
        synth_arr, synth_len = _pack(synths)
    else:
        synth_arr, synth_len = None, np.asarray(synth_lengths, dtype=np.uint32)
    if len(synth_len) != n or len(f0s) != n:
        raise ValueError("reals, synths and f0s differ in length")
    slices = [sustain_slices(int(a), int(b), sr) for a, b in zip(real_len, synth_len)]
    fr = analyse_side(real_len, [s[0] for s in slices], f0s, clips=real_arr, sr=sr, device=device)
    fs = analyse_side(synth_len, [s[1] for s in slices], f0s, clips=synth_arr, device_audio=synth_device, wav24=synth_wav24, sr=sr, device=device)
    if figures is not None:
        figures.extend(zip(fr, fs))
    return [comparison_from_figures(a, b, f0) for a, b, f0 in zip(fr, fs, f0s)]


def compare_note(real_path, synth_path, f0_hz, sr=SR, device=0):
    """The reference's compare_note on two PCM WAV files (read as they are: the tool has already re-written the real clip)."""
    y_real, y_synth = read_wav(real_path), read_wav(synth_path)
    return compare_many([y_real], [f0_hz], synths=[y_synth], sr=sr, device=device)[0]


def read_wav(path):
    """sf.read(path, dtype='float32') for PCM WAV: int / 2^(bits - 1), channels averaged; the file's rate is ignored as the script does."""
    import io
    import wave
    with open(path, "rb") as f:
        raw = bytearray(f.read())
    at = raw.find(b"fmt ")
    if at >= 0 and raw[at + 8:at + 10] == b"\xfe\xff" and raw[at + 32:at + 34] == b"\x01\x00":     # extensible PCM, as harmonics.load_audio
        raw[at + 8:at + 10] = b"\x01\x00"
    try:
        with wave.open(io.BytesIO(bytes(raw)), "rb") as w:
            channels, width, payload = w.getnchannels(), w.getsampwidth(), w.readframes(w.getnframes())
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
    data = (ints.astype(np.float64) / float(1 << (8 * width - 1))).astype(np.float32).reshape(-1, channels)
    data = data.mean(axis=1) if channels > 1 else data[:, 0]          # float32 mean, as the script's y.mean(axis=1)
    return data.astype(np.float64)


def write_wav16(path, y, sr):
    """sf.write(path, y, sr) with the default subtype: mono PCM_16, lrint(x * 32767)."""
    import wave
    q = np.clip(np.rint(np.asarray(y, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(sr))
        w.writeframes(q.tobytes())


# ---- selection and render jobs --------------------------------------------------------------------------------------------------------
def load_extractions(dirs):
    """The notes of every directory's extraction_metadata.json, each with its source directory and clip path."""
    found = []
    for d in dirs:
        meta = os.path.join(str(d), "extraction_metadata.json")
        if not os.path.exists(meta):
            print(f"  WARNING: No metadata in {d}", file=sys.stderr)
            continue
        with open(meta) as f:
            data = json.load(f)
        for note in data["notes"]:
            note["_source_dir"] = str(d)
            note["_wav_path"] = os.path.join(str(d), note["filename"])
            found.append(note)
    return found


def select_best_notes(all_notes, top_per_pitch=3, specific_notes=None):
    """midi -> the top_per_pitch best-isolated notes of that pitch (stable for equal scores), pitches ascending."""
    groups = defaultdict(list)
    for note in all_notes:
        groups[note["midi_note"]].append(note)
    chosen = {}
    for midi in sorted(groups):
        notes = sorted(groups[midi], key=lambda n: -n["isolation_score"])
        groups[midi][:] = notes                      # the script sorts the group in place
        if specific_notes and notes[0]["note_name"] not in specific_notes:
            continue
        chosen[midi] = notes[:top_per_pitch]
    return chosen


def velocity_midi(note_info, override=None):
    return override if override else max(1, min(127, int(note_info["velocity_norm"] * 127)))


def render_job(midi, vel, tier3=False, mlp=True):
    """The flags render_synth_note passes to `preamp-bench render` (whose MLP is on by default)."""
    if tier3:
        return {"note": int(midi), "velocity": int(vel), "mlp": mlp, "poweramp": True, "volume": 0.40, "speaker": 1.0}
    return {"note": int(midi), "velocity": int(vel), "mlp": mlp, "poweramp": False, "volume": 1.0, "speaker": 0.0}


def safe_name(note_name):
    return note_name.replace("#", "s").replace("♯", "s").replace("♭", "b")


def wav_names(note_name, idx, top_per_pitch):
    stem = safe_name(note_name) if top_per_pitch <= 1 else f"{safe_name(note_name)}_{idx}"
    return f"{stem}_real.wav", f"{stem}_synth.wav"


class Renders:
    """The renders of a list of (job, duration) in HBM: one batch call per distinct duration, rows [n][stride] at `ptr`."""

    def __init__(self, jobs, durations, sets=None, set_of_job=None, sr=SR, device=0):
        from . import engine, mlp
        lib = binding.load_library()
        self.lib, self.device, self.n = lib, int(device), len(jobs)
        self.lengths = np.array([int(d * sr) for d in durations], dtype=np.uint32)
        self.stride = max(int(self.lengths.max(initial=0)), 1)
        self.ptr = lib.ow_device_alloc(8 * max(self.n, 1) * self.stride, self.device)
        if not self.ptr:
            raise OwError(binding.take_error(lib))
        try:
            order = sorted(range(self.n), key=lambda i: (durations[i], i))
            self.row_of = {}
            row = 0
            groups = defaultdict(list)
            for i in order:
                groups[durations[i]].append(i)
            for dur, idx in groups.items():
                at = self.ptr + 8 * row * self.stride
                if sets is None:
                    engine.batch_render([jobs[i] for i in idx], float(sr), dur, device=device, out_device_ptr=at, stride=self.stride)
                else:
                    mlp.batch_render_mlp([jobs[i] for i in idx], sets, [set_of_job[i] for i in idx], float(sr), dur, device=device,
                                         out_device_ptr=at, stride=self.stride)
                for i in idx:
                    self.row_of[i] = row
                    row += 1
        except Exception:
            self.close()
            raise

    def row_lengths(self):
        """lengths in row order (rows are grouped by duration)."""
        out = np.zeros(self.n, dtype=np.uint32)
        for i, r in self.row_of.items():
            out[r] = self.lengths[i]
        return out

    def fetch(self):
        """The audio as a host array [n][stride], in job order."""
        host = np.zeros((max(self.n, 1), self.stride))
        if self.lib.ow_test_device_read(host.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), host.nbytes, self.device) != 0:
            raise OwError(binding.take_error(self.lib))
        return host[[self.row_of[i] for i in range(self.n)]] if self.n else host[:0]

    def close(self):
        if self.ptr:
            self.lib.ow_device_free(self.ptr, self.device)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def compare_rendered(reals, f0s, jobs, durations, sets=None, set_of_job=None, sr=SR, device=0, figures=None, audio_out=None):
    """Render jobs[i] for durations[i] seconds and compare it with reals[i], the audio analysed where the render left it, as the 24-bit
    file the command writes.  audio_out (a list) receives the renders as host rows [n][stride] and their lengths."""
    with Renders(jobs, durations, sets, set_of_job, sr, device) as r:
        rows = [r.row_of[i] for i in range(r.n)]
        # the device rows are grouped by duration: analyse in row order, then return to the callers' order
        inv = np.argsort(rows)
        out_fig = []
        comps = compare_many([reals[i] for i in inv], [f0s[i] for i in inv], synth_device=(r.ptr, r.n, r.stride), synth_lengths=r.row_lengths(),
                             synth_wav24="round", sr=sr, device=device, figures=out_fig)
        if audio_out is not None:
            audio_out.extend([r.fetch(), r.lengths.copy()])
    back = {int(j): k for k, j in enumerate(inv)}
    if figures is not None:
        figures.extend(out_fig[back[i]] for i in range(len(reals)))
    return [comps[back[i]] for i in range(len(reals))]


# ---- reports --------------------------------------------------------------------------------------------------------------------------
def _present(comparisons, key):
    return [c["comparison"][key] for c in comparisons if c["comparison"][key] is not None]


def format_comparison_report(comparisons, output_dir=None):
    bar = "=" * 70
    L = [f"\n{bar}", f"  WURLI A/B COMPARISON REPORT — {len(comparisons)} notes", bar]
    dist, decay, cent = (_present(comparisons, k) for k in ("harmonic_distance_db", "decay_diff_db_s", "centroid_diff_hz"))
    if dist:
        L += ["\n  HARMONIC DISTANCE (RMS dB, H2-H8 vs real)", f"    Mean:   {np.mean(dist):>6.1f} dB", f"    Median: {np.median(dist):>6.1f} dB",
              f"    Worst:  {max(dist):>6.1f} dB", f"    Best:   {min(dist):>6.1f} dB"]
    if decay:
        L += ["\n  DECAY RATE DIFFERENCE (synth - real, dB/s)", f"    Mean:   {np.mean(decay):>+6.1f} dB/s",
              "    (positive = synth decays faster, negative = synth sustains longer)"]
    if cent:
        L += ["\n  SPECTRAL CENTROID DIFFERENCE (synth - real, Hz)", f"    Mean:   {np.mean(cent):>+6.0f} Hz",
              "    (positive = synth brighter, negative = synth darker)"]
    octaves = defaultdict(list)
    for c in comparisons:
        octaves[c["midi_note"] // 12 - 1].append(c)
    L += ["\n  PER-OCTAVE BREAKDOWN", f"  {'Oct':>4s}  {'n':>3s}  {'HarmDist':>8s}  {'DecayΔ':>8s}  {'CentΔ':>8s}  Notes",
          f"  {'-' * 4}  {'-' * 3}  {'-' * 8}  {'-' * 8}  {'-' * 8}  {'-' * 20}"]
    for octave in sorted(octaves):
        notes = octaves[octave]
        hd, dd, cd = (_present(notes, k) for k in ("harmonic_distance_db", "decay_diff_db_s", "centroid_diff_hz"))
        hd_s = f"{np.mean(hd):>6.1f}dB" if hd else "   n/a  "
        dd_s = f"{np.mean(dd):>+6.1f}  " if dd else "   n/a  "
        cd_s = f"{np.mean(cd):>+6.0f}Hz " if cd else "   n/a  "
        L.append(f"  {octave:>4d}  {len(notes):>3d}  {hd_s}  {dd_s}  {cd_s}  {', '.join(sorted(set(c['note_name'] for c in notes)))}")
    if dist:
        L.append("\n  WORST HARMONIC MATCHES (biggest timbral gap):")
        for c in sorted(comparisons, key=lambda c: c["comparison"]["harmonic_distance_db"] or 0, reverse=True)[:5]:
            hd = c["comparison"]["harmonic_distance_db"]
            if hd is None:
                continue
            diffs = c["comparison"]["harmonic_diffs_db"]
            tail = " ".join(f"H{i + 2}:{d:+.0f}" for i, d in enumerate(diffs[:6])) if diffs else ""
            L.append(f"    {c['note_name']:>5s} iso={c['isolation']:.2f}  dist={hd:.1f}dB  {tail}")
        L.append("\n  BEST HARMONIC MATCHES (closest to real):")
        for c in sorted(comparisons, key=lambda c: c["comparison"]["harmonic_distance_db"] or 999)[:5]:
            hd = c["comparison"]["harmonic_distance_db"]
            if hd is None:
                continue
            L.append(f"    {c['note_name']:>5s} iso={c['isolation']:.2f}  dist={hd:.1f}dB")
    if output_dir:
        L += [f"\n  Output directory: {output_dir}", "  WAV pairs: <note>_real.wav / <note>_synth.wav", "  Full report: comparison_report.json"]
    return "\n".join(L) + "\n"


def print_comparison_report(comparisons, output_dir=None):
    sys.stdout.write(format_comparison_report(comparisons, output_dir))


def format_summary(all_notes):
    groups = defaultdict(list)
    for note in all_notes:
        groups[note["midi_note"]].append(note)
    bar = "=" * 60
    L = [f"\n{bar}", f"  EXTRACTION SUMMARY — {len(all_notes)} notes across {len(groups)} pitches", bar,
         f"\n  {'Note':>5s}  {'MIDI':>4s}  {'Count':>5s}  {'Best Iso':>8s}  {'Vel Range':>12s}  Sources",
         f"  {'-' * 5}  {'-' * 4}  {'-' * 5}  {'-' * 8}  {'-' * 12}  {'-' * 20}"]
    for midi in sorted(groups):
        notes = groups[midi]
        notes.sort(key=lambda n: -n["isolation_score"])
        vels = [n["velocity_norm"] for n in notes]
        sources = sorted(set(os.path.basename(os.path.normpath(n["_source_dir"])) for n in notes))
        L.append(f"  {notes[0]['note_name']:>5s}  {midi:>4d}  {len(notes):>5d}  {notes[0]['isolation_score']:>8.3f}  {min(vels):.2f}-{max(vels):.2f}   "
                 f"{', '.join(sources)}")
    span = set(range(41, 97))                       # F2 to C7
    covered = set(groups) & span
    missing = sorted(span - covered)
    L.append(f"\n  Coverage: {len(covered)}/{len(span)} Wurlitzer pitches ({len(covered) / len(span) * 100:.0f}%)")
    if missing:
        runs, run = [], [missing[0]]
        for m in missing[1:]:
            if m == run[-1] + 1:
                run.append(m)
            else:
                runs.append(run); run = [m]
        runs.append(run)
        gaps = [f"MIDI {r[0]}-{r[-1]}" if len(r) > 2 else ", ".join(f"MIDI {m}" for m in r) for r in runs]
        L.append(f"  Missing: {'; '.join(gaps)}")
    return "\n".join(L) + "\n"


def print_summary(all_notes):
    sys.stdout.write(format_summary(all_notes))


# ---- the tool's run -------------------------------------------------------------------------------------------------------------------
def plan_run(selected, top_per_pitch, output_dir, velocity=None, tier3=False):
    """What the script's loop decides per selected note before it renders, in the loop's order: the progress prefix, and either
    `missing` (no clip: the script's SKIP line) or the file names, velocity, duration and render job (None where `preamp-bench render`
    would fail, a pitch outside 33..96: the script's RENDER FAILED line)."""
    total = sum(len(v) for v in selected.values())
    plan, done = [], 0
    for midi, notes in sorted(selected.items()):
        for idx, info in enumerate(notes):
            done += 1
            head = f"  [{done}/{total}] {info['note_name']} (MIDI {midi}, iso={info['isolation_score']:.2f})..."
            if not os.path.exists(info["_wav_path"]):
                plan.append({"head": head, "missing": True, "job": None})
                continue
            real_name, synth_name = wav_names(info["note_name"], idx, top_per_pitch)
            vel = velocity_midi(info, velocity)
            ok = NOTE_LO <= midi <= NOTE_HI and 0 <= vel <= 127
            plan.append({"head": head, "missing": False, "midi": midi, "info": info, "velocity_midi": vel, "duration": max(0.5, info["duration"]),
                         "real_wav": os.path.join(str(output_dir), real_name), "synth_wav": os.path.join(str(output_dir), synth_name),
                         "job": render_job(midi, vel, tier3) if ok else None})
    return plan


def progress_tail(harmonic_distance):
    """What the script appends to a note's progress line (a distance of exactly 0.0 is falsy there)."""
    return f"dist={harmonic_distance:.1f}dB" if harmonic_distance else "n/a"


def result_entry(p, comp):
    info = p["info"]
    return {"note_name": info["note_name"], "midi_note": p["midi"], "f0_hz": info["f0_hz"], "isolation": info["isolation_score"],
            "velocity_norm": info["velocity_norm"], "velocity_midi": p["velocity_midi"], "duration": info["duration"],
            "source": os.path.basename(os.path.normpath(info["_source_dir"])), "real_wav": p["real_wav"], "synth_wav": p["synth_wav"],
            "comparison": comp}


def load_real(path, real_as_is=False):
    """The recorded clip as the script analyses it: read as float32, channels averaged, then (unless as-is) through a 16-bit file."""
    y = read_wav(path)
    return y if real_as_is else pcm16_roundtrip(y)


def rank_rows(names, tiers, per_config):
    """One row per configuration for `rank`: mean / median / worst harmonic distance, mean decay and centroid differences."""
    rows = []
    for (name, tier), comps in zip([(n, t) for n in names for t in tiers], per_config):
        dist = [c["harmonic_distance_db"] for c in comps if c["harmonic_distance_db"] is not None]
        decay = [c["decay_diff_db_s"] for c in comps if c["decay_diff_db_s"] is not None]
        cent = [c["centroid_diff_hz"] for c in comps if c["centroid_diff_hz"] is not None]

        def stat(f, v):
            return float(f(v)) if v else None
        rows.append({"weights": name, "tier": tier, "n_notes": len(comps), "harm_dist_mean_db": stat(np.mean, dist),
                     "harm_dist_median_db": stat(np.median, dist), "harm_dist_worst_db": stat(max, dist),
                     "decay_diff_mean_db_s": stat(np.mean, decay), "centroid_diff_mean_hz": stat(np.mean, cent)})
    return rows


def rank(reals, f0s, notes, velocities, durations, weight_sets, names, tiers=(2, 3), sr=SR, device=0):
    """The same notes under every (weight set, tier) configuration, rendered in one batch per distinct duration (ow_batch_render_mlp).
    weight_sets: MlpWeights, or "builtin" / None for the `identity` baseline.  Returns rank_rows."""
    from . import mlp
    real_sets, index = [], []
    for s in weight_sets:
        if s is None:
            index.append(0)
        else:
            index.append(len(real_sets))
            real_sets.append(mlp.MlpWeights.builtin() if isinstance(s, str) else s)
    jobs, soj, durs, rr, ff = [], [], [], [], []
    for si, s in enumerate(weight_sets):
        for tier in tiers:
            for i, m in enumerate(notes):
                jobs.append(render_job(m, velocities[i], tier3=(tier == 3), mlp=s is not None))
                soj.append(index[si]); durs.append(durations[i]); rr.append(reals[i]); ff.append(f0s[i])
    comps = compare_rendered(rr, ff, jobs, durs, real_sets or [mlp.MlpWeights.builtin()], soj, sr, device)
    n = len(notes)
    return rank_rows(names, list(tiers), [comps[k * n:(k + 1) * n] for k in range(len(weight_sets) * len(tiers))])
