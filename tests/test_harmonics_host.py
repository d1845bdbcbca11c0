"""The recording side's harmonics without a device: the numpy restatement (tests/harmonics_ref.py) against the outputs of the reference's
own Python (tests/golden/residuals_golden.npz), the binding's struct sizes, constants and cfg defaults, every refusal of ow_goertzel_harmonics and
ow_interharmonic_noise with its message, the segment planning of openwurli_amd/harmonics.py against the reference's pattern of skipped
windows for the seven fixture clips, the WAV reader, and the tools' text from canned results."""
import ctypes as C
import io
import json
import os
import sys
import wave
from contextlib import redirect_stdout

import numpy as np
import pytest

import harmonics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "residuals_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def clips(g):
    for i in range(int(g["n_clips"][0])):
        sr, midi, f0, vel, length = g[f"meta{i}"]
        yield i, g[f"pcm{i}"].astype(np.float64) / 32768.0, sr, int(midi), f0


# ---- the restatement against the reference ------------------------------------------------------------------------------------------------
def test_restatement_goertzel_equals_reference(golden):
    """Every extract_harmonics_goertzel call the reference made on the clips, restated: the same bits."""
    signals, plans, want = [], [], []
    for i, audio, sr, midi, f0 in clips(golden):
        for (a, b, nh), amps in zip(golden[f"gseg{i}"], golden[f"gamp{i}"]):
            c, k = ref.goertzel_plan(b - a, sr, f0, nh)
            signals.append(audio[a:b]); plans.append((c, k, ref.past_cut(sr, f0, nh))); want.append(amps[:nh])
    assert len(signals) == 33
    got = ref.goertzel_amps_many(signals, plans)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    assert np.array_equal(ref.goertzel_amps(signals[0], 44100.0, golden["meta0"][2]), want[0])
    # the cases the clips are there for: all eleven offsets on one bin, bins outside 0 < k < N // 2; and, beyond the clips (none of their
    # eight harmonics reaches it at 44.1 kHz), harmonics at or above the Nyquist cut
    assert any(len(set(k[0][k[0] >= 0])) == 1 for _, k, _ in plans)
    cut = ref.goertzel_amps(signals[-1], 44100.0, 4186.0)
    assert list(ref.past_cut(44100.0, 4186.0, 8)) == [False] * 5 + [True] * 3 and np.all(cut[5:] == 1e-20) and np.all(cut[:5] > 1e-20)
    assert np.all(ref.goertzel_plan(129, 44100.0, 100.0, 1)[1] == -1) and ref.goertzel_amps(np.ones(129), 44100.0, 100.0, 1)[0] == 1e-20


def test_restatement_noise_and_snr_equal_reference(golden):
    odd = even = 0
    for i, audio, sr, midi, f0 in clips(golden):
        assert np.array_equal(ref.interharmonic_snr(audio, sr, f0), golden[f"snr{i}"], equal_nan=True)
        a, b = ref.snr_window(len(audio), sr)
        assert np.array_equal(ref.noise_medians(audio[a:b], sr, f0), golden[f"snr_noise{i}"])
        for band in ref.noise_bands(b - a, sr, f0):
            if band is not None:
                odd += (band[1] - band[0] + 1) % 2
                even += (band[1] - band[0]) % 2
    assert odd and even                                       # np.median's two cases
    assert np.isnan(golden["snr4"][0]) and golden["snr6"][2] < 10.0 < golden["snr6"][1]
    assert ref.snr_window(2205 + 127, 44100.0) is None and ref.snr_window(2205 + 128, 44100.0) == (2205, 2333)


# ---- the binding's sizes, constants, defaults and exports (against the header: tests/test_abi_layout.py) -------------------------------------
def test_struct_layouts_header_binding():
    import openwurli_amd
    from openwurli_amd import binding as b
    assert [40, 24] == [C.sizeof(b.OwHarmonicsCfg), b.SEGMENT_DTYPE.itemsize]
    assert [b.GOERTZEL_OFFSETS, b.NOISE_MAX_BAND_BINS, b.MAX_HARMONICS] == [ref.N_OFFSETS, 4096, 8]
    cfg = b.OwHarmonicsCfg()
    assert (cfg.struct_size, cfg.segment_size, cfg.sample_rate, cfg.search_pct, cfg.wav24_mode, cfg.audio_is_device) == (40, 24, 44100.0, 0.01, b.WAV_NONE, 0)
    assert {"harmonics", "residuals"} <= set(openwurli_amd.__all__) and {"ow_goertzel_harmonics", "ow_interharmonic_noise"} <= set(b.SYMBOLS)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _segs(*rows):
    from openwurli_amd import binding as b
    return np.array([tuple(r) for r in rows], dtype=np.dtype(b.SEGMENT_DTYPE))


def _call(hiplib, fn, audio, n_rows, stride, segs, cfg, out=True, n_segs=None):
    hiplib.ow_clear_error()
    amps = np.zeros((max(len(segs), 1) if segs is not None else 1, 8))
    args = [None if audio is None else audio.ctypes.data_as(C.c_void_p), n_rows, stride, None if segs is None else segs.ctypes.data_as(C.c_void_p),
            (len(segs) if segs is not None else 0) if n_segs is None else n_segs, cfg, amps.ctypes.data_as(C.c_void_p) if out else None]
    if fn == "ow_goertzel_harmonics":
        args += [None, None]
    rc = getattr(hiplib, fn)(*args)
    msg = hiplib.ow_last_error().decode()
    hiplib.ow_clear_error()
    return rc, msg


@pytest.mark.parametrize("fn", ["ow_goertzel_harmonics", "ow_interharmonic_noise"])
def test_refusals(hiplib, fn):
    from openwurli_amd import binding as b
    Cfg = b.OwHarmonicsCfg
    audio = np.zeros((2, 1000))
    ok = _segs((0, 0, 1000, 8, 440.0))

    def refused(why, audio=audio, n_rows=2, stride=1000, segs=ok, cfg=None, **kw):
        got = _call(hiplib, fn, audio, n_rows, stride, segs, C.byref(cfg if cfg is not None else Cfg()), **kw)
        assert got == (-1, f"{fn}: {why}"), got

    assert _call(hiplib, fn, audio, 2, 1000, ok, None) == (-1, f"{fn}: null argument")
    for field, bad in (("struct_size", 32), ("segment_size", 16)):
        cfg = Cfg()
        setattr(cfg, field, bad)
        refused("ABI mismatch: ow_harmonics_cfg.struct_size / segment_size do not match this library's openwurli_hip.h (OW_ABI_VERSION 8)", cfg=cfg)
    for mode in (-2, 2):
        refused("unknown wav24_mode", cfg=Cfg(wav24_mode=mode))
    for sr in (0.0, -44100.0, float("inf"), float("nan")):
        refused("sample_rate is not a finite positive number", cfg=Cfg(sample_rate=sr))
    for pct in (-0.01, float("inf"), float("nan")):
        refused("search_pct is not a finite non-negative number", cfg=Cfg(search_pct=pct))
    refused("null argument", audio=None)
    refused("null argument", segs=None, n_segs=1)
    refused("null argument", out=False)
    for bad in ((2, 0, 1000, 8, 440.0), (0, 500, 500, 8, 440.0), (0, 600, 500, 8, 440.0), (0, 0, 1001, 8, 440.0), (0, 0, 1000, 9, 440.0)):
        refused("segment 1 out of range", segs=_segs(ok[0], bad))
    # refused before the audio is looked at: a stride the small buffer does not have
    refused("segment 0 longer than 2^22 samples", stride=(1 << 22) + 8, segs=_segs((0, 0, (1 << 22) + 1, 8, 440.0)))
    for f0 in (float("nan"), float("inf")):
        refused("segment 2: f0 is not finite", segs=_segs(ok[0], ok[0], (1, 0, 1000, 1, f0)))
    # the checks of the configuration come before an empty call returns; an empty call touches nothing
    assert _call(hiplib, fn, None, 0, 0, None, C.byref(Cfg(sample_rate=0.0)), out=False, n_segs=0)[0] == -1
    assert _call(hiplib, fn, None, 0, 0, None, C.byref(Cfg()), out=False, n_segs=0) == (0, "")


def test_noise_refuses_a_band_wider_than_the_kernel_holds(hiplib):
    from openwurli_amd import binding as b
    n = 1 << 20
    lo, hi = ref.noise_bands(n, 44100.0, 4000.0, 1)[0]
    assert hi - lo + 1 > b.NOISE_MAX_BAND_BINS
    got = _call(hiplib, "ow_interharmonic_noise", np.zeros((1, 8)), 1, n, _segs((0, 0, n, 1, 4000.0)), C.byref(b.OwHarmonicsCfg()))
    assert got == (-1, f"ow_interharmonic_noise: segment 0: the band of harmonic 1 holds {hi - lo + 1} bins, more than OW_NOISE_MAX_BAND_BINS (4096)")
    # the reference's own window is far inside: 0.15 s at 44.1 kHz, the highest band below the cut
    widest = max(b_[1] - b_[0] + 1 for b_ in ref.noise_bands(6615, 44100.0, 21900.0 / 1.5, 1))
    assert 200 < widest < 300


def test_python_calls_that_need_no_device(hiplib):
    from openwurli_amd import features
    assert features.goertzel_segments(np.zeros((1, 8)), 44100.0, []).shape == (0, 8)
    assert features.noise_segments(np.zeros((1, 8)), 44100.0, []).shape == (0, 8)
    amps, freqs, rms = features.extract_segments(np.zeros((1, 8)), 44100.0, [], method="goertzel")
    assert amps.shape == freqs.shape == (0, 8) and rms.shape == (0,)
    with pytest.raises(ValueError, match="unknown method"):
        features.extract_segments(np.zeros((1, 8)), 44100.0, [], method="dft")
    # a segment without a harmonic below the cut, or without an admissible bin, runs nothing on the device
    amps, coeffs, bins = features.goertzel_segments(np.ones((1, 200)), 44100.0, [(0, 0, 129, 1, 100.0), (0, 0, 200, 2, 21960.0), (0, 0, 200, 0, 440.0)], plan=True)
    assert amps[0, 0] == 1e-20 and np.all(amps[1, :2] == 1e-20) and np.all(amps[2] == 0.0) and np.all(bins == -1) and np.all(coeffs == 0.0)
    with pytest.raises(features.OwError, match="segment 0 out of range"):
        features.goertzel_segments(np.zeros((1, 8)), 44100.0, [(0, 0, 9, 1, 440.0)])


# ---- segment planning ---------------------------------------------------------------------------------------------------------------------
def test_plan_matches_the_reference_for_every_clip(golden):
    """plan_note against what the reference did: the segments of its Goertzel and FFT calls, in order, and the None pattern of both
    dictionaries (windows, decay points, overshoot)."""
    from openwurli_amd import harmonics
    notes = json.loads(str(golden["notes_json"]))
    seen = set()
    for i, audio, sr, midi, f0 in clips(golden):
        onset, segs = harmonics.plan_note(len(audio), sr, notes[i])
        assert onset == 0 and len(segs) == 11
        measured = [s for s in segs[:9] if s is not None]
        for key in ("gseg", "fseg"):
            assert [tuple(int(v) for v in row) for row in golden[f"{key}{i}"]] == measured, (i, key)
        for key in ("gold_json", "fft_json"):
            feat = json.loads(str(golden[f"{key}{i}"]))
            assert [feat["windows"][name] is None for name, _, _ in harmonics.WINDOWS] == [s is None for s in segs[:3]]
            assert [a is None for a in feat["decay"]["h1_amps"]] == [s is None for s in segs[3:9]]
            assert (feat["overshoot_dB"] is None) == (segs[9] is None) == (segs[10] is None)
            assert feat["duration_s"] == round(notes[i]["offset_s"] - notes[i]["onset_s"], 4)
        seen.add((tuple(s is None for s in segs[:3]), sum(s is not None for s in segs[3:9]), segs[9] is None))
    # the branches the clips were chosen for
    assert seen == {((False, False, False), 6, False), ((False, False, False), 4, False), ((False, False, False), 3, False),
                    ((False, False, True), 2, False), ((False, False, True), 1, False), ((False, True, True), 0, True)}
    # outside the audio, or empty
    assert harmonics.plan_note(1000, 44100.0, {"onset_s": 1.0, "offset_s": 2.0}) is None
    assert harmonics.plan_note(1000, 44100.0, {"onset_s": 0.01, "offset_s": 0.01}) is None
    # a note cut short by the end of the file: the windows shrink with the audio, not with the note's stated length
    onset, segs = harmonics.plan_note(44100 + 5000, 44100.0, {"onset_s": 1.0, "offset_s": 3.0})
    assert onset == 44100 and segs[0] == (0, 2205, 8) and segs[1] == (2205, 5000, 8) and segs[2] is None and segs[3] == (4410, 5000, 1) and segs[4] is None
    assert segs[9] == (0, 441, 0) and segs[10] == (4410, 5000, 0)


def test_bookkeeping_on_the_reference_s_amplitudes(golden, monkeypatch):
    """extract_many with the reference's own amplitudes in place of the device's: the dictionaries equal the reference's exactly
    (harmonic_mask -> None, the rounding, the decay fit, overshoot, centroids).  RMS comes from numpy here."""
    from openwurli_amd import harmonics, features
    notes = json.loads(str(golden["notes_json"]))
    for i, audio, sr, midi, f0 in clips(golden):
        for goertzel, key, seg_key, amp_key in ((True, "gold_json", "gseg", "gamp"), (False, "fft_json", "fseg", "famp")):
            table = {(int(a), int(b), int(nh)): (golden[f"{amp_key}{i}"][r], None if goertzel else golden[f"ffreq{i}"][r])
                     for r, (a, b, nh) in enumerate(golden[f"{seg_key}{i}"])}

            def fake(rows, sr_, segs, search_pct=0.01, device=0, wav24=None, device_audio=None, method="fft"):
                segs = list(segs)
                amps, freqs, rms = np.zeros((len(segs), 8)), np.zeros((len(segs), 8)), np.zeros(len(segs))
                for k, (row, a, b, nh, f) in enumerate(segs):
                    x = rows[row, a:b]
                    rms[k] = max(np.sqrt(np.mean(x ** 2)), 1e-20)
                    if nh:
                        assert (method == "goertzel") == goertzel
                        amps[k] = table[(a, b, nh)][0]
                        freqs[k, :nh] = [f * (h + 1) for h in range(nh)] if goertzel else table[(a, b, nh)][1][:nh]
                return amps, freqs, rms
            monkeypatch.setattr(features, "extract_segments", fake)
            got = harmonics.extract_note_features(audio, sr, notes[i], use_goertzel=goertzel)
            assert got == json.loads(str(golden[f"{key}{i}"])), (i, key)
    masked = json.loads(str(golden["fft_json1"]))["windows"]["attack"]
    assert masked["amps_linear"][4] is None and masked["freqs_hz"][7] is None and masked["amps_dB_rel_H1"][3] is not None


# ---- the WAV reader -----------------------------------------------------------------------------------------------------------------------
def _write_wav(path, ints, width, channels=1, sr=44100):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(sr)
        if width == 3:
            u = (np.asarray(ints, dtype=np.int64) & 0xFFFFFF)
            w.writeframes(np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], axis=-1).astype(np.uint8).tobytes())
        else:
            w.writeframes(np.asarray(ints, dtype={2: "<i2", 4: "<i4"}[width]).tobytes())


def test_wav_reader_round_trip(tmp_path, hiplib_host):
    from openwurli_amd import harmonics, features
    rng = np.random.default_rng(5)
    for width in (2, 3, 4):
        top = 1 << (8 * width - 1)
        ints = np.concatenate([[-top, top - 1, 0, -1, 1], rng.integers(-top, top, 500)])
        _write_wav(tmp_path / "m.wav", ints, width)
        data, sr = harmonics.load_audio(str(tmp_path / "m.wav"))
        assert sr == 44100 and data.dtype == np.float64 and np.array_equal(data, ints / float(top))
    stereo = rng.integers(-32768, 32768, (300, 2))
    _write_wav(tmp_path / "s.wav", stereo.reshape(-1), 2, channels=2)
    assert np.array_equal(harmonics.load_audio(str(tmp_path / "s.wav"))[0], (stereo / 32768.0).mean(axis=1))
    # the library's own 24-bit writer (WAVE_FORMAT_EXTENSIBLE): what it quantised is what comes back
    x = rng.uniform(-1, 1, 400)
    features.write_wav_24bit(str(tmp_path / "e.wav"), x, 44100)
    assert np.array_equal(harmonics.load_audio(str(tmp_path / "e.wav"))[0], features.quantize_24bit(x) / 8388608.0)
    # another rate: resampled by scipy's polyphase filter to the target, as the reference does
    _write_wav(tmp_path / "r.wav", rng.integers(-3000, 3000, 480), 2, sr=48000)
    data, sr = harmonics.load_audio(str(tmp_path / "r.wav"))
    assert sr == 44100 and len(data) == 441
    _write_wav(tmp_path / "b.wav", np.zeros(4, dtype=np.int64), 2)
    raw = bytearray(open(tmp_path / "b.wav", "rb").read())
    raw[20:22] = b"\x03\x00"                                   # IEEE float: not PCM
    open(tmp_path / "b.wav", "wb").write(raw)
    with pytest.raises(ValueError, match="not a PCM WAV file"):
        harmonics.load_audio(str(tmp_path / "b.wav"))


# ---- the tool's text ----------------------------------------------------------------------------------------------------------------------
def test_summary_text_and_tool_flags(golden, monkeypatch, tmp_path):
    from openwurli_amd import harmonics
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_harmonics as tool
    feats = json.loads(str(golden["features_json"]))
    want = "\n".join(["", "Extracted features for 7 notes", "  gold: 4", "  silver: 2", "  bronze: 1", "  attack window: 7/7 notes",
                      "  early_sustain window: 6/7 notes", "  sustain window: 3/7 notes", "  Decay rate: 3/7 notes", "  Overshoot: 6/7 notes"]) + "\n"
    assert harmonics.format_summary(feats) == want
    assert harmonics.format_summary([]).splitlines()[1:3] == ["Extracted features for 0 notes", "  gold: 0"]
    notes = json.loads(str(golden["notes_json"]))
    for n in notes:
        n["source_file"] = str(tmp_path / n["source_file"])
    for i, n in enumerate(notes[:2]):
        _write_wav(n["source_file"], golden[f"pcm{i}"], 2)
    (tmp_path / "scored.json").write_text(json.dumps(notes))
    seen = {}

    def fake(notes_, audio, min_tier="bronze", use_goertzel_for_gold=True, device=0, goertzel_all=False):
        seen["call"] = (len(notes_), sorted(os.path.basename(p) for p in audio), min_tier, use_goertzel_for_gold, device, goertzel_all)
        return feats[:2]
    monkeypatch.setattr(harmonics, "extract_all_harmonics", fake)
    buf = io.StringIO()
    with redirect_stdout(buf):
        tool.main(["--input", str(tmp_path / "scored.json"), "--output", str(tmp_path / "h.json"), "--min-tier", "silver", "--goertzel-all", "--device", "1"])
    # silver and up: clips 0, 1, 2, 4, 5, 6 are eligible, two of their files exist
    assert seen["call"] == (7, ["clip_0.wav", "clip_1.wav"], "silver", True, 1, True)
    text = buf.getvalue()
    assert text.count("could not read") == 4 and "Extracted features for 2 notes" in text and text.endswith(f"\nSaved to {tmp_path / 'h.json'}\n")
    assert json.loads((tmp_path / "h.json").read_text()) == feats[:2]
    with redirect_stdout(io.StringIO()):
        tool.main(["--input", str(tmp_path / "scored.json"), "--output", str(tmp_path / "h.json")])
    assert seen["call"][2:] == ("bronze", True, 0, False)


def test_extract_all_harmonics_report_and_passthrough(golden, monkeypatch):
    """Tier filter, grouping by file, the report lines in the script's order, the passthrough keys -- with the measuring stubbed out."""
    from openwurli_amd import harmonics
    notes = json.loads(str(golden["notes_json"]))
    audio = {n["source_file"]: (golden[f"pcm{i}"] / 32768.0, 44100) for i, n in enumerate(notes) if i != 3}
    calls = []

    def fake(items, device=0):
        calls.append([(it[2]["id"], it[3]) for it in items])
        return [None if it[2]["id"] == "clip_5" else {"id": it[2]["id"]} for it in items]
    monkeypatch.setattr(harmonics, "extract_many", fake)
    buf = io.StringIO()
    with redirect_stdout(buf):
        got = harmonics.extract_all_harmonics(notes, audio, min_tier="silver")
    assert calls == [[("clip_0", True), ("clip_1", False), ("clip_2", True), ("clip_4", True), ("clip_5", False), ("clip_6", True)]]
    assert [f["id"] for f in got] == ["clip_0", "clip_1", "clip_2", "clip_4", "clip_6"]
    assert got[1] == {"id": "clip_1", "isolation_tier": "silver", "isolation_score": 0.6, "velocity_midi": 64, "source_file": "clip_1.wav"}
    assert buf.getvalue().splitlines()[:3] == ["Extracting harmonics for 6 notes (>= silver)...", "  Loading clip_0.wav...", "    Extracted 1 notes"]
    calls.clear()
    with redirect_stdout(io.StringIO()) as out:
        harmonics.extract_all_harmonics(notes, audio, min_tier="bronze", use_goertzel_for_gold=False)
    assert all(not g for _, g in calls[0]) and "    ERROR loading: no audio given for clip_3.wav" in out.getvalue().splitlines()
    calls.clear()
    with redirect_stdout(io.StringIO()):
        harmonics.extract_all_harmonics(notes, audio, goertzel_all=True)
    assert all(g for _, g in calls[0])
