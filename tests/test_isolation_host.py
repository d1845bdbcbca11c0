"""Recorded-note intake without a device: the Python restatement (tests/isolation_ref.py) against the outputs of the reference's own
Python (tests/golden/isolation_golden.json, tests/golden/intake_golden.npz) bit for bit, the binding's struct sizes, window
planning, id keys and file grouping of openwurli_amd/isolation.py, the decay and collision tables against the restatement, the report
text, the tools' argument surface, and every refusal of ow_isolation_score / ow_clip_bounds that is decided before the device is touched."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import isolation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 44100


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "isolation_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def intake():
    return np.load(os.path.join(ROOT, "tests", "golden", "intake_golden.npz"))


# ---- the restatement is the reference -------------------------------------------------------------------------------------------------------
def test_restatement_scores_equal_the_reference(golden):
    notes = json.loads(json.dumps(golden["notes_in"]))
    raw = ref.score_notes(notes)
    assert json.dumps(notes, indent=2) == golden["scored_text"]
    assert len(raw) == len(golden["raw"])
    for got, want in zip(raw, golden["raw"]):
        assert (got is None and want is None) or list(got) == want
    table = ref.collision_table()
    again = json.loads(json.dumps(golden["notes_in"]))
    assert ref.score_notes(again, table=table) == raw and again == notes      # the table stands for harmonic_collision_check


def test_restatement_nudge_equals_the_stored_movement(golden):
    """The bar of the GPU test is derived from `nudge`: the restatement, with its 10 ** x moved by the same ulp, moves as the reference did."""
    raw = golden["raw"]
    move = {"temporal": 0.0, "dominance": 0.0}
    for to in (np.inf, -np.inf):
        def p10(x):
            v = 10.0 ** x
            for _ in range(golden["nudge_ulp"]):
                v = float(np.nextafter(v, to))
            return v
        shifted = ref.score_notes(json.loads(json.dumps(golden["notes_in"])), p10)
        for r, s in zip(raw, shifted):
            if r is not None:
                move["temporal"] = max(move["temporal"], abs(r[0] - s[0]))
                move["dominance"] = max(move["dominance"], abs(r[2] - s[2]))
    assert move == golden["nudge"] and golden["nudge_ulp"] == 4


def test_restatement_intake_equals_the_reference(intake):
    audio = intake["pcm"].astype(np.float64) / 32768.0
    notes = json.loads(str(intake["notes_in_json"]))
    corrected, removed, probes = ref.correct_octave_errors(notes, audio, SR)
    assert (corrected, removed) == (int(intake["corrected"][0]), int(intake["removed"][0])) == (2, 2)
    assert notes == json.loads(str(intake["notes_out_json"]))
    want = intake["probes"]
    for i, pr in enumerate(probes):
        if pr is None:
            assert np.all(np.isnan(want[i]))
            continue
        assert pr[0] == want[i, 0]
        assert pr[1] == (1e-20 if np.isnan(want[i, 1]) else max(want[i, 1], 1e-20))
        assert pr[2] == (0.0 if np.isnan(want[i, 2]) else want[i, 2]) and pr[3] == (0.0 if np.isnan(want[i, 3]) else want[i, 3])
    for i in range(int(intake["n_clips"][0])):
        x = intake[f"clip{i}"]
        assert list(ref.obm_seconds(x, SR)) == list(intake[f"clip_sec{i}"]), i
        peak, first, last = ref.clip_bounds(x)
        if peak >= 1e-10:
            assert [first, last] == list(intake[f"clip_idx{i}"]), i


# ---- the binding's sizes and the exports (against the header: tests/test_abi_layout.py) ---------------------------------------------------------
def test_struct_layouts_header_binding():
    import openwurli_amd
    from openwurli_amd import binding as b
    assert [56, 48] == [C.sizeof(b.OwIsoNote), C.sizeof(b.OwIsoCfg)] and b.ISO_NOTE_DTYPE.itemsize == 56
    assert {"isolation", "note_intake"} <= set(openwurli_amd.__all__)
    assert {"ow_isolation_score", "ow_isolation_collision_table", "ow_clip_bounds"} <= set(b.SYMBOLS)


# ---- planning ---------------------------------------------------------------------------------------------------------------------------------
def test_window_planning_keys_and_grouping(golden):
    from openwurli_amd import isolation
    notes = golden["notes_in"]
    rec, file_first, order = isolation.plan_notes(notes)
    files = list(dict.fromkeys(n["source_file"] for n in notes))           # order of first appearance
    assert sorted(order) == list(range(len(notes))) and len(file_first) == len(files) + 1 and file_first[0] == 0 and file_first[-1] == len(notes)
    for f, name in enumerate(files):
        idx = order[int(file_first[f]):int(file_first[f + 1])]
        assert idx == [i for i, n in enumerate(notes) if n["source_file"] == name]        # list order inside a file
    keys = {}
    for k, i in enumerate(order):
        n = notes[i]
        assert (rec["window_start"][k], rec["window_end"][k]) == ref.window_of(n) == isolation.plan_window(n)
        assert (rec["onset_s"][k], rec["offset_s"][k], rec["amplitude"][k], rec["midi_note"][k]) == (n["onset_s"], n["offset_s"], n["amplitude"], n["midi_note"])
        assert keys.setdefault(n["id"], rec["id_key"][k]) == rec["id_key"][k]
        scored = n["source_type"] != "obm_isolated" and ref.duration_score(n["offset_s"] - n["onset_s"]) != 0.0
        assert bool(rec["score"][k]) == scored == (golden["raw"][i] is not None)
    assert len(set(keys.values())) == len(keys) == len(notes) - 1           # the two "dup" notes share a key, nobody else does
    # the fallback of :269-271 cannot be reached by a scored note (duration >= 0.15 > 0.05); the planner has it all the same
    assert isolation.plan_window({"onset_s": 1.0, "offset_s": 1.02}) == (1.0, 1.02)
    assert isolation.plan_window({"onset_s": 1.0, "offset_s": 3.0}) == (1.0 + 0.050, 1.0 + 0.800)
    assert isolation.plan_notes([])[0].size == 0


def test_host_helpers_equal_the_restatement():
    from openwurli_amd import isolation
    for d in (0.0, 0.1499, 0.15, 0.2999, 0.3, 0.5999, 0.6, 5.0):
        assert isolation.score_duration(d) == ref.duration_score(d)
    rng = np.random.default_rng(5)
    for t, c, dom in rng.uniform(0.0, 1.0, (50, 3)):
        for d in (0.0, 0.3, 0.7, 1.0):
            got = isolation.compute_composite_score(t, c, dom, d)
            assert got == ref.composite(t, c, dom, d) and isolation.tier_from_score(got) == ref.tier(got)
    assert isolation.compute_composite_score(0.5, 0.0, 0.5, 1.0) == 0.0
    assert [isolation.tier_from_score(s) for s in (0.85, 0.849999, 0.55, 0.15, 0.149999)] == ["gold", "silver", "silver", "bronze", "reject"]


def test_decay_and_collision_tables(hiplib):
    from openwurli_amd import isolation
    rate, freq = isolation.decay_rate_table(), isolation.midi_freq_table()
    assert rate.shape == freq.shape == (128,)
    assert all(rate[m] == ref.decay_rate(m) and freq[m] == ref.midi_to_freq(m) for m in range(128))
    assert isolation.COLLISION_RATIO == 2.0 ** (50.0 / 1200.0)
    table = isolation.collision_table()
    want = ref.collision_table()
    assert table.dtype == np.uint8 and np.array_equal(table, want)
    # unison; an octave above takes the even harmonics; an octave below reaches the first four only; far apart
    assert table[60, 60] == 0 and table[60, 72] == 0b01010101 and table[72, 60] == 0xF0 and table[0, 127] == 0xFF
    # refusals of the table builder
    bad = freq.copy()
    bad[17] = np.nan
    out = np.zeros((128, 128), dtype=np.uint8)
    assert hiplib.ow_isolation_collision_table(bad.ctypes.data_as(C.c_void_p), 1.03, out.ctypes.data_as(C.c_void_p)) == -1
    assert hiplib.ow_last_error().decode() == "ow_isolation_collision_table: midi_freq[17]: value is not finite"
    assert hiplib.ow_isolation_collision_table(None, 1.03, out.ctypes.data_as(C.c_void_p)) == -1 and b"null argument" in hiplib.ow_last_error()
    assert hiplib.ow_isolation_collision_table(freq.ctypes.data_as(C.c_void_p), 1.03, None) == -1 and b"null argument" in hiplib.ow_last_error()
    hiplib.ow_clear_error()


# ---- refusals decided before the device is touched ----------------------------------------------------------------------------------------------
def _score_call(hiplib, rec, file_first, cfg=None, null=None):
    from openwurli_amd import binding as b, isolation
    rate, freq = isolation.decay_rate_table(), isolation.midi_freq_table()
    if cfg is None:
        cfg = b.OwIsoCfg(isolation.COLLISION_RATIO, rate.ctypes.data_as(C.POINTER(C.c_double)), freq.ctypes.data_as(C.POINTER(C.c_double)))
    n = rec.size
    ff = np.asarray(file_first, dtype=np.uint64)
    outs = [np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)]
    args = [rec.ctypes.data_as(C.c_void_p), n, ff.ctypes.data_as(C.c_void_p), ff.size - 1, C.byref(cfg)] + [o.ctypes.data_as(C.c_void_p) for o in outs]
    if null is not None:
        args[null] = None
    hiplib.ow_clear_error()
    rc = hiplib.ow_isolation_score(*args)
    msg = hiplib.ow_last_error().decode()
    hiplib.ow_clear_error()
    return rc, msg


def _records(n=3):
    from openwurli_amd import binding as b
    rec = np.zeros(n, dtype=np.dtype(b.ISO_NOTE_DTYPE))
    for k in range(n):
        rec[k] = (k, k + 1.0, 0.5, k + 0.05, k + 0.8, k, 60 + k, 1)
    return rec


def test_isolation_score_refusals(hiplib):
    from openwurli_amd import binding as b
    FN = "ow_isolation_score: "
    rec = _records()
    assert _score_call(hiplib, rec[:0], [0]) == (0, "")                                   # n_notes == 0
    for null in (0, 2, 5, 6, 7, 8):
        assert _score_call(hiplib, rec, [0, 3], null=null) == (-1, FN + "null argument")
    assert _score_call(hiplib, rec, [0, 3], null=4) == (-1, FN + "null argument")
    for field in ("struct_size", "note_size"):
        cfg = b.OwIsoCfg()
        setattr(cfg, field, 8)
        assert _score_call(hiplib, rec, [0, 3], cfg=cfg) == (-1, FN + "ABI mismatch: ow_iso_cfg.struct_size / note_size do not match this library's openwurli_hip.h (OW_ABI_VERSION 8)")
    assert _score_call(hiplib, rec, [0, 3], cfg=b.OwIsoCfg(1.03)) == (-1, FN + "null argument")      # no tables
    for midi in (-1, 128):
        bad = rec.copy()
        bad["midi_note"][1] = midi
        assert _score_call(hiplib, bad, [0, 3]) == (-1, FN + "note 1: midi_note outside 0..127")
    for field in ("onset_s", "offset_s", "amplitude", "window_start", "window_end"):
        for v in (np.nan, np.inf, -np.inf):
            bad = rec.copy()
            bad[field][2] = v
            assert _score_call(hiplib, bad, [0, 3]) == (-1, FN + f"note 2: {field} is not finite")
    assert _score_call(hiplib, rec, [0, 2, 1, 3]) == (-1, FN + "file 1: range is not ascending")
    assert _score_call(hiplib, rec, [0, 4, 3]) == (-1, FN + "file 0: range is not ascending")
    for ff in ([1, 3], [0, 2], [0]):
        rc, msg = _score_call(hiplib, rec, ff)
        assert rc == -1 and msg.startswith(FN + "file ranges do not cover the notes")


def test_clip_bounds_refusals(hiplib):
    FN = "ow_clip_bounds: "
    x = np.zeros((2, 8))
    lens = np.array([8, 8], dtype=np.uint32)
    peak, first, last = np.zeros(2), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(x=x, n=2, stride=8, lens=lens, on=0.1, off=0.01, outs=(peak, first, last)):
        hiplib.ow_clear_error()
        rc = hiplib.ow_clip_bounds(p(x), n, stride, p(lens), on, off, 0, p(outs[0]), p(outs[1]), p(outs[2]))
        msg = hiplib.ow_last_error().decode()
        hiplib.ow_clear_error()
        return rc, msg
    assert call(n=0) == (0, "")
    assert call(x=None) == call(lens=None) == call(outs=(None, first, last)) == call(outs=(peak, None, last)) == call(outs=(peak, first, None)) == (-1, FN + "null argument")
    assert call(on=np.nan) == (-1, FN + "onset_frac is not finite") and call(off=np.inf) == (-1, FN + "offset_frac is not finite")
    assert call(stride=0)[0] == -1
    assert call(lens=np.array([8, 9], dtype=np.uint32)) == (-1, FN + "clip 1: length 9 exceeds the stride 8")


# ---- text and tools ---------------------------------------------------------------------------------------------------------------------------
def test_report_text(golden):
    from openwurli_amd import isolation
    scored = json.loads(golden["scored_text"])
    assert isolation.format_summary(scored) == golden["report"]
    assert isolation.format_summary([]) == "\nIsolation scoring summary (0 notes):\n     gold:     0 (  0.0%)\n   silver:     0 (  0.0%)\n" \
                                           "   bronze:     0 (  0.0%)\n   reject:     0 (  0.0%)\n  usable:     0 (bronze+)\n\nPer-source breakdown:\n"


def test_score_isolation_tool_surface(golden, monkeypatch, tmp_path, capsys):
    """The tool's flags, lines and file, with the device call replaced by the restatement's numbers."""
    from openwurli_amd import isolation
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import score_isolation as tool
    seen = {}

    def fake(records, file_first, device=0, kernel_ms=False):
        seen["device"] = device
        n = len(records)
        out = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
        notes = golden["notes_in"]
        _, _, order = isolation.plan_notes(notes)
        by_file = {}
        for nt in notes:
            by_file.setdefault(nt["source_file"], []).append(nt)
        for k, i in enumerate(order):
            if records["score"][k]:
                t, c, d, mask = ref.sub_scores(notes[i], by_file[notes[i]["source_file"]])
                out[0][k], out[1][k], out[2][k], out[3][k] = t, c, d, sum(1 << h for h in range(8) if mask[h])
        return out
    monkeypatch.setattr(isolation, "isolation_scores", fake)
    src, dst = tmp_path / "notes.json", tmp_path / "scored.json"
    src.write_text(json.dumps(golden["notes_in"]))
    tool.main(["--input", str(src), "--output", str(dst), "--device", "3"])
    assert seen["device"] == 3 and dst.read_text() == golden["scored_text"]
    assert capsys.readouterr().out == f"Scoring isolation for {len(golden['notes_in'])} notes...\n" + golden["report"] + f"\nSaved to {dst}\n"
    with pytest.raises(SystemExit):
        tool.main(["--no-such-flag"])


def test_extract_notes_tool_surface(intake, monkeypatch, tmp_path, capsys):
    """--obm-only, --events, a recording without an events file; the device calls replaced by the restatement."""
    import wave
    from openwurli_amd import note_intake
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_notes as tool
    monkeypatch.setattr(note_intake, "clip_bounds", lambda clips, **k: tuple(np.array(v) for v in zip(*[ref.clip_bounds(c) for c in clips])))

    def fake_probes(notes, audio, sr, device=0):
        return [ref.probes(n, np.asarray(audio), sr) for n in notes]
    monkeypatch.setattr(note_intake, "probe_amplitudes", fake_probes)
    indir = tmp_path / "input"
    (indir / note_intake.OBM_SUBDIR).mkdir(parents=True)
    (tmp_path / "ev").mkdir()

    def write(path, pcm):
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR); w.writeframes(pcm.astype("<i2").tobytes())
    pcm = intake["pcm"]
    write(indir / "intake.wav", pcm)
    write(indir / "orphan.wav", pcm[:4410])
    write(indir / "model_render.wav", pcm[:4410])                                         # skipped by name
    fname, midi, f0 = note_intake.OBM_FILES[3]
    write(indir / note_intake.OBM_SUBDIR / fname, pcm[:11025])
    (tmp_path / "ev" / "intake.events.json").write_text(json.dumps(intake["events"].tolist()))
    out = tmp_path / "notes.json"
    notes = tool.main(["--input-dir", str(indir), "--output", str(out), "--events", str(tmp_path / "ev")])
    text = capsys.readouterr().out
    assert json.loads(out.read_text()) == notes and out.read_text() == json.dumps(notes, indent=2)
    on, off = ref.obm_seconds(pcm[:11025] / 32768.0, SR)
    assert notes[0] == {"id": f"obm_{midi}", "onset_s": round(on, 4), "offset_s": round(off, 4), "midi_note": midi, "measured_f0": f0, "amplitude": 0.63,
                        "velocity_midi": 80, "source_file": os.path.abspath(str(indir / note_intake.OBM_SUBDIR / fname)), "source_type": "obm_isolated",
                        "isolation_tier": "gold"} and list(notes[0]) == ["id", "onset_s", "offset_s", "midi_note", "measured_f0", "amplitude",
                                                                         "velocity_midi", "source_file", "source_type", "isolation_tier"]
    want = json.loads(str(intake["notes_out_json"]))
    for n in want:
        n["source_file"] = os.path.abspath(str(indir / "intake.wav"))
    assert notes[1:] == want
    assert text.count("WARNING: missing") == 12 and "  1 OBM notes extracted\n" in text and "\nFound 2 polyphonic recordings:\n  intake.wav\n  orphan.wav\n" in text
    assert "    -> 10 notes detected, verifying pitches...\n    -> 2 octave-corrected, 2 weak-removed, 8 kept\n" in text
    assert f"  ERROR processing {indir / 'orphan.wav'}: " in text and "orphan.events.json" in text
    assert f"\nTotal: 9 notes\n  basic_pitch: 8\n  obm_isolated: 1\n  MIDI range: 33-126\n\nSaved to {out}\n" in text
    notes = tool.main(["--input-dir", str(indir), "--output", str(out), "--obm-only"])
    assert len(notes) == 1 and "polyphonic" not in capsys.readouterr().out


def test_sustain_window_planning(monkeypatch):
    """note_intake.sustain_windows on hand-made clips, the device's bounds replaced by the restatement's."""
    from openwurli_amd import note_intake
    monkeypatch.setattr(note_intake, "clip_bounds", lambda clips, **k: tuple(np.array(v) for v in zip(*[ref.clip_bounds(c) for c in clips])))
    x = np.zeros(1000)
    x[100], x[400] = 0.2, 1.0                               # the first sample above a tenth of the peak is the onset
    clips = [x, x[:300], np.zeros(50), x[:120]]
    got = note_intake.sustain_windows(clips, 1000)
    assert got == [(250, 900, 100), (250, 300, 100), (0, 50, 0), (0, 120, 100)] == [ref.sustain_window(c, 1000) for c in clips]


def test_notes_from_events_fields():
    from openwurli_amd import note_intake
    got = note_intake.notes_from_events([(0.123456, 1.5, 59.6, 0.33333, [0, 1]), [2.0, 2.5, 21, 0.0], [3.0, 3.5, 108, 1.2]], "/somewhere/take 1.wav")
    assert got[0] == {"id": "take 1_0000", "onset_s": 0.1235, "offset_s": 1.5, "midi_note": 60, "measured_f0": 261.63, "amplitude": 0.3333,
                      "velocity_midi": 42, "source_file": "/somewhere/take 1.wav", "source_type": "basic_pitch", "isolation_tier": "pending"}
    assert list(got[0]) == ["id", "onset_s", "offset_s", "midi_note", "measured_f0", "amplitude", "velocity_midi", "source_file", "source_type", "isolation_tier"]
    assert (got[1]["id"], got[1]["velocity_midi"], got[2]["velocity_midi"], got[2]["midi_note"]) == ("take 1_0001", 1, 127, 108)


def test_probe_planning_equals_the_restatement(intake):
    from openwurli_amd import note_intake
    notes = json.loads(str(intake["notes_in_json"]))
    n_audio = len(intake["pcm"])
    taken = ~np.isnan(intake["probes"])
    for i, n in enumerate(notes):
        win = note_intake.plan_probe_window(n, n_audio, SR)
        assert win == ref.probe_window(n, n_audio, SR)
        assert (win is None) == (not taken[i].any())
        if win is not None:
            assert [f is not None for f in note_intake.plan_probes(n["midi_note"], SR)] == list(taken[i])
    assert note_intake.plan_probe_window(notes[8], n_audio, SR)[0] == int(notes[8]["onset_s"] * SR)      # the 0-150 ms fallback
    assert note_intake.plan_probe_window(notes[9], n_audio, SR) is None
    rng = np.random.default_rng(2)
    for a in rng.uniform(0.0, 1.0, (200, 4)) ** 4:
        assert note_intake.decide(60, *a) == ref.decide(60, *a)
    assert len(note_intake.OBM_FILES) == 13 and [m for _, m, _ in note_intake.OBM_FILES] == list(range(50, 99, 4))
