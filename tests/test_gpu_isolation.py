"""GPU parity of recorded-note intake: ow_isolation_score (k_isolation_score), ow_clip_bounds (k_clip_bounds) and the pitch check of
openwurli_amd/note_intake.py, against the outputs of the reference's own Python (tests/golden/isolation_golden.json,
tests/golden/intake_golden.npz).

Exact, at zero tolerance: masks, collision, clip bounds, every decision, the JSON and report text, and temporal / dominance of every
target with no released other (no pow on either side).
temporal and dominance of the other targets carry the device's pow(10.0, x): the bar is 2.5 x the reference's own largest movement of
that sub-score when every 10 ** x result moves 4 ulp (stored in the fixture by tests/golden/make_isolation_golden.py), the project's rule
for floors; with the fixture's 3.33e-16 (temporal) and 2.22e-16 (dominance) that is 8.3e-16 and 5.6e-16.  The test prints the largest
observed difference over the bar.
The shape tests use random notes the reference never saw: there the restatement (held to the reference bit for bit by
tests/test_isolation_host.py) stands for it, and the bar is 2.5 x the restatement's own movement under the same 4-ulp nudge on those notes.
Probe amplitudes: the tolerance tests/test_gpu_features.py applies to extract_harmonics_fft amplitudes (AMP_REL, with its floor of 1e-13
of the strongest amplitude measured on the same segment)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import isolation_ref as ref
from test_gpu_features import AMP_REL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 44100
FLOOR_RULE = 2.5


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "isolation_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def intake():
    return np.load(os.path.join(ROOT, "tests", "golden", "intake_golden.npz"))


def _check(got, order, raw_ref, masks_ref, exact, bars, what):
    """got = (temporal, collision, dominance, mask) per record; raw_ref / masks_ref / exact per note.  Returns the largest difference
    over the bar of (temporal, dominance)."""
    temporal, collision, dominance, mask = got
    worst = [0.0, 0.0]
    for k, i in enumerate(order):
        if raw_ref[i] is None:
            assert (temporal[k], collision[k], dominance[k], mask[k]) == (0.0, 0.0, 0.0, 0), (what, i)
            continue
        t, c, d = raw_ref[i]
        assert [bool(int(mask[k]) >> h & 1) for h in range(8)] == masks_ref[i], (what, i)
        assert collision[k] == c, (what, i)
        if exact[i]:
            assert temporal[k] == t and dominance[k] == d, (what, i, temporal[k], t, dominance[k], d)
        for j, (g, w) in enumerate(((temporal[k], t), (dominance[k], d))):
            worst[j] = max(worst[j], abs(g - w) / bars[j])
            assert abs(g - w) <= bars[j], (what, i, ("temporal", "dominance")[j], g, w, abs(g - w), bars[j])
    return worst


def test_isolation_score_on_the_golden_set(hiplib, golden, capsys):
    from openwurli_amd import isolation
    notes = golden["notes_in"]
    scored = json.loads(golden["scored_text"])
    rec, file_first, order = isolation.plan_notes(notes)
    got = isolation.isolation_scores(rec, file_first)
    bars = (FLOOR_RULE * golden["nudge"]["temporal"], FLOOR_RULE * golden["nudge"]["dominance"])
    worst = _check(got, order, golden["raw"], [n["harmonic_mask"] for n in scored], golden["no_released"], bars, "golden")
    with capsys.disabled():
        print(f"\n[isolation] device against reference over the bar: temporal {worst[0]:.3f} (bar {bars[0]:.3e}), dominance {worst[1]:.3f} (bar {bars[1]:.3e})")
    assert sum(golden["no_released"]) >= 4
    # the mirror: the golden JSON byte for byte, and the report
    mine = json.loads(json.dumps(notes))
    isolation.score_notes(mine)
    assert json.dumps(mine, indent=2) == golden["scored_text"]
    assert isolation.format_summary(mine) == golden["report"]


def test_score_isolation_tool_reproduces_the_golden_files(hiplib, golden, tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import score_isolation as tool
    src, dst = tmp_path / "notes.json", tmp_path / "scored_notes.json"
    src.write_text(json.dumps(golden["notes_in"]))
    tool.main(["--input", str(src), "--output", str(dst)])
    assert dst.read_text() == golden["scored_text"]
    assert golden["report"] in capsys.readouterr().out


def _random_file(rng, name, n):
    notes = []
    for k in range(n):
        onset = rng.uniform(0.0, 20.0)
        dur = float(np.exp(rng.uniform(np.log(0.1), np.log(3.0))))
        notes.append({"id": f"{name}_{k:04d}", "onset_s": round(onset, 4), "offset_s": round(onset + dur, 4), "midi_note": int(rng.integers(36, 97)),
                      "amplitude": round(float(rng.uniform(0.05, 1.0)), 4), "source_file": name, "source_type": "basic_pitch"})
    return notes


@pytest.fixture(scope="module")
def shapes():
    """Files of 1, 63, 64, 65 and 129 notes; the restatement's unrounded scores, masks and its own movement under the 4-ulp nudge."""
    rng = np.random.default_rng(77)
    files = [_random_file(rng, f"file_{n}.wav", n) for n in (1, 63, 64, 65, 129)]
    notes = [n for f in files for n in f]
    table = ref.collision_table()
    plain = json.loads(json.dumps(notes))
    raw = ref.score_notes(plain, table=table)
    move = [0.0, 0.0]
    for to in (np.inf, -np.inf):
        def p10(x):
            v = 10.0 ** x
            for _ in range(4):
                v = float(np.nextafter(v, to))
            return v
        for r, s in zip(raw, ref.score_notes(json.loads(json.dumps(notes)), p10, table)):
            if r is not None:
                move = [max(move[0], abs(r[0] - s[0])), max(move[1], abs(r[2] - s[2]))]
    assert any(r is None for r in raw) and move[0] > 0.0 and move[1] > 0.0
    return files, raw, [n["harmonic_mask"] for n in plain], (FLOOR_RULE * move[0], FLOOR_RULE * move[1])


@pytest.mark.parametrize("reverse", [False, True])
def test_shapes_wavefront_edges_and_files(hiplib, shapes, reverse):
    """1, 63, 64, 65 and 129 notes per file: a wavefront that is one note short, full, one over (a last wavefront with one live lane),
    two wavefronts and one lane; in both orders; nothing leaks from one file into the next; one call equals file by file."""
    from openwurli_amd import isolation
    files, raw, masks, bars = shapes
    index = {n["id"]: i for i, n in enumerate(n for f in files for n in f)}
    seq = files[::-1] if reverse else files
    notes = [n for f in seq for n in f]
    rec, file_first, order = isolation.plan_notes(notes)
    assert list(file_first) == list(np.cumsum([0] + [len(f) for f in seq]))
    got = isolation.isolation_scores(rec, file_first)
    to_ref = [index[notes[i]["id"]] for i in range(len(notes))]
    _check(got, order, [raw[j] for j in to_ref], [masks[j] for j in to_ref], [False] * len(notes), bars, f"reverse={reverse}")
    at = 0
    for f in seq:
        r1, ff1, _ = isolation.plan_notes(f)
        one = isolation.isolation_scores(r1, ff1)
        for a, b in zip(one, got):
            assert np.array_equal(a, b[at:at + len(f)]), f[0]["source_file"]
        at += len(f)


def test_empty_call_and_refusals_leave_the_library_usable(hiplib, golden):
    from openwurli_amd import OwError, binding as b, isolation
    rec, file_first, _ = isolation.plan_notes(golden["notes_in"])
    before = isolation.isolation_scores(rec, file_first)
    empty = isolation.isolation_scores(rec[:0], [0])
    assert all(a.size == 0 for a in empty)
    cases = []
    for field, v, msg in (("midi_note", 128, "note 5: midi_note outside 0..127"), ("midi_note", -1, "note 5: midi_note outside 0..127"),
                          ("onset_s", np.nan, "note 5: onset_s is not finite"), ("offset_s", np.inf, "note 5: offset_s is not finite"),
                          ("amplitude", -np.inf, "note 5: amplitude is not finite")):
        bad = rec.copy()
        bad[field][5] = v
        cases.append((bad, file_first, msg))
    cases.append((rec, np.array([0, 40, 20, rec.size], dtype=np.uint64), "file 1: range is not ascending"))
    for r, ff, msg in cases:
        with pytest.raises(OwError, match=msg):
            isolation.isolation_scores(r, ff)
        after = isolation.isolation_scores(rec, file_first)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    out = np.zeros(rec.size)
    cfg = b.OwIsoCfg(isolation.COLLISION_RATIO)
    assert hiplib.ow_isolation_score(rec.ctypes.data_as(C.c_void_p), rec.size, file_first.ctypes.data_as(C.c_void_p), file_first.size - 1, C.byref(cfg),
                                     out.ctypes.data_as(C.c_void_p), None, None, None) == -1
    assert hiplib.ow_last_error().decode() == "ow_isolation_score: null argument"
    hiplib.ow_clear_error()
    assert all(np.array_equal(x, y) for x, y in zip(before, isolation.isolation_scores(rec, file_first)))


# ---- ow_clip_bounds ---------------------------------------------------------------------------------------------------------------------------
def test_clip_bounds_fixture_clips(hiplib, intake):
    from openwurli_amd import note_intake
    n = int(intake["n_clips"][0])
    clips = [intake[f"clip{i}"] for i in range(n)]
    want_idx = [ref.clip_bounds(x) for x in clips]
    for perm in (list(range(n)), list(range(n))[::-1], [3, 0, 7, 5, 1, 6, 2, 4]):
        width = max(len(x) for x in clips) + 5
        rows = np.full((n, width), 7.5)                                        # junk past every length: must not be read as audio
        rows[:, -1] = np.nan
        lens = np.zeros(n, dtype=np.uint32)
        for r, i in enumerate(perm):
            rows[r, :len(clips[i])] = clips[i]
            lens[r] = len(clips[i])
        peak, first, last = note_intake.clip_bounds(rows, lens)
        assert first.dtype == last.dtype == np.int64
        for r, i in enumerate(perm):
            assert (peak[r], first[r], last[r]) == want_idx[i], (perm, i)
            if peak[r] >= 1e-10:
                assert [first[r], last[r]] == list(intake[f"clip_idx{i}"])
            got = note_intake.bounds_to_seconds(float(peak[r]), int(first[r]), int(last[r]), len(clips[i]), SR)
            assert list(got) == list(intake[f"clip_sec{i}"]), (perm, i, got)
    assert note_intake.detect_obm_bounds(clips, SR) == [tuple(intake[f"clip_sec{i}"]) for i in range(n)]
    for sr, a, b in ((SR, 150, 800), (1000, 2, 40), (1000, 500, 800)):         # extract_sustain_window's onset search and window
        assert note_intake.sustain_windows(clips, sr, a, b) == [ref.sustain_window(x, sr, a, b) for x in clips], (sr, a, b)
    # more than one pass of the block over a clip, the peak in the last partial pass, a lone late sample above the offset threshold
    x = np.zeros(256 * 5 + 3)
    x[-2], x[700], x[-1] = -2.0, 0.21, 0.03
    assert note_intake.clip_bounds([x, x[:1], x[:0]]) [0].tolist() == [2.0, 0.0, 0.0]
    peak, first, last = note_intake.clip_bounds([x, x[:1], x[:0]])
    assert (first.tolist(), last.tolist()) == ([700, -1, -1], [len(x) - 1, -1, -1])


# ---- the pitch check ----------------------------------------------------------------------------------------------------------------------------
def test_correct_octave_errors_on_the_golden_recording(hiplib, intake):
    from openwurli_amd import note_intake
    audio = intake["pcm"].astype(np.float64) / 32768.0
    notes = json.loads(str(intake["notes_in_json"]))
    got = note_intake.probe_amplitudes(notes, audio, SR)
    want = intake["probes"]
    for i, pr in enumerate(got):
        if pr is None:
            assert np.all(np.isnan(want[i])), i
            continue
        strongest = np.nanmax(np.abs(want[i]))                                 # the four probes look at one segment
        for j in range(4):
            if np.isnan(want[i, j]):
                assert pr[j] == (1e-20 if j == 1 else 0.0), (i, j)
            else:
                c = max(want[i, j], 1e-20) if j == 1 else want[i, j]
                assert abs(pr[j] - c) <= max(AMP_REL * abs(c), 1e-13 * strongest), (i, j, pr[j], c)
    corrected, removed = note_intake.correct_octave_errors(notes, audio, SR)
    assert (corrected, removed) == (int(intake["corrected"][0]), int(intake["removed"][0]))
    assert notes == json.loads(str(intake["notes_out_json"]))
    assert note_intake.correct_octave_errors([], audio, SR) == (0, 0)
    again = note_intake.notes_from_events(intake["events"].tolist(), "/recordings/intake.wav")
    assert again == json.loads(str(intake["notes_in_json"]))
