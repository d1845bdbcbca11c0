"""The pickup-law study without a device: the restatement (tests/pickup_law_ref.py) against the reference's own results
(tests/golden/pickup_law_golden.json, written by tests/golden/make_pickup_law_golden.py from ml/h3_analysis_v2.py itself), the report
text from the golden's numbers, the grid's tables from canned numbers, the carriers, the law list and every refusal of ow_pickup_law
that needs no device.
"""
import ctypes as C
import math

import numpy as np
import pytest

import pickup_law_ref as ref
from openwurli_amd import binding
from openwurli_amd import pickup_law as pl


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement's reference form on every job of the run: both carriers of every note x the 29 laws, computed once."""
    rows, keys = pl.carriers(golden["midis"])
    kinds, params = pl.script_laws()
    amps, peak = ref.jobs(rows, kinds, params)
    return {"keys": keys, "amps": amps.reshape(len(golden["midis"]), 2, 29, 8), "y_peak": peak.reshape(len(golden["midis"]), 2)}


def test_golden_meets_the_fixtures_conditions(golden):
    assert 6 <= len(golden["midis"]) <= 8 and min(golden["midis"]) >= 33 and max(golden["midis"]) <= 96
    reliable = [m for m in golden["midis"] if golden["snr_pairs"][m][1] > pl.RELIABLE_SNR_DB]
    assert reliable == golden["reliable"] and 3 <= len(reliable) < len(golden["midis"])
    assert any(not math.isnan(golden["snr_pairs"][m][1]) and golden["snr_pairs"][m][1] <= pl.RELIABLE_SNR_DB for m in golden["midis"])
    assert any(math.isnan(golden["snr_pairs"][m][1]) for m in golden["midis"])
    assert any(o["db"][2] > o["db"][1] for o in golden["obm"].values())
    assert golden["vel_scale"]["33"]["ds"] == 0.80 and golden["vel_scale"]["96"]["ds"] < 0.3
    assert all(v > 0 for v in golden["movement"].values())
    assert sorted(len(c) for c in golden["clips"].values())[:2] == [1764, 6615]      # shorter than 0.05 s and than 0.2 s


def test_restatement_is_the_reference_bit_for_bit(golden, restated):
    want = ref.golden_numbers(golden)
    for i, m in enumerate(golden["midis"]):
        assert np.array_equal(restated["amps"][i, 0, :16], want["amps"][i, 0, :16]), (m, "alpha")
        assert np.array_equal(restated["amps"][i, 1, 16:, :3], want["amps"][i, 1, 16:, :3]), (m, "k / blend")
        assert restated["y_peak"][i, 0] == want["y_peak"][i, 0], (m, "y_peak")


def test_floors_follow_the_floor_rule(golden):
    assert ref.FLOOR_FACTOR <= 2.5
    for k, v in golden["floors"].items():
        assert 0 < v <= 2.5 * golden["movement"][k], k
    # the recorded movement is the restatement's own: recomputed on two of the fixture's carriers it stays inside the record
    rows, keys = pl.carriers([33, 84], variants=("midi",))
    kinds, params = pl.script_laws()
    part = ref.movement(rows, kinds, params, [golden["obm"][m]["db"][1:3] for m, _, _ in keys])
    for k in ("amp", "db", "y_peak"):
        assert 0 < part[k] <= golden["movement"][k], (k, part[k], golden["movement"][k])


def test_report_from_the_goldens_numbers_is_the_scripts_text(golden):
    assert pl.report(golden["obm"], golden["snr_pairs"], ref.golden_numbers(golden)) == golden["report_head"]
    assert "Best alpha (min total RMS on reliable): 1.0" in golden["report_head"]


def test_report_falls_back_with_too_few_reliable_notes(golden):
    snr = {m: (float("nan"), float("nan")) for m in golden["midis"]}
    text = pl.report(golden["obm"], snr, _all_alpha(golden))
    assert "Too few reliable notes for alpha optimization." in text
    kept = [m for m in golden["midis"] if m not in (54, 66, 70)]
    assert f"Fallback: excluding known anomalous notes. Using n={len(kept)}: {kept}" in text


def _all_alpha(golden):
    """Numbers in which the k and blend carrier repeats the alpha carrier's law 0: enough for a report whose figures are not looked at."""
    numbers = ref.golden_numbers(golden)
    numbers["amps"][:, 1, :, :] = numbers["amps"][:, 0, 0:1, :]
    return numbers


def test_carriers_hold_both_of_the_scripts_scales(golden):
    rows, keys = pl.carriers(golden["midis"])
    assert rows.shape == (2 * len(golden["midis"]), 3)
    for i, m in enumerate(golden["midis"]):
        s = golden["vel_scale"][str(m)]               # the script's own two scales, each reproduced bit for bit
        assert keys[2 * i] == (m, 80, "approx") and keys[2 * i + 1] == (m, 80, "midi")
        assert list(rows[2 * i]) == [s["f0"], s["ds"], s["approx"]] and list(rows[2 * i + 1]) == [s["f0"], s["ds"], s["midi"]]
        assert (rows[2 * i, 2] != rows[2 * i + 1, 2]) == (s["approx"] != s["midi"])
    # the two scales differ only where log2 leaves midi_approx off the integer: the carrier follows whatever the exponent is handed
    assert pl.vel_scale_approx(pl.midi_to_freq(60) * (1 + 1e-9)) != pl.vel_scale_midi(60)
    assert pl.vel_scale_approx(pl.midi_to_freq(60), 100) == pl.vel_scale_midi(60, 100) == float((100 / 127.0) ** pl.velocity_exponent(60))
    assert pl.midi_to_freq(69) == 440.0 and pl.pickup_ds(60) == pl.DS_AT_C4 and pl.pickup_ds(33) == 0.80
    assert pl.reed_length_mm(33) == (3.0 - 1 / 20.0) * 25.4 and pl.reed_blank_dims(96) == (0.098 * 25.4, 0.031 * 25.4)


class _Recorder:
    """A stand-in library that keeps what ow_pickup_law was handed."""
    def __init__(self):
        self.calls = []

    def ow_pickup_law(self, car, n_car, kinds, params, n_laws, *rest):
        self.calls.append((np.ctypeslib.as_array(C.cast(kinds, C.POINTER(C.c_int32)), (n_laws,)).copy(),
                           np.ctypeslib.as_array(C.cast(params, C.POINTER(C.c_double)), (n_laws,)).copy(), n_car, rest))
        return 0


def test_arange_alphas_reach_the_call_unrounded(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(pl, "load_library", lambda: rec)
    pl.run_script([60, 72])
    (kinds, params, n_car, rest), = rec.calls            # ONE call for the whole run
    assert n_car == 4 and list(kinds) == [0] * 16 + [1] * 7 + [2] * 6
    alphas = np.arange(1.0, 2.51, 0.1)
    assert [float(p).hex() for p in params[:16]] == [float(a).hex() for a in alphas]
    assert params[3] != 1.3 and round(params[3], 1) == 1.3      # arange's 1.3000000000000003, not the literal
    assert list(params[16:]) == list(pl.KS) + list(pl.BLENDS)
    assert rest[0] == 44100.0 and rest[1] == 22050 and rest[2] == 8 and rest[3] == pl.SENSITIVITY and rest[4] == 0.90
    b0, a1 = ref.hpf_coeffs()
    assert rest[5] == b0 and rest[6] == a1


def test_grid_tables_from_canned_numbers():
    obm = {60: {"db": [0.0, -10.0, -20.0]}, 72: {"db": [0.0, -12.0, -30.0]}}
    keys = [(60, 80, "midi"), (60, 120, "midi"), (72, 80, "midi"), (72, 120, "midi")]
    kinds, params = pl.grid_laws(alphas=[1.0, 1.5], ks=[2.0])
    amps = np.zeros((4, 3, 3))
    amps[:, :, 0] = 1.0
    amps[:, 0, 1:] = [0.1, 0.01]                      # -20, -40 dB on every carrier
    amps[:, 1, 1:] = [10 ** -0.5, 0.1]                # -10, -20 dB: exact for note 60
    amps[:, 2, 1:] = [10 ** -0.6, 10 ** -1.5]         # -12, -30 dB: exact for note 72
    amps[3, 2, 0] = 0.0                               # H1 = 0: the job is left out, as the script leaves it out
    law_rows, note_rows = pl.grid_tables(obm, keys, kinds, params, amps)
    assert [(r[0], r[1], r[2]) for r in law_rows] == [("alpha", 1.0, 4), ("alpha", 1.5, 4), ("k", 2.0, 3)]
    h2e, h3e = np.array([10.0, 10.0, 8.0, 8.0]), np.array([20.0, 20.0, 10.0, 10.0])
    assert np.allclose(law_rows[0][3:], [h2e.mean(), h2e.std(), h3e.mean(), h3e.std(), np.sqrt(np.mean(h3e ** 2)), np.sqrt(np.mean(h2e ** 2 + h3e ** 2))],
                       rtol=0, atol=1e-12)
    assert [(r[0], r[1], r[2], r[3]) for r in note_rows] == [(60, 80, "alpha", 1.5), (60, 120, "alpha", 1.5), (72, 80, "k", 2.0), (72, 120, "alpha", 1.5)]
    assert all(abs(r[6]) < 1e-12 for r in note_rows[:3])
    text = pl.table_csv(pl.LAW_HEADER, law_rows).splitlines()
    assert text[0] == "family,parameter,n,h2_mean_db,h2_std_db,h3_mean_db,h3_std_db,h3_rms_db,total_rms_db" and len(text) == 4
    assert text[1].startswith("alpha,1.0,4,") and float(text[1].split(",")[3]) == law_rows[0][3]      # repr: the numbers read back exactly
    assert pl.table_csv(pl.NOTE_HEADER, note_rows).splitlines()[0] == "midi,velocity,family,parameter,h2_err_db,h3_err_db,distance_db"


def test_parse_axis():
    assert list(pl.parse_axis("1:2:0.5")) == [1.0, 1.5, 2.0]
    assert [float(x).hex() for x in pl.parse_axis("1.0:2.5:0.1")] == [float(x).hex() for x in np.arange(1.0, 2.55, 0.1)]
    assert list(pl.parse_axis("0,0.5,3")) == [0.0, 0.5, 3.0] and pl.parse_axis("").size == 0
    with pytest.raises(ValueError):
        pl.parse_axis("1:2:0")


def test_snr_windows_and_nan_rows():
    assert pl.snr_window(11025, 44100) == (2205, 8820)
    assert pl.snr_window(6615, 44100) == (2205, 6615)           # a clip that ends before 0.2 s
    assert pl.snr_window(1764, 44100) is None and pl.snr_window(2205, 44100) is None      # before 0.05 s: the script's NaN rows
    snr = pl.snr_from_magnitudes([1.0, 0.0, 2.0], [0.1, 0.1, 0.0])
    assert snr[0] == 20 * np.log10(1.0 / 0.1) and math.isnan(snr[1]) and math.isnan(snr[2])


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------
GOOD = dict(carriers=[[261.6, 0.7, 0.5]], kinds=[0], params=[1.0], sr=44100.0, n=64, nh=3, sens=1.8375, clip=0.9, b0=0.86, a1=0.72)
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    (dict(null="carriers"), "null argument"), (dict(null="kinds"), "null argument"), (dict(null="params"), "null argument"),
    (dict(null="amps"), "null argument"), (dict(null="peak"), "null argument"),
    (dict(n=3), "n_samples 3: fewer than 4"), (dict(n=0), "n_samples 0: fewer than 4"),
    (dict(nh=0), "n_harmonics 0 outside 1..8"), (dict(nh=9), "n_harmonics 9 outside 1..8"),
    (dict(kinds=[3]), "law 0: kind 3 outside 0..2"), (dict(kinds=[-1]), "law 0: kind -1 outside 0..2"),
    (dict(clip=0.0), "clip is not inside (0, 1)"), (dict(clip=1.0), "clip is not inside (0, 1)"), (dict(clip=NAN), "clip is not inside (0, 1)"),
    (dict(clip=-0.5), "clip is not inside (0, 1)"),
    (dict(sr=0.0), "sample_rate is not a finite positive number"), (dict(sr=-44100.0), "sample_rate is not a finite positive number"),
    (dict(sr=INF), "sample_rate is not a finite positive number"), (dict(sr=NAN), "sample_rate is not a finite positive number"),
    (dict(sens=NAN), "sensitivity is not finite"), (dict(b0=INF), "hpf_b0 is not finite"), (dict(a1=NAN), "hpf_a1 is not finite"),
    (dict(params=[NAN]), "law 0: parameter is not finite"),
    (dict(carriers=[[NAN, 0.7, 0.5]]), "carrier 0: f0_hz is not finite"), (dict(carriers=[[261.6, INF, 0.5]]), "carrier 0: ds is not finite"),
    (dict(carriers=[[261.6, 0.7, 0.5], [261.6, 0.7, -INF]]), "carrier 1: vel_scale is not finite"),
]


def _call(hiplib, **changes):
    a = dict(GOOD, **{k: v for k, v in changes.items() if k != "null"})
    car = np.ascontiguousarray(a["carriers"], dtype=np.float64)
    kinds, params = np.asarray(a["kinds"], dtype=np.int32), np.asarray(a["params"], dtype=np.float64)
    amps, peak = np.full((car.shape[0], kinds.size, 8), -7.0), np.full(car.shape[0], -7.0)
    ptr = {"carriers": car, "kinds": kinds, "params": params, "amps": amps, "peak": peak}
    p = {k: (None if changes.get("null") == k else v.ctypes.data_as(C.c_void_p)) for k, v in ptr.items()}
    rc = hiplib.ow_pickup_law(p["carriers"], car.shape[0], p["kinds"], p["params"], kinds.size, a["sr"], a["n"], a["nh"], a["sens"], a["clip"], a["b0"],
                              a["a1"], 0, p["amps"], p["peak"])
    return rc, amps, peak


@pytest.mark.parametrize("changes,reason", REFUSALS, ids=[r + " " + ",".join(c) for c, r in REFUSALS])
def test_refusals_before_any_device_work(hiplib, changes, reason):
    rc, amps, peak = _call(hiplib, **changes)
    assert rc < 0
    assert binding.take_error(hiplib) == "ow_pickup_law: " + reason
    assert np.all(amps == -7.0) and np.all(peak == -7.0)            # the outputs are untouched


def test_nothing_to_do_returns_zero_without_a_device(hiplib):
    for changes in (dict(kinds=[], params=[]), dict(carriers=np.zeros((0, 3)))):
        rc, amps, peak = _call(hiplib, **changes)
        assert rc == 0 and np.all(amps == -7.0) and np.all(peak == -7.0)


def test_python_layer_checks_its_lists():
    with pytest.raises(ValueError, match="2 law kinds and 1 parameters"):
        pl.pickup_law([[261.6, 0.7, 0.5]], [0, 1], [1.0])
