"""ow_pickup_law (k_pickup_law) against the reference's own results on the fixture of tests/golden/pickup_law_golden.json and against the
restatement (tests/pickup_law_ref.py), and step 1 of the script (openwurli_amd.pickup_law.interharmonic_snr over ow_dft_magnitudes)
against the reference's per-clip values.

Floors.  The golden's `movement` is the restatement's own movement on the run's jobs (both carriers of every note x the 29 laws at 22 050
samples) with the DFT sums in sample order instead of pairwise and with every sin / cos / pow result moved by one ulp (five patterns):
1.69e-15 V on an amplitude, 1.72e-12 dB on H2 / H3 re H1, 1.11e-16 on y_peak.  The floors are 2.5 x those (the project's rule); the
device's distances are printed by the tests and recorded in DESIGN.md (section 10, the pickup-law study).  The dB floors apply where the
figures are harmonics (the script's size and the 2 050-sample case); at 64 and 4 samples the window holds less than a period of the
carrier and the amplitudes alone are compared.
"""
import ctypes as C
import math

import numpy as np
import pytest

import note_audit_ref as nar
import pickup_law_ref as ref
from openwurli_amd import binding
from openwurli_amd import pickup_law as pl

pytestmark = pytest.mark.gpu

EDGE_CARRIERS = [[55.0, 0.80, 0.675], [1046.5022612023945, 0.40, 0.64], [261.6255653005986, 0.70, 0.525]]
EDGE_KINDS = [0, 0, 1, 1, 2, 2, 0]
EDGE_PARAMS = [1.0, 1.7000000000000006, 0.0, 1.5, 0.4, 1.0, 2.5]


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


@pytest.fixture(scope="module")
def device_run(golden):
    """The whole run of the script in ONE call, shared."""
    return pl.run_script(golden["midis"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def distances(got_a, got_p, want_a, want_p, with_db=True):
    d = {"amp": float(np.nanmax(np.abs(got_a - want_a))), "y_peak": float(np.nanmax(np.abs(got_p - want_p)))}
    if with_db:
        d["db"] = float(np.nanmax(np.abs(ref.db_re_h1(got_a) - ref.db_re_h1(want_a))))
    return d


def test_parity_at_the_scripts_size(golden, device_run):
    want = ref.golden_numbers(golden)                       # NaN where the script computes nothing: nanmax leaves those out
    assert device_run["amps"].shape == want["amps"].shape and np.all(np.isfinite(device_run["amps"])) and np.all(device_run["amps"][..., 0] > 1e-3)
    d = distances(device_run["amps"], device_run["y_peak"], want["amps"], want["y_peak"])
    print("\ndevice against the reference: " + ", ".join(f"{k} {v:.3e} (floor {golden['floors'][k]:.3e})" for k, v in d.items()))
    assert np.count_nonzero(~np.isnan(want["amps"])) == len(golden["midis"]) * (16 * 8 + 13 * 3)
    for k, v in d.items():
        assert v <= golden["floors"][k], (k, v, golden["floors"][k])


def test_report_text_is_the_scripts(golden, device_run, tmp_path):
    import wave
    obm = {}
    for m, o in golden["obm"].items():
        path = tmp_path / o["source_file"]
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(golden["sample_rate"])
            w.writeframes(golden["clips"][m].astype("<i2").tobytes())
        obm[m] = dict(o, source_file=str(path))
    text = pl.report(obm, pl.measure_snr(obm), device_run)
    assert text == golden["report_head"]


@pytest.mark.parametrize("n", [2050, 64, 4])
@pytest.mark.parametrize("nh", [1, 3, 8])
def test_tile_edges(golden, n, nh):
    # 2 050: the DFT starts mid-tile at 1 025 and the last tile holds 2 samples; 64: one full tile; 4: the smallest run
    got_a, got_p = pl.pickup_law(EDGE_CARRIERS, EDGE_KINDS, EDGE_PARAMS, n_samples=n, n_harmonics=nh)
    want_a, want_p = ref.jobs(EDGE_CARRIERS, EDGE_KINDS, EDGE_PARAMS, n=n, n_harm=nh, sequential=True)
    assert got_a.shape == (3, 7, nh) and np.all(np.isfinite(got_a)) and np.max(want_a) > 1e-4
    d = distances(got_a, got_p, want_a, want_p, with_db=(n == 2050 and nh >= 3))
    print(f"\n[n={n} nh={nh}] " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    for k, v in d.items():
        assert v <= golden["floors"][k], (k, v, golden["floors"][k])


def test_clip_active(golden):
    carriers = [[220.0, 1.5, 0.8], [987.7666025122483, 2.0, 0.6]]           # ds * vel_scale = 1.2 > clip
    kinds, params = [0, 1, 2, 0, 1, 2], [1.0, 0.0, 0.5, 1.6, 2.0, 1.0]
    got_a, got_p = pl.pickup_law(carriers, kinds, params, n_samples=2050, n_harmonics=8, clip=0.9)
    want_a, want_p = ref.jobs(carriers, kinds, params, n=2050, n_harm=8, clip=0.9, sequential=True)
    assert list(got_p) == [0.9, 0.9] == list(want_p)
    d = distances(got_a, got_p, want_a, want_p)
    print("\n[clip active] " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    for k, v in d.items():
        assert v <= golden["floors"][k], (k, v, golden["floors"][k])
    # kind 0 with p = 1.0 is kind 1 with p = 0.0: pow(x, 1.0) is x, and * (1 + 0 y) is * 1
    assert np.array_equal(bits(got_a[:, 0]), bits(got_a[:, 1]))


def _many_laws(n):
    # 66 laws of kind 0 first: 64 of them fill a wavefront, 65 need a second one; beyond, the kinds mix, so that with 130 laws the
    # wavefronts of kind 0 (64 + 23) hold other laws than with 65
    kinds = [0 if i < 66 else i % 3 for i in range(n)]
    params = [1.0 + 0.011 * i if k == 0 else 0.037 * i if k == 1 else (i % 41) / 40.0 for i, k in enumerate(kinds)]
    return np.asarray(kinds, dtype=np.int32), np.asarray(params)


@pytest.mark.parametrize("n_laws", [1, 64, 65, 130])
def test_jobs_do_not_depend_on_each_other(n_laws):
    carriers = np.asarray(EDGE_CARRIERS)
    kinds, params = _many_laws(130)
    full_a, full_p = pl.pickup_law(carriers, kinds, params, n_samples=2050, n_harmonics=3)       # 130 laws: chunks of 64 + a rest, per kind
    a, p = pl.pickup_law(carriers[:1], kinds[:n_laws], params[:n_laws], n_samples=2050, n_harmonics=3)
    assert np.array_equal(bits(a), bits(full_a[:1, :n_laws])) and np.array_equal(bits(p), bits(full_p[:1]))
    # reversed laws, permuted carriers
    ra, rp = pl.pickup_law(carriers[[2, 0, 1]], kinds[:n_laws][::-1], params[:n_laws][::-1], n_samples=2050, n_harmonics=3)
    assert np.array_equal(bits(ra[[1, 2, 0]][:, ::-1]), bits(full_a[:, :n_laws])) and np.array_equal(bits(rp[[1, 2, 0]]), bits(full_p))
    if n_laws in (1, 65):                                   # law by law
        for j in range(n_laws):
            one, _ = pl.pickup_law(carriers[:1], kinds[j:j + 1], params[j:j + 1], n_samples=2050, n_harmonics=3)
            assert np.array_equal(bits(one[0, 0]), bits(full_a[0, j])), j
    # fewer harmonics: the same first ones
    a1, _ = pl.pickup_law(carriers[:1], kinds[:n_laws], params[:n_laws], n_samples=2050, n_harmonics=1)
    assert np.array_equal(bits(a1[..., 0]), bits(a[..., 0]))


def test_grid_of_three_alphas_is_three_single_runs(golden):
    alphas = [1.0, 1.25, 2.0]
    law_csv, note_csv, amps = pl.grid(golden["obm"], alphas=alphas, velocities=(60, 100))
    assert amps.shape == (2 * len(golden["midis"]), 3, 3)
    for j, a in enumerate(alphas):
        one_csv, _, one = pl.grid(golden["obm"], alphas=[a], velocities=(60, 100))
        assert np.array_equal(bits(one[:, 0]), bits(amps[:, j])), a
        assert one_csv.splitlines()[1] == law_csv.splitlines()[1 + j]
    assert len(note_csv.splitlines()) == 1 + 2 * len(golden["midis"])


def test_interharmonic_snr_against_the_reference(golden):
    midis = golden["midis"]
    clips = [golden["clips"][m].astype(np.float64) / 32768.0 for m in midis]
    h_amps, snr = pl.interharmonic_snr(clips, [golden["obm"][m]["f0"] for m in midis], [golden["sample_rate"]] * len(midis))
    worst = 0.0
    for i, m in enumerate(midis):
        want_h, want_s = golden["snr"][str(m)]["h_amps"], golden["snr"][str(m)]["snr"]
        w = pl.snr_window(len(clips[i]), golden["sample_rate"])
        if w is None:                                       # shorter than 0.05 s: the script's NaN rows
            assert m == 96 and all(v is None for v in want_h + want_s) and np.all(np.isnan(h_amps[i])) and np.all(np.isnan(snr[i]))
            continue
        n = w[1] - w[0]
        assert (n == 4410) == (m == 84)                     # the clip that ends before 0.2 s
        delta = nar.analysis_rel(n) * (2.0 / n) * float(np.sum(np.abs(clips[i][w[0]:w[1]])))      # ow_dft_magnitudes' floor on one magnitude
        worst = max(worst, float(np.max(np.abs(h_amps[i] - want_h))) / delta)
        assert np.max(np.abs(h_amps[i] - want_h)) <= delta, m
        for h in range(8):
            noise = want_h[h] / 10 ** (want_s[h] / 20)
            bound = 20 / math.log(10) * 1.01 * (delta / want_h[h] + delta / noise) + 1e-13
            assert abs(snr[i][h] - want_s[h]) <= bound, (m, h, snr[i][h], want_s[h], bound)
    print(f"\n[inter-harmonic SNR] worst harmonic magnitude difference / floor {worst:.3f}")


def test_refusals_on_the_device_path():
    L = binding.load_library()
    car = np.ascontiguousarray(EDGE_CARRIERS)
    kinds, params = np.asarray([0, 1], dtype=np.int32), np.asarray([1.0, 0.5])
    amps, peak = np.full((3, 2, 3), -7.0), np.full(3, -7.0)
    args = lambda n_laws, device: (car.ctypes.data_as(C.c_void_p), 3, kinds.ctypes.data_as(C.c_void_p), params.ctypes.data_as(C.c_void_p), n_laws, 44100.0, 256, 3,  # noqa: E731
                                   1.8375, 0.9, 0.86, 0.72, device, amps.ctypes.data_as(C.c_void_p), peak.ctypes.data_as(C.c_void_p))
    assert L.ow_pickup_law(*args(2, 4096)) < 0              # no such device: refused by the runtime, before any launch
    assert binding.take_error(L).startswith("ow_pickup_law: ")
    assert np.all(amps == -7.0) and np.all(peak == -7.0)
    assert L.ow_pickup_law(*args(0, 0)) == 0                # nothing to do
    assert np.all(amps == -7.0) and np.all(peak == -7.0)
    assert L.ow_pickup_law(*args(2, 0)) == 0, binding.take_error(L)      # a refused call leaves nothing behind for the next one
    assert np.all(amps > 0) and np.all(peak > 0)
