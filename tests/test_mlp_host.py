"""Run-time MLP corrections, the part that needs no device: the checker (tests/c/mlp_eval_ref.cpp) pinned to the oracle, the exported
default weight set, the JSON round trip and the host-side refusals of ow_mlp_infer / ow_batch_render_corrected / ow_batch_render_mlp."""
import ctypes as C

import numpy as np
import pytest

import mlp_eval_ref as ref

_VP = C.c_void_p


def _p(a):
    return a.ctypes.data_as(_VP)


@pytest.fixture(scope="module")
def builtin(hiplib_host):
    from openwurli_amd.mlp import MlpWeights
    return MlpWeights.builtin()


def test_restated_infer_with_the_default_weights_is_the_oracles(oracle, builtin):
    """Every note 21..108 x six velocities, bit for bit: pins the restatement's infer AND the set ow_mlp_default_weights exports to the
    oracle's mlp_infer over the baked constants."""
    L = oracle.lib()
    w = builtin.flat()
    for note in range(21, 109):
        for vel in (0.0, 1.0 / 127.0, 0.3, 64.0 / 127.0, 1.0, 1.5):
            want = np.zeros(11)
            L.owo_mlp_infer(note, C.c_double(vel), _p(want))
            got = ref.infer(w, note, vel)
            assert got.tobytes() == want.tobytes(), (note, vel, got, want)


@pytest.mark.parametrize("note,vel", [(60, 100), (76, 50), (40, 127)])
def test_restated_render_is_the_oracles(oracle, builtin, note, vel):
    """The restated job with infer's corrections = the oracle's job with mlp on; with the identity = mlp off.  Bit for bit, with the
    flags ml/render_model_notes.py passes and with the command's own defaults (power amp, speaker)."""
    dur = 0.05
    corr = ref.infer(builtin.flat(), note, vel / 127.0)
    for kw in (dict(volume=1.0, speaker=0.0, poweramp=False), dict(volume=0.6, speaker=1.0, poweramp=True)):
        on = oracle.batch_render_job_ex(note, vel, dur, ref.SR, mlp=True, **kw)
        off = oracle.batch_render_job_ex(note, vel, dur, ref.SR, mlp=False, **kw)
        assert on.size == int(dur * ref.SR)
        assert np.array_equal(ref.render(note, vel, dur, corr, **kw), on)
        assert np.array_equal(ref.render(note, vel, dur, ref.IDENTITY, **kw), off)
    if note != 40:                                   # 40 lies below the fade: identity either way
        assert not np.array_equal(oracle.batch_render_job_ex(note, vel, dur, ref.SR, mlp=True), oracle.batch_render_job_ex(note, vel, dur, ref.SR, mlp=False))


def test_restated_render_takes_the_other_flags(oracle, builtin):
    """--displacement-scale lands after note-on, --no-attack-noise, --no-preamp: as owo_batch_render_job_ex."""
    corr = ref.infer(builtin.flat(), 72, 64 / 127.0)
    assert not np.array_equal(corr, ref.IDENTITY)
    for kw in (dict(displacement_scale=0.3), dict(no_attack_noise=True), dict(no_preamp=True)):
        assert np.array_equal(ref.render(72, 64, 0.03, corr, **kw),
                              oracle.batch_render_job_ex(72, 64, 0.03, ref.SR, volume=1.0, speaker=0.0, poweramp=False, mlp=True, **kw))


def test_json_round_trip_and_refusals(builtin):
    """from_json(to_json(builtin())) keeps every double; a network of another shape is refused with a clear message.

    The reference tree holds no model_weights.json (ml/ keeps only the scripts; the trained set lives in mlp_weights.rs), so there is no
    golden file to compare the built-in set with: the first test above pins it through the oracle's constants instead."""
    import json
    from openwurli_amd.mlp import MlpWeights
    d = builtin.to_json()
    back = MlpWeights.from_json(json.loads(json.dumps(d)))
    assert back.flat().tobytes() == builtin.flat().tobytes()
    assert back == builtin and builtin.flat().size == ref.N_WEIGHTS
    small = json.loads(json.dumps(d))
    small["hidden_size"] = 8
    small["layers"][0]["weights"] = small["layers"][0]["weights"][:8]; small["layers"][0]["bias"] = small["layers"][0]["bias"][:8]
    small["layers"][1]["weights"] = [r[:8] for r in small["layers"][1]["weights"][:8]]; small["layers"][1]["bias"] = small["layers"][1]["bias"][:8]
    small["layers"][2]["weights"] = [r[:8] for r in small["layers"][2]["weights"]]
    with pytest.raises(ValueError, match="hidden"):
        MlpWeights.from_json(small)
    wrong = json.loads(json.dumps(d))
    wrong["layers"][1]["activation"] = "tanh"
    with pytest.raises(ValueError, match="relu"):
        MlpWeights.from_json(wrong)
    two = json.loads(json.dumps(d))
    two["layers"] = two["layers"][:2]
    with pytest.raises(ValueError, match="3 layers"):
        MlpWeights.from_json(two)
    ragged = json.loads(json.dumps(d))
    ragged["layers"][2]["weights"] = ragged["layers"][2]["weights"][:10]
    with pytest.raises(ValueError, match="w3"):
        MlpWeights.from_json(ragged)
    p = builtin.perturbed(0.02, 11)
    assert p != builtin and p == builtin.perturbed(0.02, 11) and p != builtin.perturbed(0.02, 12)
    assert np.array_equal(p.target_stds, builtin.target_stds)


def test_default_weights_null(hiplib_host):
    hiplib_host.ow_clear_error()
    assert hiplib_host.ow_mlp_default_weights(None) < 0
    assert b"ow_mlp_default_weights" in hiplib_host.ow_last_error()
    hiplib_host.ow_clear_error()


SENTINEL = -12345.5


def _jobs(n):
    from openwurli_amd import binding
    arr = (binding.OwJob * n)()
    for i in range(n):
        arr[i].note, arr[i].velocity, arr[i].mlp, arr[i].volume, arr[i].r_ldr = 60 + i, 100, 1, 1.0, 1e6
    return arr


def _refused(lib, rc, *words):
    msg = lib.ow_last_error().decode()
    lib.ow_clear_error()
    assert rc < 0, msg
    for w in words:
        assert w in msg, (w, msg)


def test_corrected_render_refusals(hiplib_host, builtin):
    """A null pointer, a non-finite correction, a decay offset <= 0: refused on the host (this runs without a device), the message names
    the job and the field, the output buffer is untouched."""
    from openwurli_amd import binding
    lib = hiplib_host
    jobs, cfg = _jobs(4), binding.OwBatchCfg(44100.0, 0.001)
    out = np.full((4, 64), SENTINEL)
    good = np.tile(ref.IDENTITY, (4, 1))
    lib.ow_clear_error()
    _refused(lib, lib.ow_batch_render_corrected(jobs, 4, C.byref(cfg), None, _p(out), 64, 0), "ow_batch_render_corrected", "null", "corr")
    _refused(lib, lib.ow_batch_render_corrected(None, 4, C.byref(cfg), _p(good), _p(out), 64, 0), "ow_batch_render_corrected", "null")
    _refused(lib, lib.ow_batch_render_corrected(jobs, 4, None, _p(good), _p(out), 64, 0), "ow_batch_render_corrected", "null")
    _refused(lib, lib.ow_batch_render_corrected(jobs, 4, C.byref(cfg), _p(good), None, 64, 0), "ow_batch_render_corrected", "null")
    for job, col, value, field in ((2, 3, float("nan"), "freq_offsets_cents[3]"), (1, 0, float("inf"), "freq_offsets_cents[0]"),
                                   (3, 5, 0.0, "decay_offsets[0]"), (0, 9, -0.5, "decay_offsets[4]"), (2, 7, float("nan"), "decay_offsets[2]"),
                                   (1, 10, float("-inf"), "ds_correction")):
        bad = good.copy()
        bad[job, col] = value
        _refused(lib, lib.ow_batch_render_corrected(jobs, 4, C.byref(cfg), _p(bad), _p(out), 64, 0), "job %d" % job, field)
    assert np.all(out == SENTINEL)


def test_mlp_render_refusals(hiplib_host, builtin):
    from openwurli_amd import binding
    lib = hiplib_host
    jobs, cfg = _jobs(4), binding.OwBatchCfg(44100.0, 0.001)
    out = np.full((4, 64), SENTINEL)
    sets = np.ascontiguousarray(np.stack([builtin.flat(), builtin.perturbed(0.02, 11).flat()]))
    soj = np.array([0, 1, 0, 1], dtype=np.uint32)
    lib.ow_clear_error()
    _refused(lib, lib.ow_batch_render_mlp(jobs, 4, C.byref(cfg), _p(sets), 2, None, _p(out), 64, 0), "ow_batch_render_mlp", "null", "set_of_job")
    _refused(lib, lib.ow_batch_render_mlp(jobs, 4, C.byref(cfg), None, 2, _p(soj), _p(out), 64, 0), "ow_batch_render_mlp", "null", "sets")
    _refused(lib, lib.ow_batch_render_mlp(None, 4, C.byref(cfg), _p(sets), 2, _p(soj), _p(out), 64, 0), "ow_batch_render_mlp", "null")
    _refused(lib, lib.ow_batch_render_mlp(jobs, 4, C.byref(cfg), _p(sets), 2, _p(soj), None, 64, 0), "ow_batch_render_mlp", "null")
    bad_soj = np.array([0, 1, 2, 1], dtype=np.uint32)
    _refused(lib, lib.ow_batch_render_mlp(jobs, 4, C.byref(cfg), _p(sets), 2, _p(bad_soj), _p(out), 64, 0), "job 2", "set_of_job", "n_sets")
    at = {"w1[3][1]": 3 * 2 + 1, "b1[15]": 32 + 15, "w2[2][5]": 48 + 2 * 16 + 5, "b2[0]": 304, "w3[10][15]": 320 + 10 * 16 + 15, "b3[4]": 496 + 4,
          "target_means[10]": 507 + 10, "target_stds[0]": 518}
    for field, k in at.items():
        for value in (float("nan"), float("inf")):
            bad = sets.copy()
            bad[1, k] = value
            _refused(lib, lib.ow_batch_render_mlp(jobs, 4, C.byref(cfg), _p(bad), 2, _p(soj), _p(out), 64, 0), "set 1", field)
    assert np.all(out == SENTINEL)


def test_infer_refusals(hiplib_host, builtin):
    lib = hiplib_host
    notes = np.array([60, 70, 80], dtype=np.uint8)
    vels = np.array([0.5, 0.6, 0.7])
    out = np.full((2, 3, 11), SENTINEL)
    raw = np.full((2, 3, 11), SENTINEL)
    sets = np.ascontiguousarray(np.stack([builtin.flat(), builtin.flat()]))
    lib.ow_clear_error()
    _refused(lib, lib.ow_mlp_infer(None, 2, _p(notes), _p(vels), 3, 0, _p(out), _p(raw)), "ow_mlp_infer", "null", "sets")
    _refused(lib, lib.ow_mlp_infer(_p(sets), 2, None, _p(vels), 3, 0, _p(out), _p(raw)), "ow_mlp_infer", "null")
    _refused(lib, lib.ow_mlp_infer(_p(sets), 2, _p(notes), None, 3, 0, _p(out), _p(raw)), "ow_mlp_infer", "null")
    _refused(lib, lib.ow_mlp_infer(_p(sets), 2, _p(notes), _p(vels), 3, 0, None, _p(raw)), "ow_mlp_infer", "null")
    bad = sets.copy()
    bad[0, 48 + 16 * 7 + 9] = float("nan")
    _refused(lib, lib.ow_mlp_infer(_p(bad), 2, _p(notes), _p(vels), 3, 0, _p(out), _p(raw)), "set 0", "w2[7][9]")
    bad_v = vels.copy()
    bad_v[1] = float("nan")
    _refused(lib, lib.ow_mlp_infer(_p(sets), 2, _p(notes), _p(bad_v), 3, 0, _p(out), _p(raw)), "point 1", "velocity")
    assert np.all(out == SENTINEL) and np.all(raw == SENTINEL)
