"""Run-time MLP corrections on the GPU: ow_mlp_infer (k_mlp_infer: weight sets evaluated on the matrix cores), ow_batch_render_corrected
(explicit corrections per job) and ow_batch_render_mlp (a weight set per job), against the CPU restatement tests/c/mlp_eval_ref.cpp
(pinned to the oracle bit for bit by tests/test_mlp_host.py).

Weight sets: A = the built-in one, B = A.perturbed(0.02, 11), B' = A.perturbed(0.02, 12), C = A with b3 = +-50 alternating (every output
the built-in set trains saturates a clamp; infer only: ds pinned at 1.2 is the pickup's pole-stress region, mlp_correction.rs:128-132, and no parity input)."""
import ctypes as C

import numpy as np
import pytest

import mlp_eval_ref as ref
from test_gpu_render_flags import SUBSET

pytestmark = pytest.mark.gpu

SR = ref.SR
DUR = 0.3


@pytest.fixture(scope="module")
def sets(hiplib):
    from openwurli_amd.mlp import MlpWeights
    a = MlpWeights.builtin()
    return {"A": a, "B": a.perturbed(0.02, 11), "B2": a.perturbed(0.02, 12), "C": ref.set_c(a)}


def _subset_jobs(mlp):
    return [dict(note=n, velocity=v, mlp=mlp) for n, v in SUBSET]


def test_infer_against_the_restatement(hiplib, sets):
    """3 sets x 200 points (a ragged last wavefront).  Raw outputs within the MFMA-vs-scalar figure of test_mlp_mfma (1e-13 of
    max(|raw|, 1)), finished corrections within its 1e-10 (cents) / 1e-12 (decay, ds); set C sits on the clamps exactly where the fade is
    1 -- on the eight outputs whose raw value passes a clamp: b3 = +-50 does not saturate the built-in set's three untrained cents outputs
    (zero weights, std 1, mean 0: raw = +-50 cents, inside +-100), which must come back as +-50 exactly instead; points with fade 0 are the identity, bitwise; the built-in set through sets == NULL and passed explicitly give identical bits."""
    from openwurli_amd import mlp
    notes, vels = ref.infer_points(200)
    order = ("A", "B", "C")
    got, raw = mlp.infer([sets[k] for k in order], notes, vels, raw=True)
    assert got.shape == raw.shape == (3, 200, 11) and np.all(np.isfinite(got)) and np.all(np.isfinite(raw))
    fades = np.array([ref.fade(n) for n in notes])
    assert np.any(fades == 0.0) and np.any(fades == 1.0) and np.any((fades > 0.0) & (fades < 1.0))
    for s, k in enumerate(order):
        want, want_raw = ref.infer_many(sets[k].flat(), notes, vels)
        d_raw = np.abs(raw[s] - want_raw) / np.maximum(np.abs(want_raw), 1.0)
        print(k, "raw", d_raw.max(), "cents", np.abs(got[s][:, :5] - want[:, :5]).max(), "decay/ds", np.abs(got[s][:, 5:] - want[:, 5:]).max())
        assert d_raw.max() < 1e-13, (k, d_raw.max())
        assert np.abs(got[s][:, :5] - want[:, :5]).max() < 1e-10, k
        assert np.abs(got[s][:, 5:] - want[:, 5:]).max() < 1e-12, k
        assert got[s][fades == 0.0].tobytes() == np.tile(ref.IDENTITY, (int(np.sum(fades == 0.0)), 1)).tobytes(), k
    # set C: where the restatement's raw output lies beyond its clamp -- every decay ratio, ds and the two cents outputs the built-in set
    # trains; its three untrained cents outputs have zero weights, unit std and zero mean, so their raw value is b3 = +-50 cents itself,
    # inside the +-100 clamp -- the correction is the clamp value exactly; the others are held by the bars above
    _, c_raw = ref.infer_many(sets["C"].flat(), notes, vels)
    hi = np.array([i % 2 == 0 for i in range(11)])
    beyond = np.where(hi, c_raw > ref.CLAMP_HI, c_raw < ref.CLAMP_LO)                 # [200][11]
    saturating = np.all(beyond, axis=0)
    assert np.array_equal(saturating, np.any(beyond, axis=0)) and int(saturating.sum()) >= 8 and np.all(saturating[5:])
    clamp = np.where(hi, ref.CLAMP_HI, ref.CLAMP_LO)
    full = got[2][fades == 1.0]
    assert full.shape[0] > 50
    want_c = np.concatenate([clamp[:5] * 1.0, 1.0 + (clamp[5:] - 1.0) * 1.0])
    assert full[:, saturating].tobytes() == np.tile(want_c[saturating], (full.shape[0], 1)).tobytes()
    assert np.array_equal(full[:, ~saturating], np.tile(sets["C"].b3[~saturating], (full.shape[0], 1)))
    assert mlp.infer(None, notes, vels).tobytes() == got[0:1].tobytes()
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("preamp_kind", [0, 1])
def test_corrected_with_identity_is_the_plain_render_without_mlp(hiplib, preamp_kind):
    """All corrections identity and mlp = 1 in the jobs (ignored) = ow_batch_render of the same jobs with mlp = 0: the same bits."""
    import openwurli_amd as ow
    from openwurli_amd import mlp
    got = mlp.batch_render_corrected(_subset_jobs(True), np.tile(ref.IDENTITY, (len(SUBSET), 1)), duration_s=DUR, preamp_kind=preamp_kind)
    plain = ow.batch_render(_subset_jobs(False), duration_s=DUR, preamp_kind=preamp_kind)
    assert got.shape == plain.shape == (len(SUBSET), int(DUR * SR)) and np.max(np.abs(plain)) > 1e-5
    assert np.array_equal(got, plain)


@pytest.fixture(scope="module")
def parity(hiplib, sets):
    """The 66 parity jobs and their corrections: ow_mlp_infer of A, of B, and the hand-written set, interleaved."""
    from openwurli_amd import mlp
    jobs = ref.interleaved_jobs()
    assert len(jobs) == 66
    notes = np.array([n for n, _ in ref.PARITY_PAIRS], dtype=np.uint8)
    vels = np.array([v / 127.0 for _, v in ref.PARITY_PAIRS])
    inferred = mlp.infer([sets["A"], sets["B"]], notes, vels)                 # [2][22][11]
    corr = np.array([ref.HAND if s == 2 else inferred[s, k // 3] for k, (_, _, s) in enumerate(jobs)])
    corr.setflags(write=False)
    return jobs, corr


@pytest.mark.parametrize("no_preamp", [False, True])
def test_corrected_against_the_restatement(hiplib, oracle, parity, no_preamp):
    """66 jobs (two voice blocks, the second ragged), neighbouring lanes with different corrections, each against the restatement fed the
    same corrections: the batch bar and floor of every batch test; with --no-preamp (no solver in the path, only the voice moves) the
    1e-12 floor of test_no_preamp."""
    from openwurli_amd import mlp
    jobs, corr = parity
    got = mlp.batch_render_corrected([dict(note=n, velocity=v, no_preamp=no_preamp) for n, v, _ in jobs], corr, duration_s=DUR)
    want = ref.render_many([(n, v) for n, v, _ in jobs], corr, DUR, no_preamp=no_preamp)
    floor = 1e-12 if no_preamp else oracle.ABS_FLOOR_BATCH
    worst = 0.0
    for k, (n, v, s) in enumerate(jobs):
        rep = oracle.parity_report(got[k], want[k], abs_floor=floor)
        worst = max(worst, rep["worst_ratio"])
        assert rep["n_bad"] == 0, (no_preamp, n, v, s, rep)
        assert rep["peak"] > 1e-5, (n, v, s)
    print("no_preamp", no_preamp, "worst error / tolerance", worst)
    # the corrections are heard: a job of the hand-written source differs from its neighbour of set A
    assert not np.array_equal(got[0], got[2])


def _mlp_jobs(sets):
    """22 pairs x sets {A, B, B'}: job j = 3 pair + set, set_of_job interleaved; one job in three has mlp = 0, rotating through the sets
    (job j is off when j % 3 == (j // 3) % 3), so every set keeps jobs that are on."""
    jobs, soj = [], []
    for p, (n, v) in enumerate(ref.PARITY_PAIRS):
        for s in range(3):
            jobs.append(dict(note=n, velocity=v, mlp=(s != p % 3)))
            soj.append(s)
    return jobs, np.array(soj, dtype=np.uint32), [sets["A"], sets["B"], sets["B2"]]


def test_render_mlp_is_infer_then_corrected(hiplib, oracle, sets):
    """ow_batch_render_mlp = ow_mlp_infer + ow_batch_render_corrected, bit for bit (identity where mlp = 0), on the host and with
    out_is_device = 1.  Set A's jobs are within the batch bar of the oracle's mlp=True render.  They are NOT asserted bit-identical to
    ow_batch_render(mlp = 1): that path evaluates the network in scalar order inside the voice kernel, this one on the matrix cores."""
    from openwurli_amd import mlp
    jobs, soj, three = _mlp_jobs(sets)
    got = mlp.batch_render_mlp(jobs, three, soj, duration_s=DUR)
    notes = np.array([j["note"] for j in jobs], dtype=np.uint8)
    vels = np.array([j["velocity"] / 127.0 for j in jobs])
    inferred = mlp.infer(three, notes, vels)                                  # [3][66][11]
    corr = np.array([inferred[soj[k], k] if jobs[k]["mlp"] else ref.IDENTITY for k in range(len(jobs))])
    assert sum(1 for j in jobs if not j["mlp"]) == 22
    two_step = mlp.batch_render_corrected(jobs, corr, duration_s=DUR)
    assert got.shape == (66, int(DUR * SR)) and np.array_equal(got, two_step)
    n_a = 0
    for k, j in enumerate(jobs):
        if soj[k] == 0 and j["mlp"]:
            c = oracle.batch_render_job_ex(j["note"], j["velocity"], DUR, SR, volume=1.0, speaker=0.0, mlp=True, poweramp=False)
            rep = oracle.parity_report(got[k], c, abs_floor=oracle.ABS_FLOOR_BATCH)
            assert rep["n_bad"] == 0 and rep["peak"] > 1e-5, (j, rep)
            n_a += 1
    assert n_a >= 14
    # the same into a device buffer
    n = int(DUR * SR)
    buf = hiplib.ow_device_alloc(8 * 66 * n, 0)
    assert buf
    try:
        assert mlp.batch_render_mlp(jobs, three, soj, duration_s=DUR, out_device_ptr=buf, stride=n) is None
        back = np.zeros((66, n))
        assert hiplib.ow_test_device_read(back.ctypes.data_as(C.c_void_p), C.c_void_p(buf), back.nbytes, 0) == 0
    finally:
        hiplib.ow_device_free(buf, 0)
    assert np.array_equal(back, got)


def test_the_existing_render_is_untouched_by_the_new_entry_points(hiplib, sets):
    """ow_batch_render with mlp on and off, before and after a call to each new entry point in the same process: the same bits (no state
    left behind, the built-in constants not overwritten)."""
    import openwurli_amd as ow
    from openwurli_amd import mlp
    before = [ow.batch_render(_subset_jobs(m), duration_s=DUR) for m in (True, False)]
    assert not np.array_equal(before[0], before[1])
    notes = np.array([n for n, _ in SUBSET], dtype=np.uint8)
    vels = np.array([v / 127.0 for _, v in SUBSET])
    corr = mlp.infer([sets["C"], sets["B"]], notes, vels)
    mlp.batch_render_corrected(_subset_jobs(True), corr[1], duration_s=0.05)
    mlp.batch_render_mlp(_subset_jobs(True), [sets["B"], sets["C"]], [k % 2 for k in range(len(SUBSET))], duration_s=0.05)
    after = [ow.batch_render(_subset_jobs(m), duration_s=DUR) for m in (True, False)]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_render_and_extract_per_set(hiplib, sets):
    """mlp.render_and_extract: two sets x 4 pairs at 0.5 s, each dictionary = extract_model_features of the host copy of
    batch_render_mlp's audio for that set."""
    from openwurli_amd import features, mlp
    pairs = [(60, 80), (72, 100), (76, 50), (84, 127)]
    two = [sets["A"], sets["B"]]
    got = mlp.render_and_extract(pairs, two, duration_s=0.5)
    assert len(got) == 2
    jobs = [dict(note=m, velocity=v) for _ in two for m, v in pairs]
    audio = mlp.batch_render_mlp(jobs, two, [s for s in range(2) for _ in pairs], duration_s=0.5)
    for s in range(2):
        want = features.extract_model_features(audio[4 * s:4 * s + 4], SR, pairs)
        assert got[s] == want
        assert set(got[s]) == set(pairs)
    assert got[0] != got[1]
