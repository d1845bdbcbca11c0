"""The chain kernels against the bits of a recorded build (tests/golden/chain_bits_parent.npz, tools/record_chain_bits.py).  tanh_fast,
power_amp, the exponentials and the preamp step are shared by every chain kernel, so the cross-kernel bit-identity tests cannot see a
change that is common to all of them; these renders can.  Pools of 1, 65 and 130 engines on the lane = engine kernels (k_preamp_pair +
k_post<false, true>): one lane, a full wavefront plus one lane, two full plus two; the 65-engine pool again on the lane-pair kernels
(k_preamp + k_post<true>) and streamed (k_chain_stream).  The bench chord (keys 33..96) at three of the instance velocities, tremolo
depth 0.5, one tremolo phase per engine; blocks of 512, 37 and 1 samples.  Every bit of the output blocks, of both solver states' rows
and of the preamp tap has to equal the recording, and no NaN reset may have fired (the reference substitutes a state there, which would
let a wrong value pass)."""
import os

import numpy as np
import pytest

import chain_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_bits_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(cases.CHAIN_CASES))
def test_chain_bits_equal_the_recorded_build(hiplib, golden, name):
    import openwurli_amd as ow
    got = cases.run_chain(ow, name)
    assert int(got["resets"].sum()) == 0, got["resets"]
    assert int(golden[f"{name}/resets"].sum()) == 0
    assert float(got["peak"][0]) > 1e-3
    for key, a in got.items():
        want = golden[f"{name}/{key}"]
        assert a.dtype == want.dtype and a.shape == want.shape, (name, key)
        if a.tobytes() != want.tobytes():
            bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != want.view(np.uint8).reshape(a.shape + (-1,)))
            pytest.fail(f"{name}/{key}: differs from {golden['meta'].tolist()} first at index {bad[0].tolist()} ({len(bad)} bytes)")


def test_chain_bits_fixture_names_its_origin(golden):
    meta = golden["meta"].tolist()
    assert any(m.startswith("commit=") and len(m) > 14 for m in meta) and any(m.startswith("box=") and len(m) > 4 for m in meta), meta
    assert os.path.getsize(GOLDEN) < 100 * 1024
