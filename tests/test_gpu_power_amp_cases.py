"""The output stage against the bits of a recorded build (tests/golden/power_amp_cases_parent.npz, tools/record_chain_bits.py): the
power amp's exponential is a restatement of the device library's exp() and the polynomial steps of tanh_fast and of that exponential are
written as three-address fused multiply-adds (fma3), so every argument has to give the bits of the build that called the library.
64 engines x 129 samples x 2 chain samples = 16 512 inputs of the power amp per case, with post_pair 0 (k_post<true>) and 1
(k_post<false, true>): a silent engine, taps from below a microvolt up to +-4 V (chords of 1..64 keys from pp to ff; volts by a finite
kick of the preamp's output node), and engines struck right before the recorded blocks, whose taps grow from zero through the crossover
region (|A error| near 0.013 V), where the Newton loop goes from one sweep to two, three and four.  Most sweeps are taken elsewhere:
the oracle's `info` (owo_output_stage_block, tests/post_stage_cases.py) finds five to eight only for |tap| in 1.0512 .. 1.2864 V,
where the closed-loop estimate meets the +-22 V rail (eight in 1.27472 .. 1.27707 V).  A kick leaves the tap at -kick, +kick, ... for
the block, so the kicks here (0.5, 1, 2, 4 V: alone three, four, two and two sweeps) enter that band only where the engine's chord carries
a 1 V kick into it for a few samples; tests/test_gpu_post_stage.py places kicks inside it and compares with the oracle in f64."""
import os

import numpy as np
import pytest

import chain_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "power_amp_cases_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(cases.PA_CASES))
def test_power_amp_bits_equal_the_recorded_build(hiplib, golden, name):
    import openwurli_amd as ow
    got = cases.run_power_amp(ow, name)
    assert int(got["resets"].sum()) == 0, got["resets"]
    # the inputs the case is about
    n_inputs = cases.PA_ENGINES * sum(cases.PA_LENGTHS) * 2
    assert n_inputs >= 4096
    tap = got["tap_absmax"]
    assert tap[0] == 0.0, "engine 0 is silent"
    assert float(got["tap_absmin_nonzero"][0]) <= 1e-6 and float(tap.max()) >= 2.0, (got["tap_absmin_nonzero"], tap.max())
    for lo in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0):         # some engine peaks in every decade in between
        assert np.any((tap > lo) & (tap <= 10.0 * lo)), lo
    for key, a in got.items():
        want = golden[f"{name}/{key}"]
        assert a.dtype == want.dtype and a.shape == want.shape, (name, key)
        if a.tobytes() != want.tobytes():
            bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != want.view(np.uint8).reshape(a.shape + (-1,)))
            pytest.fail(f"{name}/{key}: differs from {golden['meta'].tolist()} first at index {bad[0].tolist()} ({len(bad)} bytes)")


def test_power_amp_fixture_names_its_origin(golden):
    meta = golden["meta"].tolist()
    assert any(m.startswith("commit=") and len(m) > 14 for m in meta) and any(m.startswith("box=") and len(m) > 4 for m in meta), meta
    assert os.path.getsize(GOLDEN) < 100 * 1024
