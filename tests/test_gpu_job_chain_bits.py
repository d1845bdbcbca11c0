"""The job-side chain kernels against the bits of a recorded build (tests/golden/job_chain_bits_parent.npz, tools/record_chain_bits.py):
k_job_chain<MEL>, k_job_chain_wide, k_job_chain_fused, k_job_chain_row, k_bark_chain_row, k_pbench<MEL>, k_pbench_row and k_poly_chain.
Each carries the same statements for a fresh preamp's start, its step with the NaN reset, the half-band pairs and the output stage; the
form-against-form tests cannot see a change made to all of them, these renders can.  Cases (tests/chain_bits_cases.py): the batch render
of 37 jobs at 44 100 and 96 000 Hz in each of test_chain_wide_is_bit_identical's five forced forms and the default, with LDR values on
every side of set_ldr_resistance's clamp and hysteresis and one job whose preamp output is never finite (the adapter's NaN reset); two
jobs with --no-preamp / --tremolo-depth; the 37 jobs on the melange preamp; bark-audit, the preamp measurements (r_reset != r_ldr on
some points), render-poly and centroid-track (the DC solve at the clamped --ldr).  Every bit of every row has to equal the recording:
one SHA-256 per row, and two rows per case kept so that a failure in them names a sample -- whole where a row is 2 205 samples, their
first 2 205 where it is longer (a measurement's trace is 22 050, a chord's row 9 261: whole, the fixture would pass the size limit of a
committed file).  (render-poly's chords are 0.21 s, not 0.05 s: the command refuses a render that ends before its measuring window
starts, at sample 8 820.  A measurement is 22 050 samples whatever is asked; on the melange preamp with these resistances the call takes
about 15 s, the one slow case here.)"""
import os

import numpy as np
import pytest

import chain_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "job_chain_bits_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    return {k: (g[str(a)[1:]] if a.dtype.kind == "U" and k != "meta" else a) for k, a in g.items()}      # "=<name>": the same bits as that array


@pytest.mark.parametrize("name", list(cases.JOB_CASES))
def test_job_chain_bits_equal_the_recorded_build(hiplib, golden, name):
    import openwurli_amd as ow
    got = cases.run_job_case(ow, name)
    print(f"\n[{name}] peak {float(got['peak'][0]):.6g}")
    assert float(got["peak"][0]) > 1e-3
    assert sorted(f"{name}/{k}" for k in got) == sorted(k for k in golden if k.startswith(name + "/"))
    # whole rows first: their failure names a sample
    for key, a in sorted(got.items(), key=lambda kv: kv[0].endswith("_sha")):
        want = golden[f"{name}/{key}"]
        assert a.dtype == want.dtype and a.shape == want.shape, (name, key)
        if a.tobytes() != want.tobytes():
            bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != want.view(np.uint8).reshape(a.shape + (-1,)))
            pytest.fail(f"{name}/{key}: differs from {golden['meta'].tolist()} first at index {bad[0].tolist()[:-1]} ({len(bad)} bytes)")
    if name.startswith("batch_") and not name.endswith(("_flags", "_melange")):
        assert got["row_peaks"][36] == 0.0            # the job whose preamp resets at every sample renders silence, as the oracle's does


def test_job_chain_bits_fixture_names_its_origin(golden):
    meta = golden["meta"].tolist()
    assert any(m.startswith("commit=") and len(m) > 14 for m in meta) and any(m.startswith("box=") and len(m) > 4 for m in meta), meta
    assert os.path.getsize(GOLDEN) < 450 * 1024        # SHA-256 per row and two row heads per case; whole rows would be 10 MB
