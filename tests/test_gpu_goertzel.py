"""GPU parity of ow_goertzel_harmonics (k_goertzel) on the fixture clips of tests/golden/residuals_golden.npz.

Exact: against the numpy restatement (tests/harmonics_ref.py, held bit for bit to the reference by tests/test_harmonics_host.py) run with
the coefficients and bins the library reports.  Every operation of the recurrence and of the magnitude is a single IEEE operation on
both sides, so the tolerance is zero; that covers the order of the recurrence, the absence of contraction, the first-maximum selection,
the removal of duplicate bins and the range rules for k.
Against the reference's own amplitudes, where numpy's cos supplied the coefficient: 2.5 x the reference's own movement of that amplitude
when its coefficient moves one ulp (stored in the fixture), the project's rule for floors; exact where the library's coefficients equal
numpy's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import harmonics_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import features_oracle as fo  # noqa: E402

SR = 44100.0


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "residuals_golden.npz"))


@pytest.fixture(scope="module")
def rows(golden):
    """The seven clips as rows of one matrix, zero padded."""
    n = int(golden["n_clips"][0])
    out = np.zeros((n, max(len(golden[f"pcm{i}"]) for i in range(n))))
    for i in range(n):
        out[i, :len(golden[f"pcm{i}"])] = golden[f"pcm{i}"] / 32768.0
    return out


@pytest.fixture
def dev_rows(hiplib, rows):
    """The same matrix in a device buffer."""
    dev = hiplib.ow_device_alloc(rows.nbytes, 0)
    assert dev and hiplib.ow_test_device_write(C.c_void_p(dev), rows.ctypes.data_as(C.c_void_p), rows.nbytes, 0) == 0
    yield dev
    hiplib.ow_device_free(dev, 0)


def mixed_batch(golden):
    """Lengths 129, 2205, 4410, 5292, 6615 and 26460, 0 / 1 / 8 harmonics, 64 recurrences or fewer and more than 64 in a segment, a note
    whose eleven offsets fall on one bin (MIDI 33, N = 2205: k = 3), bins outside 0 < k < N // 2 (N = 129: 55 Hz gives k = 0, 21900 Hz
    gives k = 64), harmonics past the Nyquist cut (the MIDI 96 clip searched around 4186 Hz: H6..H8)."""
    f = [golden[f"meta{i}"][2] for i in range(7)]
    return [(0, 0, 2205, 8, f[0]), (0, 2205, 8820, 8, f[0]), (0, 8820, 35280, 8, f[0]), (0, 4410, 8820, 1, f[0]), (0, 66150, 70560, 1, f[0]),
            (5, 0, 5292, 8, f[5]), (5, 0, 5292, 8, 4186.0), (5, 100, 229, 8, f[5]), (3, 1000, 1129, 8, f[3]), (3, 2205, 8820, 8, f[3]),
            (4, 0, 2205, 8, f[4]), (4, 0, 2205, 1, f[4]), (4, 2205, 8820, 8, f[4]), (2, 0, 129, 1, f[2]), (2, 3, 2208, 8, f[2]),
            (1, 2205, 8820, 8, f[1]), (6, 0, 2205, 0, f[6]), (6, 8820, 26460, 8, f[6]), (1, 0, 39690, 8, 27.5),
            (4, 1000, 1129, 8, f[4]), (3, 1000, 1129, 1, 21900.0), (2, 0, 19845, 8, f[2])]


def restated(x, segs, coeffs, bins):
    signals = [x[r, a:b] for r, a, b, nh, f0 in segs]
    plans = [(coeffs[i, :s[3]], bins[i, :s[3]], ref.past_cut(SR, s[4], s[3])) for i, s in enumerate(segs)]
    return ref.goertzel_amps_many(signals, plans)


def test_exact_against_restatement_with_the_library_s_plan(hiplib, golden, rows, dev_rows):
    from openwurli_amd import features
    segs = mixed_batch(golden)
    assert {b - a for _, a, b, _, _ in segs} >= {129, 2205, 4410, 5292, 6615, 26460} and {s[3] for s in segs} == {0, 1, 8}
    want = {}
    for wav24, x in ((None, rows), ("round", fo.quantize_round(rows) / 8388608.0), ("truncate", fo.quantize_truncate(rows) / 8388608.0)):
        for on_device in (False, True):
            amps, coeffs, bins = features.goertzel_segments(None if on_device else rows, SR, segs, wav24=wav24, plan=True,
                                                            device_audio=(dev_rows, rows.shape[0], rows.shape[1]) if on_device else None)
            if wav24 not in want:
                want[wav24] = restated(x, segs, coeffs, bins)
                n_rec = [len({int(k) for k in bins[i, h] if k >= 0}) for i in range(len(segs)) for h in range(8)]
                per_seg = [sum(n_rec[8 * i:8 * i + 8]) for i in range(len(segs))]
                assert max(per_seg) > 64 and 0 < min(p for p in per_seg if p) <= 11      # both loops of the kernel, both lane slots
                assert np.all(bins[10, 0] == 3)                                            # eleven offsets, one bin
                assert np.all(bins[6, 5:] == -1) and np.all(bins[6, :5] >= 0) and np.all(bins[16] == -1)   # past the cut; no harmonics asked for
                assert np.all(bins[19, :3] == -1) and np.all(bins[19, 3] >= 0) and set(bins[20, 0]) == {63, -1}   # k <= 0; k >= N // 2
            for i, (s, w) in enumerate(zip(segs, want[wav24])):
                assert np.array_equal(amps[i, :s[3]], w), (wav24, on_device, i, amps[i], w)
                assert np.all(amps[i, s[3]:] == 0.0)
    assert np.all(want[None][6][5:] == 1e-20) and np.all(want[None][19][:3] == 1e-20)
    # int16 samples are fixed points of the rounding quantiser (m / 2^15 * (2^23 - 1) rounds to 256 m); the truncating one moves them
    assert any(not np.array_equal(a, b) for a, b in zip(want[None], want["truncate"]))
    # one signal through the drop-in, and the method switch of extract_segments: the same numbers, the nominal frequencies
    one = features.extract_harmonics_goertzel(rows[0, 2205:8820], SR, segs[1][4])
    assert np.array_equal(one, want[None][1])
    a2, f2, r2 = features.extract_segments(rows, SR, segs[:2], method="goertzel")
    assert np.array_equal(a2[1], want[None][1]) and np.array_equal(f2[1], [segs[1][4] * (h + 1) for h in range(8)]) and np.all(r2 == 0.0)


def test_against_the_reference_s_amplitudes(hiplib, golden, rows):
    """Every extract_harmonics_goertzel call the reference made on the seven clips, in one call."""
    from openwurli_amd import features
    segs, want, moved = [], [], []
    for i in range(7):
        for (a, b, nh), amps, ulp in zip(golden[f"gseg{i}"], golden[f"gamp{i}"], golden[f"gulp{i}"]):
            segs.append((i, int(a), int(b), int(nh), golden[f"meta{i}"][2])); want.append(amps); moved.append(ulp)
    got, coeffs, bins = features.goertzel_segments(rows, SR, segs, plan=True)
    worst = 0.0
    for k, (s, w, m) in enumerate(zip(segs, want, moved)):
        c, b = ref.goertzel_plan(s[2] - s[1], SR, s[4], s[3])
        assert np.array_equal(bins[k, :s[3]], b)
        same = np.array_equal(coeffs[k, :s[3]], c)
        for h in range(s[3]):
            err = abs(got[k, h] - w[h]) / w[h]
            worst = max(worst, err / m[h] if m[h] > 0 else (0.0 if err == 0 else np.inf))
            print(f"seg {k} H{h + 1}: rel err {err:.3e}, one-ulp movement {m[h]:.3e}, coefficients equal numpy's: {same}")
            assert err == 0.0 if same else err <= 2.5 * m[h], (k, h, got[k, h], w[h], m[h])
        assert np.all(got[k, s[3]:] == 0.0)
    print("worst error in units of the one-ulp movement:", worst)
