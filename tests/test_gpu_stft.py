"""GPU: ow_stft_profile (the LDS FFT: mean spectrum and centroid of many clips per call) and ow_frame_rms against the float64 form of
tests/wurli_compare_ref.py, the numerical contract of openwurli_hip.h.

The bar per bin of mean_mag is |dev - ref| <= 1e-11 * max over the clip's frames of sum |frame * window|: that l1 sum bounds every bin,
an f64 FFT errs by about eps * log2 N ~ 3e-15 of the l2 norm, so the factor leaves three orders of magnitude for two implementations'
twiddles and is still four orders below float32.  The centroid's bar follows from it: with every |X_k| within d of the reference,
p_k = |X_k|^2 moves by at most 2 |X_k| d + d^2, and c = sum f_k p_k / (sum p_k + 1e-10) by at most 2 f_max sum |dp_k| / (sum p_k + 1e-10).
Row padding is NaN: one NaN in an output means that something at or beyond lengths[c] was read."""
import ctypes as C

import numpy as np
import pytest

import wurli_compare_ref as ref
from openwurli_amd import wurli_compare as wc

pytestmark = pytest.mark.gpu
SR = 44100.0


def _lengths(n, hop, stride):
    return [0, 1, n - 1, n, n + hop - 1, n + hop, 3 * n + 7, stride]


def _clips(seed, lengths, stride):
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal((len(lengths), stride))
    for c, n in enumerate(lengths):
        x[c, n:] = np.nan
    return x


def _wav24_round(v):
    q = np.sign(v) * np.floor(np.abs(v) * 8388607.0 + 0.5)          # round half away from zero
    return np.clip(q, -8388607.0, 8388607.0) / 8388608.0


def _reference(x, lengths, n_fft, hop, wav24=None):
    """(mean_mag, centroid, bar per clip, centroid bar per clip) of the float64 restatement."""
    mm, ce, bar, cbar = [], [], [], []
    for c, n in enumerate(lengths):
        y = x[c, :n] if wav24 is None else _wav24_round(x[c, :n])
        S, freqs, prod = ref.spectrogram(y, n_fft, hop, np.float64)
        l1 = np.abs(prod.astype(np.float64)).sum(axis=1)
        d = 1e-11 * float(l1.max())
        power = S ** 2
        mm.append(S.mean(axis=1))
        ce.append(float(np.mean(np.sum(freqs[:, None] * power, axis=0) / (np.sum(power, axis=0) + 1e-10))))
        bar.append(d)
        cbar.append(float(np.mean(2.0 * (SR / 2) * np.sum(2.0 * S * d + d * d, axis=0) / (np.sum(power, axis=0) + 1e-10))))
    return np.array(mm), np.array(ce), np.array(bar), np.array(cbar)


CASES = [(64, 1), (64, 16), (64, 512), (128, 32), (128, 512), (4096, 1024), (4096, 512), (8192, 2048), (8192, 512)]


@pytest.mark.parametrize("n_fft,hop", CASES)
def test_stft_profile_against_the_float64_restatement(hiplib, n_fft, hop):
    stride = max(3 * n_fft + 7, n_fft + hop) + 57
    lengths = _lengths(n_fft, hop, stride)
    x = _clips(n_fft + hop, lengths, stride)
    mm, ce = wc.stft_profile(x, lengths, n_fft, hop, SR)
    assert not np.isnan(mm).any() and not np.isnan(ce).any()
    want_mm, want_ce, bar, cbar = _reference(x, lengths, n_fft, hop)
    err = np.abs(mm - want_mm).max(axis=1)
    print("n_fft", n_fft, "hop", hop, "err / bar", (err / np.maximum(bar, 1e-300)).tolist(), "centroid err", np.abs(ce - want_ce).tolist(), "bar", cbar.tolist())
    assert np.all(err <= bar), (err, bar)
    assert np.all(np.abs(ce - want_ce) <= cbar), (ce, want_ce, cbar)
    assert np.all(mm[0] == 0.0) and ce[0] == 0.0 and mm[6].max() > 1.0        # an empty clip is one frame of zeros
    # each output alone gives the same bits, and a clip's numbers do not depend on its neighbours
    only_mm, none = wc.stft_profile(x, lengths, n_fft, hop, SR, centroid=False)
    none2, only_ce = wc.stft_profile(x[5:7], lengths[5:7], n_fft, hop, SR, mean_mag=False)
    assert none is None and none2 is None and only_mm.tobytes() == mm.tobytes() and only_ce.tobytes() == ce[5:7].tobytes()


def test_stft_profile_of_the_24_bit_file(hiplib):
    n_fft, hop, stride = 4096, 512, 3 * 4096
    lengths = [5000, 3 * 4096, 100]
    x = _clips(7, lengths, stride)
    x[1, :10] = [1.5, -1.5, 0.5 / 8388607.0, -0.5 / 8388607.0, 1.0, -1.0, 0.0, 2.5 / 8388607.0, 1e-9, -1e-9]      # clipped, ties, tiny
    mm, ce = wc.stft_profile(x, lengths, n_fft, hop, SR, wav24="round")
    want_mm, want_ce, bar, cbar = _reference(x, lengths, n_fft, hop, wav24="round")
    assert np.all(np.abs(mm - want_mm).max(axis=1) <= bar) and np.all(np.abs(ce - want_ce) <= cbar)
    as_is, _ = wc.stft_profile(x, lengths, n_fft, hop, SR)
    assert np.abs(as_is - mm).max() > 1e-9                                    # the quantiser is not a no-op


@pytest.mark.parametrize("n_fft", [64, 128, 4096, 8192])
def test_unit_impulse_has_a_flat_spectrum(hiplib, n_fft):
    """Independent of numpy's FFT: x = delta(n - n0) gives |X_k| = window[n0] for every k."""
    win = wc.hann_f32(n_fft)
    n0s = [1, 2, n_fft // 2 - 1, n_fft // 2, n_fft // 3, n_fft - 2]
    x = np.zeros((len(n0s), n_fft))
    for c, n0 in enumerate(n0s):
        x[c, n0] = 1.0
    mm, ce = wc.stft_profile(x, None, n_fft, 512, SR)
    for c, n0 in enumerate(n0s):
        assert win[n0] > 0.0 and np.all(np.abs(mm[c] - win[n0]) <= 1e-11 * win[n0]), (n_fft, n0)
    # a flat spectrum's centroid: sum_k f_k / (M + 1 + 1e-10 / w^2) ~ sr / 4
    assert np.all(np.abs(ce[2:4] - SR / 4) <= 1e-6)


@pytest.mark.parametrize("frame_len,hop", [(2048, 512), (1024, 128)])
def test_frame_rms(hiplib, frame_len, hop):
    stride = 3 * frame_len + 7 + 57
    lengths = _lengths(frame_len, hop, stride)
    x = _clips(frame_len, lengths, stride)
    rms, nf, ss = wc.frame_rms(x, lengths, frame_len, hop)
    assert not np.isnan(rms).any() and not np.isnan(ss).any()
    for c, n in enumerate(lengths):
        want = ref.rms_envelope(x[c, :n], frame_len, hop, np.float64)
        assert nf[c] == len(want) == wc.frame_count(n, frame_len, hop)
        # a sum of frame_len squares in another order, then one division and one square root
        assert np.all(np.abs(rms[c, :nf[c]] - want) <= frame_len * 2.0 ** -52 * want), c
        assert np.all(rms[c, nf[c]:] == 0.0)
        v = x[c, :n].astype(np.float32).astype(np.float64)
        exact = float(np.sum(v.astype(np.longdouble) ** 2))
        assert abs(ss[c] - exact) <= max(n, 1) * 2.0 ** -52 * exact, c
    assert nf[:6].tolist() == [1, 1, 1, 1, 1, 2] and nf[6] == (2 * frame_len + 7) // hop + 1 and ss[0] == 0.0 and rms[0, 0] == 0.0
    again, nf2, none = wc.frame_rms(x[3:], lengths[3:], frame_len, hop, sum_sq=False)
    assert none is None and again.tobytes() == rms[3:].tobytes() and nf2.tolist() == nf[3:].tolist()


def test_rows_in_device_memory_give_the_same_bits(hiplib):
    n_fft, hop, stride = 4096, 512, 9000
    lengths = [9000, 4096, 4500, 17]
    x = _clips(3, lengths, stride)
    dev = hiplib.ow_device_alloc(x.nbytes, 0)
    assert dev and hiplib.ow_test_device_write(C.c_void_p(dev), x.ctypes.data_as(C.c_void_p), x.nbytes, 0) == 0
    try:
        for mode in (None, "round"):
            host = wc.stft_profile(x, lengths, n_fft, hop, SR, wav24=mode)
            there = wc.stft_profile(None, lengths, n_fft, hop, SR, wav24=mode, device_audio=(dev, 4, stride))
            assert host[0].tobytes() == there[0].tobytes() and host[1].tobytes() == there[1].tobytes() and host[0][0].max() > 1.0
            h_rms = wc.frame_rms(x, lengths, 1024, 128, wav24=mode)
            d_rms = wc.frame_rms(None, lengths, 1024, 128, wav24=mode, device_audio=(dev, 4, stride))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(h_rms, d_rms))
        # a view into the rows: what compare_many does for the sustain slices
        off = wc.stft_profile(None, [8000, 3000, 3500, 0], n_fft, hop, SR, device_audio=(dev + 8 * 1000, 4, stride))
        want = wc.stft_profile(np.ascontiguousarray(x[:, 1000:]), [8000, 3000, 3500, 0], n_fft, hop, SR)
        assert off[0].tobytes() == want[0].tobytes() and off[1].tobytes() == want[1].tobytes()
    finally:
        hiplib.ow_device_free(dev, 0)


def test_refusals(hiplib):
    from openwurli_amd import binding
    x = np.zeros((2, 256)); lens = np.array([256, 100], dtype=np.uint32); win = np.ones(64); mm = np.zeros((2, 33)); ce = np.zeros(2)
    rms = np.zeros((2, 8)); nf = np.zeros(2, dtype=np.uint32); ss = np.zeros(2)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)       # noqa: E731

    def stft(clips=x, n=2, stride=256, lengths=lens, window=win, n_fft=64, hop=16, sr=SR, mode=-1, out_mm=mm, out_ce=ce):
        rc = hiplib.ow_stft_profile(p(clips), n, stride, p(lengths), p(window), n_fft, hop, sr, mode, 0, 0, p(out_mm), p(out_ce))
        return rc, binding.take_error(hiplib)

    def frms(clips=x, n=2, stride=256, lengths=lens, frame_len=64, hop=32, mode=-1, out=rms, fs=8, out_nf=nf, out_ss=ss):
        rc = hiplib.ow_frame_rms(p(clips), n, stride, p(lengths), frame_len, hop, mode, 0, 0, p(out), fs, p(out_nf), p(out_ss))
        return rc, binding.take_error(hiplib)

    for bad in (0, 1, 32, 63, 96, 8191, 16384, 1 << 31):
        assert stft(n_fft=bad) == (-1, f"ow_stft_profile: n_fft of {bad} is not a power of two in 64..8192"), bad
    assert stft(hop=0) == (-1, "ow_stft_profile: hop is 0: the reference's frame loop would never end")
    assert stft(mode=2) == (-1, "ow_stft_profile: unknown wav24_mode")
    for sr in (0.0, -1.0, float("nan"), float("inf")):
        assert stft(sr=sr) == (-1, "ow_stft_profile: sample_rate is not a finite positive number")
    for kw in ({"clips": None}, {"lengths": None}, {"window": None}, {"out_mm": None, "out_ce": None}):
        assert stft(**kw) == (-1, "ow_stft_profile: null argument"), kw
    assert stft(lengths=np.array([256, 257], dtype=np.uint32)) == (-1, "ow_stft_profile: clip 1: length 257 beyond the stride of 256 samples")
    assert stft(n=0, clips=None, lengths=None) == (0, "")
    assert frms(frame_len=0) == (-1, "ow_frame_rms: frame_len is 0")
    assert frms(hop=0) == (-1, "ow_frame_rms: hop is 0: the reference's frame loop would never end")
    assert frms(mode=7) == (-1, "ow_frame_rms: unknown wav24_mode")
    for kw in ({"clips": None}, {"lengths": None}, {"out": None}, {"out_nf": None}):
        assert frms(**kw) == (-1, "ow_frame_rms: null argument"), kw
    assert frms(lengths=np.array([300, 1], dtype=np.uint32)) == (-1, "ow_frame_rms: clip 0: length 300 beyond the stride of 256 samples")
    assert frms(fs=6) == (-1, "ow_frame_rms: clip 0: frames_stride smaller than its 7 frames")
    assert frms(n=0, clips=None) == (0, "")
    # after the refusals the same arguments still run
    assert stft()[0] == 0 and frms()[0] == 0 and nf.tolist() == [7, 2]
