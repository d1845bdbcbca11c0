"""ctypes loader of the CPU restatement of a render with run-time MLP corrections (tests/c/mlp_eval_ref.cpp, over the oracle's headers).
tests/native.py has oracle/Makefile build it into oracle/_build when it is out of date, and declares its functions from that source.

Also here, because the host and the GPU tests share them: the weight sets, the points and the jobs the tests use, and the restatement's
renders, computed once per process and never modified.
"""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import native

SR = 44100.0
N_WEIGHTS = 529
IDENTITY = np.array([0.0] * 5 + [1.0] * 5 + [1.0])
CLAMP_LO = np.array([-100.0] * 5 + [0.3] * 5 + [0.7])        # mlp_correction.rs:118-132
CLAMP_HI = np.array([100.0] * 5 + [3.0] * 5 + [1.2])
_LOCK = threading.Lock()
_VP = C.c_void_p


def lib():
    L = native.load("mlp_eval_ref")
    assert L.omr_weights_doubles() == N_WEIGHTS
    return L


def fade(note):
    """mlp_correction.rs:66-75, the same expressions."""
    midi = float(note)
    if midi < 65.0:
        return min(max((midi - (65.0 - 12.0)) / 12.0, 0.0), 1.0)
    if midi > 97.0:
        return min(max(((97.0 + 12.0) - midi) / 12.0, 0.0), 1.0)
    return 1.0


def infer(weights_flat, note, velocity, raw=False):
    """The restated infer with the weights as arguments: corrections [11] (and the denormalised outputs [11])."""
    w = np.ascontiguousarray(weights_flat, dtype=np.float64)
    assert w.shape == (N_WEIGHTS,)
    out, r = np.zeros(11), np.zeros(11)
    lib().omr_infer(w.ctypes.data_as(_VP), int(note), float(velocity), out.ctypes.data_as(_VP), r.ctypes.data_as(_VP) if raw else None)
    return (out, r) if raw else out


def infer_many(weights_flat, notes, velocities):
    """(corrections [n, 11], raw [n, 11])."""
    got = [infer(weights_flat, n, v, raw=True) for n, v in zip(notes, velocities)]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


# ---- the restatement's renders, computed once per process and shared by the tests (never modified) ----------------------------------
_RENDERS = {}


def render(note, vel_u8, dur, corr, sr=SR, volume=1.0, speaker=0.0, r_ldr=1e6, tremolo_depth=0.0, displacement_scale=None, poweramp=False,
           no_preamp=False, no_attack_noise=False, no_rail_sag=False, preamp_kind=0, power_amp_kind=0):
    """The restated `preamp-bench render` job with `corr` [11] at note-on; the defaults are what ml/render_model_notes.py passes (and the
    package's job defaults)."""
    c = np.ascontiguousarray(corr, dtype=np.float64)
    assert c.shape == (11,)
    key = (int(note), int(vel_u8), float(dur), c.tobytes(), float(sr), float(volume), float(speaker), float(r_ldr), float(tremolo_depth),
           displacement_scale, bool(poweramp), bool(no_preamp), bool(no_attack_noise), bool(no_rail_sag), int(preamp_kind), int(power_amp_kind))
    with _LOCK:
        got = _RENDERS.get(key)
    if got is None:
        n = int(dur * sr)
        out = np.zeros(max(n, 1))
        opts = np.array([volume, speaker, r_ldr, tremolo_depth, float("nan") if displacement_scale is None else displacement_scale])
        flags = (2 if poweramp else 0) | (4 if no_preamp else 0) | (8 if no_attack_noise else 0) | (16 if no_rail_sag else 0)
        m = lib().omr_render(int(note), int(vel_u8), float(dur), float(sr), opts.ctypes.data_as(_VP), flags, int(preamp_kind), int(power_amp_kind),
                             c.ctypes.data_as(_VP), out.ctypes.data_as(_VP), out.size)
        got = out[:m]
        got.setflags(write=False)
        with _LOCK:
            _RENDERS[key] = got
    return got


def render_many(jobs, corrs, dur, threads=16, **kw):
    """[row] of (note, velocity) jobs with their corrections, on at most 16 host threads (ctypes drops the GIL); the first goes alone, so
    whatever the oracle's headers settle lazily is built once."""
    jobs = list(jobs)
    lib()
    first = render(jobs[0][0], jobs[0][1], dur, corrs[0], **kw)
    with ThreadPoolExecutor(max_workers=min(threads, 16)) as ex:
        rest = list(ex.map(lambda k: render(jobs[k][0], jobs[k][1], dur, corrs[k], **kw), range(1, len(jobs))))
    return [first] + rest


# ---- what the tests share ----------------------------------------------------------------------------------------------------------
def set_c(builtin):
    """The built-in set with b3 replaced by +-50 alternating: every output saturates a clamp."""
    from openwurli_amd.mlp import MlpWeights
    arrays = {name: getattr(builtin, name).copy() for name in ("w1", "b1", "w2", "b2", "w3", "b3", "target_means", "target_stds")}
    arrays["b3"] = np.array([50.0 if i % 2 == 0 else -50.0 for i in range(11)])
    return MlpWeights(**arrays)


EDGE_NOTES = (40, 52, 53, 54, 64, 65, 97, 98, 108, 109)      # fade zero, both fade edges, both range edges and beyond


def infer_points(n=200, seed=5):
    """n (note, normalised velocity) points: random notes in 21..108 plus EDGE_NOTES; the velocities include 0, 1 and 1.5."""
    rng = np.random.default_rng(seed)
    notes = rng.integers(21, 109, size=n).astype(np.uint8)
    vels = rng.uniform(0.0, 1.0, size=n)
    notes[:len(EDGE_NOTES)] = EDGE_NOTES
    vels[10], vels[11], vels[12] = 0.0, 1.0, 1.5
    vels[0], vels[5] = 1.5, 0.0
    return notes, vels


PARITY_NOTES = (33, 40, 48, 57, 60, 66, 72, 84, 91, 96, 76)
PARITY_PAIRS = [(n, v) for n in PARITY_NOTES for v in (50, 127)]          # 22
HAND = np.array([30.0, -30.0, 30.0, -30.0, 30.0, 0.6, 1.7, 0.6, 1.7, 0.6, 0.85])      # cents +-30, decay 0.6 / 1.7, ds 0.85


def interleaved_jobs():
    """The 66 parity jobs: the 22 pairs x 3 sources, the sources interleaved so neighbouring lanes differ.  [(note, velocity, source)]."""
    return [(n, v, s) for (n, v) in PARITY_PAIRS for s in range(3)]
