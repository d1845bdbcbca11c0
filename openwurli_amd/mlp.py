"""The note-on MLP's corrections as data of a batch render (ml/: train -> model_weights.json -> listen, without rebuilding the library).

The reference bakes the 2 -> 16 -> 16 -> 11 network into mlp_weights.rs at compile time.  Here a weight set is a value: `infer` evaluates
many sets at many (note, velocity) points on the GPU, `batch_render_mlp` renders jobs with a weight set per job, `batch_render_corrected`
with the eleven corrections themselves per job (e.g. the residual-derived targets of ml/compute_residuals.py).  No CPU fallback.
"""
import ctypes as C
import json
import os

import numpy as np

from . import binding
from .binding import OwError

HIDDEN, OUTPUTS, INPUTS = binding.MLP_HIDDEN, binding.MLP_OUTPUTS, 2
_SHAPES = (("w1", (HIDDEN, INPUTS)), ("b1", (HIDDEN,)), ("w2", (HIDDEN, HIDDEN)), ("b2", (HIDDEN,)), ("w3", (OUTPUTS, HIDDEN)), ("b3", (OUTPUTS,)),
           ("target_means", (OUTPUTS,)), ("target_stds", (OUTPUTS,)))
N_DOUBLES = sum(int(np.prod(s)) for _, s in _SHAPES)          # 529 = sizeof(ow_mlp_weights) / 8
IDENTITY = np.array([0.0] * 5 + [1.0] * 5 + [1.0])            # MlpCorrections::identity (mlp_correction.rs:49-55): cents, decay ratios, ds
CORRECTION_NAMES = tuple(f"freq_offset_cents_{h}" for h in range(2, 7)) + tuple(f"decay_offset_{h}" for h in range(2, 7)) + ("ds_correction",)


class MlpWeights:
    """One weight set: w1 [16][2], b1 [16], w2 [16][16], b2 [16], w3 [11][16], b3 [11], target_means [11], target_stds [11] (float64)."""

    def __init__(self, **arrays):
        for name, shape in _SHAPES:
            a = np.array(arrays[name], dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"MlpWeights.{name}: shape {a.shape}, expected {shape}")
            setattr(self, name, a)

    @classmethod
    def from_flat(cls, flat):
        flat = np.asarray(flat, dtype=np.float64).ravel()
        if flat.size != N_DOUBLES:
            raise ValueError(f"a weight set is {N_DOUBLES} doubles, got {flat.size}")
        arrays, at = {}, 0
        for name, shape in _SHAPES:
            n = int(np.prod(shape))
            arrays[name] = flat[at:at + n].reshape(shape)
            at += n
        return cls(**arrays)

    def flat(self):
        """The set as ow_mlp_weights lays it out: 529 doubles."""
        return np.concatenate([getattr(self, name).ravel() for name, _ in _SHAPES])

    @classmethod
    def builtin(cls):
        """`ow_mlp_default_weights`: the set the library's own note-ons use (host only, no device)."""
        lib = binding.load_library()
        flat = np.zeros(N_DOUBLES)
        if lib.ow_mlp_default_weights(flat.ctypes.data_as(C.c_void_p)) != 0:
            raise OwError(binding.take_error(lib))
        return cls.from_flat(flat)

    @classmethod
    def from_json(cls, path_or_dict):
        """The `model_weights.json` ml/train_mlp.py:226-267 exports and ml/generate_rust_weights.py:46-76 reads."""
        if isinstance(path_or_dict, dict):
            data = path_or_dict
        else:
            with open(os.fspath(path_or_dict)) as f:
                data = json.load(f)
        layers = data.get("layers")
        if not isinstance(layers, list) or len(layers) != 3:
            raise ValueError(f"model weights: expected 3 layers, got {len(layers) if isinstance(layers, list) else layers!r}")
        acts = [layer.get("activation") for layer in layers]
        if acts != ["relu", "relu", "linear"]:
            raise ValueError(f"model weights: expected activations relu / relu / linear, got {acts}")
        sizes = (data.get("input_size"), data.get("hidden_size"), data.get("output_size"))
        if sizes != (INPUTS, HIDDEN, OUTPUTS):
            raise ValueError(f"model weights: input / hidden / output size {sizes}, this library evaluates {(INPUTS, HIDDEN, OUTPUTS)}")
        try:
            return cls(w1=layers[0]["weights"], b1=layers[0]["bias"], w2=layers[1]["weights"], b2=layers[1]["bias"],
                       w3=layers[2]["weights"], b3=layers[2]["bias"], target_means=data["target_means"], target_stds=data["target_stds"])
        except KeyError as e:
            raise ValueError(f"model weights: missing {e}") from None

    def to_json(self):
        """The dictionary train_mlp.py's export_weights writes (json.dump keeps every double: repr round-trips)."""
        layers = [{"weights": getattr(self, w).tolist(), "bias": getattr(self, b).tolist(), "activation": act}
                  for w, b, act in (("w1", "b1", "relu"), ("w2", "b2", "relu"), ("w3", "b3", "linear"))]
        return {"architecture": "MLP", "input_size": INPUTS, "output_size": OUTPUTS, "hidden_size": HIDDEN, "layers": layers,
                "target_means": self.target_means.tolist(), "target_stds": self.target_stds.tolist(),
                "input_normalization": {"midi_range": [21, 108], "velocity_range": [0, 127]}}

    def perturbed(self, rel, seed):
        """Every weight and bias of the three layers times (1 + rel x N(0, 1)); the target normalisation is kept.  For tests and sweeps."""
        rng = np.random.default_rng(seed)
        arrays = {name: getattr(self, name).copy() for name, _ in _SHAPES}
        for name in ("w1", "b1", "w2", "b2", "w3", "b3"):
            arrays[name] = arrays[name] * (1.0 + rel * rng.standard_normal(arrays[name].shape))
        return MlpWeights(**arrays)

    def __eq__(self, other):
        return isinstance(other, MlpWeights) and np.array_equal(self.flat(), other.flat())

    __hash__ = None


def _pack_sets(sets):
    """None (the built-in set) or a list of MlpWeights -> (pointer or None, count, the array that owns the memory)."""
    if sets is None:
        return None, 1, None
    if isinstance(sets, MlpWeights):
        sets = [sets]
    sets = list(sets)
    flat = np.ascontiguousarray(np.stack([s.flat() for s in sets])) if sets else np.zeros((0, N_DOUBLES))
    return flat.ctypes.data_as(C.c_void_p), len(sets), flat


def infer(sets, notes, velocities, device=0, raw=False):
    """`MlpCorrections::infer` (mlp_correction.rs:61-140) for every (set, point): float64 [n_sets, n_points, 11] = 5 frequency offsets in
    cents, 5 decay ratios, the displacement-scale correction.  sets: list of MlpWeights, or None for the built-in set; notes: MIDI bytes;
    velocities: normalised (0..1, clamped like the reference's).  raw=True also returns the denormalised network outputs before the fade
    outside MIDI 65..97 and the clamps."""
    lib = binding.load_library()
    ptr, n_sets, keep = _pack_sets(sets)
    no = np.ascontiguousarray(notes, dtype=np.uint8).ravel()
    ve = np.ascontiguousarray(velocities, dtype=np.float64).ravel()
    if no.size != ve.size:
        raise ValueError("notes and velocities differ in length")
    out = np.zeros((n_sets, no.size, OUTPUTS))
    raw_out = np.zeros((n_sets, no.size, OUTPUTS)) if raw else None
    rc = lib.ow_mlp_infer(ptr, n_sets, no.ctypes.data_as(C.c_void_p), ve.ctypes.data_as(C.c_void_p), no.size, int(device),
                          out.ctypes.data_as(C.c_void_p), raw_out.ctypes.data_as(C.c_void_p) if raw else None)
    del keep
    if rc != 0:
        raise OwError(binding.take_error(lib))
    return (out, raw_out) if raw else out


def _job_array(jobs):
    jobs = list(jobs)
    arr = (binding.OwJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        arr[i].note = int(j["note"]); arr[i].velocity = int(j["velocity"])
        arr[i].mlp = 1 if j.get("mlp", True) else 0
        arr[i].poweramp = 1 if j.get("poweramp", False) else 0
        arr[i].volume = float(j.get("volume", 1.0)); arr[i].speaker = float(j.get("speaker", 0.0)); arr[i].r_ldr = float(j.get("r_ldr", 1e6))
        arr[i].tremolo_depth = float(j.get("tremolo_depth", 0.0))
        arr[i].no_preamp = 1 if j.get("no_preamp", False) else 0
        arr[i].no_attack_noise = 1 if j.get("no_attack_noise", False) else 0
        ds = j.get("displacement_scale")
        arr[i].has_displacement_scale = 0 if ds is None else 1
        arr[i].displacement_scale = 0.0 if ds is None else float(ds)
    return arr, len(jobs)


def _render(call, n_jobs, sample_rate, duration_s, out_device_ptr, stride):
    """call(out pointer, stride, out_is_device) -> samples per job; the out_device_ptr / stride handling of engine.batch_render."""
    lib = binding.load_library()
    n = int(duration_s * sample_rate)
    stride = int(stride or n)
    if out_device_ptr is not None:
        if call(C.c_void_p(out_device_ptr), stride, 1) < 0:
            raise OwError(binding.take_error(lib))
        return None
    out = np.zeros((n_jobs, stride), dtype=np.float64)
    got = call(out.ctypes.data_as(C.c_void_p), stride, 0)
    if got < 0:
        raise OwError(binding.take_error(lib))
    return out[:, :got]


def batch_render_corrected(jobs, corrections, sample_rate=44100.0, duration_s=2.0, device=0, preamp_kind=0, out_device_ptr=None, stride=None,
                           power_amp_kind=0, no_rail_sag=False):
    """`engine.batch_render` with job j's note-on taking corrections[j] ([n_jobs, 11]: 5 cents, 5 decay ratios, ds) in place of what the
    network would return; a job's `mlp` key is ignored.  Every other key and keyword means what it means to `batch_render`."""
    lib = binding.load_library()
    arr, n_jobs = _job_array(jobs)
    corr = np.ascontiguousarray(corrections, dtype=np.float64)
    if corr.shape != (n_jobs, OUTPUTS):
        raise ValueError(f"corrections: shape {corr.shape}, expected {(n_jobs, OUTPUTS)}")
    cfg = binding.OwBatchCfg(float(sample_rate), float(duration_s), int(device), int(preamp_kind), int(power_amp_kind), 1 if no_rail_sag else 0)
    return _render(lambda out, st, on_dev: lib.ow_batch_render_corrected(arr, n_jobs, C.byref(cfg), corr.ctypes.data_as(C.c_void_p), out, st, on_dev),
                   n_jobs, sample_rate, duration_s, out_device_ptr, stride)


def batch_render_mlp(jobs, sets, set_of_job, sample_rate=44100.0, duration_s=2.0, device=0, preamp_kind=0, out_device_ptr=None, stride=None,
                     power_amp_kind=0, no_rail_sag=False):
    """`engine.batch_render` with the network's weights per job: job j with `mlp` on (the default here) takes the corrections of
    sets[set_of_job[j]] at (note, velocity / 127), a job with mlp=False the identity.  The network runs on the GPU in front of the
    voices; nothing passes through the host in between.  sets: list of MlpWeights, or None for the built-in set."""
    lib = binding.load_library()
    arr, n_jobs = _job_array(jobs)
    ptr, n_sets, keep = _pack_sets(sets)
    soj = np.ascontiguousarray(set_of_job, dtype=np.uint32).ravel()
    if soj.size != n_jobs:
        raise ValueError(f"set_of_job: {soj.size} entries for {n_jobs} jobs")
    cfg = binding.OwBatchCfg(float(sample_rate), float(duration_s), int(device), int(preamp_kind), int(power_amp_kind), 1 if no_rail_sag else 0)
    try:
        return _render(lambda out, st, on_dev: lib.ow_batch_render_mlp(arr, n_jobs, C.byref(cfg), ptr, n_sets, soj.ctypes.data_as(C.c_void_p), out, st, on_dev),
                       n_jobs, sample_rate, duration_s, out_device_ptr, stride)
    finally:
        del keep


def render_and_extract(pairs, sets, sample_rate=44100.0, duration_s=2.0, device=0, preamp_kind=0, wav24="round", jobs_extra=None):
    """`features.render_and_extract` for several weight sets in ONE render: every (midi, velocity) pair with every set (None in the list =
    the `--no-mlp` baseline, i.e. identity corrections), the audio staying in HBM for `extract_model_features`.
    Returns one features dictionary per entry of `sets`, in order."""
    from .features import extract_model_features
    lib = binding.load_library()
    pairs, sets = list(pairs), list(sets)
    if not pairs or not sets:
        return [{} for _ in sets]
    real = [s for s in sets if s is not None]
    index, k = [], 0
    for s in sets:
        index.append(0 if s is None else k)
        k += s is not None
    extra = dict(jobs_extra or {})
    jobs = [dict(extra, note=m, velocity=v, mlp=s is not None) for s in sets for m, v in pairs]
    set_of_job = [index[i] for i in range(len(sets)) for _ in pairs]
    n = int(duration_s * sample_rate)
    buf = lib.ow_device_alloc(8 * len(jobs) * n, int(device))
    if not buf:
        raise OwError(binding.take_error(lib))
    try:
        batch_render_mlp(jobs, real or None, set_of_job, sample_rate=sample_rate, duration_s=duration_s, device=device, preamp_kind=preamp_kind,
                         out_device_ptr=buf, stride=n)
        out = []
        for i in range(len(sets)):
            rows = buf + 8 * i * len(pairs) * n
            out.append(extract_model_features(None, sample_rate, pairs, device, wav24, device_audio=(rows, len(pairs), n, n)))
        return out
    finally:
        lib.ow_device_free(buf, int(device))
