"""The renders behind tests/golden/chain_bits_parent.npz and tests/golden/power_amp_cases_parent.npz: what tools/record_chain_bits.py
records with one build of the library and what tests/test_gpu_chain_bits.py / tests/test_gpu_power_amp_cases.py render again with the
current one.  tanh_fast, power_amp and the preamp step are shared by every chain kernel, so the cross-kernel bit-identity tests cannot
see a change common to all of them: these renders pin the bits of a known build instead.

Every array a run returns goes into the fixture under `<case>/<name>`; a block that is too large to keep whole is kept as the rows of a
few engines plus a SHA-256 over all of it."""
import ctypes
import hashlib

import numpy as np

SR = 48000.0
NOTES = list(range(33, 97))                                           # the bench chord
VELOCITIES = [(40 + (37 * k) % 88) / 127.0 for k in (0, 1, 2)]        # bench.py's instance velocities of instances 0, 1, 2
LENGTHS = (512, 37, 1)           # sixteen whole staging chunks of the pair preamp, a partial chunk, the shortest block
LANE = {"chain_fused": 0, "preamp_wide": 0, "chain_stream": 0}        # the two-launch lane path at any pool size

# name -> (engines, switches, streamed into a pinned host block)
CHAIN_CASES = {
    "pair_1": (1, dict(LANE, preamp_pair=1, post_pair=1), False),         # one lane
    "pair_65": (65, dict(LANE, preamp_pair=1, post_pair=1), False),       # a full wavefront plus one lane
    "pair_130": (130, dict(LANE, preamp_pair=1, post_pair=1), False),     # two full wavefronts plus two lanes
    "lanepair_65": (65, dict(LANE, preamp_pair=0, post_pair=0), False),   # k_preamp + k_post<true>
    "stream_65": (65, dict(LANE, chain_stream=1, out_direct=1), True),    # k_chain_stream
}


def kept_engines(n):
    """Engines whose rows the fixture keeps whole: the first and last lane of every wavefront that has them, and the pool's last."""
    return sorted({e for e in (0, 63, 64, 127, 128, n - 1) if 0 <= e < n})


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def run_chain(ow, name):
    """Render LENGTHS on the pool of CHAIN_CASES[name]: the bench chord at three of the instance velocities, tremolo depth 0.5, one
    tremolo phase per engine.  Returns {array name: array}."""
    n, switches, streamed = CHAIN_CASES[name]
    g = ow.EnginePool(SR, n)
    g.set_sample_rate(SR)
    g.ensure_buffer_capacity(1024)
    for k, v in switches.items():
        g.set_switch(k, v)
        assert g.get_switch(k) == v, (k, v)
    if n > 1:
        g.stagger_tremolo(n)
    for k in range(n):
        e = g[k]
        e.set_volume(0.5); e.set_tremolo_depth(0.5); e.set_speaker_character(0.0); e.set_mlp_enabled(True)
        for note in NOTES:
            e.note_on(note, VELOCITIES[k % 3])
    sel = kept_engines(n)
    stride = max(LENGTHS)
    host = g.alloc_host_block(stride) if streamed else None
    res = {}
    for b, length in enumerate(LENGTHS):
        if streamed:
            g.render_into(host[0], stride, length)
            out = np.ctypeslib.as_array((ctypes.c_float * (n * stride)).from_address(host[0])).reshape(n, stride)[:, :length].copy()
        else:
            out = g.render(length)
        states = np.stack([np.stack([g[k].read_preamp_state(False), g[k].read_preamp_state(True)]) for k in range(n)])
        res[f"out{b}"] = out[sel].copy()
        res[f"out{b}_sha"] = digest(out)
        res[f"state{b}"] = states[sel].copy()
        res[f"state{b}_sha"] = digest(states)
        res[f"pre{b}_sha"] = digest(g.preamp_out(length * 2))
    res["resets"] = np.array([(g[k].diag().output_nan_resets, g[k].diag().preamp_nan_resets) for k in range(n)], dtype=np.int64)
    res["peak"] = np.array([max(float(np.abs(res[f"out{b}"]).max()) for b in range(len(LENGTHS)))])
    if streamed:
        g.free_host_block(host)
    g.close()
    return res


# ---- the output stage alone: 64 engines x (96 + 33) samples x 2 chain samples = 16 512 inputs of the power amp per case
PA_ENGINES = 64
PA_WARM = (1000,) * 6        # rendered before the recorded blocks: the chords of the first half of the pool are in full swing by then
PA_KICKS = {24: 0.5, 25: -0.5, 26: 1.0, 27: -1.0, 28: 2.0, 29: -2.0, 30: 4.0, 31: -4.0}    # engine -> volts added to the main state's OUT node
PA_LENGTHS = (96, 33)        # more than one 64-sample chunk of the output stage and a ragged one
PA_CASES = {"post_pair_0": 0, "post_pair_1": 1}


def pa_engine_setup(k):
    """(notes, velocity, volume) of engine k.  Engine 0 is silent.  Engines 1..31 are struck before the warm-up block: from one soft
    key to the whole bench chord at ff, so the preamp tap runs from microvolts into the preamp's clipping.  Engines 32..63 are struck
    right before the first recorded block: their taps grow from zero through the microvolt range, where the power amp's crossover term
    (|A error| near 0.013 V) makes its Newton loop take most sweeps.  The loudest chord leaves about 0.4 V at the tap (the volume acts
    behind the power amp), so the volts come from PA_KICKS: a finite kick of the preamp's output node before the first recorded block
    (the hook of tests/test_gpu_preamp_pair.py::test_preamp_pair_finite_kicks), which the tap carries for the next samples."""
    if k == 0:
        return [], 0.0, 0.5
    j = (k - 1) % 31                       # 0..30 in both halves
    count = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)[j % 12]
    notes = [NOTES[(5 * j + 7 * i) % 64] for i in range(count)]
    notes = sorted(set(notes))
    velocity = (0.02, 0.1, 0.3, 0.6, 1.0)[(j // 3) % 5] if j % 3 else 1.0
    volume = (1e-6, 1e-3, 0.05, 0.5, 1.0)[j % 5]
    return notes, velocity, volume


def run_power_amp(ow, name):
    g = ow.EnginePool(SR, PA_ENGINES)
    g.set_sample_rate(SR)
    g.ensure_buffer_capacity(max(PA_WARM))
    for k, v in dict(LANE, preamp_pair=1, post_pair=PA_CASES[name]).items():
        g.set_switch(k, v)
        assert g.get_switch(k) == v, (k, v)
    g.stagger_tremolo(PA_ENGINES)
    for k in range(PA_ENGINES):
        e = g[k]
        notes, velocity, volume = pa_engine_setup(k)
        e.set_volume(volume); e.set_tremolo_depth(0.5); e.set_speaker_character((k % 3) * 0.5); e.set_mlp_enabled(True)
        if k < 32:
            for note in notes:
                e.note_on(note, velocity)
    for length in PA_WARM:
        g.render(length, to_host=False)
    for k in range(32, PA_ENGINES):
        notes, velocity, _ = pa_engine_setup(k)
        for note in notes:
            g[k].note_on(note, velocity)
    for k, dv in PA_KICKS.items():
        g[k].poke_preamp_node(6, float(g[k].read_preamp_state(False)[2 + 6] + dv))
    res = {}
    taps = []
    for b, length in enumerate(PA_LENGTHS):
        res[f"out{b}"] = g.render(length)
        taps.append(g.preamp_out(length * 2))
        res[f"pre{b}_sha"] = digest(taps[-1])
    tap = np.abs(np.concatenate(taps, axis=1))
    res["tap_absmax"] = tap.max(axis=1)                                             # per engine, volts at the preamp tap
    res["tap_absmin_nonzero"] = np.array([tap[tap > 0.0].min()])
    res["resets"] = np.array([(g[k].diag().output_nan_resets, g[k].diag().preamp_nan_resets) for k in range(PA_ENGINES)], dtype=np.int64)
    g.close()
    return res
