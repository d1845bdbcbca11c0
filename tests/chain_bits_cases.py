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
    (|A error| near 0.013 V) takes its Newton loop from one sweep to two, three and four (the oracle's `info`, owo_output_stage_block: two
    from 1.8e-6 V, three from 1.3e-5 V, four from 2.9e-5 V).  The loop takes MOST sweeps -- five to eight -- only for |tap| in
    1.0512 .. 1.2864 V, where the closed-loop estimate meets the +-22 V rail; the engines here cross that band only in passing
    (tests/post_stage_cases.py places kicks inside it).  The loudest chord leaves about 0.4 V at the tap (the volume acts
    behind the power amp), so the volts come from PA_KICKS: a finite kick of the preamp's output node before the first recorded block
    (the hook of tests/test_gpu_preamp_pair.py::test_preamp_pair_finite_kicks), which the tap carries, alternating in sign, for the
    blocks that follow: 0.5, 1, 2 and 4 V alone take three, four, two and two sweeps."""
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


# ---- the job-side chain kernels (k_job_chain<MEL>, _wide, _fused, _row, k_bark_chain_row, k_pbench<MEL>, k_pbench_row, k_poly_chain): what
# tests/golden/job_chain_bits_parent.npz holds and tests/test_gpu_job_chain_bits.py renders again.  Each carries the same statements for a
# fresh preamp's start, its step with the NaN reset, the half-band pairs and the output stage, so an edit made to all of them reaches
# every form at once and the form-against-form tests cannot see it.
JOB_DUR = 0.05                   # 2 205 samples at 44 100 Hz: a remainder against the chunk sizes 16, 24 and 64
JOB_KEEP = 2205                  # samples of a kept row (a batch row whole; the head of a longer one)
_ENV = ("OW_CHAIN_WIDE", "OW_JOB_FUSED", "OW_JOB_OVERLAP", "OW_JOB_ROW", "OW_BARK_ROW", "OW_BARK_CHUNK", "OW_PBENCH_ROW", "OW_PBENCH_CHUNK",
        "OW_POLY_CHUNK", "OW_CENTROID_CHUNK")
# tests/test_gpu_parity.py::test_chain_wide_is_bit_identical's five forced forms, and the library's own choice
JOB_FORMS = {"default": {}, "0": {"OW_CHAIN_WIDE": "0", "OW_JOB_FUSED": "0"}, "1": {"OW_CHAIN_WIDE": "1"},
             "1-quad": {"OW_CHAIN_WIDE": "1", "OW_JOB_ROW": "0"}, "1-one-wavefront": {"OW_CHAIN_WIDE": "1", "OW_JOB_FUSED": "0"},
             "1-after-voices": {"OW_CHAIN_WIDE": "1", "OW_JOB_OVERLAP": "0"}}
# static LDR values: no move, inside the 0.01 ohm hysteresis, below the 1 kohm clamp (the oracle runs it without a NaN reset), and the
# cell's range as in test_chain_wide_is_bit_identical
JOB_R = (1e6, 1e6 + 0.005, 500.0, 2.5e4, 1e6, 4e4, 1e5, 1e6, 7e5)
_JOB_NOTES, _JOB_VELS = (33, 48, 60, 72, 84, 91, 96, 40, 55, 67, 79), (127, 50, 100, 20, 110, 64, 90, 35, 80)


def batch_jobs():
    """37 jobs = one lane-pair workgroup plus five, or four full row / quad workgroups plus a ragged one; mixed like
    test_chain_wide_is_bit_identical's.  The last job's displacement scale is infinite: the reed signal is not finite, `main - shadow` is
    not, and the adapter's NaN reset fires at every chain sample (the oracle does the same and renders silence) -- no other job-path test
    reaches that branch, and a wrong value in it is replaced by the reset."""
    jobs = [dict(note=_JOB_NOTES[k % 11], velocity=_JOB_VELS[k % 9], mlp=bool(k & 1), poweramp=bool(k & 2), volume=1.0 - 0.1 * (k % 4),
                 speaker=0.25 * (k % 5), r_ldr=JOB_R[k % 9]) for k in range(37)]
    jobs[36]["displacement_scale"] = float("inf")
    return jobs


# name -> (what, arguments)
JOB_CASES = {}
for _sr in (44100.0, 96000.0):                                   # 96 000 Hz: no oversampling
    for _form in JOB_FORMS:
        JOB_CASES[f"batch_{int(_sr)}_{_form}"] = ("batch", dict(sr=_sr, form=_form, kind=0, flags=False))
# --no-preamp and --tremolo-depth: a call with a tremolo runs on k_job_chain<false> whatever the switches say
JOB_CASES["batch_44100_flags"] = ("batch", dict(sr=44100.0, form="default", kind=0, flags=True))
JOB_CASES["batch_44100_melange"] = ("batch", dict(sr=44100.0, form="default", kind=1, flags=False))
for _kind, _rows in ((0, ("0", "1")), (1, (None,))):
    for _row in _rows:
        JOB_CASES[f"bark_{'melange' if _kind else 'legacy'}" + (f"_row{_row}" if _row else "")] = ("bark", dict(kind=_kind, row=_row))
        JOB_CASES[f"pbench_{'melange' if _kind else 'legacy'}" + (f"_row{_row}" if _row else "")] = ("pbench", dict(kind=_kind, row=_row))
JOB_CASES["poly"] = ("poly", {})
JOB_CASES["centroid"] = ("centroid", {})


def _rows_of(res, name, a, keep=(0, -1)):
    """One SHA-256 per row of a [rows][...] block and the head of two rows."""
    a = np.ascontiguousarray(a)
    res[f"{name}_sha"] = np.stack([digest(r) for r in a])
    for k in keep:
        res[f"{name}_row{k % len(a)}"] = a[k].reshape(-1)[:JOB_KEEP].copy()


def run_job_case(ow, name):
    """Returns {array name: array}; `peak` is the largest magnitude of the case's audio."""
    import os
    what, arg = JOB_CASES[name]
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    res = {}
    try:
        if what == "batch":
            os.environ.update(JOB_FORMS[arg["form"]])
            jobs = batch_jobs()
            if arg["flags"]:
                jobs = jobs[:5] + [dict(jobs[5], no_preamp=True), dict(jobs[6], tremolo_depth=0.5)]
            out = ow.batch_render(jobs, arg["sr"], JOB_DUR, preamp_kind=arg["kind"])
            assert out.shape == (len(jobs), int(JOB_DUR * arg["sr"]))
            _rows_of(res, "out", out, keep=(0, len(jobs) - 2))          # the last job is the silent one
            res["peak"] = np.array([np.abs(out).max()])
            res["row_peaks"] = np.abs(out).max(axis=1)
        elif what == "bark":
            import bark_audit_ref
            from openwurli_amd import bark_audit as ba
            from openwurli_amd.intermod_audit import NOTE_JOB_DTYPE
            notes, vels = (33, 41, 48, 57, 60, 66, 72, 79, 84, 90, 96), (127, 100, 80, 40, 20)      # test_gpu_bark_audit.py's _form_jobs(9)
            jobs = np.zeros(9, dtype=NOTE_JOB_DTYPE)
            jobs["note"], jobs["velocity"] = [notes[i % 11] for i in range(9)], [vels[i % 5] for i in range(9)]
            if arg["row"] is not None:
                os.environ["OW_BARK_ROW"] = arg["row"]
            rows, taps = ba.run_jobs(jobs, arg["kind"], *bark_audit_ref.SHORT_SIZE, taps=True)
            res["rows"] = np.frombuffer(rows.tobytes(), dtype=np.uint8).copy()
            res["taps_sha"] = np.stack([digest(r) for r in taps])      # per job: reed, pickup and preamp taps
            _rows_of(res, "pre", taps[:, 2])                           # the tap behind the chain, two rows whole
            res["peak"] = np.array([np.abs(taps[:, 2]).max()])
        elif what == "pbench":
            from openwurli_amd import preamp_bench as pb
            freqs = [20.0, 55.0, 110.0, 220.0, 440.0, 1000.0, 2000.0, 5000.0, 10000.0, 15000.0, 20000.0]
            amps = [0.001, 0.005, 0.02, 0.001, 0.05, 0.001, 0.005, 0.001, 0.02, 0.001, 0.005]
            r = [JOB_R[k % 9] for k in range(11)]
            r_reset = [1e6, 1e6, 1e6, 1.9e4, 2.5e4, 500.0, 1e5, 1e6 + 0.005, 7e5, 1e6, 4e4]          # differs from r_ldr on seven points
            if arg["row"] is not None:
                os.environ["OW_PBENCH_ROW"] = arg["row"]
            rows, trace = pb.run_points(pb.make_points(freqs, amps, r, r_reset), arg["kind"], trace=True)
            res["rows"] = np.frombuffer(rows.tobytes(), dtype=np.uint8).copy()
            _rows_of(res, "trace", trace)
            res["peak"] = np.array([np.abs(trace).max()])
        elif what == "poly":
            from openwurli_amd import render_poly as rp
            # the command's measuring window starts at sample 8 820, so a chord cannot be shorter than 0.2 s: 0.21 s = 9 261 samples
            chords = [((60,), (100,), 0.6, 1.0, 1e6, False), ((48, 55), (90, 70), 0.8, 0.5, 500.0, True), ((38, 59, 62), (45, 40, 110), 1.0, 0.0, 4e4, False)]
            rows, audio = rp.run_chords(chords, 0.21, final=True, separate_sum=True, residual=True)
            res["rows"] = np.frombuffer(rows.tobytes(), dtype=np.uint8).copy()
            for k, a in audio.items():
                _rows_of(res, k, a)
            res["peak"] = np.array([np.abs(audio["final"]).max()])
        elif what == "centroid":
            from openwurli_amd import centroid_track as ct
            # set_ldr_resistance(r) before reset(): the DC solve runs at the clamped --ldr
            jobs = [dict(note=n, velocity=v, ldr=r) for n, v, r in ((60, 100, 1e6), (33, 127, 1e6 + 0.005), (96, 110, 500.0), (72, 64, 2.5e4))]
            jobs.append(dict(note=48, velocity=90, ldr=7e5, no_preamp=True))
            rows, frames, audio = ct.run_jobs(jobs, JOB_DUR, end_ms=40.0, audio=True)
            res["rows"] = np.frombuffer(rows.tobytes(), dtype=np.uint8).copy()
            res["frames"] = frames.copy()
            _rows_of(res, "audio", audio)
            res["peak"] = np.array([np.abs(audio).max()])
    finally:
        for k in _ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return res
