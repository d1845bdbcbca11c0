"""k_preamp_pair (ow_kernels.h): the legacy preamp on the lane path with lane = engine -- main and shadow solver state in one lane, the
per-engine work done once, the two Newton loops in one wave-uniform loop -- against k_preamp (lane = (engine, main | shadow)).  The same
bits at the preamp tap, in both solver states' rows and at the output, block by block, and the same reset counters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANE_PATH = {"chain_fused": 0, "preamp_wide": 0, "chain_stream": 0}     # the two-launch lane path at any pool size


def _run(ow, sr, n_eng, pair, lengths, events, stagger=0, state_engines=None):
    """Render `lengths` on a pool forced onto k_preamp (pair 0) or k_preamp_pair (pair 1); events[b](g) runs before block b."""
    osr = 2 if sr < 88200.0 else 1
    g = ow.EnginePool(sr, n_eng)
    g.set_sample_rate(sr)
    for k, v in LANE_PATH.items():
        g.set_switch(k, v)
    g.set_switch("preamp_pair", pair)
    assert g.get_switch("preamp_pair") == pair
    if stagger:
        g.stagger_tremolo(stagger)
    for k in range(n_eng):
        e = g[k]
        e.set_tremolo_depth((k % 5) * 0.25); e.set_volume(0.3 + 0.05 * (k % 8)); e.set_speaker_character((k % 3) * 0.4)
        for note in (40 + k % 30, 60 + k % 3, 67 + k % 20):
            e.note_on(note, 0.5 + 0.4 * ((k * 37) % 101) / 101.0)
    sel = range(n_eng) if state_engines is None else state_engines
    outs, pres, states = [], [], []
    for b, n in enumerate(lengths):
        if b in events:
            events[b](g)
        outs.append(g.render(n).copy())
        pres.append(g.preamp_out(n * osr).copy())
        states.append(np.stack([np.stack([g[k].read_preamp_state(False), g[k].read_preamp_state(True)]) for k in sel]))
    diags = [(g[k].diag().output_nan_resets, g[k].diag().preamp_nan_resets) for k in sel]
    g.close()
    return outs, pres, states, diags


def _same(a, b, what):
    outs0, pres0, st0, d0 = a
    outs1, pres1, st1, d1 = b
    for i in range(len(outs0)):
        assert pres0[i].tobytes() == pres1[i].tobytes(), (what, i, "preamp tap")
        assert st0[i].tobytes() == st1[i].tobytes(), (what, i, "preamp state rows")
        assert outs0[i].tobytes() == outs1[i].tobytes(), (what, i, "output")
    assert d0 == d1, (what, "diag")


def _restrike_all(g):
    for k in range(g.n):
        g[k].note_on(60 + k % 3, 1.0)          # a sounding key: the steal pass, on every engine of the pool


def _depth_ramp(g):
    for k in range(0, g.n, 3):
        g[k].set_tremolo_depth(1.0 - (k % 5) * 0.25)


@pytest.mark.parametrize("sr", [44100.0, 48000.0, 96000.0])
def test_preamp_pair_is_bit_identical_small_pool(hiplib, sr):
    """256 engines (four wavefronts of the pair kernel, eight of k_preamp): a sustained chord, a depth ramp that starts mid-block (blocks
    of 97 / 300 samples against the 32- and 64-sample staging chunks), a re-strike of every engine, ragged block lengths incl. 1, and an
    output NaN guard event followed by the deferred preamp / oversampler reset, at both oversampled rates and at osr = 1."""
    import openwurli_amd as ow
    lengths = [512, 97, 300, 1, 64, 33, 512, 256]
    hot = 131

    def nan_out(g):
        g[hot].set_volume(1e308)                   # a non-finite output -> NaN guard -> deferred preamp / oversampler reset

    def calm(g):
        g[hot].set_volume(0.5); g[7].reset(); g[7].note_on(55, 0.9)

    events = {1: _depth_ramp, 3: _restrike_all, 4: nan_out, 5: calm}
    a = _run(ow, sr, 256, 0, lengths, events)
    b = _run(ow, sr, 256, 1, lengths, events)
    _same(a, b, ("256", sr))
    assert a[3][hot][0] >= 1, a[3][hot]                        # the guard did fire
    assert max(float(np.abs(o).max()) for o in a[0]) > 1e-3


def test_preamp_pair_is_bit_identical_ragged_ranges(hiplib):
    """4 133 engines: not a multiple of 64 or of 32 (a ragged last wavefront in both kernels), staggered tremolo phase groups, a
    mid-block depth ramp, a whole-pool re-strike, and single-engine ranges that start at e0 > 0 (WurliEngine::warm_up of one engine renders
    that engine alone).  Solver-state rows are compared on a sample of engines across the wavefront boundaries."""
    import openwurli_amd as ow
    sr, n_eng = 48000.0, 4133
    lengths = [512, 300, 97, 512]
    sel = sorted({0, 1, 31, 32, 63, 64, 65, 127, 2047, 2048, 2049, 4095, 4096, 4127, 4128, 4131, 4132} | set(range(5, n_eng, 97)))

    def ranges(g):
        _depth_ramp(g)
        g[77].warm_up(); g[4130].warm_up()

    events = {1: ranges, 2: _restrike_all}
    a = _run(ow, sr, n_eng, 0, lengths, events, stagger=13, state_engines=sel)
    b = _run(ow, sr, n_eng, 1, lengths, events, stagger=13, state_engines=sel)
    _same(a, b, "4133")
    assert max(float(np.abs(o).max()) for o in a[0]) > 1e-3


def test_preamp_pair_nan_reset(hiplib):
    """The preamp's own NaN reset (dk_preamp_legacy.rs:610-615), driven by the node poke of
    test_gpu_parity.py::test_preamp_nan_reset_in_every_chain_kernel: NaN in a main state, NaN in a shadow state, and infinity a block later,
    on engines in different wavefronts of both kernels.  Same counters, same bits in that block and after it."""
    import openwurli_amd as ow
    sr, n_eng, length = 48000.0, 200, 96

    def poke_nan(g):
        g[1].poke_preamp_node(6, float("nan")); g[70].poke_preamp_node(2, float("nan"), shadow=True)

    def poke_inf(g):
        g[133].poke_preamp_node(0, float("inf"))

    res = {}
    for pair in (0, 1):
        res[pair] = _run(ow, sr, n_eng, pair, [length] * 5, {2: poke_nan, 3: poke_inf})
    _same(res[0], res[1], "nan reset")
    d = res[1][3]
    assert d[1][1] >= 1 and d[70][1] >= 1 and d[133][1] >= 1 and d[0][1] == 0, (d[1], d[70], d[133], d[0])
    for o in res[1][0]:
        assert np.all(np.isfinite(o))


def test_preamp_pair_finite_kicks(hiplib):
    """Finite kicks of node voltages (sizes from the single-step corpus, tests/dk_step_cases.py: microvolts to tens of volts), main states
    and shadow states, on engines spread over the wavefronts of both kernels: in k_preamp a kicked state's wavefront iterates with its 63
    neighbours, in k_preamp_pair with the other state of its own lane too.  Same bits in the kicked block and after it; no reset counted."""
    import dk_step_cases as dk
    import openwurli_amd as ow
    sr, n_eng, length = 48000.0, 200, 96

    def kick(g):
        for i, dv in enumerate(dk.KICK_MAGS):
            k = (i * 37 + 3) % n_eng
            for shadow, sign in ((False, 1.0), (True, -1.0)) if i % 2 else ((True, 1.0),):
                now = g[k].read_preamp_state(shadow)
                g[k].poke_preamp_node(i % 8, float(now[2 + i % 8] + sign * dv), shadow=shadow)

    res = {}
    for pair in (0, 1):
        res[pair] = _run(ow, sr, n_eng, pair, [length] * 5, {2: kick})
    _same(res[0], res[1], "finite kicks")
    assert all(d == (0, 0) for d in res[1][3]), res[1][3]
    assert res[1][2][2].tobytes() != res[1][2][1].tobytes()
    for o in res[1][0]:
        assert np.all(np.isfinite(o))


def test_preamp_pair_default_threshold(hiplib):
    """The switch: -1 (default) picks the pair kernel from 131 072 engines; 0 / 1 force it; only those three values."""
    import openwurli_amd as ow
    g = ow.EnginePool(48000.0, 4)
    assert g.get_switch("preamp_pair") in (-1, 0, 1)
    for v in (1, 0, -1):
        g.set_switch("preamp_pair", v)
        assert g.get_switch("preamp_pair") == v
    g.set_switch("preamp_pair", 5)
    assert g.get_switch("preamp_pair") == 1
    g.close()
