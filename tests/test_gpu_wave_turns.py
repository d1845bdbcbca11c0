"""k_preamp_pair and k_post<false, true> in workgroups of eight wavefronts that take turns by progress (ow_wave_turns.h): against the
lane-pair kernels (k_preamp + k_post<true>), which keep their one-wavefront workgroups.  Turn-taking only changes which wavefront of a
SIMD is issued first, so the preamp tap, every chain-state row and the f32 block carry the same bits, block by block."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANE_PATH = {"chain_fused": 0, "preamp_wide": 0, "chain_stream": 0}     # the two-launch lane path at any pool size
CS_COUNT = 137                                                          # OW_TEST_CS_COUNT (include/openwurli_hip_test.h)
BLOCKS = (1, 31, 32, 33, 64, 65, 512)       # around the 32-sample staging chunk of the preamp and the 64-sample one of the output stage
# one lane; a full wavefront; one lane in a second wavefront; wavefront 4 the only partner of wavefront 0 (257) and ragged; five whole
# wavefronts: 0 has a partner, 1..3 have none; a ragged last wavefront of a whole workgroup; a whole workgroup; a second workgroup of one
# lane; three workgroups, the last ragged
POOLS = (1, 64, 65, 257, 320, 511, 512, 513, 1100)


def _depth_ramp(g):
    for k in range(0, g.n, 3):
        g[k].set_tremolo_depth(1.0 - (k % 5) * 0.25)


def _restrike_all(g):
    for k in range(g.n):
        g[k].note_on(60 + k % 3, 1.0)          # a sounding key: the steal pass, on every engine of the pool


def _run(sr, n_eng, pair, lengths, events):
    """Render `lengths` on a pool forced onto k_preamp_pair + k_post<false, true> (pair 1) or k_preamp + k_post<true> (pair 0);
    events[b](g) runs before block b.  Per block: (f32 block, preamp tap, all chain-state rows of all engines)."""
    import openwurli_amd as ow
    g = ow.EnginePool(sr, n_eng)
    g.set_sample_rate(sr)
    for k, v in dict(LANE_PATH, preamp_pair=pair, post_pair=pair).items():
        g.set_switch(k, v)
        assert g.get_switch(k) == v, (k, v)
    if n_eng > 1:
        g.stagger_tremolo(min(n_eng, 13))
    for k in range(n_eng):
        e = g[k]
        e.set_tremolo_depth((k % 5) * 0.25); e.set_volume(0.3 + 0.05 * (k % 8)); e.set_speaker_character((k % 3) * 0.4)
        for note in (40 + k % 30, 60 + k % 3, 67 + k % 20):
            e.note_on(note, 0.5 + 0.4 * ((k * 37) % 101) / 101.0)
    blocks = []
    for b, n in enumerate(lengths):
        if b in events:
            events[b](g)
        out = g.render(n).copy()
        pre = g.preamp_out(n * 2).copy()
        rows = np.stack([g[k].read_chain_rows(0, CS_COUNT) for k in range(n_eng)])
        blocks.append((out, pre, rows))
    diags = [(g[k].diag().output_nan_resets, g[k].diag().preamp_nan_resets) for k in range(n_eng)]
    g.close()
    return blocks, diags


def _same(ref, got, what):
    for b, ((o0, p0, r0), (o1, p1, r1)) in enumerate(zip(ref[0], got[0])):
        assert p0.tobytes() == p1.tobytes(), (what, b, "preamp tap")
        assert r0.tobytes() == r1.tobytes(), (what, b, "chain-state rows")
        assert o0.tobytes() == o1.tobytes(), (what, b, "output")
    assert ref[1] == got[1], (what, "diag")
    assert max(float(np.abs(o).max()) for o, _, _ in got[0]) > 1e-3, what


POOL_EVENTS = {2: _depth_ramp, 4: _restrike_all}


@functools.lru_cache(maxsize=None)
def _pool_reference(sr, n_eng):
    return _run(sr, n_eng, 0, BLOCKS, POOL_EVENTS)


@pytest.mark.parametrize("n_eng,sr", [(n, 48000.0) for n in POOLS] + [(65, 44100.0), (513, 44100.0)])
def test_wave_turns_pool_sizes(hiplib, n_eng, sr):
    """A struck chord, a depth ramp and a re-strike of every engine, tremolo phases staggered, in blocks of BLOCKS samples."""
    _same(_pool_reference(sr, n_eng), _run(sr, n_eng, 1, BLOCKS, POOL_EVENTS), (n_eng, sr))


def test_wave_turns_sub_ranges(hiplib):
    """Ranges that start inside a wavefront and inside a workgroup: warm_up of one engine renders that engine alone (e0 = 77: not a
    multiple of 64; 577 and 1099: nor of 512, in the second and third workgroup of a whole-pool launch), between whole-pool blocks."""
    def ranges(g):
        _depth_ramp(g)
        for k in (77, 577, 1099):
            g[k].warm_up()

    events = {1: ranges, 2: _restrike_all}
    lengths = (65, 33, 64)
    ref = _run(48000.0, 1100, 0, lengths, events)
    _same(ref, _run(48000.0, 1100, 1, lengths, events), "sub-ranges")


def test_wave_turns_one_wavefront_falls_behind(hiplib):
    """Finite kicks of node voltages (tests/test_gpu_preamp_pair.py::test_preamp_pair_finite_kicks: microvolts to tens of volts, main
    and shadow states), all of them in wavefront 2 of a 512-engine pool: that wavefront iterates its Newton loop to the end while its
    partner on the SIMD (wavefront 6) and every other wavefront take the short way, so the two drift apart and their priorities flip."""
    import dk_step_cases as dk
    first = 2 * 64

    def kick(g):
        for i, dv in enumerate(dk.KICK_MAGS):
            k = first + (i * 37 + 3) % 64
            for shadow, sign in ((False, 1.0), (True, -1.0)) if i % 2 else ((True, 1.0),):
                now = g[k].read_preamp_state(shadow)
                g[k].poke_preamp_node(i % 8, float(now[2 + i % 8] + sign * dv), shadow=shadow)

    events = {1: kick, 3: kick}
    lengths = (96,) * 5
    ref = _run(48000.0, 512, 0, lengths, events)
    got = _run(48000.0, 512, 1, lengths, events)
    _same(ref, got, "kicks in one wavefront")
    assert all(d == (0, 0) for d in got[1]), got[1]
    assert got[0][1][2][first:first + 64].tobytes() != got[0][0][2][first:first + 64].tobytes()
    for o, _, _ in got[0]:
        assert np.all(np.isfinite(o))
