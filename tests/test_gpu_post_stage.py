"""The output stage of every chain kernel against the oracle's, one block at a time, in f64 (tests/post_stage_cases.py has the corpus, the
comparison and its measured bars; tests/test_oracle_post_stage_cases.py what they rest on).

Eleven kernels of the engine path carry a copy of the stage: k_post<false>, k_post<true>, k_post<false,true>, k_chain_fused<true|false>,
k_chain_row<true|false, 8|16>, k_chain_stream and the tail of k_post_mpa.  Each is selected with the settable switches on pools of 1, 33,
65 and 130 engines; engine k plays recipe k of the corpus from start rows written through ow_test_engine_write_chain_rows, for blocks of
1, 2, 37, 64, 65 and 129 samples (k_chain_row<.,16> is what a block above 128 samples gets: 129 only; <.,8> the others).  After each
block the rows read back and the f32 block have to be what the oracle's stage function makes of the same rows, the same setter calls and
the tap the kernel actually read (EnginePool.preamp_out; power_amp_out with the melange power amp, whose output is the stage's input):
bit-equal smoothers, character, a2, a3, thermal coefficient and flags bit, untouched coefficients without a redesign, everything else
inside the measured bars, every f32 sample float32(oracle f64) or -- within the bar of a rounding midpoint -- its neighbour.

Worst error over its bar per form and class: profiles/post_stage_f64.md (printed here with -s)."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_binding as ob
import post_stage_cases as ps

pytestmark = pytest.mark.gpu

OS_RATES, BASE_RATES = (44100.0, 48000.0), (96000.0,)
AUTO = dict(chain_fused=-1, chain_row=-1, chain_stream=-1, post_pair=-1, preamp_wide=-1, out_direct=-1)    # every switch a form touches, at its default
LANE = dict(AUTO, chain_fused=0, preamp_wide=0, chain_stream=0)
SHORT = tuple(n for n in ps.LENGTHS if n <= 128)
# form -> (rates, switches, block lengths, streamed into a pinned host block, melange power amp)
FORMS = {
    "k_post<false>": (BASE_RATES, dict(LANE), ps.LENGTHS, False, False),
    "k_post<true>": (OS_RATES, dict(LANE, post_pair=0), ps.LENGTHS, False, False),
    "k_post<false,true>": (OS_RATES, dict(LANE, post_pair=1), ps.LENGTHS, False, False),
    "k_chain_fused<true>": (OS_RATES, dict(AUTO, chain_fused=1, chain_row=0), ps.LENGTHS, False, False),
    "k_chain_fused<false>": (BASE_RATES, dict(AUTO, chain_fused=1, chain_row=0), ps.LENGTHS, False, False),
    "k_chain_row<true,8>": (OS_RATES, dict(AUTO, chain_fused=1, chain_row=1), SHORT, False, False),
    "k_chain_row<true,16>": (OS_RATES, dict(AUTO, chain_fused=1, chain_row=1), (129,), False, False),
    "k_chain_row<false,8>": (BASE_RATES, dict(AUTO, chain_fused=1, chain_row=1), SHORT, False, False),
    "k_chain_row<false,16>": (BASE_RATES, dict(AUTO, chain_fused=1, chain_row=1), (129,), False, False),
    "k_chain_stream": (OS_RATES, dict(LANE, chain_stream=1, out_direct=1), ps.LENGTHS, True, False),
    "k_post_mpa": (OS_RATES + BASE_RATES, dict(AUTO), ps.LENGTHS, False, True),
}
PARAMS = [(form, rate) for form, spec in FORMS.items() for rate in spec[0]]

_POOLS = {}


@pytest.fixture(scope="module")
def pools(hiplib):
    """One pool per (rate, size, power-amp kind), shared by the forms: set up once (setters, chords, a warm block), then only switches,
    rows and drives change."""
    import openwurli_amd as ow

    def get(rate, n, melange_pa):
        key = (rate, n, melange_pa)
        if key not in _POOLS:
            g = ow.EnginePool(rate, n, power_amp_kind=1 if melange_pa else 0)
            g.ensure_buffer_capacity(1024)
            if melange_pa:
                g.enable_power_amp_tap()
            for k in range(n):
                ps.engine_setup(g[k], ps.RECIPES[ps.recipe_of(k, n)], k)
            g.render(768, to_host=False)
            _POOLS[key] = g
        return _POOLS[key]
    yield get
    for g in _POOLS.values():
        g.close()
    _POOLS.clear()


def _plan(lib, melange_pa, rate, n, length, pinned, switches):
    out = C.create_string_buffer(128)
    sw = ",".join(f"{k}={v}" for k, v in switches.items())
    assert lib.ow_test_block_plan(0, 1 if melange_pa else 0, int(rate < 88200.0), 1, n, length, int(pinned), sw.encode(), out, 128) == 0
    return out.value.decode()


def _block(g, rate, n, length, streamed, melange_pa, host, write_rows=True):
    """One block under test on pool g: drives, start rows, setters, render; -> per engine (recipe, rows_in, tap, rows_after, f32)."""
    osr = ps.osr_of(rate)
    rows_in = []
    for k in range(n):
        e = g[k]
        recipe = ps.RECIPES[ps.recipe_of(k, n)]
        if write_rows:
            rows = ps.start_rows(recipe, rate)
            for a, b in ps.WRITE_SPANS:
                e.write_chain_rows(a, rows[a:b])
        else:
            rows = np.zeros(ob.STAGE_ROW_COUNT)
            rows[ps.READ_SPAN[0]:ps.READ_SPAN[1]] = e.read_chain_rows(ps.READ_SPAN[0], ps.READ_SPAN[1] - ps.READ_SPAN[0])
        ps.engine_before_block(e, recipe, k, lambda: (e.read_preamp_state(False)[8], e.read_preamp_state(True)[8]))
        rows_in.append(rows)
    if streamed:
        g.render_into(host[0], host[1], length)
        out = np.ctypeslib.as_array((C.c_float * (n * host[1])).from_address(host[0])).reshape(n, host[1])[:, :length].copy()
    else:
        out = g.render(length)
    tap = g.power_amp_out(length * osr) if melange_pa else g.preamp_out(length * osr)
    res = []
    for k in range(n):
        after = np.zeros(ob.STAGE_ROW_COUNT)
        after[ps.READ_SPAN[0]:ps.READ_SPAN[1]] = g[k].read_chain_rows(ps.READ_SPAN[0], ps.READ_SPAN[1] - ps.READ_SPAN[0])
        res.append((ps.RECIPES[ps.recipe_of(k, n)], rows_in[k], tap[k], after, out[k]))
    return res


def _check(form, rate, n, length, melange_pa, results, worst, counts, only_family=None, written=True):
    fails = []
    amp = ob.STAGE_AMP_IDENTITY if melange_pa else ob.STAGE_AMP_BEHAVIORAL
    # engines that share the wavefront which runs their stage: eight behind the melange amp and in a fused / row workgroup, 32 in the
    # lane-pair layouts, 64 with lane = engine
    per_wave = 8 if melange_pa or form.startswith(("k_chain_fused", "k_chain_row")) else (32 if form in ("k_post<true>", "k_chain_stream") else 64)
    for k, (recipe, rows_in, tap, after, f32) in enumerate(results):
        if only_family and recipe["family"] != only_family:
            continue
        if rows_in[ps.FLAGS] != 0.0:                     # the stage's own bit comes in clear: the preamp half took the last block's
            rows_in = rows_in.copy(); rows_in[ps.FLAGS] = ps.u64(int(np.array([rows_in[ps.FLAGS]]).view(np.uint64)[0]) & ~1)
        ref = ps.reference(rate, recipe, rows_in, tap, length, amp)
        where = (f"{form} at {rate:g} Hz, pool of {n}, block of {length}, engine {k} (lane position {k % per_wave} of {per_wave}), "
                 f"recipe {recipe['name']} of family {recipe['family']}")
        f, ratios, near = ps.compare(rows_in, ref, after, f32, where=where)
        want = ps.expect_fired(recipe, rate)
        if written and want is not None and bool(ref[2]["fired"].any()) != want:
            f.append(f"guard recipe: fired {bool(ref[2]['fired'].any())}, the recipe says {want} [{where}]")
        fails += f
        for key, r in ratios.items():
            worst[key] = max(worst.get(key, 0.0), r)
        counts["neighbour"] += near
        counts["samples"] += length
        counts["blocks"] += 1
        counts["fired"] += int(ref[2]["fired"].any())
        counts["sweeps"] += np.bincount(ref[2]["sweeps"], minlength=9)
    return fails


def _report(form, rate, worst, counts):
    cells = " | ".join(f"{worst.get(k, 0.0):.3f}" for k in ps.BAR_KEYS)
    print(f"\n| {form} | {rate:g} | {cells} | {counts['neighbour']} / {counts['samples']} | {counts['blocks']} | {counts['fired']} | "
          f"{counts['sweeps'][1:].tolist()} |")


@pytest.mark.parametrize("form,rate", PARAMS)
def test_output_stage_equals_the_oracles(hiplib, pools, form, rate):
    rates, switches, lengths, streamed, melange_pa = FORMS[form]
    worst, counts = {}, dict(neighbour=0, samples=0, blocks=0, fired=0, sweeps=np.zeros(9, dtype=np.int64))
    fails = []
    for n in ps.POOLS:
        g = pools(rate, n, melange_pa)
        for key, v in switches.items():
            g.set_switch(key, v)
        host = g.alloc_host_block(max(ps.LENGTHS)) if streamed else None
        for length in lengths:
            plan = _plan(hiplib, melange_pa, rate, n, length, streamed, switches)
            assert plan == form or plan.endswith(" + " + form), (plan, form, n, length)
            fails += _check(form, rate, n, length, melange_pa, _block(g, rate, n, length, streamed, melange_pa, host), worst, counts)
        if streamed:
            g.free_host_block(host)
    _report(form, rate, worst, counts)
    # accepted neighbours: no more than the perturbed oracle itself shows on the corpus (a share of the samples, rounded up to a whole one)
    assert counts["neighbour"] <= math.ceil(ps.MEASURED_NEIGHBOUR_SHARE * counts["samples"]), counts
    assert not fails, f"{len(fails)} failures, the first of them:\n" + "\n".join(fails[:12])
    assert counts["blocks"] == sum(ps.POOLS) * len(lengths)


@pytest.mark.parametrize("form", list(FORMS))
def test_guard_block_hands_clean_rows_to_the_next(hiplib, pools, form):
    """Two consecutive blocks on the guard family: the first from the written rows (the guard fires where the recipe says), the second from
    whatever the first left -- the rows are read, not written, in between -- so a wrong row written back at a block's end, or a reset that
    reaches the next block late, shows in the second comparison.  After a block in which the guard fired the flags bit is set and the
    decimator and speaker states are zero; after the next one the bit is clear again."""
    rates, switches, lengths, streamed, melange_pa = FORMS[form]
    rate = rates[0]
    n = 65
    g = pools(rate, n, melange_pa)
    for key, v in switches.items():
        g.set_switch(key, v)
    host = g.alloc_host_block(max(ps.LENGTHS)) if streamed else None
    first, second = (129, 129) if lengths == (129,) else (65, 37)
    worst, counts = {}, dict(neighbour=0, samples=0, blocks=0, fired=0, sweeps=np.zeros(9, dtype=np.int64))
    one = _block(g, rate, n, first, streamed, melange_pa, host)
    fails = _check(form, rate, n, first, melange_pa, one, worst, counts, only_family="guard")
    fired_engines = []
    for k, (recipe, rows_in, tap, after, f32) in enumerate(one):
        if ps.expect_fired(recipe, rate):
            fired_engines.append(k)
            assert int(np.array([after[ps.FLAGS]]).view(np.uint64)[0]) & 1 == 1, (k, recipe["name"])
            zero = list(ps.CLASS_ROWS["half_band"]) + list(ps.CLASS_ROWS["biquad_state"])
            if recipe["name"] != "guard_hpf_1e41_loud" and not melange_pa:       # (a loud chord goes on after the reset; the melange amp's rest is not 0)
                assert not after[zero].any(), (k, recipe["name"], after[zero])
            assert g[k].diag().output_nan_resets >= 1
    two = _block(g, rate, n, second, streamed, melange_pa, host, write_rows=False)
    fails += _check(form, rate, n, second, melange_pa, two, worst, counts, only_family="guard", written=False)
    for k in fired_engines:
        assert int(np.array([two[k][3][ps.FLAGS]]).view(np.uint64)[0]) & 1 == 0, (k, two[k][0]["name"])
        assert np.isfinite(two[k][4]).all() and np.isfinite(two[k][2]).all()
    if streamed:
        g.free_host_block(host)
    _report(form + " (guard, two blocks)", rate, worst, counts)
    assert len(fired_engines) >= (2 if rate >= 88200.0 else 3) and counts["fired"] >= len(fired_engines)
    assert not fails, f"{len(fails)} failures, the first of them:\n" + "\n".join(fails[:12])
