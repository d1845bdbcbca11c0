"""Every voice kernel against the oracle's voice block, one block at a time, from any voice record (tests/voice_block_cases.py has the
corpus, the comparison and its measured bars; tests/test_oracle_voice_block_cases.py what they rest on).

Forms, selected with the settable switches: k_voice's slot pass (force_general) and steal pass (voice_steal = 0), k_voice_steady<false,0>
(voice_skew = 0), <true,0> (after a warm block that reports more than one jitter grid), <false,1> attack, <false,2> steal, <false,3>
release -- and k_voice behind the release variant where that declines a wavefront ("declined").  Per block: write the records
(ow_test_engine_write_voice_record), render, read the voice-sum tap and every record back, compare with owo_voice_block of the same start
record: integer state and constants bit-equal, pair / envelope / drift / charge / noise state / samples inside the bars, the silent bit as
active_voice_count() after the block, the transient bit as the lists the next block is packed into; blocks_* say that the form under test
rendered the block.  What they say is which LIST was launched.  The release and steal variants run over the same list as the k_voice launch
behind them and each wavefront decides through voice_steal_takes, which no status reports: that a variant took the blocks voice_block_cases.
declines() says it takes, and left the others, is not asserted here (a variant that declined everything would leave k_voice's results,
which pass too).  The recorded table shows it indirectly: the release and steal rows differ from k_voice's on the same records.

Pools of 1, 63, 65 and 130 single-voice engines (engine k plays recipe k of those the form may take), one pool of 64-, 3-, 61-, 40- and
30-voice engines, one of five wavefronts with chosen jitter grids, one of full engines that steal; 44.1 and 48 kHz.

Worst error over its bar per form and class: profiles/voice_block_f64.md (printed here with -s)."""
import numpy as np
import pytest

import oracle_binding as ob
import voice_block_cases as vc

pytestmark = pytest.mark.gpu

DEFAULT = dict(force_general=0, voice_skew=1, voice_attack=1, voice_release=1, voice_steal=1)
FORMS = {
    "k_voice": dict(DEFAULT, force_general=1),
    "steady": dict(DEFAULT, voice_skew=0),
    "skewed": dict(DEFAULT),
    "attack": dict(DEFAULT),
    "release": dict(DEFAULT),
    "declined": dict(DEFAULT),
    "k_voice_steal": dict(DEFAULT, voice_steal=0),
    "steal": dict(DEFAULT),
}
SLOT_FORMS = ("k_voice", "steady", "skewed", "attack", "release", "declined")
LIST_OF = {"k_voice": "general", "steady": "steady", "skewed": "steady", "attack": "attack", "release": "general", "declined": "general"}
CAPACITY = 2048
WARM = 32                                   # a steady block this long reports its wavefronts' jitter grids

_POOLS = {}
_STATE = {}                                 # (rate, n) -> what the API calls so far left in slot 0 of every engine: None | "held" | "released"


@pytest.fixture(scope="module")
def pools(hiplib):
    import openwurli_amd as ow

    def get(rate, n, tag="single"):
        key = (rate, n, tag)
        if key not in _POOLS:
            g = ow.EnginePool(rate, n)
            g.ensure_buffer_capacity(CAPACITY)
            _POOLS[key] = g
            _STATE[key] = [None] * n
        return _POOLS[key], _STATE[key]
    yield get
    for g in _POOLS.values():
        g.close()
    _POOLS.clear(); _STATE.clear()


def _switches(g, form):
    for k, v in FORMS[form].items():
        g.set_switch(k, v)


def _masks(g, k):
    return int(g._lib.ow_test_engine_masks(g[k]._h, 0)), int(g._lib.ow_test_engine_masks(g[k]._h, 1))


def _lists(g):
    return {k: g.get_switch("blocks_" + k) for k in ("steady", "attack", "general", "steal")}


def _blocks(n_voices):
    return (n_voices + 63) // 64


def _establish(g, state, rate, want):
    """slot 0 of every engine Held or Releasing as `want` says, nothing else sounding: through the API (a voice is freed by letting it fall
    silent), then one sample so that no op is pending"""
    _switches(g, "steady")
    for k in range(g.n):
        if state[k] is not None and _masks(g, k)[0] == 0:      # freed since: it fell silent in a block that was not under test
            state[k] = None
    kill = [k for k in range(g.n) if state[k] is not None and not (state[k] == want[k] or (state[k] == "held" and want[k] == "released"))]
    if kill:
        quiet = vc.silent_record(rate)
        for k in kill:
            g[k].write_voice_record(0, quiet)
        g.render(1, to_host=False)
        for k in kill:
            assert g[k].active_voice_count() == 0, k
            state[k] = None
    touched = False
    for k in range(g.n):
        if state[k] is None:
            g[k].note_on(60, 0.5); state[k] = "held"; touched = True
        if state[k] == "held" and want[k] == "released":
            g[k].note_off(60); state[k] = "released"; touched = True
    if touched:
        g.render(1, to_host=False)
    for k in range(g.n):
        assert _masks(g, k) == (1, 0), (k, _masks(g, k))


def _warm(rate, rec):
    """a record on the same jitter grid that stays in the steady list and does not fall silent: what the warm block renders"""
    r = vc.bank(rate)[(60, 0.7)]["steady"].copy()
    r[vc.SAMPLE] = rec[vc.SAMPLE]
    return r


def _valid(rate, form, L):
    return [r for r in vc.recipes(rate) if L in vc.lengths_of(r) and form in vc.forms_of(r["setup"], vc.record(r, L))]


class Table:
    def __init__(self):
        self.worst = {}
        self.blocks = self.voices = 0

    def add(self, ratios):
        for k, v in ratios.items():
            self.worst[k] = max(self.worst.get(k, 0.0), v)

    def row(self, *head):
        cells = " | ".join(f"{self.worst.get(k, 0.0):.3f}" for k in vc.CLASSES)
        print("\n| " + " | ".join(str(h) for h in head) + f" | {cells} | {self.blocks} | {self.voices} |")


def _slot_block(g, state, rate, form, L, offset, table):
    """one block of a pool of single-voice engines under `form`: -> failures"""
    n = g.n
    valid = _valid(rate, form, L)
    assert valid, (form, L)
    mine = [valid[(k + offset) % len(valid)] for k in range(n)]
    _establish(g, state, rate, [r["setup"] for r in mine])
    recs = [vc.record(r, L) for r in mine]
    _switches(g, form)
    if form == "skewed":
        for k in range(n):
            g[k].write_voice_record(0, _warm(rate, recs[k]))
        g.render(WARM, to_host=False)
        if g.get_switch("voice_skew_active") != 1:
            return None                                      # one jitter grid per wavefront: nothing to skew (asserted by the caller)
    for k in range(n):
        g[k].write_voice_record(0, recs[k])
    g.render(L, to_host=False)
    lists = _lists(g)
    assert lists == {**dict(steady=0, attack=0, general=0, steal=0), LIST_OF[form]: _blocks(n)}, (form, L, lists)
    tap = g.voice_sum(L)
    fails = []
    expect = dict(steady=0, attack=0, general=0)
    for k in range(n):
        where = f"{form} at {rate:g} Hz, pool of {n}, block of {L}, engine {k} (lane {k % 64}), recipe {mine[k]['name']} of family {mine[k]['family']}"
        ref = ob.voice_block(recs[k], False, L)
        got = g[k].read_voice_record(0)
        f, ratios = vc.compare(recs[k], ref, got, tap[k], where=where, carried_amp=form == "release")
        fails += f
        table.add(ratios)
        if (g[k].active_voice_count() == 0) != ref[2]["silent"]:
            fails.append(f"silent bit: {g[k].active_voice_count()} voices sound after the block, the reference says silent = {ref[2]['silent']} [{where}]")
        if ref[2]["silent"]:
            state[k] = None
        else:
            expect["steady" if not ref[2]["transient"] else ("general" if state[k] == "released" else "attack")] += 1
    table.blocks += 1; table.voices += n
    # the transient bit: which lists the next block is packed into
    if form != "k_voice" and sum(expect.values()) > 0:           # (a block without voices packs no lists)
        g.render(1, to_host=False)
        lists = _lists(g)
        want = {k: _blocks(v) for k, v in expect.items()}
        if {k: lists[k] for k in want} != want:
            fails.append(f"transient bits: the next block's lists are {lists}, the reference's bits give {want} [{form} at {rate:g} Hz, pool of {n}, block of {L}]")
    return fails


# (the skewed variant needs two jitter grids in one wavefront: a pool of one engine never has them)
PARAMS = [(form, rate, n) for form in SLOT_FORMS for rate in vc.RATES for n in vc.POOLS if not (form == "skewed" and n == 1)]


@pytest.mark.parametrize("form,rate,n", PARAMS)
def test_slot_voice_block_equals_the_oracles(hiplib, pools, form, rate, n):
    g, state = pools(rate, n)
    table = Table()
    fails = []
    skipped = 0
    lengths = vc.LENGTHS + ((vc.LONG,) if n == 65 and form in ("k_voice", "steady", "skewed") else ())
    for i, L in enumerate(lengths):
        f = _slot_block(g, state, rate, form, L, 7 * i, table)
        if f is None:
            skipped += 1
        else:
            fails += f
    table.row(form, f"{rate:g}", n)
    assert not fails, f"{len(fails)} failures, the first of them:\n" + "\n".join(fails[:12])
    assert skipped == 0, (skipped, form, n)


# ---- wavefronts with chosen jitter grids ----------------------------------------------------------------------------------------------------
GRIDS = (tuple(range(16)), (0, 15), (0, 8), (3, 4, 5), (7,))


@pytest.mark.parametrize("rate", vc.RATES)
def test_skewed_clocks_on_chosen_grids(hiplib, pools, rate):
    """Five wavefronts of 64 single-voice engines whose sample counters leave all sixteen residues mod 16, {0, 15}, {0, 8}, {3, 4, 5} and the
    single residue 7 (no delay: the plain loop inside the skewed kernel)."""
    g, state = pools(rate, 64 * len(GRIDS), "grids")
    base = vc.bank(rate)[(60, 0.7)]["steady"]
    table = Table()
    fails = []
    _establish(g, state, rate, ["held"] * g.n)
    for L in (32, 33, 47, 65, 129):
        # the counter's residue is the grid; a renormalisation point on the block's first sample (residue 0) or 16 / 32 samples in, less the residue
        recs = [vc.at_sample(base, 1024 * (4 + k % 5) - 16 * (k % 3) + GRIDS[k // 64][k % len(GRIDS[k // 64])]) for k in range(g.n)]
        _switches(g, "skewed")
        for rounds in range(2):
            for k in range(g.n):
                g[k].write_voice_record(0, recs[k])
            if rounds == 0:
                g.render(WARM, to_host=False)
                assert g.get_switch("voice_skew_active") == 1
        g.render(L, to_host=False)
        assert _lists(g) == dict(steady=len(GRIDS), attack=0, general=0, steal=0)
        tap = g.voice_sum(L)
        for k in range(g.n):
            ref = ob.voice_block(recs[k], False, L)
            f, ratios = vc.compare(recs[k], ref, g[k].read_voice_record(0), tap[k],
                                   where=f"skewed at {rate:g} Hz, grids {GRIDS[k // 64]}, block of {L}, engine {k} (lane {k % 64})")
            fails += f
            table.add(ratios)
        table.blocks += 1; table.voices += g.n
    table.row("skewed (chosen grids)", f"{rate:g}", g.n)
    assert not fails, f"{len(fails)} failures, the first of them:\n" + "\n".join(fails[:12])


# ---- engines with many voices -----------------------------------------------------------------------------------------------------------------
VOICES = (64, 3, 61, 40, 30)                # the two-halves reduction; two engines sharing a wavefront; two that cannot


@pytest.mark.parametrize("form", ("k_voice", "steady", "skewed"))
@pytest.mark.parametrize("rate", vc.RATES)
def test_many_voice_engines(hiplib, pools, form, rate):
    """The voice-sum tap against the slot-order sum of the reference voices, the samples' bar taken once per voice; every record as in the
    single-voice pools."""
    g, state = pools(rate, len(VOICES), "many")
    if state[0] is None:
        for k, nv in enumerate(VOICES):
            for s in range(nv):
                g[k].note_on(33 + s, 0.5)
            state[k] = "held"
        g.render(1, to_host=False)
    for k, nv in enumerate(VOICES):
        assert _masks(g, k) == ((1 << nv) - 1, 0), k
    table = Table()
    fails = []
    for L in (1, 24, 33, 65, 129):
        valid = [r for r in _valid(rate, "steady", L) if r["setup"] == "held" and not ob.voice_block(vc.record(r, L), False, max(L, WARM))[2]["silent"]]
        recs = {(k, s): vc.record(valid[(5 * k + s) % len(valid)], L) for k, nv in enumerate(VOICES) for s in range(nv)}
        _switches(g, form)
        for rounds in range(2 if form == "skewed" else 1):
            for (k, s), r in recs.items():
                g[k].write_voice_record(s, r)
            if form == "skewed" and rounds == 0:
                g.render(WARM, to_host=False)
                assert g.get_switch("voice_skew_active") == 1
        g.render(L, to_host=False)
        assert _lists(g) == {**dict(steady=0, attack=0, general=0, steal=0), LIST_OF[form]: 4}, _lists(g)
        tap = g.voice_sum(L)
        for k, nv in enumerate(VOICES):
            acc, room = np.zeros(L), 0.0
            for s in range(nv):
                where = f"{form} at {rate:g} Hz, engine of {nv} voices, block of {L}, slot {s}"
                ref = ob.voice_block(recs[(k, s)], False, L)
                assert not ref[2]["silent"], where
                f, ratios = vc.compare(recs[(k, s)], ref, g[k].read_voice_record(s), None, where=where)
                fails += f
                table.add(ratios)
                acc = acc + ref[1]
                room += vc.BARS["samples"] * vc.samples_scale(recs[(k, s)], ref[0], ref[1])
            d = np.abs(tap[k] - acc)
            table.add({"samples": float(d.max() / room)})
            if d.max() > room:
                fails.append(f"samples: sample {int(np.argmax(d))} of the sum is {float(d.max()):.3e} from the slot-order sum of the reference voices, "
                             f"bar {room:.3e} [{form} at {rate:g} Hz, engine of {nv} voices, block of {L}]")
            assert g[k].active_voice_count() == nv
        table.blocks += 1; table.voices += sum(VOICES)
    table.row(form + " (many voices)", f"{rate:g}", len(VOICES))
    assert not fails, f"{len(fails)} failures, the first of them:\n" + "\n".join(fails[:12])


# ---- steal voices -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("k_voice_steal", "steal"))
@pytest.mark.parametrize("rate", vc.RATES)
def test_steal_voice_block_equals_the_oracles(hiplib, pools, form, rate):
    """Full engines, one per steal recipe.  Before every block a note-on steals a slot (the API's way to a steal voice), one sample applies
    it, the 64 slot voices are written with post_pickup_gain 0 (each adds an exact zero to the sum) and the steal voice with the recipe's
    record.  A steal record is compared while the counter it leaves is > 0: the kernels drop the voice where the reference steps on."""
    recipes = vc.steal_recipes(rate)
    g, state = pools(rate, len(recipes), "steal")
    mute = vc.bank(rate)[(60, 0.7)]["steady"].copy()
    mute[vc.GAIN] = 0.0; mute[vc.DECAY:vc.DECAY + 7] = 1.0          # never silent, never heard
    if state[0] is None:
        for k in range(g.n):
            for s in range(64):
                g[k].note_on(33 + s, 0.5)
            state[k] = "held"
        g.render(1, to_host=False)
        for k in range(g.n):
            for s in range(64):
                g[k].write_voice_record(s, mute)
    table = Table()
    fails = []
    compared = 0
    for i, L in enumerate(vc.LENGTHS):
        _switches(g, "steady")
        g.render(256, to_host=False)                                  # earlier crossfades run out: none is longer than 240 samples
        assert not any(_masks(g, k)[1] for k in range(g.n))
        slots = []
        for k in range(g.n):
            g[k].note_on(40 + i, 0.5)
        g.render(1, to_host=False)
        mine = [recipes[(k + i) % len(recipes)] for k in range(g.n)]
        recs = [vc.record(r, L) for r in mine]
        for k in range(g.n):
            main, steal = _masks(g, k)
            assert main == (1 << 64) - 1 and bin(steal).count("1") == 1, (k, hex(main), hex(steal))
            slots.append(steal.bit_length() - 1)
            g[k].write_voice_record(slots[k], mute)
            g[k].write_voice_record(slots[k], recs[k], steal=True)
        _switches(g, form)
        g.render(L, to_host=False)
        lists = _lists(g)
        assert lists["steal"] == g.n and lists["steady"] == g.n and lists["attack"] == 0 and lists["general"] == 0, lists
        tap = g.voice_sum(L)
        for k in range(g.n):
            where = (f"{form} at {rate:g} Hz, block of {L}, engine {k}, slot {slots[k]}, recipe {mine[k]['name']}"
                     f"{' (the variant declines: k_voice)' if form == 'steal' and vc.declines(recs[k]) else ''}")
            ref = ob.voice_block(recs[k], True, L)
            f, ratios = vc.compare(recs[k], ref, g[k].read_voice_record(slots[k], steal=True), tap[k], steal=True, where=where,
                                   carried_amp=form == "steal" and not vc.declines(recs[k]))
            fails += f
            table.add(ratios)
            compared += vc.steal_record_compared(ref[0])
            if vc.lo32(recs[k], vc.STEAL) < L and tap[k][vc.lo32(recs[k], vc.STEAL):].any():
                fails.append(f"the sum row is not zero behind the crossfade's end [{where}]")
        table.blocks += 1; table.voices += g.n
    table.row(form, f"{rate:g}", g.n)
    assert not fails, f"{len(fails)} failures, the first of them:\n" + "\n".join(fails[:12])
    assert compared >= 0.4 * table.voices, (compared, table.voices)
