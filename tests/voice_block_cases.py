"""A voice one block at a time, from any voice record: corpus and comparison behind tests/test_oracle_voice_block_cases.py (CPU) and
tests/test_gpu_voice_block.py (k_voice, k_voice_steady and its skewed, attack, steal and release variants).

A voice block is a pure function (record, L) -> (record after, L samples, status bits).  The oracle evaluates it (oracle_binding.voice_block:
the unchanged Voice::render on a Voice built from the record); a kernel has to reproduce it from the same record, written through
ow_test_engine_write_voice_record, and is read back through ow_test_engine_read_voice_record and the voice-sum tap.

A RECIPE is (set-up calls through the API, the record to write, which block lengths it is for); which kernel form may take it follows from
the set-up and the record's own state (forms_of).  Start records are harvested on the CPU from oracle engines (notes 33, 60, 84 and 96,
velocities 0, 0.0005, 0.3, 0.7 and 1) and then edited, so every form and both sides start from the same bits.  Velocity 0 gives seven modes
without amplitude; 0.0005 is the `square` branch of the onset shape (exponent >= 1.999) with amplitudes that show it, 1.0 the cosine
(<= 1.001), 0.3 and 0.7 the pow between.  Note 84 is there for the damper: 96 has none (>= 92), and 84 has the short 8 ms ramp.

Records stay inside what the host guarantees, because the kernels rely on it:
  * damper rates rise with the mode (mode 6 decides whether exp_neg_poly's 1/8 limit holds for all seven);
  * 0 <= envelope <= 1 and 0 < decay <= 1 (the folded kernel's radius never grows);
  * counters are consistent with the flags: ramp-done only with the damper bit, a fade-in only while noise is left, a steal counter
    no larger than its length; pairs have radius 1 to 1e-9.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import oracle_binding as ob
import voice_path_numpy as vp

# VF_* of openwurli_amd/csrc/ow_types.h (OW_TEST_VF_* of include/openwurli_hip_test.h, guarded there by static_asserts)
S, C, ENV, DRIFT, COS_INC, SIN_INC, PHASE_INC, AMP, DECAY, DRATE, DMULT = 0, 7, 14, 21, 28, 35, 42, 49, 56, 63, 70
ONSET_INC, ONSET_EXP, DRAMP, DCOUNT, Q, DS, GAIN, NAMP, NB0, NS1, NS2 = 77, 78, 79, 80, 81, 82, 83, 84, 85, 90, 91
SAMPLE, ONSET_N, RNG, NCNT, FLAGS, STEAL, BETA, JREV, JDIFF, NDECAY, VSR, COUNT = 92, 93, 94, 95, 96, 97, 98, 99, 100, 101, 102, 103
assert COUNT == ob.VOICE_RECORD_FIELDS

RATES = (44100.0, 48000.0)
LENGTHS = (1, 2, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 64, 65, 129)     # the 16-sample jitter grid, the 24- and 32-sample chunks, the skew ring
LONG = 1030                                                                       # two renormalisation points in one block: counter family only
POOLS = (1, 63, 65, 130)                  # packed wavefronts of single-voice engines: one lane, a partly filled one, several segments
NOTES, VELS = (33, 60, 84, 96), (0.0, 0.0005, 0.3, 0.7, 1.0)
FORMS = ("k_voice", "steady", "skewed", "attack", "release", "declined")          # of a slot voice; steal voices: "k_voice_steal", "steal"


def u64(x):
    return float(np.array([int(x) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)[0])


def bits(rec, f):
    return int(np.asarray(rec, dtype=np.float64)[f:f + 1].view(np.uint64)[0])


def lo32(rec, f):
    return bits(rec, f) & 0xFFFFFFFF


def hi32(rec, f):
    return bits(rec, f) >> 32


# ---- harvest ------------------------------------------------------------------------------------------------------------------------------
_BANK = {}


def bank(rate):
    """{(note, velocity): dict(struck, burst, steady, released)}: the voice's record right after note_on, 200 samples later (noise running,
    filter states non-zero), 3000 samples later (past every onset ramp and burst) and that record with the damper fields of a note_off."""
    if rate not in _BANK:
        b = {}
        for note in NOTES:
            for vel in VELS:
                # (the blocks in between through the oracle's block function: an engine frees a voice without amplitude after its first block)
                e = ob.OracleEngine(rate)
                e.note_on(note, vel)
                d = dict(struck=e.voice_record(0))
                e.note_off(note)
                off = e.voice_record(0)
                e.close()
                d["burst"] = ob.voice_block(d["struck"], False, 200)[0]
                d["steady"] = ob.voice_block(d["burst"], False, 2800)[0]
                d["released"] = d["steady"].copy()
                for f in tuple(range(DRATE, DMULT + 7)) + (DRAMP, DCOUNT, FLAGS):
                    d["released"][f] = off[f]
                b[(note, vel)] = d
        _BANK[rate] = b
    return _BANK[rate]


def silent_record(rate):
    """a record that Voice::is_silent after any block: how a test frees a slot"""
    r = bank(rate)[(60, 0.7)]["steady"].copy()
    r[ENV:ENV + 7] = 0.0
    return r


def fade_len(rate):
    return int(rate * 0.005)                       # engine.rs:318


# ---- edits --------------------------------------------------------------------------------------------------------------------------------
def at_sample(rec, n, radius=True):
    """the record with its sample counter at n (mod 2^64) and its pairs at radius 1 +- 1e-9 by turns: a renormalisation that is skipped,
    doubled or late then shows at 1e-9"""
    r = rec.copy()
    r[SAMPLE] = u64(n)
    if radius:
        for m in range(7):
            k = 1.0 + (1e-9 if m % 2 == 0 else -1e-9)
            r[S + m] *= k; r[C + m] *= k
    return r


def with_noise(rec, rem, fade, src=None):
    r = rec.copy()
    r[NCNT] = u64(rem | (fade << 32))
    if src is not None:
        r[NS1], r[NS2], r[NAMP] = src[NS1], src[NS2], src[NAMP]
    return r


def with_damper(rec, dcount, done):
    r = rec.copy()
    r[DCOUNT] = float(dcount)
    r[FLAGS] = u64((bits(r, FLAGS) & ~3) | 1 | (2 if done else 0))
    return r


def with_steal(rec, left, length):
    r = rec.copy()
    r[STEAL] = u64(left | (length << 32))
    return r


def state_of(rec):
    """which phase the record is in: what the kernels' own test says (VoiceRegs::in_transient)"""
    if bits(rec, FLAGS) & 1:
        return "damp"
    return "attack" if bits(rec, SAMPLE) < bits(rec, ONSET_N) or lo32(rec, NCNT) > 0 else "steady"


def declines(rec):
    """voice_steal_takes says no: the release / steal variant leaves the block to k_voice"""
    return bits(rec, SAMPLE) < bits(rec, ONSET_N) or lo32(rec, NCNT) > 0 or (bool(bits(rec, FLAGS) & 1) and not rec[DRATE + 6] <= 0.125)


def forms_of(setup, rec):
    """the kernel forms that may render this slot voice: k_voice always (force_general); otherwise what the host's lists and the kernels' own
    entry tests make of the slot's state and the record"""
    st = state_of(rec)
    if st == "steady":
        return ("k_voice", "steady", "skewed")
    if setup == "held":
        # a held slot whose record damps is not something the API produces: the host would send it to the attack variant, which refuses it
        return ("k_voice", "attack") if st == "attack" else ()
    return ("k_voice", "declined") if declines(rec) else ("k_voice", "release")


# ---- recipes ------------------------------------------------------------------------------------------------------------------------------
def _r(name, family, setup, make, lengths=None):
    return dict(name=name, family=family, setup=setup, make=make, lengths=lengths)


_RECIPES = {}


def recipes(rate):
    """The slot-voice recipes at `rate`: [dict(name, family, setup 'held' | 'released', make(L) -> record, lengths None | tuple)]."""
    if rate in _RECIPES:
        return _RECIPES[rate]
    B = bank(rate)
    out = []
    mid, top, low, dmp = B[(60, 0.7)], B[(96, 1.0)], B[(33, 0.3)], B[(84, 0.7)]

    # -- counter: every residue of sample & 15, the renormalisation point on the first, middle and last sample, counters at 1024 n and
    # past 2^32 (the kernels rebuild a 64-bit counter from a 32-bit countdown)
    for r in range(16):
        out.append(_r(f"residue_{r}", "counter", "held", lambda L, r=r: at_sample(mid["steady"], 2048 - r)))
    for n in (1023, 1024, 1025, 2047, 2 ** 32 - 3, 2 ** 32 + 1024 - 2, 2 ** 32 - 16, 2 ** 40 + 1024 - 1):
        out.append(_r(f"sample_{n}", "counter", "held", lambda L, n=n: at_sample(low["steady"], n)))
    out.append(_r("renorm_first", "counter", "held", lambda L: at_sample(mid["steady"], 3072)))
    out.append(_r("renorm_middle", "counter", "held", lambda L: at_sample(mid["steady"], 3072 - L // 2)))
    out.append(_r("renorm_last", "counter", "held", lambda L: at_sample(mid["steady"], 3072 - (L - 1))))
    out.append(_r("renorm_next", "counter", "held", lambda L: at_sample(mid["steady"], 3072 - L)))            # the block ends one sample short of it
    out.append(_r("renorm_twice", "counter", "held", lambda L: at_sample(mid["steady"], 1020), lengths=(LONG,)))
    out.append(_r("renorm_twice_2e32", "counter", "held", lambda L: at_sample(low["steady"], 2 ** 32 - 3), lengths=(LONG,)))      # 2^32 and 2^32 + 1024: samples 3 and 1027
    # sample 0 is not a renormalisation point (reed.rs:294 `&& self.sample > 0`); small counters are inside the onset ramp and the burst
    for n in (0, 1, 15, 16):
        def small(L, n=n):
            r = at_sample(mid["struck"], n)
            nrem = lo32(mid["struck"], NCNT)
            return with_noise(r, nrem - n, max(16 - n, 0))
        out.append(_r(f"sample_{n}", "counter", "held", small))

    # -- envelope: upper modes at and below the 1e-290 branch of the folded kernel, the fastest and the slowest decay, no amplitude, and
    # the -80 dB test as a decision of the case
    tiny = (1e-280, 2e-290, 5e-291, 1e-300, 1e-310, 0.0)
    fastest = min(float(B[k]["steady"][DECAY + 6]) for k in B)

    def tiny_env(L, decay=None, base=mid):
        r = at_sample(base["steady"], 5000, radius=False)
        r[ENV + 1:ENV + 7] = tiny
        if decay is not None:
            r[DECAY + 1:DECAY + 7] = decay
        return r
    out.append(_r("tiny_envelopes", "envelope", "held", tiny_env))
    out.append(_r("tiny_envelopes_decay_1", "envelope", "held", lambda L: tiny_env(L, 1.0)))
    out.append(_r("tiny_envelopes_fastest", "envelope", "held", lambda L: tiny_env(L, fastest)))
    out.append(_r("tiny_envelopes_top_note", "envelope", "held", lambda L: tiny_env(L, None, top)))
    out.append(_r("tiny_envelopes_renorm", "envelope", "held", lambda L: at_sample(tiny_env(L), 4096 - L // 2)))
    out.append(_r("no_amplitude", "envelope", "held", lambda L: at_sample(B[(60, 0.0)]["steady"], 2048 - L // 2)))
    out.append(_r("no_amplitude_tiny", "envelope", "held", lambda L: tiny_env(L, None, B[(33, 0.0)])))

    def around_80_db(L, loud_mode, base=mid):
        r = base["steady"].copy()
        r[DECAY:DECAY + 7] = 1.0                                   # the envelope the block leaves is the one written
        for m in range(7):
            a = abs(float(r[AMP + m]))
            r[ENV + m] = min(1.0, 1e-4 * (1.03 if m == loud_mode else 0.97) / a) if a > 0.0 else 1.0
        return r
    out.append(_r("minus_80_db_all_below", "envelope", "held", lambda L: around_80_db(L, -1)))
    out.append(_r("minus_80_db_mode_0_above", "envelope", "held", lambda L: around_80_db(L, 0)))
    out.append(_r("minus_80_db_all_below_low", "envelope", "held", lambda L: around_80_db(L, -1, low)))
    out.append(_r("minus_80_db_mode_0_above_low", "envelope", "held", lambda L: around_80_db(L, 0, low)))
    # ... and every other mode alone above it, where its amplitude lets an envelope of at most 1 get there
    for tag, base in (("", mid), ("_low", low), ("_ff", B[(60, 1.0)]), ("_low_ff", B[(33, 1.0)])):
        for m in range(1, 7):
            if 1.03e-4 / max(abs(float(base["steady"][AMP + m])), 1e-300) <= 1.0 and not any(x["name"].startswith(f"minus_80_db_mode_{m}_") for x in out):
                out.append(_r(f"minus_80_db_mode_{m}_above{tag}", "envelope", "held", lambda L, m=m, base=base: around_80_db(L, m, base)))

    # -- pickup: the input on either side of the 0.94 knee, on both signs, and a charge off its rest
    def pickup(L, peak, sign, q, base=top):
        r = at_sample(base["steady"], 4100, radius=False)
        if sign < 0:
            r[S:S + 7] = -r[S:S + 7]; r[C:C + 7] = -r[C:C + 7]
        r[Q] = q
        x = reed_sum(r, L)
        r[DS] = peak / float(np.max(np.abs(x)))
        return r
    for i, peak in enumerate((0.5, 0.935, 0.945, 0.975, 1.2)):
        for j, sign in enumerate((1, -1)):
            q = (1.0, 0.3, 3.0)[(2 * i + j) % 3]                      # each of the three on each side of the knee
            out.append(_r(f"pickup_{peak}_{'pos' if sign > 0 else 'neg'}", "pickup", "held", lambda L, p=peak, s=sign, q=q: pickup(L, p, s, q)))
    out.append(_r("pickup_0.945_low_note", "pickup", "held", lambda L: pickup(L, 0.945, 1, 1.0, low)))

    # -- attack: an onset ramp or a noise burst that ends on, before and after every chunk edge; the three shapes of the onset gain
    lefts = (1, 2, 23, 24, 25, 31, 32, 33, "L-1", "L", "L+1")
    fades = (16, 9, 1, 0)
    keys = [(60, 1.0), (60, 0.0005), (60, 0.3), (33, 0.7), (60, 0.0)]          # cosine, square, pow, pow on the longest ramp, no amplitude
    for i, left in enumerate(lefts):
        def attack(L, i=i, left=left):
            b = B[keys[i % len(keys)]]
            res = lambda v: {"L-1": max(L - 1, 1), "L": L, "L+1": L + 1}.get(v, v)
            on, nz = res(left), res(lefts[(i + 4) % len(lefts)])
            r = at_sample(b["struck"], bits(b["struck"], ONSET_N) - on, radius=False)
            return with_noise(r, nz, min(fades[i % 4], nz), b["burst"])
        out.append(_r(f"onset_left_{left}", "attack", "held", attack))
    for i, left in enumerate(lefts):
        def burst(L, i=i, left=left):
            b = B[keys[(i + 2) % len(keys)]]
            res = lambda v: {"L-1": max(L - 1, 1), "L": L, "L+1": L + 1}.get(v, v)
            r = at_sample(b["struck"], bits(b["struck"], ONSET_N) - res(lefts[(i + 7) % len(lefts)]), radius=False)
            return with_noise(r, res(left), min(fades[(i + 1) % 4], res(left)), b["burst"])
        out.append(_r(f"noise_left_{left}", "attack", "held", burst))
    out.append(_r("ramp_over_noise_running", "attack", "held", lambda L: with_noise(at_sample(mid["steady"], 4000 + L, radius=False), 40, 0, mid["burst"])))
    out.append(_r("noise_over_ramp_running", "attack", "held",
                  lambda L: with_noise(at_sample(low["struck"], bits(low["struck"], ONSET_N) - 40, radius=False), 0, 0)))
    out.append(_r("struck", "attack", "held", lambda L: mid["struck"].copy()))
    out.append(_r("struck_top_note", "attack", "held", lambda L: top["struck"].copy()))

    # -- damper (a released slot): the ramp's end on the first sample, on either side of a 24-sample chunk edge and on the last sample,
    # ramp lengths with and without a fraction, the rate at exp_neg_poly's limit, past it, no damper at all, the ten-second timeout
    for note in (33, 60, 84):
        b = B[(note, 0.7)]
        ramp = float(b["released"][DRAMP])
        for where in (0, 23, 24, "L-1", "beyond"):
            def damp(L, b=b, ramp=ramp, where=where):
                j = {"L-1": L - 1, "beyond": L + 5}.get(where, where)
                return with_damper(b["released"], int(np.floor(ramp)) - j, False)      # t > ramp first holds on sample j of the block
            out.append(_r(f"damper_{note}_ends_at_{where}", "damper", "released", damp))
        out.append(_r(f"damper_{note}_just_released", "damper", "released", lambda L, b=b: b["released"].copy()))
        out.append(_r(f"damper_{note}_ramp_done", "damper", "released", lambda L, b=b, ramp=ramp: with_damper(b["released"], int(ramp) + 100, True)))

    def rate6(L, rate_6, base=dmp):
        r = with_damper(base["released"], int(np.floor(float(base["released"][DRAMP]))) - (L - 1), False)    # t / ramp near 1 in this block
        r[DRATE + 6] = rate_6; r[DMULT + 6] = float(np.exp(-rate_6))
        return r
    out.append(_r("damper_rate_0.125", "damper", "released", lambda L: rate6(L, 0.125)))
    out.append(_r("damper_rate_0.13", "damper", "released", lambda L: rate6(L, 0.13)))
    out.append(_r("released_in_burst", "damper", "released",
                  lambda L: with_noise(with_damper(mid["released"], 10, False), 30, 0, mid["burst"])))
    out.append(_r("released_no_damper", "damper", "released", lambda L: at_sample(top["released"], 6000, radius=False)))
    # modes without amplitude under the damper: the damper variants carry amplitude x envelope, which is 0 there, and have to step the
    # envelope on its own (a whole voice struck at velocity 0 -- it falls silent with the block --, and one mode of a sounding voice)
    for tag, zb in (("", B[(60, 0.0)]), ("_84", B[(84, 0.0)])):
        zramp = int(np.floor(float(zb["released"][DRAMP])))
        out.append(_r(f"released_no_amplitude_in_ramp{tag}", "damper", "released", lambda L, zb=zb: with_damper(zb["released"], 10, False)))
        out.append(_r(f"released_no_amplitude_ramp_ending{tag}", "damper", "released", lambda L, zb=zb, zramp=zramp: with_damper(zb["released"], zramp - L // 2, False)))
        out.append(_r(f"released_no_amplitude_ramp_done{tag}", "damper", "released", lambda L, zb=zb, zramp=zramp: with_damper(zb["released"], zramp + 50, True)))

    def one_mode_zero(L, m, dcount, done):
        r = with_damper(mid["released"], dcount, done)
        r[AMP + m] = 0.0
        return r
    mramp = int(np.floor(float(mid["released"][DRAMP])))
    out.append(_r("released_mode_1_no_amplitude_in_ramp", "damper", "released", lambda L: one_mode_zero(L, 1, 40, False)))
    out.append(_r("released_mode_2_no_amplitude_ramp_ending", "damper", "released", lambda L: one_mode_zero(L, 2, mramp - L // 2, False)))
    out.append(_r("released_mode_1_no_amplitude_ramp_done", "damper", "released", lambda L: one_mode_zero(L, 1, mramp + 7, True)))
    for over in (0, 1):
        out.append(_r(f"ten_seconds_{'over' if over else 'not_yet'}", "damper", "released",
                      lambda L, over=over: with_damper(mid["released"], int(10.0 * rate) - L + over, True)))
    for r_ in out:
        r_["rate"] = rate
    _RECIPES[rate] = out
    return out


def steal_recipes(rate):
    """Steal-voice recipes: a damping (or still sounding, or freshly struck) voice with 1 .. L + 1 samples of its crossfade left."""
    B = bank(rate)
    n = fade_len(rate)
    out = []
    lefts = (1, 23, 24, 25, "L", "L+1", n)
    bases = [("damping", lambda L: with_damper(B[(60, 0.7)]["released"], 300, False)),
             ("ramp_ending", lambda L: with_damper(B[(84, 1.0)]["released"], int(float(B[(84, 1.0)]["released"][DRAMP])) - L // 2, False)),
             ("ramp_done", lambda L: with_damper(B[(33, 0.3)]["released"], 5000, True)),
             ("held", lambda L: at_sample(B[(96, 1.0)]["steady"], 2048 - L // 3))]
    for i, left in enumerate(lefts):
        for name, base in (bases[i % 4], bases[(i + 1) % 4]):
            def make(L, left=left, base=base):
                return with_steal(base(L), {"L": L, "L+1": L + 1}.get(left, left), n)
            out.append(_r(f"steal_{name}_left_{left}", "steal", "steal", make))
    zb, zm = B[(60, 0.0)]["released"], B[(60, 0.7)]["released"].copy()
    zm[AMP + 1] = 0.0; zm[AMP + 4] = 0.0
    zr = int(np.floor(float(zb[DRAMP])))
    out.append(_r("steal_no_amplitude_in_ramp", "steal", "steal", lambda L: with_steal(with_damper(zb, 10, False), n, n)))
    out.append(_r("steal_no_amplitude_ramp_ending", "steal", "steal", lambda L: with_steal(with_damper(zb, zr - L // 2, False), L + 1, n)))
    out.append(_r("steal_no_amplitude_ramp_done", "steal", "steal", lambda L: with_steal(with_damper(zb, zr + 50, True), n, n)))
    out.append(_r("steal_two_modes_no_amplitude_ramp_ending", "steal", "steal", lambda L: with_steal(with_damper(zm, zr - L // 2, False), n, n)))
    out.append(_r("steal_in_burst", "steal", "steal", lambda L: with_steal(with_noise(B[(60, 1.0)]["burst"], 50, 0), 100, n)))      # the variant declines
    out.append(_r("steal_rate_0.13", "steal", "steal", lambda L: with_steal(_rate6(B[(84, 0.7)]["released"], 0.13), 64, n)))        # ... here too
    for r_ in out:
        r_["rate"] = rate
    return out


def _rate6(rec, rate_6):
    r = with_damper(rec, 20, False)
    r[DRATE + 6] = rate_6; r[DMULT + 6] = float(np.exp(-rate_6))
    return r


def lengths_of(recipe):
    return recipe["lengths"] or LENGTHS


def reed_sum(rec, L):
    """the pickup's input before the displacement scale over the next L samples of the record (the numpy restatement's tap)"""
    return vp.voice_block(rec, False, L)[2]["x"]


_RECORDS = {}


def record(recipe, L):
    """the recipe's start record for a block of L samples (made once)"""
    key = (recipe["rate"], recipe["name"], L)
    if key not in _RECORDS:
        _RECORDS[key] = recipe["make"](L)
    return _RECORDS[key].copy()


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
# Bit-equal on both sides: integer state (sample counter, both RNG words, noise and fade counters, flags, the damper's count -- an integer
# carried in a double --, the steal counter) and every field a block only reads.
EXACT = (SAMPLE, RNG, NCNT, FLAGS, DCOUNT, STEAL)
CONSTANT = tuple(range(COS_INC, DMULT + 7)) + (ONSET_INC, ONSET_EXP, DRAMP, DS, GAIN) + tuple(range(NB0, NB0 + 5)) + (ONSET_N, BETA, JREV, JDIFF, NDECAY, VSR)
# The rest by class, |got - ref| relative to the class's scale in the case: the largest magnitude among the class's fields before and after
# the block -- per mode for the pair, the envelope and the drift (the modes' envelopes lie orders of magnitude apart, and the point of the
# test is a wrong upper mode).  A sample is ((q (1 - y) - 1) 1.8375) gain: a difference of two numbers of the size of q, so its rounding noise
# is that of 1.8375 gain q whatever is left after the cancellation; the samples' scale is the larger of the block's peak and that (with
# the block's peak alone a voice without amplitude has no scale at all).  Where an envelope's scale is subnormal the measure is steps of
# the smallest subnormal, as in post_stage_cases.py.
CLASSES = ("pair", "envelope", "drift", "q", "noise", "samples", "subnormal_steps", "subnormal_steps_carried")
SUBNORMAL_SCALE = 1e-290                       # the kernels' `env > 1e-290`: below it a pair is not compared
MIN_NORMAL = 2.2250738585072014e-308
SUBNORMAL_STEP = 4.9406564584124654e-324
FLOOR_RULE = ob.FLOOR_RULE
# MEASURED[class]: the larger of (a) the f64 oracle's error against the long-double run of the same block and (b) the oracle's own movement
# when the record's continuous fields (pair, envelope, drift, charge, noise state) are moved to a neighbouring double, over the CPU corpus;
# BARS = 2.5 x that.  tests/test_oracle_voice_block_cases.py::test_bars_are_measured asserts both.  With each: the case that set it.
MEASURED = {
    "pair": 6.390e-15,             # 48 kHz, renorm_twice, 1030 samples, mode 2's sine, against long double
    "envelope": 1.802e-15,         # 48 kHz, renorm_twice, 1030 samples, mode 1: 1030 roundings of the product
    "drift": 1.269e-15,            # 44.1 kHz, renorm_twice_2e32, 1030 samples, mode 2: 65 updates
    "q": 3.168e-15,                # 44.1 kHz, noise_left_L-1, 49 samples
    "noise": 2.071e-14,            # 44.1 kHz, onset_left_24, 25 samples: the band-pass state s1 near a zero crossing
    "samples": 4.850e-15,          # 48 kHz, pickup_1.2_neg, 64 samples, sample 46: tanh past the knee
    "subnormal_steps": 2.0,        # 44.1 kHz, damper_84_ends_at_0, 15 samples: mode 3's envelope damped into the subnormals
    "subnormal_steps_carried": 2.0,   # 48 kHz, damper_84_ends_at_0, 23 samples, mode 3: amplitude x envelope stepped by the oracle (below)
}
BARS = {k: FLOOR_RULE * v for k, v in MEASURED.items()}
# The folded amplitude (deviation 9's class): subnormal_steps_carried.  The release and steal variants of the steady kernel carry
# ae = amplitude x envelope as one recurrence and give the envelope back as ae / amplitude, so what is rounded to the subnormal grid, sample
# after sample, is ae, and one step of ae is 1 / amplitude steps of the envelope.  For those forms (carried_amp) an envelope whose amplitude
# x envelope is subnormal is therefore measured in steps of ae, and the bar is measured on the reference the same way as the others: the
# oracle steps the carried quantity itself (carried_record: amplitude x envelope written in the envelope's place) against the long-double
# run and under the one-ulp change.  Found by tests/test_gpu_voice_block.py on steal_ramp_ending_* at 48 kHz: mode 3 of note 84 (amplitude
# 6.6e-7) enters at 9.6e-315 -- 1 300 steps of ae -- and comes back up to 2 steps of ae, 2.3e6 of the envelope, away.


def carried_record(rec):
    """-> (the record with amplitude x envelope in the envelope's place for the modes where that product is subnormal, those modes): what
    the damper variants carry through the block"""
    r = rec.copy()
    modes = []
    for m in range(7):
        a = abs(float(rec[AMP + m]))
        p = a * float(rec[ENV + m])
        if 0.0 < a < 1.0 and 0.0 < p < MIN_NORMAL:
            r[ENV + m] = p
            modes.append(m)
    return r, modes


def _same(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def _rel(d, scale):
    if d == 0.0:
        return 0.0
    return d / scale if scale > 0.0 else float("inf")


def pair_excluded(ref_rec):
    """modes whose pair is not compared: the reference envelope after the block is below 1e-290, where the folded kernel documents that
    it cannot give the pair back"""
    return [m for m in range(7) if not ref_rec[ENV + m] >= SUBNORMAL_SCALE]


def steal_record_compared(ref_rec):
    """a steal voice whose fade has run out is dropped by the kernels and stepped on by the reference: compared only while its counter is > 0"""
    return lo32(ref_rec, STEAL) > 0


def samples_scale(rec_in, ref_rec, ref_y):
    return max(float(np.max(np.abs(ref_y))), 1.8375 * abs(float(rec_in[GAIN])) * max(abs(float(rec_in[Q])), abs(float(ref_rec[Q]))))


def class_errors(rec_in, ref_rec, ref_y, got_rec, got_y, n_voices=1, carried_amp=False):
    """{class: (error, where)} of one voice block; got_y / ref_y None: the samples are not part of it (multi-voice engines compare the sum).
    carried_amp: the form carries amplitude x envelope (see BARS)."""
    err = {k: (0.0, "") for k in CLASSES}

    def put(k, e, where):
        if e > err[k][0] or (np.isnan(e) and not np.isnan(err[k][0])):
            err[k] = (float("inf") if np.isnan(e) else e, where)

    skip = pair_excluded(ref_rec)
    for m in range(7):
        if m not in skip:
            sc = max(abs(rec_in[S + m]), abs(rec_in[C + m]), abs(ref_rec[S + m]), abs(ref_rec[C + m]))
            for f in (S + m, C + m):
                put("pair", _rel(0.0 if _same(got_rec[f], ref_rec[f]) else abs(got_rec[f] - ref_rec[f]), sc), f"field {f} (mode {m})")
        d = 0.0 if _same(got_rec[ENV + m], ref_rec[ENV + m]) else abs(got_rec[ENV + m] - ref_rec[ENV + m])
        sc = max(abs(rec_in[ENV + m]), abs(ref_rec[ENV + m]))
        amp = abs(float(rec_in[AMP + m]))
        if carried_amp and 0.0 < amp < 1.0 and 0.0 < amp * sc < MIN_NORMAL:
            put("subnormal_steps_carried", d * amp / SUBNORMAL_STEP, f"field {ENV + m} (envelope of mode {m}, in steps of amplitude x envelope)")
        elif 0.0 < sc < MIN_NORMAL:
            put("subnormal_steps", d / SUBNORMAL_STEP, f"field {ENV + m} (envelope of mode {m})")
        else:
            put("envelope", _rel(d, sc), f"field {ENV + m} (mode {m})")
        d = 0.0 if _same(got_rec[DRIFT + m], ref_rec[DRIFT + m]) else abs(got_rec[DRIFT + m] - ref_rec[DRIFT + m])
        put("drift", _rel(d, max(abs(rec_in[DRIFT + m]), abs(ref_rec[DRIFT + m]))), f"field {DRIFT + m} (mode {m})")
    put("q", _rel(0.0 if _same(got_rec[Q], ref_rec[Q]) else abs(got_rec[Q] - ref_rec[Q]), max(abs(rec_in[Q]), abs(ref_rec[Q]))), f"field {Q}")
    put("noise", _rel(0.0 if _same(got_rec[NAMP], ref_rec[NAMP]) else abs(got_rec[NAMP] - ref_rec[NAMP]), max(abs(rec_in[NAMP]), abs(ref_rec[NAMP]))), f"field {NAMP}")
    sc = max(abs(rec_in[NS1]), abs(rec_in[NS2]), abs(ref_rec[NS1]), abs(ref_rec[NS2]))
    for f in (NS1, NS2):
        put("noise", _rel(0.0 if _same(got_rec[f], ref_rec[f]) else abs(got_rec[f] - ref_rec[f]), sc), f"field {f}")
    if ref_y is not None:
        d = np.where(ref_y == got_y, 0.0, np.abs(got_y - ref_y))
        d = np.where(np.isnan(d), np.inf, d)
        i = int(np.argmax(d))
        put("samples", _rel(float(d[i]), samples_scale(rec_in, ref_rec, ref_y)) / n_voices, f"sample {i}")
    return err


def compare(rec_in, ref, got_rec, got_y, steal=False, bars=None, where="", carried_amp=False):
    """-> (failures [str], {class: error / bar}).  ref = (record, y, info) of the reference; got_y None: samples compared elsewhere."""
    bars = BARS if bars is None else bars
    ref_rec, ref_y, _ = ref
    fails = []
    if steal and not steal_record_compared(ref_rec):
        d = np.abs(got_y - ref_y) if got_y is not None else np.zeros(1)
        e = _rel(float(d.max()), samples_scale(rec_in, ref_rec, ref_y))
        if got_y is not None and e > bars["samples"]:
            fails.append(f"samples: error {e:.3e} of the block's peak at sample {int(np.argmax(d))}, bar {bars['samples']:.3e} [{where}]")
        return fails, {"samples": e / bars["samples"] if bars["samples"] > 0 else (0.0 if e == 0 else float("inf"))}
    exact = EXACT + CONSTANT
    for f in exact:
        if not _same(got_rec[f], ref_rec[f]):
            kind = "left as written" if f in CONSTANT else "bit-equal"
            fails.append(f"field {f}: {got_rec[f]!r} (bits {bits(got_rec, f):#x}) != reference {ref_rec[f]!r} ({bits(ref_rec, f):#x}), a {kind} field [{where}]")
    err = class_errors(rec_in, ref_rec, ref_y if got_y is not None else None, got_rec, got_y, carried_amp=carried_amp)
    ratios = {}
    for k, (e, at) in err.items():
        ratios[k] = e / bars[k] if bars[k] > 0.0 else (0.0 if e == 0.0 else float("inf"))
        if ratios[k] > 1.0:
            fails.append(f"{k}, {at}: error {e:.3e} of the class's scale, bar {bars[k]:.3e} [{where}]")
    return fails, ratios
