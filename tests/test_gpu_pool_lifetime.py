"""The pool owns its device resources: an acquisition that fails -- in pool creation, in a buffer grow, in the first device burst -- leaks
nothing and leaves no half-built state behind.  The failures are host exceptions injected by ow_test_fail_acquire_after
(openwurli_hip_test.h) in place of the k-th acquisition; ow_test_live_resources counts what the library owns.

Every scenario runs in a fresh child process (this file, run as a script) that prints one JSON line: inside the pytest process the pools
of other tests and the trajectory feeder thread acquire and release concurrently, and the counter would not be deterministic."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
TRAJ_SR = 16000.0       # the trajectory scenario settles a Twin-T oscillator (2 s of chain-rate steps) some 25 times: a low rate keeps that short
STRIDE = 8
BLOCK = 64
# preamp kind, power amp kind, tremolo kind, engines, a block length beyond the fresh pool's capacity (a lone engine starts with
# OW_MAX_BLOCK = 8192 samples, so the 4096 that grows every other pool would be no grow at all there)
CONFIGS = {"legacy-1": (0, 0, 0, 1, 16384),            # the lone-instance path
           "melange-64": (1, 1, 0, 64, 4096)}          # melange preamp and amp, Twin-T; the smallest pool with the attention summary
HOOK = "ow_test_fail_acquire_after"

pytestmark = pytest.mark.gpu


def _run_child(scenario, config, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), scenario, config], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_failed_create_releases_everything(hiplib, config):
    r = _run_child("create", config, {"OW_TREM_TRAJ": "0"})        # no process-wide store: the pool is the only owner
    print(r)
    assert r["N"] > 0 and r["after_free"] == 0
    assert [f["k"] for f in r["fails"]] == sorted({k for k in (0, 1, 2, 5, 10, 20, 40, r["N"] - 1) if k < r["N"]})
    for f in r["fails"]:
        assert f["null"] and HOOK in f["err"] and f["live"] == 0, f
    assert r["peak"] > 0.0 and r["identical"] and r["end"] == 0


def test_failed_create_with_trajectory(hiplib):
    r = _run_child("trajectory", "legacy-1")
    probes, rows = r["probes"], r["rows"]              # rows: consecutive indices from the last one before the store's creation
    print([x["k"] for x in probes], [(x["k"], x["pool"], x.get("traj")) for x in rows], r["seconds"])
    assert all(x["live"] == 0 for x in probes + rows), (probes, rows)
    assert [x["k"] for x in rows] == list(range(rows[0]["k"], rows[0]["k"] + len(rows)))
    assert len(probes) >= 1 and not rows[0]["pool"] and rows[1]["pool"] and rows[1]["traj"] == 0
    for x in probes + rows[:-1]:
        if x["pool"]:       # inside the store's creation: a working pool without the trajectory
            assert x["traj"] == 0 and x["works"], x
        else:               # anywhere else: no pool, and the error names the hook
            assert HOOK in x["err"], x
    assert rows[-1]["pool"] and rows[-1]["traj"] == 1 and rows[-1]["works"], rows[-1]        # past the last acquisition: nothing injected


@pytest.mark.parametrize("config", list(CONFIGS))
def test_failed_buffer_grow_leaves_a_usable_pool(hiplib, config):
    """After each of the four failures the pool renders block 2, 3, 4, 5 of its note; the twin, which never saw one, renders the same."""
    r = _run_child("grow", config)
    print(r)
    assert r["peak"] > 0.0 and r["first_identical"]
    assert [x["k"] for x in r["rows"]] == [0, 1, 2, 3]
    for x in r["rows"]:
        assert HOOK in x["err"] and x["next_err"] == "" and x["identical"], x
    assert r["end"] == 0


def test_failed_first_burst_is_retried(hiplib):
    r = _run_child("burst", "melange-64")
    print(r)
    assert HOOK in r["err1"] and r["bursts"] == [0, 0, 1]           # the failed burst went to the host path, the next one to the device
    assert r["err2"] == "" and r["masks1"] and r["masks2"] and r["states2"]
    assert r["peak"] > 0.0 and r["block1"] and r["block2"]


# ---- the child ------------------------------------------------------------------------------------------------------------------------
class _Child:
    def __init__(self, config):
        sys.path.insert(0, ROOT)
        import openwurli_amd as ow
        from openwurli_amd import binding
        self.ow, self.binding, self.L = ow, binding, binding.load_library()
        self.pre, self.amp, self.trem, self.n, self.grow_len = CONFIGS[config]

    def live(self):
        return int(self.L.ow_test_live_resources())

    def settled_live(self, target):
        """A store dropped from the registry while the feeder thread looks at it is released by that thread, a moment later."""
        for _ in range(5000):
            if self.live() == target:
                break
            time.sleep(0.001)
        return self.live()

    def pool(self, fail_at=-1, sr=SR):
        """(pool, None), or (None, the error) when ow_pool_new_kinds returned NULL; fail_at >= 0 arms the hook for the creation."""
        self.L.ow_clear_error()
        self.L.ow_test_fail_acquire_after(fail_at)
        try:
            return self.ow.EnginePool(sr, self.n, 0, self.pre, self.amp, self.trem), None
        except self.ow.OwError as ex:
            return None, str(ex)
        finally:
            self.L.ow_test_fail_acquire_after(-1)

    def strike(self, p):
        for e in range(self.n):
            p[e].note_on(48 + e % 24, 0.8)

    def masks(self, p):
        return [int(self.L.ow_test_engine_masks(p[e]._h, w)) for e in range(self.n) for w in (0, 1)]

    def create(self):
        base = self.live()
        p, _ = self.pool()
        N = self.live() - base
        self.strike(p)
        ref = p.render(BLOCK)
        p.close()
        after_free = self.live() - base
        fails = []
        for k in sorted({k for k in (0, 1, 2, 5, 10, 20, 40, N - 1) if k < N}):
            q, err = self.pool(k)
            if q:
                q.close()
            fails.append(dict(k=k, null=q is None, err=err or "", live=self.live() - base))
        p, _ = self.pool()
        self.strike(p)
        out = p.render(BLOCK)
        p.close()
        return dict(N=N, after_free=after_free, fails=fails, identical=bool(np.array_equal(ref, out)), peak=float(np.max(np.abs(ref))), end=self.live() - base)

    def trajectory(self):
        """Every index inside the store's creation, found without paying for all the creations that fail before it (each sets up and tears
        down the pool's nine streams, some 55 ms): probe every STRIDE-th index upwards until one yields a pool, walk down from there to the
        first index that does not, then up until a pool comes back on the trajectory.  (The store's creation acquires a stream, sixteen
        marks and seven buffers; were it ever shorter than the stride, the probes could step over it and the test would find no index.)"""
        self.L.ow_test_clear_settle_caches()
        base, t0 = self.live(), time.perf_counter()

        def attempt(k):
            p, err = self.pool(k, TRAJ_SR)
            row = dict(k=k, pool=p is not None, err=err or "")
            if p:
                row["traj"] = p.get_switch("trem_traj")
                try:
                    self.strike(p)
                    out = np.concatenate([p.render(BLOCK) for _ in range(4)], axis=1)
                    row["works"] = bool(np.all(np.isfinite(out)) and np.max(np.abs(out)) > 0.0)
                except self.ow.OwError as ex:
                    row["works"], row["err"] = False, str(ex)
                p.close()
            self.L.ow_test_clear_settle_caches()
            row["live"] = self.settled_live(base) - base
            return row
        probes = [attempt(0)]
        while not probes[-1]["pool"] and probes[-1]["k"] < 2000:
            probes.append(attempt(probes[-1]["k"] + STRIDE))
        rows = [probes.pop()]
        while rows[0]["pool"] and rows[0]["k"] > 0:
            rows.insert(0, attempt(rows[0]["k"] - 1))
        while not (rows[-1]["pool"] and rows[-1]["traj"] == 1) and len(rows) < 200:      # on the trajectory: nothing was injected any more
            rows.append(attempt(rows[-1]["k"] + 1))
        return dict(probes=probes, rows=rows, seconds=round(time.perf_counter() - t0, 2))

    def grow(self):
        L = self.L
        L.ow_test_clear_settle_caches()
        base = self.live()
        (p, _), (twin, _) = self.pool(), self.pool()
        self.strike(p); self.strike(twin)
        ref, ref_twin = p.render(BLOCK), twin.render(BLOCK)
        rows = []
        for k in range(4):
            L.ow_clear_error()
            L.ow_test_fail_acquire_after(k)
            if k % 2 == 0:
                L.ow_pool_ensure_buffer_capacity(p._h, self.grow_len)
            else:
                L.ow_pool_render(p._h, None, 0, self.grow_len)
            L.ow_test_fail_acquire_after(-1)
            row = dict(k=k, err=self.binding.take_error(L))
            out = np.zeros((self.n, BLOCK), dtype=np.float32)
            L.ow_pool_render(p._h, out.ctypes.data, BLOCK, BLOCK)
            row["next_err"] = self.binding.take_error(L)
            row["identical"] = bool(np.array_equal(out, twin.render(BLOCK)))
            rows.append(row)
        p.close(); twin.close()
        L.ow_test_clear_settle_caches()
        return dict(first_identical=bool(np.array_equal(ref, ref_twin)), peak=float(np.max(np.abs(ref))), rows=rows, end=self.settled_live(base) - base)

    def burst(self):
        L = self.L
        (p, _), (twin, _) = self.pool(), self.pool()
        p.set_switch("midi_device", 1); twin.set_switch("midi_device", 0)
        dt = np.dtype(self.binding.MIDI_DTYPE)
        ev1 = np.array([(e, 0, k, 0, 0.7) for e in range(self.n) for k in (48 + e % 24, 76)], dtype=dt)          # grouped by engine
        ev2 = np.array([x for e in range(self.n) for x in ((e, 1, 76, 0, 0.0), (e, 0, 60, 0, 0.9))], dtype=dt)
        bursts = [p.get_switch("midi_device_bursts")]
        L.ow_clear_error()
        L.ow_test_fail_acquire_after(1)                     # the second of the five first-burst allocations
        p.midi(ev1)
        L.ow_test_fail_acquire_after(-1)
        err1 = self.binding.take_error(L)
        twin.midi(ev1)
        bursts.append(p.get_switch("midi_device_bursts"))
        masks1 = self.masks(p) == self.masks(twin)
        o1, t1 = p.render(BLOCK), twin.render(BLOCK)        # (the host path queued ops: they are drained before the next burst)
        p.midi(ev2)
        err2 = self.binding.take_error(L)
        twin.midi(ev2)
        bursts.append(p.get_switch("midi_device_bursts"))
        o2, t2 = p.render(BLOCK), twin.render(BLOCK)
        states = lambda g: [(g[e].slot_state(s), g[e].slot_note(s)) for e in range(self.n) for s in range(64)]
        r = dict(err1=err1, err2=err2, bursts=bursts, masks1=masks1, masks2=self.masks(p) == self.masks(twin), states2=states(p) == states(twin),
                 block1=bool(np.array_equal(o1, t1)), block2=bool(np.array_equal(o2, t2)), peak=float(np.max(np.abs(o2))))
        p.close(); twin.close()
        return r


if __name__ == "__main__":
    child = _Child(sys.argv[2])
    print(json.dumps(getattr(child, sys.argv[1])()))
