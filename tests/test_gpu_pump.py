"""ow_pump_measure (k_pump_points) against the CPU restatement of the pump commands (tests/pump_ref.py): static points, resistance
schedules, placement and chunking, and the five Python commands at reduced flags.

Figures measured on one MI355X (feature row f10, has them with the restatement's own one-ulp movement beside them) are printed
by every test before it asserts."""
import math

import numpy as np
import pytest

import pump_ref as ref
from openwurli_amd import pump

pytestmark = pytest.mark.gpu

_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _reference(kind):
    """The restatement on the static / the schedule points (computed once, shared, never changed)."""
    if ("ref", kind) not in _CACHE:
        pts = ref.static_test_points() if kind == "static" else ref.schedule_test_points()
        rows, traces = ref.run_points(pts)
        _CACHE[("ref", kind)] = (pts, rows, traces)
    return _CACHE[("ref", kind)]


def _device(hiplib, kind):
    if ("dev", kind) not in _CACHE:
        pts = _reference(kind)[0]
        _CACHE[("dev", kind)] = pump.run_points(pts, trace=True)
    return _CACHE[("dev", kind)]


def _compare(kind, hiplib):
    pts, rrows, rtraces = _reference(kind)
    drows, dtraces = _device(hiplib, kind)
    worst = 0.0
    failures = []
    for i, p in enumerate(pts):
        n = int(p["capture"])
        rt, dt = rtraces[i], dtraces[i][:n]
        peak = float(np.max(np.abs(rt)))
        b = ref.PUMP_REL * peak
        figures = {"trace": float(np.max(np.abs(dt - rt))), "extra": abs(float(drows[i]["extra"]) - float(rrows[i]["extra"]))}
        for f in ("mean", "min", "max"):
            figures[f] = abs(float(drows[i][f]) - float(rrows[i][f]))
        ratio = max(figures.values()) / peak
        worst = max(worst, ratio)
        print(f"{kind} {i}: sr={p['sample_rate']:.0f} R={p['r_settle']:.6g} amp={p['in_amp']} sched={p['schedule']} peak={peak:.4f} "
              + " ".join(f"{k}={v:.3e}" for k, v in figures.items()) + f" ratio={ratio:.3e}"
              + f" counters dev nr/be/damp/nan={[int(drows[i][c]) for c in pump.ROW_COUNTERS]} ref={[int(rrows[i][c]) for c in pump.ROW_COUNTERS]}")
        for k, v in figures.items():
            if not v <= b:
                failures.append((i, k, v, b))
        for f in ("std", "pair_std", "raw_std"):                  # as variances: 2 sigma_ref b + b^2 + (n + 4) 2^-52 max|y|^2
            sr_, sd = float(rrows[i][f]), float(drows[i][f])
            bar = 2.0 * sr_ * b + b * b + (n + 4) * 2.0 ** -52 * peak * peak
            dv = abs(sd * sd - sr_ * sr_)
            print(f"    {f}: dev={sd:.9e} ref={sr_:.9e} |dvar|={dv:.3e} bar={bar:.3e}")
            if not dv <= bar:
                failures.append((i, f, dv, bar))
        if int(drows[i]["be_fallbacks"]) != int(rrows[i]["be_fallbacks"]) or int(drows[i]["nan_resets"]) != int(rrows[i]["nan_resets"]):
            failures.append((i, "counters", [int(drows[i][c]) for c in pump.ROW_COUNTERS], [int(rrows[i][c]) for c in pump.ROW_COUNTERS]))
        assert np.all(dtraces[i][n:] == 0.0)
    print(f"{kind}: worst ratio to the trace peak {worst:.3e} (PUMP_REL {ref.PUMP_REL:.1e})")
    assert not failures, failures


def test_static_points_match_the_restatement(hiplib):
    _compare("static", hiplib)


def test_schedules_match_the_restatement(hiplib):
    _compare("schedule", hiplib)


def test_static_sums_are_the_traces_sums(hiplib):
    """sum, sum_sq, the pair sums and max_step are the serial reductions of the very samples the trace holds."""
    for kind in ("static", "schedule"):
        pts = _reference(kind)[0]
        drows, dtraces = _device(hiplib, kind)
        for i, p in enumerate(pts):
            y = dtraces[i][:int(p["capture"])].tolist()
            s = ss = 0.0
            for v in y:
                s += v
                ss += v * v
            assert s == float(drows[i]["sum"]) and ss == float(drows[i]["sum_sq"]), (kind, i)
            assert min(y) == float(drows[i]["min"]) and max(y) == float(drows[i]["max"]), (kind, i)
            prev = [float(drows[i]["extra"])] + y[:-1] if p["extra_sample"] else [y[0]] + y[:-1]
            assert max(abs(a - b) for a, b in zip(y, prev)) == float(drows[i]["max_step"]), (kind, i)
            ps = pss = 0.0
            for k in range(len(y) // 2):
                pm = 0.5 * (y[2 * k] + y[2 * k + 1])
                ps += pm
                pss += pm * pm
            pairs = len(y) // 2
            assert ps / pairs == float(drows[i]["pair_mean"]), (kind, i)
            assert math.sqrt(max(pss / pairs - (ps / pairs) ** 2, 0.0)) == float(drows[i]["pair_std"]), (kind, i)


def _alone(hiplib):
    """Every base point run in a call of its own: the bits it must return wherever it is placed."""
    if "alone" not in _CACHE:
        base = ref.placement_points()
        res = [pump.run_points(base[i:i + 1], trace=True) for i in range(base.size)]
        _CACHE["alone"] = (base, [r[0][0] for r in res], [r[1][0] for r in res])
    return _CACHE["alone"]


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_placement_and_chunking_change_no_bit(hiplib, monkeypatch, n):
    base, arows, atraces = _alone(hiplib)
    rng = np.random.default_rng(1000 + n)
    pick = rng.permutation(np.arange(n) % base.size)
    pts = base[pick]
    cap = int(pts["capture"].max())

    def check(rows, traces):
        for k, src in enumerate(pick):
            assert rows[k].tobytes() == arows[src].tobytes(), (n, k, int(src))
            if traces is not None:
                m = int(base[src]["capture"])
                assert np.array_equal(_bits(traces[k][:m]), _bits(atraces[src][:m])) and np.all(traces[k][m:cap] == 0.0), (n, k, int(src))
    check(pump.run_points(pts), None)
    monkeypatch.setenv("OW_PUMP_CHUNK", "64")
    check(*pump.run_points(pts, trace=True))


def _parse_csv(text, columns):
    lines = [ln for ln in text.splitlines() if not ln.startswith("#")]
    assert lines[0] == columns
    return np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])


def test_command_pump_sweep(hiplib, tmp_path):
    r = pump.pump_sweep(points=8, settle=2048, avg=256, csv=str(tmp_path / "s.csv"))
    direct = pump.run_points(pump.sweep_points(points=8, settle=2048, avg=256))
    assert r["rows"].tobytes() == direct.tobytes()
    tab = _parse_csv(open(r["csv"]).read(), "r_ldr,pump_v,pump_std,pump_min,pump_max")
    assert tab.shape == (8, 5)
    assert np.allclose(tab[:, 1], direct["mean"], rtol=1e-9, atol=0) and np.allclose(tab[:, 0], pump.log_grid(1000.0, 1_000_000.0, 8), rtol=1e-6)
    assert r["report"].startswith("pump-sweep: 8 points from 1000 Ω to 1000000 Ω (log), settle=2048, avg=256, SR=48000 Hz\n")
    print(r["report"])


def test_command_pump_trace(hiplib, tmp_path):
    r = pump.pump_trace(settle=2048, samples=256, csv=str(tmp_path / "t.csv"))
    rows, tr = pump.run_points(pump.trace_points(settle=2048, samples=256), trace=True)
    assert np.array_equal(_bits(r["trace"]), _bits(tr[0])) and r["rows"].tobytes() == rows.tobytes()
    tab = _parse_csv(open(r["csv"]).read(), "sample,pump_v")
    assert tab.shape == (256, 2) and np.allclose(tab[:, 1], tr[0], rtol=1e-9, atol=0)
    cpu = ref.trace_stats(tr[0])
    assert r["stats"]["mean"] == cpu["mean"] and r["stats"]["std"] == cpu["std"] and r["stats"]["band_rms"] == cpu["band_rms"]
    print(r["report"])


def test_command_pump_spike(hiplib, tmp_path):
    prefix = str(tmp_path / "spike")
    r = pump.pump_spike(settle=1024, avg=64, csv_prefix=prefix)
    assert r["points"].size == 832
    direct = pump.run_points(pump.spike_points(1024, 64))
    assert r["rows"].tobytes() == direct.tobytes()
    srow, strace = pump.run_points(pump.slew_point(1024), trace=True)
    assert np.array_equal(_bits(r["slew_trace"]), _bits(strace[0])) and float(r["slew_row"]["max_step"]) == float(srow[0]["max_step"])
    w = _parse_csv(open(prefix + "_width.csv").read(), "r_ldr,pump_v,pair_std,raw_std")
    s = _parse_csv(open(prefix + "_samplerate.csv").read(), "sample_rate,r_ldr,pump_v,raw_std")
    a = _parse_csv(open(prefix + "_audio.csv").read(), "input_amp,r_ldr,pump_v,raw_std")
    sl = _parse_csv(open(prefix + "_slew.csv").read(), "sample,r_ldr,pump_v")
    assert w.shape == (256, 4) and s.shape == (256, 4) and a.shape == (320, 4) and sl.shape == (48000, 3)
    assert np.allclose(np.concatenate([w[:, 1], s[:, 2], a[:, 2]]), direct["pair_mean"], rtol=1e-9, atol=0)
    assert np.allclose(sl[:, 2], strace[0], rtol=1e-9, atol=0)
    print(r["report"])


def test_command_pump_step(hiplib, tmp_path):
    r = pump.pump_step(settle=2048, samples=256, csv=str(tmp_path / "st.csv"))
    rows, tr = pump.run_points(pump.step_points(settle=2048, samples=256), trace=True)
    assert np.array_equal(_bits(r["trace"]), _bits(tr[0])) and r["rows"].tobytes() == rows.tobytes()
    tab = _parse_csv(open(r["csv"]).read(), "sample,pump_v,pump_avg2")
    assert tab.shape == (256, 3) and np.allclose(tab[:, 1], tr[0], rtol=1e-9, atol=0)
    cpu = ref.step_tail(tr[0])
    assert all(r["tail"][k] == cpu[k] for k in cpu)
    print(r["report"])


def test_command_pump_sinusoid(hiplib, tmp_path):
    kw = dict(freq=88_200.0 / 2048.0, cycles=1.0, settle=2048)
    r = pump.pump_sinusoid(csv=str(tmp_path / "si.csv"), **kw)
    rows, tr = pump.run_points(pump.sinusoid_points(**kw), trace=True)
    assert int(r["points"][0]["capture"]) == 2048
    assert np.array_equal(_bits(r["trace"]), _bits(tr[0])) and r["rows"].tobytes() == rows.tobytes()
    tab = _parse_csv(open(r["csv"]).read(), "sample,r_ldr,pump_v,pump_avg2")
    assert tab.shape == (2048, 4) and np.allclose(tab[:, 2], tr[0], rtol=1e-9, atol=0) and np.allclose(tab[:, 1], r["r_ldr"], rtol=1e-6)
    assert pump.sinusoid_bifurcations(tr[0]) == ref.sinusoid_bifurcations(tr[0])
    print(r["report"])
