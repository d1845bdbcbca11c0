"""The pump measurements on the device: host mirror of ``preamp-bench pump-sweep`` / ``pump-trace`` / ``pump-spike`` / ``pump-step`` /
``pump-sinusoid`` (tools/preamp-bench/src/main.rs:2329-3063) over the C-ABI (``ow_pump_measure``).

The five commands characterise the DC "pump" of the melange 12-node preamp's shadow path as a function of R_ldr.  They drive
``gen_preamp::process_sample`` directly on a ``CircuitState::default()``: one point is one run of one such state, and every point of a
command runs on its own lane in ONE library call (pump-spike: one call for its three static grids, 832 points, and one for its slew).

Each command returns a dict with its rows, its CSV text (``csv_text``, or ``csv_texts`` by file suffix for pump-spike), its stderr report
(``report``) and the path(s) it wrote; the report's "done in X s" line carries this run's own time.  What the reference computes from the
whole trace after the run -- pump-trace's two-pass sigma and its five one-pole high-pass RMS figures, pump-step's tail statistics,
pump-sinusoid's bifurcation count -- is host work here too, in the reference's order of operations.
"""
import ctypes as C
import math
import os
import tempfile
import time

import numpy as np

from .binding import OwError, OwPumpCfg, OwPumpPoint, OwPumpRow, check, load_library, take_error  # noqa: F401
from .centroid_track import rust_display
from ._rust_text import _e, _f, as_usize

STATIC, STEP, RAMP, LOGCOS = 0, 1, 2, 3                     # include/openwurli_hip.h OW_PUMP_*
CODEGEN_SR = 48000.0                                        # gen_preamp::SAMPLE_RATE

# numpy views of include/openwurli_hip.h ow_pump_point / ow_pump_row
POINT_DTYPE = np.dtype(OwPumpPoint)
ROW_FIELDS = ("sum", "sum_sq", "mean", "std", "min", "max", "pair_mean", "pair_std", "raw_std", "extra", "max_step")
ROW_COUNTERS = ("nr_exhausted", "be_fallbacks", "voltage_damps", "nan_resets")
ROW_DTYPE = np.dtype(OwPumpRow)


def temp_default(filename: str) -> str:
    """main.rs:123-128."""
    return os.path.join(tempfile.gettempdir(), filename)


def log_grid(lo: float, hi: float, n: int):
    """The commands' log spacing (main.rs:2372-2374, 2386): exp(ln(lo) + step * i), step = (ln(hi) - ln(lo)) / (n - 1)."""
    ln_min = math.log(lo)
    step = (math.log(hi) - ln_min) / (n - 1)
    return [math.exp(ln_min + step * i) for i in range(n)]


def make_point(sample_rate, r_settle, settle, capture, in_amp=0.0, in_freq=0.0, extra_sample=0, schedule=STATIC, r_to=0.0, ln_mid=0.0, ln_amp=0.0,
               sched_freq=0.0):
    p = np.zeros(1, dtype=POINT_DTYPE)
    p[0] = (sample_rate, r_settle, settle, capture, in_amp, in_freq, extra_sample, schedule, r_to, ln_mid, ln_amp, sched_freq)
    return p


def static_points(sample_rate, r_ldrs, settle, capture, in_amp=0.0, in_freq=0.0) -> np.ndarray:
    p = np.zeros(len(r_ldrs), dtype=POINT_DTYPE)
    p["sample_rate"], p["r_settle"], p["settle"], p["capture"], p["in_amp"], p["in_freq"] = sample_rate, r_ldrs, settle, capture, in_amp, in_freq
    return p


def run_points(points, device=0, trace=False):
    """``ow_pump_measure`` on a POINT_DTYPE array: a ROW_DTYPE array (and, with trace, f64 [n][largest capture]: a row's tail beyond its
    own capture is 0)."""
    L = load_library()
    pts = np.ascontiguousarray(points, dtype=POINT_DTYPE).ravel()
    rows = np.zeros(pts.size, dtype=ROW_DTYPE)
    stride = int(pts["capture"].max()) if pts.size else 0
    tr = np.zeros((pts.size, stride)) if trace else None
    cfg = OwPumpCfg(int(device))
    check(L, L.ow_pump_measure(pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(cfg), rows.ctypes.data_as(C.c_void_p),
                               tr.ctypes.data_as(C.c_void_p) if trace else None, stride))
    return (rows, tr) if trace else rows


# ---- pump-sweep (main.rs:2340-2431) -------------------------------------------------------------------------------------------------
def sweep_points(ldr_min=1_000.0, ldr_max=1_000_000.0, points=256, settle=60_000, avg=4_096, sample_rate=48_000.0) -> np.ndarray:
    if not (ldr_min > 0.0 and ldr_max > ldr_min):
        raise ValueError("assertion failed: ldr_min > 0.0 && ldr_max > ldr_min")
    if not points >= 2:
        raise ValueError("assertion failed: points >= 2")
    return static_points(sample_rate, log_grid(ldr_min, ldr_max, int(points)), int(settle), int(avg))


def format_sweep_csv(r_ldrs, rows) -> str:
    out = ["r_ldr,pump_v,pump_std,pump_min,pump_max"]
    out += [f"{_e(r, 6)},{_e(q['mean'], 9)},{_e(q['std'], 6)},{_e(q['min'], 9)},{_e(q['max'], 9)}" for r, q in zip(r_ldrs, rows)]
    return "\n".join(out) + "\n"


def format_sweep_report(r_ldrs, rows, ldr_min, ldr_max, settle, avg, sample_rate, seconds, csv_path) -> str:
    n = len(r_ldrs)
    out = [f"pump-sweep: {n} points from {_f(ldr_min, '.0f')} Ω to {_f(ldr_max, '.0f')} Ω (log), settle={settle}, avg={avg}, SR={_f(sample_rate, '.0f')} Hz"]
    for i, (r, q) in enumerate(zip(r_ldrs, rows)):
        if i % 32 == 0 or i + 1 == n:
            out.append(f"  [{i:3d}/{n}] R_ldr = {_f(r, '10.0f')} Ω  pump = {_e(q['mean'], 6, True)} V  (σ = {_e(q['std'], 2)}, "
                       f"span = {_e(float(q['max']) - float(q['min']), 2)})")
    out.append(f"pump-sweep: done in {_f(seconds, '.1f')}s → {csv_path}")
    return "\n".join(out) + "\n"


def pump_sweep(ldr_min=1_000.0, ldr_max=1_000_000.0, points=256, settle=60_000, avg=4_096, sample_rate=48_000.0, csv=None, device=0):
    csv = temp_default("pump_sweep.csv") if csv is None else csv
    pts = sweep_points(ldr_min, ldr_max, points, settle, avg, sample_rate)
    t0 = time.perf_counter()
    rows = run_points(pts, device)
    seconds = time.perf_counter() - t0
    text = format_sweep_csv(pts["r_settle"], rows)
    if csv:
        with open(csv, "w", newline="") as f:
            f.write(text)
    return {"points": pts, "rows": rows, "csv_text": text, "csv": csv,
            "report": format_sweep_report(pts["r_settle"], rows, ldr_min, ldr_max, int(settle), int(avg), sample_rate, seconds, csv)}


# ---- pump-trace (main.rs:2441-2540) -------------------------------------------------------------------------------------------------
TRACE_BANDS = (0.1, 1.0, 10.0, 100.0, 1000.0)


def trace_stats(buf):
    """main.rs:2482-2516 on the captured samples: mean, std (two-pass), min, max, band_rms[5].  Sums run in sample order."""
    buf = np.asarray(buf, dtype=np.float64)
    n = buf.size
    mean = float(np.cumsum(buf)[-1]) / n
    d = buf - mean
    std = math.sqrt(float(np.cumsum(d * d)[-1]) / n)
    dt = 1.0 / 48_000.0
    xs = buf.tolist()
    band_rms = []
    for fc in TRACE_BANDS:
        rc = 1.0 / (2.0 * math.pi * fc)
        a = rc / (rc + dt)
        py, px, acc = 0.0, xs[0], 0.0
        for x in xs:
            y = a * (py + x - px)
            py, px = y, x
            acc += y * y
        band_rms.append(math.sqrt(acc / n))
    return {"mean": mean, "std": std, "min": float(buf.min()), "max": float(buf.max()), "band_rms": band_rms}


def format_trace_csv(buf) -> str:
    return "\n".join(["sample,pump_v"] + [f"{i},{_e(y, 9)}" for i, y in enumerate(np.asarray(buf).tolist())]) + "\n"


def format_trace_report(ldr, settle, samples, st, seconds, csv_path) -> str:
    out = [f"pump-trace: R_ldr = {_f(ldr, '.0f')} Ω, settle = {settle}, samples = {samples} ({_f(samples / 48_000.0, '.3f')} s @ 48 kHz)",
           f"  mean   = {_e(st['mean'], 9, True)} V",
           f"  std    = {_e(st['std'], 6)} V",
           f"  span   = {_e(st['max'] - st['min'], 6)} V  (min {_e(st['min'], 6, True)}, max {_e(st['max'], 6, True)})",
           "  HPF RMS above:"]
    out += [f"    {_f(fc, '7.1f')} Hz : {_e(v, 6)} V" for fc, v in zip(TRACE_BANDS, st["band_rms"])]
    out.append(f"pump-trace: done in {_f(seconds, '.1f')}s → {csv_path}")
    return "\n".join(out) + "\n"


def trace_points(ldr=1_000_000.0, settle=400_000, samples=131_072) -> np.ndarray:
    return static_points(CODEGEN_SR, [ldr], int(settle), int(samples))


def pump_trace(ldr=1_000_000.0, settle=400_000, samples=131_072, csv=None, device=0):
    csv = temp_default("pump_trace.csv") if csv is None else csv
    pts = trace_points(ldr, settle, samples)
    t0 = time.perf_counter()
    rows, tr = run_points(pts, device, trace=True)
    st = trace_stats(tr[0])
    text = format_trace_csv(tr[0])
    if csv:
        with open(csv, "w", newline="") as f:
            f.write(text)
    seconds = time.perf_counter() - t0
    return {"points": pts, "rows": rows, "trace": tr[0], "stats": st, "csv_text": text, "csv": csv,
            "report": format_trace_report(ldr, int(settle), int(samples), st, seconds, csv)}


# ---- pump-spike (main.rs:2571-2798) -------------------------------------------------------------------------------------------------
SPIKE_RATES = (44_100.0, 48_000.0, 88_200.0, 96_000.0)
SPIKE_AMPS = (0.0, 0.001, 0.005, 0.020, 0.100)
SPIKE_WIDTH = (46_500.0, 48_500.0, 256)
SPIKE_GRID = (30_000.0, 70_000.0, 64)
SPIKE_SLEW = (30_000.0, 70_000.0, 48_000.0, 1.0)           # r_start, r_end, sr, ramp_seconds


def spike_points(settle=400_000, avg=8_192):
    """The three static grids in the command's order: width (256), sample rate (4 x 64, settle proportional to the rate), audio (5 x 64
    with a 1 kHz sine at 48 kHz): 832 points for one call."""
    if int(avg) % 2:
        raise ValueError("--avg must be even to cancel Nyquist 2-cycle")
    settle, avg = int(settle), int(avg)
    parts = [static_points(CODEGEN_SR, log_grid(*SPIKE_WIDTH), settle, avg)]
    grid = log_grid(*SPIKE_GRID)
    for sr in SPIKE_RATES:
        parts.append(static_points(sr, grid, as_usize(float(settle) * sr / 48_000.0), avg))
    for amp in SPIKE_AMPS:
        parts.append(static_points(CODEGEN_SR, grid, settle, avg, amp, 1000.0))
    return np.concatenate(parts)


def slew_point(settle=400_000) -> np.ndarray:
    r_start, r_end, sr, secs = SPIKE_SLEW
    return make_point(sr, r_start, int(settle), as_usize(secs * sr), extra_sample=1, schedule=RAMP, r_to=r_end)


def slew_resistances(n_ramp: int):
    r_start, r_end = SPIKE_SLEW[0], SPIKE_SLEW[1]
    return [r_start + (r_end - r_start) * (k / (n_ramp - 1)) for k in range(n_ramp)]


def format_spike(pts, rows, slew_trace, slew_row, prefix):
    """The four CSV texts (by suffix) and the stderr report."""
    csvs, out = {}, []
    nw, ng = SPIKE_WIDTH[2], SPIKE_GRID[2]
    # test 1
    lines, sus = ["r_ldr,pump_v,pair_std,raw_std"], []
    for p, q in zip(pts[:nw], rows[:nw]):
        lines.append(f"{_e(p['r_settle'], 6)},{_e(q['pair_mean'], 9)},{_e(q['pair_std'], 6)},{_e(q['raw_std'], 6)}")
        if q["raw_std"] > 0.1:
            sus.append((p["r_settle"], q["pair_mean"], q["raw_std"]))
    csvs["width"] = "\n".join(lines) + "\n"
    out.append(f"[1/4] WIDTH: 256 points in [{_f(SPIKE_WIDTH[0], '.0f')}, {_f(SPIKE_WIDTH[1], '.0f')}] Ω …")
    out.append(f"  → {len(sus)} points with raw_std > 0.1 V (spike candidates):")
    out += [f"      R={_f(r, '.1f')} Ω  pump={_f(m, '+.4f')} V  raw_std={_f(s, '.4f')} V" for r, m, s in sus]
    out.append(f"  CSV: {prefix}_width.csv")

    def hits_of(p, q):
        return [(a["r_settle"], b["pair_mean"], b["raw_std"]) for a, b in zip(p, q) if b["raw_std"] > 0.1]

    def hit_lines(hits, none_text):
        return [none_text] if not hits else [f"  → spike: R={_f(r, '.1f')} Ω  pump={_f(m, '+.4f')} V  raw_std={_f(s, '.4f')} V" for r, m, s in hits]
    # test 2
    lines, at = ["sample_rate,r_ldr,pump_v,raw_std"], nw
    for sr in SPIKE_RATES:
        p, q = pts[at:at + ng], rows[at:at + ng]
        at += ng
        out.append(f"[2/4] SR={_f(sr, '.0f')} Hz: 64 points in [{_f(SPIKE_GRID[0], '.0f')}, {_f(SPIKE_GRID[1], '.0f')}] Ω …")
        lines += [f"{_f(sr, '.0f')},{_e(a['r_settle'], 6)},{_e(b['pair_mean'], 9)},{_e(b['raw_std'], 6)}" for a, b in zip(p, q)]
        out += hit_lines(hits_of(p, q), f"  → NO SPIKE at SR={_f(sr, '.0f')}")
    csvs["samplerate"] = "\n".join(lines) + "\n"
    out.append(f"  CSV: {prefix}_samplerate.csv")
    # test 3
    lines = ["input_amp,r_ldr,pump_v,raw_std"]
    for amp in SPIKE_AMPS:
        p, q = pts[at:at + ng], rows[at:at + ng]
        at += ng
        out.append(f"[3/4] AUDIO amp={_f(amp, '.4f')} V @1 kHz: 64 points in [{_f(SPIKE_GRID[0], '.0f')}, {_f(SPIKE_GRID[1], '.0f')}] Ω …")
        lines += [f"{_e(amp, 6)},{_e(a['r_settle'], 6)},{_e(b['pair_mean'], 9)},{_e(b['raw_std'], 6)}" for a, b in zip(p, q)]
        out += hit_lines(hits_of(p, q), f"  → NO SPIKE at amp={_f(amp, '.4f')}")
    csvs["audio"] = "\n".join(lines) + "\n"
    out.append(f"  CSV: {prefix}_audio.csv")
    # test 4
    r_start, r_end, sr, secs = SPIKE_SLEW
    n_ramp = len(slew_trace)
    out.append(f"[4/4] SLEW: R ramps {_f(r_start, '.0f')} → {_f(r_end, '.0f')} Ω over {rust_display(secs)} s ({n_ramp} samples) …")
    rs = slew_resistances(n_ramp)
    csvs["slew"] = "\n".join(["sample,r_ldr,pump_v"] + [f"{k},{_e(r, 6)},{_e(y, 9)}" for k, (r, y) in enumerate(zip(rs, np.asarray(slew_trace).tolist()))]) + "\n"
    out.append(f"  → max sample-to-sample step during slew: {_f(slew_row['max_step'], '.4f')} V (compare to ~0.5 V static-R spike)")
    out.append(f"  CSV: {prefix}_slew.csv")
    out.append("pump-spike: all 4 tests complete.")
    return csvs, "\n".join(out) + "\n"


def pump_spike(settle=400_000, avg=8_192, csv_prefix="/tmp/pump_spike", device=0):
    pts = spike_points(settle, avg)
    rows = run_points(pts, device)
    sp = slew_point(settle)
    srow, strace = run_points(sp, device, trace=True)
    csvs, report = format_spike(pts, rows, strace[0], srow[0], csv_prefix)
    paths = {}
    for suffix, text in csvs.items():
        paths[suffix] = f"{csv_prefix}_{suffix}.csv"
        if csv_prefix:
            with open(paths[suffix], "w", newline="") as f:
                f.write(text)
    return {"points": pts, "rows": rows, "slew_point": sp, "slew_row": srow[0], "slew_trace": strace[0], "csv_texts": csvs, "csvs": paths, "report": report}


# ---- pump-step (main.rs:2817-2918) --------------------------------------------------------------------------------------------------
def step_points(ldr_from=1_000_000.0, ldr_to=19_000.0, sample_rate=88_200.0, settle=750_000, samples=720_000) -> np.ndarray:
    return make_point(sample_rate, ldr_from, int(settle), int(samples), extra_sample=1, schedule=STEP, r_to=ldr_to)


def step_tail(buf):
    """main.rs:2874-2888: tail_mean, tail_std over the pair means of the last 10 %, initial, total_swing."""
    buf = np.asarray(buf, dtype=np.float64)
    samples = buf.size
    tail = buf[(samples * 9 // 10) & ~1:]
    pairs = tail.size // 2
    pm = 0.5 * (tail[0:2 * pairs:2] + tail[1:2 * pairs:2])
    s = float(np.cumsum(pm)[-1]) if pairs else 0.0
    ss = float(np.cumsum(pm * pm)[-1]) if pairs else 0.0
    with np.errstate(all="ignore"):
        tail_mean = float(np.float64(s) / np.float64(pairs))
        var = float(np.float64(ss) / np.float64(pairs) - np.float64(tail_mean) * np.float64(tail_mean))
    tail_std = math.sqrt(0.0 if not var > 0.0 else var)           # f64::max(NaN, 0.0) is 0.0
    initial = 0.5 * (float(buf[0]) + float(buf[1]))
    return {"tail_mean": tail_mean, "tail_std": tail_std, "initial": initial, "total_swing": tail_mean - initial}


def format_step_csv(buf, ldr_from, ldr_to, sample_rate, settled) -> str:
    ys = np.asarray(buf).tolist()
    n = len(ys)
    out = [f"# pump-step  r_from={_e(ldr_from, 6)}  r_to={_e(ldr_to, 6)}  sr={_f(sample_rate, '.0f')}  settled_at_from={_e(settled, 9)}", "sample,pump_v,pump_avg2"]
    for i in range(0, n, 2):
        p = 0.5 * (ys[i] + ys[i + 1]) if i + 1 < n else ys[i]
        out.append(f"{i},{_e(ys[i], 9)},{_e(p, 9)}")
        if i + 1 < n:
            out.append(f"{i + 1},{_e(ys[i + 1], 9)},{_e(p, 9)}")
    return "\n".join(out) + "\n"


def format_step_report(ldr_from, ldr_to, sample_rate, settle, samples, settled, tail, seconds, csv_path) -> str:
    secs = _f(samples / sample_rate, ".3f")
    return "\n".join([
        f"pump-step: R_from={_f(ldr_from, '.0f')} Ω → R_to={_f(ldr_to, '.0f')} Ω  SR={_f(sample_rate, '.0f')} Hz  settle={settle}  samples={samples} ({secs} s)",
        f"  settled value at R_from: {_f(settled, '+.6f')} V",
        f"  initial (pair-mean after step):  {_f(tail['initial'], '+.6f')} V",
        f"  tail (last 10% pair-mean):       mean={_f(tail['tail_mean'], '+.6f')} V  std={_e(tail['tail_std'], 3)} V",
        f"  total swing:                     {_f(tail['total_swing'], '+.6f')} V  ({samples} samples = {secs} s of capture)",
        f"pump-step: done in {_f(seconds, '.1f')}s → {csv_path}"]) + "\n"


def pump_step(ldr_from=1_000_000.0, ldr_to=19_000.0, sample_rate=88_200.0, settle=750_000, samples=720_000, csv=None, device=0):
    csv = temp_default("pump_step.csv") if csv is None else csv
    pts = step_points(ldr_from, ldr_to, sample_rate, settle, samples)
    t0 = time.perf_counter()
    rows, tr = run_points(pts, device, trace=True)
    seconds = time.perf_counter() - t0
    tail = step_tail(tr[0])
    text = format_step_csv(tr[0], ldr_from, ldr_to, sample_rate, rows[0]["extra"])
    if csv:
        with open(csv, "w", newline="") as f:
            f.write(text)
    return {"points": pts, "rows": rows, "trace": tr[0], "tail": tail, "csv_text": text, "csv": csv,
            "report": format_step_report(ldr_from, ldr_to, sample_rate, int(settle), int(samples), rows[0]["extra"], tail, seconds, csv)}


# ---- pump-sinusoid (main.rs:2937-3063) ----------------------------------------------------------------------------------------------
def sinusoid_samples(cycles, sample_rate, freq) -> int:
    return as_usize(cycles * sample_rate / freq)                  # main.rs:2968


def sinusoid_points(ldr_min=19_000.0, ldr_max=1_000_000.0, freq=5.6, cycles=10.0, sample_rate=88_200.0, settle=750_000) -> np.ndarray:
    ln_mid = 0.5 * (math.log(ldr_max) + math.log(ldr_min))      # main.rs:2964-2965
    ln_amp = 0.5 * (math.log(ldr_max) - math.log(ldr_min))
    return make_point(sample_rate, ldr_max, int(settle), sinusoid_samples(cycles, sample_rate, freq), extra_sample=1, schedule=LOGCOS, ln_mid=ln_mid,
                      ln_amp=ln_amp, sched_freq=freq)


def sinusoid_resistances(point):
    """main.rs:2966-2967, 2996-2997: the resistance before each captured sample."""
    dt, omega = 1.0 / float(point["sample_rate"]), 2.0 * math.pi * float(point["sched_freq"])
    ln_mid, ln_amp = float(point["ln_mid"]), float(point["ln_amp"])
    return [math.exp(ln_mid + ln_amp * math.cos(omega * (k * dt))) for k in range(int(point["capture"]))]


def sinusoid_bifurcations(ys) -> int:
    """main.rs:3018-3032: pair-mean steps above 0.1 V."""
    ys = np.asarray(ys).tolist()
    n, count = len(ys), 0
    prev = 0.5 * (ys[0] + ys[1])
    for i in range(2, n, 2):
        pm = 0.5 * (ys[i] + (ys[i + 1] if i + 1 < n else ys[i]))
        if abs(pm - prev) > 0.1:
            count += 1
        prev = pm
    return count


def format_sinusoid_csv(rs, ys, ldr_min, ldr_max, freq, sample_rate, cycles) -> str:
    ys = np.asarray(ys).tolist()
    n = len(ys)
    out = [f"# pump-sinusoid  ldr_min={_e(ldr_min, 6)}  ldr_max={_e(ldr_max, 6)}  freq={_f(freq, '.6f')}  sr={_f(sample_rate, '.0f')}  cycles={rust_display(cycles)}",
           "sample,r_ldr,pump_v,pump_avg2"]
    for i in range(n):
        if i % 2 == 0 and i + 1 < n:
            pm = 0.5 * (ys[i] + ys[i + 1])
        elif i > 0:
            pm = 0.5 * (ys[i - 1] + ys[i])
        else:
            pm = ys[i]
        out.append(f"{i},{_e(rs[i], 6)},{_e(ys[i], 9)},{_e(pm, 9)}")
    return "\n".join(out) + "\n"


def format_sinusoid_report(point, ldr_min, ldr_max, freq, cycles, rs, ys, max_dy, seconds, csv_path) -> str:
    sr, samples = float(point["sample_rate"]), int(point["capture"])
    max_dr, prev = 0.0, ldr_max                                   # main.rs:2993, 3002-3010
    for r in rs:
        max_dr, prev = max(max_dr, abs(r - prev)), r
    y_min, y_max = float(np.min(ys)), float(np.max(ys))
    return "\n".join([
        f"pump-sinusoid: R = exp({_f(point['ln_mid'], '.3f')} + {_f(point['ln_amp'], '.3f')}·cos(2π·{rust_display(freq)}·t))  R ∈ [{_f(ldr_min, '.0f')}, {_f(ldr_max, '.0f')}] Ω",
        f"  SR={_f(sr, '.0f')} Hz  cycles={rust_display(cycles)}  samples={samples} ({_f(samples / sr, '.3f')} s)  settle={int(point['settle'])}",
        f"  pump range: [{_f(y_min, '.3f')}, {_f(y_max, '.3f')}] V (span {_f(y_max - y_min, '.3f')} V)",
        f"  max sample-to-sample step:  dR={_f(max_dr, '.2f')} Ω  dY={_f(max_dy, '.4f')} V",
        f"  bifurcation events (pair-step > 0.1 V): {sinusoid_bifurcations(ys)}  (expect 0 for slewed-R)",
        f"pump-sinusoid: done in {_f(seconds, '.1f')}s → {csv_path}"]) + "\n"


def pump_sinusoid(ldr_min=19_000.0, ldr_max=1_000_000.0, freq=5.6, cycles=10.0, sample_rate=88_200.0, settle=750_000, csv=None, device=0):
    csv = temp_default("pump_sinusoid.csv") if csv is None else csv
    pts = sinusoid_points(ldr_min, ldr_max, freq, cycles, sample_rate, settle)
    t0 = time.perf_counter()
    rows, tr = run_points(pts, device, trace=True)
    seconds = time.perf_counter() - t0
    rs = sinusoid_resistances(pts[0])
    text = format_sinusoid_csv(rs, tr[0], ldr_min, ldr_max, freq, sample_rate, cycles)
    if csv:
        with open(csv, "w", newline="") as f:
            f.write(text)
    return {"points": pts, "rows": rows, "trace": tr[0], "r_ldr": rs, "csv_text": text, "csv": csv,
            "report": format_sinusoid_report(pts[0], ldr_min, ldr_max, freq, cycles, rs, tr[0], rows[0]["max_step"], seconds, csv)}


__all__ = ["STATIC", "STEP", "RAMP", "LOGCOS", "POINT_DTYPE", "ROW_DTYPE", "ROW_FIELDS", "ROW_COUNTERS", "temp_default", "log_grid", "make_point",
           "static_points", "run_points", "sweep_points", "format_sweep_csv", "format_sweep_report", "pump_sweep", "trace_points", "trace_stats",
           "format_trace_csv", "format_trace_report", "pump_trace", "spike_points", "slew_point", "slew_resistances", "format_spike", "pump_spike",
           "step_points", "step_tail", "format_step_csv", "format_step_report", "pump_step", "sinusoid_samples", "sinusoid_points",
           "sinusoid_resistances", "sinusoid_bifurcations", "format_sinusoid_csv", "format_sinusoid_report", "pump_sinusoid"]
