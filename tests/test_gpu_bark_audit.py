"""GPU parity of `preamp-bench bark-audit` (tools/preamp-bench/src/main.rs:551-664) through ow_bark_audit, against the CPU restatement
tests/c/bark_audit_ref.cpp (cmd_bark_audit's loop body in the reference's statement order over the oracle).

Three layers.  The stage rows (reed, pickup, preamp) go through oracle.parity_report with the floors tests/test_gpu_calibrate.py applies
to the same stages.  The figures are then checked against the device's OWN rows: the peaks bit for bit, each magnitude against the
restatement's serial dft_magnitude on the returned row within the a-priori bound analysis_cap(n) x (2 / n) sum |x_i| of an n-term sum
(note_audit_ref.ANALYSIS_REL was measured on windows up to 4 410 samples, this command's is 11 025: the test prints the worst difference
it sees, DESIGN.md records it).  End to end, every figure lies within the bar derived in bark_audit_ref's docstring from the rows'
per-sample tolerances -- no number is chosen by hand -- and the report's text is compared exactly for the jobs
tests/test_bark_audit_host.py shows to be clear of every rounding boundary by those bars.

The two forms of the legacy chain (OW_BARK_ROW=0/1) must give the same bits, and a job the same bits alone, among 65, in chunks of two,
and with or without taps.
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import bark_audit_ref as ref
import note_audit_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"default": ref.DEFAULT_SIZE, "short": ref.SHORT_SIZE}
KINDS = {"legacy": 0, "melange": 1}


def _jobs(pairs):
    from openwurli_amd.intermod_audit import NOTE_JOB_DTYPE
    j = np.zeros(len(pairs), dtype=NOTE_JOB_DTYPE)
    j["note"], j["velocity"] = [p[0] for p in pairs], [p[1] for p in pairs]
    return j


def _all_jobs(size):
    return list(ref.TAP_JOBS) + list(ref.TEXT_JOBS[size])


@pytest.fixture(scope="module")
def device_runs(hiplib):
    """{(size name, kind name): (jobs, rows, taps)}: one call with taps per size and preamp kind, shared by the tests (never modified)."""
    from openwurli_amd import bark_audit as ba
    for v in ("OW_BARK_ROW", "OW_BARK_CHUNK"):
        assert v not in os.environ
    out = {}
    for sn, size in SIZES.items():
        for kn, kind in KINDS.items():
            jobs = _all_jobs(size)
            rows, taps = ba.run_jobs(_jobs(jobs), kind, size[0], size[1], taps=True)
            taps.setflags(write=False)
            out[sn, kn] = (jobs, rows, taps)
    return out


@pytest.fixture(scope="module")
def cpu_runs():
    return {(sn, kn): ref.run_many(_all_jobs(size), size, kind) for sn, size in SIZES.items() for kn, kind in KINDS.items()}


@pytest.mark.parametrize("kn", list(KINDS))
@pytest.mark.parametrize("sn", list(SIZES))
def test_taps_against_the_restatement(oracle, device_runs, cpu_runs, sn, kn):
    jobs, rows, taps = device_runs[sn, kn]
    floors = ref.stage_floors(oracle, KINDS[kn])
    n, m0 = ref.samples(SIZES[sn][0]), ref.samples(SIZES[sn][1])
    assert taps.shape == (len(jobs), 3, n)
    for i, (job, c) in enumerate(zip(jobs, cpu_runs[sn, kn])):
        if job not in ref.TAP_JOBS:
            continue
        assert (c.n, c.m0) == (n, m0) == (int(rows[i]["window_end"]), int(rows[i]["window_start"]))
        for k, stage in enumerate(ref.STAGES):
            rep = oracle.parity_report(taps[i, k], c.taps[k], abs_floor=floors[k])
            print(f"\n[bark taps {sn}/{kn} {job} {stage}] worst ratio {rep['worst_ratio']:.3e} ({rep['worst_branch']}), max abs err {rep['max_abs_err']:.3e}")
            assert rep["n_bad"] == 0, (job, stage, rep)


@pytest.mark.parametrize("kn", list(KINDS))
@pytest.mark.parametrize("sn", list(SIZES))
def test_figures_against_the_devices_own_taps(device_runs, sn, kn):
    jobs, rows, taps = device_runs[sn, kn]
    worst = 0.0
    for i, job in enumerate(jobs):
        r = rows[i]
        assert (int(r["note"]), int(r["velocity"])) == job
        w = slice(int(r["window_start"]), int(r["window_end"]))
        n = w.stop - w.start
        assert r["reed_peak"] == np.max(np.abs(taps[i, 0, w])) and r["pu_peak"] == np.max(np.abs(taps[i, 1, w]))      # bit for bit
        assert r["y_peak"] == r["reed_peak"] * r["displacement_scale"]
        f0 = float(r["fundamental_hz"])
        for k, stage in ((1, "pu"), (2, "pre")):
            x = taps[i, k, w]
            scale = 2.0 / n * float(np.sum(np.abs(x)))
            for h, f in (("h1", f0), ("h2", 2.0 * f0)):
                got, want = float(r[f"{stage}_{h}"]), ref.dft_magnitude(x, f)
                rel = abs(got - want) / scale
                worst = max(worst, rel)
                assert abs(got - want) <= note_audit_ref.analysis_cap(n) * scale, (job, stage, h, got, want, rel)
            h1, h2 = float(r[f"{stage}_h1"]), float(r[f"{stage}_h2"])
            assert r[f"{stage}_h2_h1"] == (h2 / h1 if h1 > 1e-15 else 0.0)
    n = ref.samples(SIZES[sn][0]) - ref.samples(SIZES[sn][1])
    print(f"\n[bark analysis {sn}/{kn}] window {n}: worst |device - serial| / ((2 / n) sum |x|) = {worst:.3e}; a-priori cap "
          f"{note_audit_ref.analysis_cap(n):.3e}; within ANALYSIS_REL {note_audit_ref.ANALYSIS_REL:.1e}: {worst <= note_audit_ref.ANALYSIS_REL}")


@pytest.mark.parametrize("kn", list(KINDS))
@pytest.mark.parametrize("sn", list(SIZES))
def test_figures_and_text_end_to_end(oracle, device_runs, cpu_runs, sn, kn):
    from openwurli_amd import bark_audit as ba
    jobs, rows, _ = device_runs[sn, kn]
    floors = ref.stage_floors(oracle, KINDS[kn])
    compared = 0
    for i, (job, c) in enumerate(zip(jobs, cpu_runs[sn, kn])):
        b = ref.bars(c, floors)
        for f in ref.FIELDS:
            got, want, bar = float(rows[i][f]), getattr(c.row, f), getattr(b, f)
            print(f"[bark {sn}/{kn} {job}] {f} {got:.9g} (ref {want:.9g}, bar {bar:.2e}, off {abs(got - want):.2e})")
            assert abs(got - want) <= bar, (job, f, got, want, bar)
        clear = ref.text_is_clear(c, b)
        if kn == "legacy" and job in ref.TEXT_JOBS[SIZES[sn]]:
            assert clear, job                                # tests/test_bark_audit_host.py asserts the same on the CPU
        if clear:
            assert ba.format_report(rows[i:i + 1]) == ba.format_report([ref.record(job[0], job[1], c)]), job
            compared += 1
    assert compared >= (len(ref.TEXT_JOBS[SIZES[sn]]) if kn == "legacy" else 1)


def _form_jobs(count):
    notes, vels = (33, 41, 48, 57, 60, 66, 72, 79, 84, 90, 96), (127, 100, 80, 40, 20)
    return _jobs([(notes[i % len(notes)], vels[i % len(vels)]) for i in range(count)])


@pytest.mark.parametrize("count,sn", [(1, "short"), (8, "short"), (9, "short"), (33, "short"), (9, "default")])
def test_row_and_lane_pair_forms_give_the_same_bits(hiplib, monkeypatch, count, sn):
    """k_bark_chain_row against k_job_chain<false> at JOB_OUT_PA_INPUT: one workgroup with one job, a full one, a full one plus one, more
    than one lane-pair wavefront's 32."""
    from openwurli_amd import bark_audit as ba
    size = SIZES[sn]
    jobs = _form_jobs(count)
    got = {}
    for form in ("0", "1"):
        monkeypatch.setenv("OW_BARK_ROW", form)
        got[form] = ba.run_jobs(jobs, 0, size[0], size[1], taps=True)
    assert got["0"][0].tobytes() == got["1"][0].tobytes()
    assert np.array_equal(got["0"][1], got["1"][1])
    assert np.all(np.max(np.abs(got["1"][1][:, 2, :]), axis=1) > 0.0)      # the preamp rows are there


@pytest.mark.parametrize("kn", list(KINDS))
def test_a_job_does_not_depend_on_its_call(hiplib, monkeypatch, device_runs, kn):
    """Alone, inside a call of 65 jobs (a voice block plus one), in chunks of two, with or without taps: the same bits."""
    from openwurli_amd import bark_audit as ba
    size, kind = ref.SHORT_SIZE, KINDS[kn]
    monkeypatch.delenv("OW_BARK_CHUNK", raising=False)
    monkeypatch.delenv("OW_BARK_ROW", raising=False)
    many = _form_jobs(65)
    rows65, taps65 = ba.run_jobs(many, kind, size[0], size[1], taps=True)
    assert ba.run_jobs(many, kind, size[0], size[1]).tobytes() == rows65.tobytes()                   # asking for taps changes no number
    for i in (0, 31, 32, 63, 64):
        r1, t1 = ba.run_jobs(many[i:i + 1], kind, size[0], size[1], taps=True)
        assert r1.tobytes() == rows65[i:i + 1].tobytes() and np.array_equal(t1[0], taps65[i]), i
    # chunks of two, the last of one job: all 65 jobs in 33 chunks for the legacy preamp; the melange calls are ten times as
    # long, so the first five jobs in three chunks there
    m = 65 if kn == "legacy" else 5
    monkeypatch.setenv("OW_BARK_CHUNK", "2")
    rows2, taps2 = ba.run_jobs(many[:m], kind, size[0], size[1], taps=True)
    assert rows2.tobytes() == rows65[:m].tobytes() and np.array_equal(taps2, taps65[:m])
    # and the shared fixture's call, other neighbours again
    jobs, rows, taps = device_runs["short", kn]
    monkeypatch.delenv("OW_BARK_CHUNK")
    r1, t1 = ba.run_jobs(_jobs(jobs[1:2]), kind, size[0], size[1], taps=True)
    assert r1.tobytes() == rows[1:2].tobytes() and np.array_equal(t1[0], taps[1])


def test_grid_equals_the_per_call_rows(hiplib):
    from openwurli_amd import bark_audit as ba
    notes, layers = (36, 60, 84), (50, 110)
    by_kind, text = ba.grid(notes, layers)
    assert [k for k, _ in by_kind] == [0, 1]
    want = []
    for kind, rows in by_kind:
        per = np.concatenate([ba.bark_audit([n], layers, kind) for n in notes])
        assert rows.tobytes() == per.tobytes()
        assert [(int(r["note"]), int(r["velocity"])) for r in rows] == [(n, v) for n in notes for v in layers]
        want.append((kind, per))
    assert text == ba.format_grid_csv(want) and text.count("\n") == 1 + 12 and text.startswith(ba.GRID_HEADER + "\n36,50,legacy,")


def test_the_tool_prints_the_commands_report(hiplib, oracle):
    """python tools/bark_audit.py: the command's default 5 notes x 4 velocities.  The text is the formatter's of the device's rows; every
    line whose job is clear of rounding by its bars is the restatement's line, character for character."""
    from openwurli_amd import bark_audit as ba
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bark_audit as tool
    buf = io.StringIO()
    with redirect_stdout(buf):
        tool.main([])
    jobs = [(n, v) for n in ba.DEFAULT_NOTES for v in ba.DEFAULT_VELOCITIES]
    assert buf.getvalue() == ba.format_report(ba.bark_audit(), 4, 5)
    runs = ref.run_many(jobs, ref.DEFAULT_SIZE, 0)
    want = ba.format_report([ref.record(n, v, r) for (n, v), r in zip(jobs, runs)], 4, 5).splitlines()
    got = buf.getvalue().splitlines()
    assert len(got) == len(want) == 4 + 20 + 5 + 8
    rows = [k for k, line in enumerate(want) if k >= 4 and line and k < 4 + 25]
    assert len(rows) == 20
    floors = ref.stage_floors(oracle, 0)
    clear = 0
    for k, r in zip(rows, runs):
        if ref.text_is_clear(r, ref.bars(r, floors)):
            assert got[k] == want[k], (k, got[k], want[k])
            clear += 1
    assert clear >= 10
    assert [g for k, g in enumerate(got) if k not in rows] == [w for k, w in enumerate(want) if k not in rows]
