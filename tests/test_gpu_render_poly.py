"""GPU parity of `preamp-bench render-poly` (tools/preamp-bench/src/main.rs:1397-1592) through ow_render_poly, against the CPU restatement
tests/c/render_poly_ref.cpp.

Sample bars, with F = render_poly_ref.ABS_FLOOR_POLY (measured on the CPU by tests/test_render_poly_host.py under the project's floor rule):
  final          oracle.parity_report(.., abs_floor=F), n_bad == 0
  separate_sum   per sample within the SUM over the voices k of max(1e-5 max(|s_k|, 1e-3 peak_k), F), s_k the restatement's per-voice rows
  residual       within the bar of final plus the bar of separate_sum (errors add)
Row figures: win_peak and sqrt(win_mean_sq) within the largest sample bar inside the window; the dB fields exactly the reference's
expressions on the device's own linear values, and within the dB equivalent of that bound of the restatement's.  intermod_ratio_db is
asserted on the chords of render_poly_ref.CHORDS, all of which keep the residual's RMS at least 10 x above the RMS of its bar (checked on
the CPU in the host test).
"""
import math
import os

import numpy as np
import pytest

import render_poly_ref as ref

pytestmark = pytest.mark.gpu

F = ref.ABS_FLOOR_POLY
SHORT = [k for k in ref.CHORDS if k != "default"]          # the 1 s chords run in ONE call (mixed n_notes), the default chord at its 3 s


def _dev_chord(ch):
    return (ch.notes, ch.velocities, ch.volume, ch.speaker, ch.ldr, ch.no_poweramp)


@pytest.fixture(scope="module")
def parity():
    """{name: (device row, {final, separate_sum, residual}, restatement)}"""
    from openwurli_amd import render_poly as rp
    out = {}
    refs = dict(zip(ref.CHORDS, ref.render_many(ref.CHORDS.values())))
    for names in (["default"], SHORT):
        dur = ref.CHORDS[names[0]].duration
        assert all(ref.CHORDS[k].duration == dur for k in names)
        rows, audio = rp.run_chords([_dev_chord(ref.CHORDS[k]) for k in names], dur, final=True, separate_sum=True, residual=True)
        for i, k in enumerate(names):
            out[k] = (rows[i], {a: audio[a][i] for a in audio}, refs[k])
    return out


def _worst(err, bar):
    i = int(np.argmax(err / bar))
    return {"worst_index": i, "err": float(err[i]), "bar": float(bar[i]), "worst_ratio": float(err[i] / bar[i]), "n_bad": int((err > bar).sum())}


@pytest.mark.parametrize("name", list(ref.CHORDS))
def test_samples_against_the_restatement(oracle, parity, name):
    row, au, r = parity[name]
    assert au["final"].size == r.final.size
    rep = oracle.parity_report(au["final"], r.final, abs_floor=F)
    ws = _worst(np.abs(au["separate_sum"] - r.separate_sum), ref.separate_bar(r.voices, F))
    wr = _worst(np.abs(au["residual"] - r.residual), ref.residual_bar(r, F))
    print(f"\n[render-poly {name}] final {rep}\n  separate_sum {ws}\n  residual {wr}")
    assert rep["peak"] > 1e-3 and rep["n_bad"] == 0, rep
    assert ws["n_bad"] == 0, ws
    assert wr["n_bad"] == 0, wr


def _db_tol(v, bar):
    """dB equivalent of a linear value v known to +- bar."""
    assert 0.0 < bar < v, (v, bar)
    return max(20.0 * math.log10(1.0 + bar / v), -20.0 * math.log10(1.0 - bar / v))


@pytest.mark.parametrize("name", list(ref.CHORDS))
def test_row_figures_against_the_restatement(parity, name):
    row, au, r = parity[name]
    n = r.final.size
    w = ref.window(n)
    bars = (ref.final_bar(r.final, F), ref.separate_bar(r.voices, F), ref.residual_bar(r, F))
    sigs = (au["final"], au["separate_sum"], au["residual"])
    # the whole-render peaks and the window figures are those of the device's own audio ...
    assert row["peak"] == np.abs(au["final"]).max() and row["residual_peak"] == np.abs(au["residual"]).max()
    tol_rms = []
    for k in range(3):
        bar = float(bars[k][w].max())
        assert row["win_peak"][k] == np.abs(sigs[k][w]).max()
        seq = 0.0
        for x in sigs[k][w].tolist():                      # the reference's summation order
            seq += x * x
        assert row["win_mean_sq"][k] == seq / (w.stop - w.start)
        # ... within the largest sample bar inside the window of the restatement's ...
        rms_d, rms_c = math.sqrt(row["win_mean_sq"][k]), math.sqrt(r.row["win_mean_sq"][k])
        print(f"[render-poly {name}] {('poly', 'separate', 'residual')[k]}: win_peak dev {abs(row['win_peak'][k] - r.row['win_peak'][k]):.3e} "
              f"rms dev {abs(rms_d - rms_c):.3e} bar {bar:.3e}; dB dev peak {abs(row['peak_db'][k] - r.row['peak_db'][k]):.2e} rms {abs(row['rms_db'][k] - r.row['rms_db'][k]):.2e}")
        assert abs(row["win_peak"][k] - r.row["win_peak"][k]) <= bar
        assert abs(rms_d - rms_c) <= bar
        # ... the dB fields exactly the reference's expressions (main.rs:916-927, 2241-2247) on the device's linear values ...
        assert row["peak_db"][k] == (20.0 * math.log10(row["win_peak"][k]) if row["win_peak"][k] > 1e-15 else -120.0)
        assert row["rms_db"][k] == (10.0 * math.log10(row["win_mean_sq"][k]) if row["win_mean_sq"][k] > 0.0 else -120.0)
        # ... and within the dB equivalent of the bound of the restatement's
        assert abs(row["peak_db"][k] - r.row["peak_db"][k]) <= _db_tol(r.row["win_peak"][k], bar)
        tol_rms.append(_db_tol(rms_c, bar))
        assert abs(row["rms_db"][k] - r.row["rms_db"][k]) <= tol_rms[k]
    assert row["intermod_ratio_db"] == row["rms_db"][0] - row["rms_db"][2]
    assert ref.ratio_is_assertable(r, F)
    print(f"[render-poly {name}] intermod_ratio_db {row['intermod_ratio_db']:.4f} against {r.row['intermod_ratio_db']:.4f}, tolerance {tol_rms[0] + tol_rms[2]:.2e}")
    assert abs(row["intermod_ratio_db"] - r.row["intermod_ratio_db"]) <= tol_rms[0] + tol_rms[2]


@pytest.mark.parametrize("no_poweramp", [False, True])
def test_single_note_chord(oracle, no_poweramp):
    """n = 1: the shared chain and the one separate chain run the same operations on the same samples."""
    import openwurli_amd as ow
    from openwurli_amd import render_poly as rp
    note, vel, dur = 57, 90, 0.5
    rows, au = rp.run_chords([((note,), (vel,), 0.60, 1.0, 1e6, no_poweramp)], dur, final=True, separate_sum=True, residual=True)
    assert au["final"][0].tobytes() == au["separate_sum"][0].tobytes()
    assert not au["residual"][0].any()
    assert rows["rms_db"][0][2] == -120.0 and rows["peak_db"][0][2] == -120.0 and rows["residual_peak"][0] == 0.0
    assert rows["intermod_ratio_db"][0] == rows["rms_db"][0][0] + 120.0
    # seed + 0 and 1 Mohm: the same job as `render` (tests/test_render_poly_host.py has the restatements bit for bit)
    job = ow.batch_render([{"note": note, "velocity": vel, "mlp": True, "poweramp": not no_poweramp, "volume": 0.60, "speaker": 1.0, "r_ldr": 1e6}],
                          44100.0, dur)[0]
    rep = oracle.parity_report(au["final"][0], job, abs_floor=oracle.ABS_FLOOR_BATCH)
    print(f"\n[render-poly single note, no_poweramp={no_poweramp}] against ow_batch_render {rep}")
    assert rep["peak"] > 1e-3 and rep["n_bad"] == 0, rep
    c = ref.render([note], [vel], dur, 0.60, 1.0, 1e6, no_poweramp=no_poweramp)
    assert oracle.parity_report(au["final"][0], c.final, abs_floor=F)["n_bad"] == 0


def test_bit_independence(monkeypatch):
    """A chord's rows and audio do not change with its position in the call, the other chords present (mixed n_notes, a full wavefront of
    31 notes among them), OW_POLY_CHUNK, or which outputs were requested."""
    from openwurli_amd import render_poly as rp
    dur = 0.25
    probe = rp.make_chord((48, 55, 64), (100, 70, 90), 0.7, 0.8, 60_000.0, False)
    all3 = dict(final=True, separate_sum=True, residual=True)
    alone_r, alone_a = rp.run_chords(probe, dur, **all3)
    rng = np.random.default_rng(4242)

    def others(n):
        out = []
        for i in range(n):
            k = (1, 2, 3, 5, 9, 31)[i % 6]
            out.append(rp.make_chord(rng.integers(33, 97, k), rng.integers(20, 128, k), float(rng.uniform(0.2, 1.0)), float(rng.uniform(0.0, 1.0)),
                                     float(np.exp(rng.uniform(np.log(5e3), np.log(1e6)))), bool(i % 4 == 3)))
        return np.concatenate(out)
    grid = None
    for n in (7, 40):
        other = others(n)
        for pos in sorted({0, n // 2, n - 1}):
            grid = other.copy()
            grid[pos] = probe[0]
            r, a = rp.run_chords(grid, dur, **all3)
            assert r[pos:pos + 1].tobytes() == alone_r.tobytes(), (n, pos)
            for k in all3:
                assert np.array_equal(a[k][pos], alone_a[k][0]), (n, pos, k)
    whole_r, whole_a = rp.run_chords(grid, dur, **all3)                 # 40 chords, the probe last
    # which outputs were requested
    assert rp.run_chords(grid, dur).tobytes() == whole_r.tobytes()
    for k in all3:
        r, a = rp.run_chords(grid, dur, **{k: True})
        assert r.tobytes() == whole_r.tobytes() and list(a) == [k] and np.array_equal(a[k], whole_a[k]), k
    # the documented chunk cap: 40 chords in 14 chunks
    monkeypatch.setenv("OW_POLY_CHUNK", "3")
    ch_r, ch_a = rp.run_chords(grid, dur, **all3)
    assert ch_r.tobytes() == whole_r.tobytes()
    for k in all3:
        assert np.array_equal(ch_a[k], whole_a[k]), k


def _near_boundary(x, decimals, eps=1e-4):
    s = abs(x) * 10 ** decimals
    return abs((s - int(s)) - 0.5) <= eps * 10 ** decimals


def test_report_wavs_and_grid_csv(parity, tmp_path):
    """The printed report and the grid CSV equal the restatement's, except within 1e-4 dB of a rounding boundary of the printed digit."""
    from openwurli_amd import render_poly as rp
    ch = ref.CHORDS["default"]
    out = str(tmp_path / "poly.wav")
    got = rp.render_poly(output=out, normalize=True)                    # every default of the command
    row, au, r = parity["default"]
    assert got["row"].tobytes() == row.tobytes() and np.array_equal(got["final"], au["final"]) and np.array_equal(got["residual"], au["residual"])
    crow = np.zeros(1, dtype=rp.ROW_DTYPE)[0]
    for k in ref.ROW:
        crow[k] = r.row[k]
    want = rp.format_report(ch.notes, ch.velocities, ch.duration, ch.volume, ch.speaker, crow, out)
    gl, wl = got["report"].splitlines(), want.splitlines()
    assert len(gl) == len(wl) == 18 and gl[0] == "Polyphonic render complete" and gl[16] == f"  Output:    {out}"
    values = {6: [rp.to_dbfs(r.row["peak"])], 9: [r.row["peak_db"][0], r.row["rms_db"][0]], 10: [r.row["peak_db"][1], r.row["rms_db"][1]],
              11: [r.row["peak_db"][2], r.row["rms_db"][2]], 12: [r.row["intermod_ratio_db"]]}
    for i, (a, b) in enumerate(zip(gl, wl)):
        assert a == b or (i in values and any(_near_boundary(v, 1) for v in values[i])), (i, a, b)
    for path, sig, sc in ((out, got["final"], rp.wav_scales(row["peak"], row["residual_peak"], True)[0]),
                          (got["residual_output"], got["residual"], 0.5 / row["residual_peak"])):
        assert path.endswith(".wav") and os.path.getsize(path) == 68 + 3 * 132300
        b = open(path, "rb").read()
        d = b[b.index(b"data") + 8:]
        i = int(np.argmax(np.abs(sig)))
        assert int.from_bytes(d[3 * i:3 * i + 3], "little", signed=True) == int(math.copysign(math.floor(abs(sig[i]) * sc * 8388607.0 + 0.5), sig[i]))
    # the grid CSV: every dyad of six notes, in one call
    chords = rp.dyad_grid(45, 50, (90, 70), volume=0.5)
    rows = rp.run_chords(chords, 0.5)
    rr = ref.render_many([ref.Chord(tuple(c["notes"][:2]), (90, 70), 0.5, 0.5, 1.0, 1e6, False) for c in chords])
    crows = rows.copy()
    crows["intermod_ratio_db"] = [x.row["intermod_ratio_db"] for x in rr]
    gl, wl = rp.format_grid_csv(chords, rows).splitlines(), rp.format_grid_csv(chords, crows).splitlines()
    assert len(gl) == 16 and gl[0] == wl[0] == "note_a,note_b,vel_a,vel_b,intermod_ratio_db" and gl[1].startswith("45,46,90,70,")
    for a, b, x in zip(gl[1:], wl[1:], rr):
        assert a == b or _near_boundary(x.row["intermod_ratio_db"], 2), (a, b)


def test_refusals_through_the_c_abi_on_the_device(hiplib):
    from openwurli_amd import binding, render_poly as rp
    with pytest.raises(binding.OwError, match="note 97"):
        rp.run_chords([((60, 97), (90, 90))], 0.25)
    with pytest.raises(binding.OwError, match="OW_PREAMP_MELANGE12"):
        rp.run_chords([((60, 64), (90, 90))], 0.25, preamp_kind=1)
    r = rp.run_chords([((60, 64), (90, 90))], 0.25)                     # the library still works after a refusal
    assert np.isfinite(r["intermod_ratio_db"]).all() and r["peak"][0] > 1e-3
