"""bench.py --dump-outputs on the device: the file holds what the last timed step rendered, sample for sample.  The bench runs in this
process (no child of a GPU-initialised process) on a small pool; the reference is the same script replayed on a fresh pool here, every
render call's block read back from HBM whole.  92 warm-up + 2 timed steps end on the step cut at the 1.0 s re-strike (384 + 128 samples),
so the piece the bench had to read out before its second render call is covered too."""
import json
import os

import numpy as np
import pytest


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_step(hiplib, tmp_path, capsys, monkeypatch):
    import bench
    import openwurli_amd as ow
    monkeypatch.setenv("OW_NOISE_SEED", os.environ.get("OW_NOISE_SEED", "1"))
    # a sample of 64 of the 256 engines in four runs of 16: the read-out of a big pool, one device read per run
    monkeypatch.setattr(bench, "DUMP_ENGINE_ROWS", 64)
    monkeypatch.setattr(bench, "DUMP_ENGINE_RUN", 16)
    n, warm, steps = 256, 92, 2
    rc = bench.main(["--gpus", "1", "--instances", str(n), "--steps", str(steps), "--warmup", str(warm), "--dump-outputs", str(tmp_path)])
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert rc == 0 and line["steps"] == steps and line["ms_per_step"] > 0.0
    audio = np.load(tmp_path / "audio.npy")
    rows = np.load(tmp_path / "audio_engines.npy").astype(int)
    runs = bench.dump_engine_runs(n)
    assert len(runs) == 4 and np.array_equal(rows, np.concatenate([np.arange(s, s + c) for s, c in runs]))
    assert audio.dtype == np.float32 and audio.shape == (64, bench.BUF)

    pool = ow.EnginePool(bench.SR, n, device=0)
    try:
        pool.set_sample_rate(bench.SR)
        pool.ensure_buffer_capacity(bench.BUF)
        pool.stagger_tremolo(n)
        for k in range(n):
            e = pool[k]
            e.set_volume(0.5); e.set_tremolo_depth(0.5); e.set_speaker_character(0.0); e.set_mlp_enabled(True)
        strike, restrike = bench.build_events(n, "strike"), bench.build_events(n, "restrike")
        pos = 0
        for _ in range(warm + steps):
            pieces, done = [], 0
            while done < bench.BUF:
                if pos % bench.EPOCH == 0:
                    pool.midi(strike if pos == 0 else restrike)
                m = min(bench.BUF - done, bench.EPOCH - pos % bench.EPOCH)
                pool.render(m, to_host=False)
                pieces.append(pool.last_block()[:, :m])
                pos += m
                done += m
    finally:
        pool.close()
    assert [p.shape[1] for p in pieces] == [384, 128]
    ref = np.concatenate(pieces, axis=1)
    assert np.max(np.abs(ref)) > 1e-3
    assert np.array_equal(audio, ref[rows])
