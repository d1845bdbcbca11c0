"""Wall time of wurli_compare for --pairs note pairs of --duration seconds (default 512 x 1.5 s: notes 33..96 x eight velocity layers, tier
2, MLP on) in a warm process: the renders (one batch call, the audio stays in HBM) and the analysis of both sides (compare_many: four
calls per side) separately, against the numpy float32 restatement of the reference's analysis (tests/wurli_compare_ref.py) on --threads
host processes: --cpu-pairs timed pairs, scaled by count.  Also the new FFT against direct summation: ow_stft_profile (n_fft 4096, hop 512,
centroid only: k_stft_frames) and ow_centroid_analyze (window 4096, hop 512: k_centroid_frames, bins 50 Hz .. sr / 4 only) on the same
--dft-rows rows in HBM.  Prints ONE JSON line; it measures, it does not gate.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _cpu_pair(args):
    import numpy as np
    import wurli_compare_ref as ref
    y_real, y_synth, f0 = args
    ref.pair_figures(y_real, y_synth, f0, np.float32)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--duration", type=float, default=1.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-pairs", type=int, default=16)
    ap.add_argument("--dft-rows", type=int, default=64)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import wurli_compare_ref as ref
    from openwurli_amd import centroid_track as ct, wurli_compare as wc

    notes = [33 + (i % 64) for i in range(a.pairs)]
    vels = [(20, 35, 50, 65, 80, 95, 110, 127)[(i // 64) % 8] for i in range(a.pairs)]
    f0s = [440.0 * 2.0 ** ((m - 69) / 12.0) for m in notes]
    uniq = {m: wc.pcm16_roundtrip(ref.golden_clip(m, 440.0 * 2.0 ** ((m - 69) / 12.0), a.duration)) for m in sorted(set(notes))}
    reals = [uniq[m] for m in notes]
    jobs = [wc.render_job(m, v) for m, v in zip(notes, vels)]
    durs = [a.duration] * a.pairs
    res = {"metric": "wurli_compare_wall", "pairs": a.pairs, "duration_s": a.duration}
    with wc.Renders(jobs[:8], durs[:8]) as r:               # warm-up: library, context, kernels
        wc.compare_many(reals[:8], f0s[:8], synth_device=(r.ptr, r.n, r.stride), synth_lengths=r.row_lengths(), synth_wav24="round")
    t_render, t_analysis = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = wc.Renders(jobs, durs)
        t1 = time.perf_counter()
        try:
            comps = wc.compare_many(reals, f0s, synth_device=(r.ptr, r.n, r.stride), synth_lengths=r.row_lengths(), synth_wav24="round")
            t2 = time.perf_counter()
            if len(t_render) == 0:
                n = int(r.lengths[0])
                rows = min(a.dft_rows, r.n)
                t = []
                for _k in range(3):
                    t3 = time.perf_counter(); wc.stft_profile(None, [n] * rows, 4096, 512, device_audio=(r.ptr, rows, r.stride), mean_mag=False)
                    t.append(time.perf_counter() - t3)
                res["stft_4096_s"], res["dft_rows"], res["frames_per_row"] = float(np.median(t)), rows, wc.frame_count(n, 4096, 512)
                t = []
                for _k in range(3):
                    t3 = time.perf_counter(); ct.analyze_device(r.ptr, rows, r.stride, n, 4096, 512, n); t.append(time.perf_counter() - t3)
                res["centroid_frames_4096_s"] = float(np.median(t))
        finally:
            r.close()
        t_render.append(t1 - t0); t_analysis.append(t2 - t1)
    res["render_s"], res["render_all_s"] = float(np.median(t_render)), t_render
    res["analysis_s"], res["analysis_all_s"] = float(np.median(t_analysis)), t_analysis
    res["analysis_spread"] = (max(t_analysis) - min(t_analysis)) / res["analysis_s"]
    dist = [c["harmonic_distance_db"] for c in comps if c["harmonic_distance_db"] is not None]
    res["harm_dist_mean_db"] = float(np.mean(dist)) if dist else None
    if not a.no_cpu:
        from multiprocessing import get_context
        k = min(a.cpu_pairs, a.pairs)
        idx = np.linspace(0, a.pairs - 1, k).astype(int)
        # the render side of a timed pair: a synthetic 24-bit clip (the restatement's cost does not depend on the samples)
        work = [(reals[i], np.round(ref.golden_clip(1000 + int(i), f0s[i] * 1.001, a.duration) * 8388607.0) / 8388608.0, f0s[i]) for i in idx]
        with get_context("spawn").Pool(min(a.threads, k)) as pool:
            pool.map(_cpu_pair, work[:min(a.threads, k)])          # start the workers, import numpy
            t0 = time.perf_counter(); pool.map(_cpu_pair, work, chunksize=1); dt = time.perf_counter() - t0
        res["cpu_s_timed"], res["cpu_pairs_timed"], res["cpu_threads"] = dt, k, min(a.threads, k)
        res["cpu_s_scaled"] = dt * a.pairs / k
    print(json.dumps(res))


if __name__ == "__main__":
    main()
