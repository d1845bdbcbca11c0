// openwurli-hip: analysis kernels of the note audits (`preamp-bench intermod-audit --render` and `overshoot`,
// tools/preamp-bench/src/main.rs:822-903, 2147-2239).  Both commands look at Voice::render_note's output alone: k_job_voice leaves the
// rows in HBM, the kernels here reduce them to a few sums per row, the host finishes (division, sqrt, dB, verdicts).
//
//   k_dft_probes    dft_magnitude's (re, im) sums (:893-903) of one window of every row at up to n_probes frequencies per row.
//                   Workgroup = (probe, row); the 256 threads stride over the window, each sample costs one f64 sincos.  Bound by that
//                   sincos, not by memory: a row's window (66 150 samples = 529 KB) is read once per probe and stays in L2 meanwhile.
//   k_window_stats  max |x| or the sum of x^2 over up to four windows of every row.  Workgroup = (window, row).
// Both reduce through one fixed LDS tree, so a (row, probe) or (row, window) gives the same bits wherever it runs; no atomics.
#pragma once
#include "ow_pbench_kernels.h"

namespace owdev {

#define OW_NA_THREADS 256

// sh[0] = sum of the 256 per-thread values in a fixed order: (t, t + 128), then (t, t + 64), ... (t, t + 1)
OW_DEV double na_tree_sum(double* sh, double v) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = OW_NA_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();                                           // sh is reused by the caller's next reduction
    return r;
}

// sig [rows][stride]; freqs [rows][n_probes], NaN = no probe (nothing is computed or written for it); sums [rows][n_probes][2] = (re, im) of
//   for (i, s) in sig[row][start..start + n]: phase = 2.0 * PI * freq * i as f64 / sr; re += s * phase.cos(); im -= s * phase.sin()
// with the terms of thread t (i = t, t + 256, ...) added in ascending i, then the tree.  blockIdx.y + row0 = row.
__global__ __launch_bounds__(OW_NA_THREADS) void k_dft_probes(const double* __restrict__ sig, size_t stride, size_t start, size_t n, double sr,
                                                              const double* __restrict__ freqs, uint32_t n_probes, uint32_t row0,
                                                              double* __restrict__ sums) {
    __shared__ double sh[OW_NA_THREADS];
    const size_t row = (size_t)row0 + blockIdx.y;
    const size_t slot = row * n_probes + blockIdx.x;
    const double freq = freqs[slot];
    if (freq != freq) return;                                  // the whole workgroup: no barrier is left waiting
    const double* __restrict__ x = sig + row * stride + start;
    const double tpf = OW_PB_TWO_PI * freq;
    double re = 0.0, im = 0.0;
    for (size_t i = threadIdx.x; i < n; i += OW_NA_THREADS) {
        double sn, cs;
        sincos(tpf * (double)i / sr, &sn, &cs);
        const double s = x[i];
        re += s * cs;
        im -= s * sn;
    }
    re = na_tree_sum(sh, re);
    im = na_tree_sum(sh, im);
    if (threadIdx.x == 0) {
        sums[2 * slot] = re;
        sums[2 * slot + 1] = im;
    }
}

enum { NA_WIN_PEAK = 0, NA_WIN_SUM_SQ = 1 };
#define OW_NA_MAX_WINDOWS 4
struct OwNaWindows {                        // per call; the host has clamped every edge to the rows' length, end >= start
    uint32_t start[OW_NA_MAX_WINDOWS], end[OW_NA_MAX_WINDOWS], kind[OW_NA_MAX_WINDOWS];
    uint32_t count, row0;
};

// out [rows][count]: NA_WIN_PEAK: signal[start..end].iter().map(|x| x.abs()).fold(0.0, f64::max) -- f64::max returns the other operand
// when one is NaN, as fmax does, so NaN samples are ignored and an empty window gives 0; NA_WIN_SUM_SQ: the sum of x * x, thread t adding
// its samples (start + t, start + t + 256, ...) in ascending order, then the tree.  blockIdx.x = window, blockIdx.y + row0 = row.
__global__ __launch_bounds__(OW_NA_THREADS) void k_window_stats(const double* __restrict__ sig, size_t stride, OwNaWindows w, double* __restrict__ out) {
    __shared__ double sh[OW_NA_THREADS];
    const size_t row = (size_t)w.row0 + blockIdx.y;
    const uint32_t k = blockIdx.x;
    const double* __restrict__ x = sig + row * stride;
    const uint32_t e = w.end[k];
    double r;
    if (w.kind[k] == NA_WIN_PEAK) {
        double pk = 0.0;
        for (uint32_t i = w.start[k] + threadIdx.x; i < e; i += OW_NA_THREADS) pk = fmax(pk, fabs(x[i]));
        const int t = threadIdx.x;
        sh[t] = pk;
        __syncthreads();
#pragma unroll
        for (int s = OW_NA_THREADS / 2; s > 0; s >>= 1) {
            if (t < s) sh[t] = fmax(sh[t], sh[t + s]);
            __syncthreads();
        }
        r = sh[0];
    } else {
        double acc = 0.0;
        for (uint32_t i = w.start[k] + threadIdx.x; i < e; i += OW_NA_THREADS) acc += x[i] * x[i];
        r = na_tree_sum(sh, acc);
    }
    if (threadIdx.x == 0) out[row * w.count + k] = r;
}

}  // namespace owdev
