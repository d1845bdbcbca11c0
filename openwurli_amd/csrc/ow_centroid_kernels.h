// openwurli-hip: the analysis stage of `preamp-bench centroid-track` (tools/preamp-bench/src/main.rs:1925-2135): the spectral centroid
// of many short Hann frames of many rows, one workgroup per (row, frame).
//
// spectral_centroid (:1931-1958) is a brute-force DFT: for every bin k of k_min..=k_max it walks the frame's N windowed samples in
// order, forms phase = 2.0 * PI * k * i / N left to right and accumulates re += s * cos(phase), im -= s * sin(phase); the bins'
// |X_k|^2 are then added in ascending k, weighted by their frequency.  Here a thread is a bin, so every accumulation keeps the
// reference's order and operands; the only differences to the host are the device's sin / cos.  The frame is staged once through LDS
// (x * hann, the product the reference forms before the DFT, :2050-2054) and every thread reads it front to back: all lanes of a wave
// read the same address, which the LDS serves as a broadcast.  What bounds the kernel is the f64 sincos per (bin, sample): about a
// hundred instructions, most of them f64, against one LDS read, one division and four f64 operations of the DFT itself (DESIGN.md,
// section 10, centroid-track).
#pragma once
#include "ow_voice_dev.h"

namespace owdev {

struct OwCentroidGrid {        // the frame grid of a call, formed on the host (api_centroid.inc)
    uint32_t window;           // N = window_samples, 1..OW_CENTROID_MAX_WINDOW
    uint32_t hop;              // hop_samples >= 1
    uint32_t frames;           // frames per row
    uint32_t k_min, k_max;     // bins, k_min <= k_max <= N / 2
    uint32_t row0;             // first row of this launch (rows beyond 65 535 take further launches)
    double freq_resolution;    // 44100 / N, the host's IEEE quotient
};

// signals: [rows][stride]; hann: [N], the command's periodic form 0.5 * (1 - cos(2 pi i / N)) from the host (its libm's bits);
// frames: [rows][frames].  grid = (frames, rows of the launch); dynamic LDS = (N + bins) doubles.  A frame j covers samples
// [j * hop, j * hop + N), which the host has checked to end inside the row (pos + N <= len <= stride).
__global__ __launch_bounds__(256) void k_centroid_frames(const double* __restrict__ signals, size_t stride, const double* __restrict__ hann,
                                                         OwCentroidGrid g, double* __restrict__ frames) {
    extern __shared__ double cf_lds[];
    double* xs = cf_lds;                  // [N] windowed frame
    double* mag = cf_lds + g.window;      // [bins] mag_sq per bin
    const uint32_t N = g.window;
    const size_t row = (size_t)g.row0 + blockIdx.y;
    const double* x = signals + row * stride + (size_t)blockIdx.x * g.hop;
    for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) xs[i] = x[i] * hann[i];
    __syncthreads();
    const double n_f = (double)N;
    for (uint32_t k = g.k_min + threadIdx.x; k <= g.k_max; k += blockDim.x) {
        const double two_pi_k = 2.0 * 3.14159265358979323846 * (double)k;       // 2.0 * PI * k as f64 ...
        double re = 0.0, im = 0.0;
        for (uint32_t i = 0; i < N; ++i) {
            const double s = xs[i];
            const double phase = ow_div(two_pi_k * (double)i, n_f);             // ... * i as f64 / n as f64
            double sn, cs;
            sincos(phase, &sn, &cs);                                            // one argument reduction for the pair
            re += s * cs;
            im -= s * sn;
        }
        mag[k - g.k_min] = re * re + im * im;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double weighted_sum = 0.0, power_sum = 0.0;
        for (uint32_t k = g.k_min; k <= g.k_max; ++k) {                         // ascending k, the reference's order
            const double mag_sq = mag[k - g.k_min];
            weighted_sum += ((double)k * g.freq_resolution) * mag_sq;
            power_sum += mag_sq;
        }
        // a plain comparison: a NaN power takes the else branch, as in the reference
        frames[row * g.frames + blockIdx.x] = power_sum > 0.0 ? weighted_sum / power_sum : 0.0;
    }
}

}  // namespace owdev
