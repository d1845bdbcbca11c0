// openwurli-hip: the recording side of the ML loop (gfx950, f64): harmonics of recorded notes by a Goertzel bank
// (ml/goertzel_utils.py:34-57, goertzel_mag) and the inter-harmonic noise floor (ml/compute_residuals.py:59-127,
// measure_interharmonic_snr).
//
//   k_goertzel_quant     block = segment          the samples as a 24-bit WAV reads back (feat_wav24), written once per segment;
//                                                 launched only when a quantiser is asked for
//   k_goertzel           block = one wavefront = one segment; lane = recurrence (segment, bin k):
//                            s0 = (x + (coeff * s1)) - s2; s2 = s1; s1 = s0        over the N samples, three single IEEE operations
//                        (__dmul_rn / __dadd_rn / __dsub_rn: never contracted, whatever the build's flags say).  Returns (s1, s2);
//                        magnitude, the maximum over a harmonic's bins and the floors are the host's.
//                        All lanes of the wavefront share x[n]: the segment pointer is formed from blockIdx alone, so the samples
//                        arrive through scalar loads, OW_GOERTZEL_CHUNK of them per request, and sit in SGPRs.
//                        Recurrences per lane: a segment has at most 8 harmonics x 11 offsets = 88 distinct bins, so a lane carries
//                        two slots (recurrences lane and lane + 64) and one wavefront covers any segment.  A wavefront with at most
//                        64 recurrences runs the one-slot loop.  The chain is three dependent f64 operations per sample, each a
//                        quarter-rate instruction (16 lanes a cycle: 4 cycles of issue) with a result latency of about twice that,
//                        so one slot alone keeps the pipe at most half busy; the second slot fills it where a segment has the bins
//                        for it, and elsewhere the other wavefronts of the SIMD do: the kernel needs 20 VGPRs and no LDS, so
//                        eight wavefronts per SIMD are resident and three already cover the latency.  More slots per lane would only
//                        idle lanes: the lanes of a wavefront must share a segment, and a segment has no more recurrences to give.
//   k_feat_band_median   block = (segment, band), 4 wavefronts: |X_k| * 2 / N / 0.5 at EVERY bin of the band by the direct summation
//                        of k_feat_peaks (same windowed copy, same exact-phase twiddles re-seeded every OW_FEAT_RESEED steps), the
//                        magnitudes in LDS, np.median of them by rank counting (even count: mean of the two middle values).
//                        A band holds 0.08 f N / sr bins: about 260 at 22 kHz and N = 6615.  OW_BAND_MAX_BINS = 4096 (32 KB of LDS)
//                        is the limit; the host refuses a segment whose widest band exceeds it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ow_features.h"

namespace owdev {

struct OwGoertzelSegDev {
    uint64_t x_off;              // first sample of the segment in the source buffer (the audio, or the quantised copy)
    uint64_t q_off;              // where k_goertzel_quant puts its copy
    uint32_t n;                  // samples
    uint32_t rec0, n_rec;        // this segment's recurrences: coeff[rec0 .. rec0 + n_rec), n_rec <= 128
    uint32_t pad;
};

#define OW_GOERTZEL_CHUNK 8      // samples per scalar request
#define OW_GOERTZEL_MAX_REC 128  // two slots x 64 lanes
#define OW_BAND_MAX_BINS 4096    // bins of one noise band held in LDS

__global__ __launch_bounds__(256) void k_goertzel_quant(const double* __restrict__ audio, const OwGoertzelSegDev* __restrict__ segs,
                                                        double* __restrict__ xq, int wav24_mode) {
    const OwGoertzelSegDev s = segs[blockIdx.x];
    const double* x = audio + s.x_off;
    double* q = xq + s.q_off;
    for (uint32_t i = threadIdx.x; i < s.n; i += 256) q[i] = feat_wav24(x[i], wav24_mode);
}

__device__ inline double goertzel_step(double x, double coeff, double s1, double s2) {
    return __dsub_rn(__dadd_rn(x, __dmul_rn(coeff, s1)), s2);
}

// One wavefront's loop.  The samples of a chunk are requested while the chunk before it still has seven of its eight steps to run and
// are first touched behind those, so a request has that arithmetic to arrive behind.
template <bool TWO>
__device__ inline void goertzel_run(const double* __restrict__ x, uint32_t n, double ca, double cb, double* out) {
    double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
    auto step = [&](double v) {
        const double a0 = goertzel_step(v, ca, a1, a2);
        a2 = a1; a1 = a0;
        if (TWO) {
            const double b0 = goertzel_step(v, cb, b1, b2);
            b2 = b1; b1 = b0;
        }
    };
    const uint32_t n_chunks = n / OW_GOERTZEL_CHUNK;
    if (n_chunks) {
        double cur[OW_GOERTZEL_CHUNK], nxt[OW_GOERTZEL_CHUNK];
#pragma unroll
        for (int j = 0; j < OW_GOERTZEL_CHUNK; ++j) cur[j] = x[j];
        step(cur[0]);
        for (uint32_t c = 1; c < n_chunks; ++c) {
            const double* xn = x + (size_t)c * OW_GOERTZEL_CHUNK;
#pragma unroll
            for (int j = 0; j < OW_GOERTZEL_CHUNK; ++j) nxt[j] = xn[j];
            __builtin_amdgcn_sched_barrier(0);      // the request stays in front of the arithmetic it hides behind
#pragma unroll
            for (int j = 1; j < OW_GOERTZEL_CHUNK; ++j) step(cur[j]);
            step(nxt[0]);
#pragma unroll
            for (int j = 1; j < OW_GOERTZEL_CHUNK; ++j) cur[j] = nxt[j];
        }
#pragma unroll
        for (int j = 1; j < OW_GOERTZEL_CHUNK; ++j) step(cur[j]);
    }
    for (uint32_t i = n_chunks * OW_GOERTZEL_CHUNK; i < n; ++i) step(x[i]);
    out[0] = a1; out[1] = a2; out[2] = b1; out[3] = b2;
}

// src: the audio or the quantised copy; out[rec] = (s1, s2)
__global__ __launch_bounds__(64) void k_goertzel(const double* __restrict__ src, const OwGoertzelSegDev* __restrict__ segs, int use_q,
                                                 const double* __restrict__ coeff, double2* __restrict__ out) {
    const OwGoertzelSegDev s = segs[blockIdx.x];
    const double* x = src + (use_q ? s.q_off : s.x_off);     // wave-uniform: blockIdx and kernel arguments only
    const uint32_t lane = threadIdx.x;
    const bool has_a = lane < s.n_rec, has_b = lane + 64 < s.n_rec;
    const double ca = has_a ? coeff[s.rec0 + lane] : 0.0;
    const double cb = has_b ? coeff[s.rec0 + lane + 64] : 0.0;
    double r[4];
    if (s.n_rec > 64) goertzel_run<true>(x, s.n, ca, cb, r);
    else goertzel_run<false>(x, s.n, ca, cb, r);
    if (has_a) out[s.rec0 + lane] = make_double2(r[0], r[1]);
    if (has_b) out[s.rec0 + lane + 64] = make_double2(r[2], r[3]);
}

struct OwBandDev {               // one per (segment, band)
    uint32_t seg;
    uint32_t k_lo, k_hi;         // inclusive bin range, at most OW_BAND_MAX_BINS bins; k_lo > k_hi: no band (the host reports 1e-20)
    uint32_t pad;
};

__global__ __launch_bounds__(256) void k_feat_band_median(const OwSegDev* __restrict__ segs, const OwBandDev* __restrict__ bands,
                                                          const double* __restrict__ xw, double* __restrict__ medians) {
    __shared__ double mag[OW_BAND_MAX_BINS];
    __shared__ double mid[2];
    const OwBandDev b = bands[blockIdx.x];
    if (threadIdx.x < 2) mid[threadIdx.x] = __longlong_as_double(0x7FF8000000000000ll);   // a NaN among the magnitudes leaves it: np.median's answer
    if (b.k_lo > b.k_hi) {                                   // block-uniform
        if (threadIdx.x == 0) medians[blockIdx.x] = 0.0;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const OwSegDev s = segs[b.seg];
    const double* x = xw + s.xw_off;
    const uint64_t nfft = 4ull * s.n;
    const uint32_t nb = min(b.k_hi - b.k_lo + 1, (uint32_t)OW_BAND_MAX_BINS);
    const double N = (double)s.n;
    // as k_feat_peaks: bins dealt to the 4 wavefronts in groups of OW_FEAT_J, lanes stride over n
    for (uint32_t g0 = wave * OW_FEAT_J; g0 < nb; g0 += 4 * OW_FEAT_J) {
        double wr[OW_FEAT_J], wi[OW_FEAT_J], sr[OW_FEAT_J], si[OW_FEAT_J], ar[OW_FEAT_J], ai[OW_FEAT_J];
        uint64_t kk[OW_FEAT_J];
#pragma unroll
        for (int j = 0; j < OW_FEAT_J; ++j) {
            kk[j] = b.k_lo + min(g0 + j, nb - 1);            // the tail group repeats its last bin (not stored)
            feat_twiddle(kk[j], 64, nfft, sr[j], si[j]);
            ar[j] = 0.0; ai[j] = 0.0;
        }
        uint32_t step = 0;
        for (uint32_t n = lane; n < s.n; n += 64, ++step) {
            if ((step % OW_FEAT_RESEED) == 0) {
#pragma unroll
                for (int j = 0; j < OW_FEAT_J; ++j) feat_twiddle(kk[j], n, nfft, wr[j], wi[j]);
            }
            const double v = x[n];
#pragma unroll
            for (int j = 0; j < OW_FEAT_J; ++j) {
                ar[j] += v * wr[j];
                ai[j] += v * wi[j];
                const double t = wr[j] * sr[j] - wi[j] * si[j];
                wi[j] = wr[j] * si[j] + wi[j] * sr[j];
                wr[j] = t;
            }
        }
#pragma unroll
        for (int j = 0; j < OW_FEAT_J; ++j) {
            double re = ar[j], im = ai[j];
            for (int o = 32; o > 0; o >>= 1) { re += __shfl_xor(re, o); im += __shfl_xor(im, o); }
            if (lane == 0 && g0 + j < nb) mag[g0 + j] = hypot(re, im) * 2.0 / N / 0.5;   // np.abs(rfft) * 2.0 / N / 0.5
        }
    }
    __syncthreads();
    // np.median: the element of rank (nb - 1) / 2 and the one of rank nb / 2 in the sorted order (ties ordered by index), their mean
    const uint32_t r_lo = (nb - 1) / 2, r_hi = nb / 2;
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        const double m = mag[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < nb; ++j) {
            const double o = mag[j];
            rank += (o < m || (o == m && j < i)) ? 1u : 0u;
        }
        if (rank == r_lo) mid[0] = m;
        if (rank == r_hi) mid[1] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) medians[blockIdx.x] = r_lo == r_hi ? mid[0] : (mid[0] + mid[1]) / 2.0;
}

}  // namespace owdev
