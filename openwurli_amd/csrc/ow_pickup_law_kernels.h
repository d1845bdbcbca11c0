// openwurli-hip: the pickup-law study of ml/h3_analysis_v2.py on the device (gfx950, f64): a sine reed through clip, a pickup law, the
// one-pole high-pass and a DFT probe per harmonic over the second half of the signal -- compute_harmonics (:58-94) and its two inline
// variants (:291-319, :346-375) for many (carrier, law) jobs per call.
//
//   k_pickup_law   a wavefront is one carrier and up to 64 law points of ONE kind, one lane per law.  The host sorts the laws by kind
//                  (stable) and cuts them into such chunks; blockIdx = carrier * n_chunks + chunk.
//
// Per tile of 64 samples lane j computes the carrier side of sample i0 + j once: y (sine, scale, clip) and, from n / 2 on, the
// (cos, sin) pair of each of the nh <= 8 harmonics -- at most 17 transcendentals.  It parks them in LDS as tile[value][sample] (17 x 64
// doubles: the 64 lanes write 64 consecutive doubles, no bank conflict).  Then every lane walks the tile's samples in order and reads
// each value as a same-address broadcast: per sample a lane is left with one pow (kind 0) or two divisions (kinds 1, 2), the three-term
// recurrence and 2 nh multiply-adds into register accumulators.  The kind is wave-uniform, so the walk has no divergent branch.  The
// tile is single-buffered: the wavefront is the workgroup, so filling and walking alternate within one instruction stream and the other
// wavefronts of the SIMD fill the gaps.  A lane's numbers never depend on the other lanes or on which chunk it sits in.
//
// Arithmetic: every operation that the reference states is one IEEE operation here (__dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn: never
// contracted), in the reference's order; sin, cos and pow are the device library's.  The DFT sums run in ascending k inside the lane
// (numpy sums pairwise).  y_peak is a max: exact in any order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace owdev {

constexpr int PL_TILE = 64;            // samples per tile = lanes per wavefront
constexpr int PL_MAX_H = 8;            // OW_MAX_HARMONICS
constexpr int PL_VALUES = 1 + 2 * PL_MAX_H;

struct OwPlChunkDev {                  // one wavefront's share of the laws, sorted by kind
    uint32_t kind, first, count, pad;
};

// the law on one clipped displacement y, |y| <= clip < 1
template <int KIND> __device__ inline double pl_law(double y, double p, double one_minus_p) {
    const double g = __dsub_rn(1.0, y);
    // p == 1: the law in use, which the k = 0 and blend = 0 points restate.  The host's pow returns g itself there; the device library's
    // is within an ulp of g, not always on it (measured: amplitudes 1 to 3 ulps apart), so the exact case is taken by a select.
    if (KIND == 0) return __ddiv_rn(y, p == 1.0 ? g : pow(g, p));
    const double asym = __ddiv_rn(y, g);
    if (KIND == 1) return __dmul_rn(asym, __dadd_rn(1.0, __dmul_rn(p, y)));
    const double sym = __ddiv_rn(y, __dsub_rn(1.0, __dmul_rn(y, y)));
    return __dadd_rn(__dmul_rn(one_minus_p, asym), __dmul_rn(p, sym));
}

// the walk over `cnt` samples of the tile that starts at sample i0; `dft` (wave-uniform per sample) from sample `start` on
template <int KIND>
__device__ inline void pl_walk(const double* tile, int cnt, uint32_t i0, uint32_t start, int nh, double p, double one_minus_p, double sens, double b0,
                               double a1, double& xp, double& yp, double (&re)[PL_MAX_H], double (&im)[PL_MAX_H]) {
#pragma unroll 2
    for (int s = 0; s < cnt; ++s) {
        const double y = tile[s];
        const double v = __dmul_rn(pl_law<KIND>(y, p, one_minus_p), sens);
        const double out = __dadd_rn(__dsub_rn(__dmul_rn(b0, v), __dmul_rn(b0, xp)), __dmul_rn(a1, yp));
        xp = v;
        yp = out;
        if (i0 + (uint32_t)s >= start) {
#pragma unroll
            for (int h = 0; h < PL_MAX_H; ++h) {
                if (h < nh) {
                    re[h] = __dadd_rn(re[h], __dmul_rn(out, tile[(1 + 2 * h) * PL_TILE + s]));
                    im[h] = __dadd_rn(im[h], __dmul_rn(out, tile[(2 + 2 * h) * PL_TILE + s]));
                }
            }
        }
    }
}

// carriers: [n_carriers][3] = f0, ds, vel_scale.  params / dest: the laws in sorted order and the caller's index of each.
// amps: [n_carriers][n_laws][nh]; y_peak: [n_carriers] (written by chunk 0).
__global__ __launch_bounds__(PL_TILE) void k_pickup_law(const double* __restrict__ carriers, const OwPlChunkDev* __restrict__ chunks, uint32_t n_chunks,
                                                        const double* __restrict__ params, const uint32_t* __restrict__ dest, uint32_t n_laws, double sr,
                                                        uint32_t n, int nh, double sens, double clip, double b0, double a1,
                                                        double* __restrict__ amps, double* __restrict__ y_peak) {
    __shared__ double tile[PL_VALUES * PL_TILE];
    const uint32_t carrier = blockIdx.x / n_chunks, chunk = blockIdx.x - carrier * n_chunks;
    const OwPlChunkDev ck = chunks[chunk];
    const int lane = threadIdx.x;
    const bool live = (uint32_t)lane < ck.count;
    const uint32_t item = ck.first + (live ? (uint32_t)lane : 0u);      // an idle lane walks with the chunk's first law and writes nothing
    const double p = params[item], one_minus_p = __dsub_rn(1.0, p);
    const double f0 = carriers[3 * (size_t)carrier], ds = carriers[3 * (size_t)carrier + 1], vel_scale = carriers[3 * (size_t)carrier + 2];
    const double two_pi = __dmul_rn(2.0, 3.141592653589793);
    const double w0 = __dmul_rn(two_pi, f0);
    const uint32_t start = n / 2, quarter = n / 4, m = n - start;

    double re[PL_MAX_H], im[PL_MAX_H];
#pragma unroll
    for (int h = 0; h < PL_MAX_H; ++h) re[h] = im[h] = 0.0;
    double xp = 0.0, yp = 0.0, peak = 0.0;

    for (uint32_t i0 = 0; i0 < n; i0 += PL_TILE) {
        const uint32_t i = i0 + (uint32_t)lane;
        const int cnt = (int)min((uint32_t)PL_TILE, n - i0);
        __syncthreads();                                                // the previous walk has read the tile
        if (i < n) {
            const double t = __ddiv_rn((double)i, sr);
            const double reed = __dmul_rn(vel_scale, sin(__dmul_rn(w0, t)));
            const double y = fmin(fmax(__dmul_rn(reed, ds), -clip), clip);
            tile[lane] = y;
            if (i >= quarter) peak = fmax(peak, fabs(y));
            if (i >= start) {
                const double k = (double)(i - start);
#pragma unroll
                for (int h = 0; h < PL_MAX_H; ++h) {
                    if (h < nh) {
                        const double wh = __dmul_rn(two_pi, __dmul_rn((double)(h + 1), f0));
                        const double phase = __ddiv_rn(__dmul_rn(wh, k), sr);
                        double sn, cs;
                        sincos(phase, &sn, &cs);
                        tile[(1 + 2 * h) * PL_TILE + lane] = cs;
                        tile[(2 + 2 * h) * PL_TILE + lane] = sn;
                    }
                }
            }
        }
        __syncthreads();
        if (ck.kind == 0) pl_walk<0>(tile, cnt, i0, start, nh, p, one_minus_p, sens, b0, a1, xp, yp, re, im);
        else if (ck.kind == 1) pl_walk<1>(tile, cnt, i0, start, nh, p, one_minus_p, sens, b0, a1, xp, yp, re, im);
        else pl_walk<2>(tile, cnt, i0, start, nh, p, one_minus_p, sens, b0, a1, xp, yp, re, im);
    }

    if (chunk == 0) {                                                   // max |y| over i >= n / 4: the lanes' maxima, any order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) peak = fmax(peak, __shfl_xor(peak, off, 64));
        if (lane == 0) y_peak[carrier] = peak;
    }
    if (live) {
        double* row = amps + ((size_t)carrier * n_laws + dest[item]) * (size_t)nh;
        const double md = (double)m;
#pragma unroll
        for (int h = 0; h < PL_MAX_H; ++h) {
            if (h < nh) {
                const double r = __ddiv_rn(re[h], md), q = -__ddiv_rn(im[h], md);
                row[h] = __dmul_rn(2.0, sqrt(__dadd_rn(__dmul_rn(r, r), __dmul_rn(q, q))));
            }
        }
    }
}

}  // namespace owdev
