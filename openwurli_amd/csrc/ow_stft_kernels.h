// openwurli-hip: the analysis of tools/wurli_compare.py (compute_stft :46-58 and its two callers :61-78, :122-127; the RMS envelopes
// :95-107, :136-147, :130-133) for many clips per call (gfx950, f64).
//
//   k_stft_twiddles  tw[t] = e^{-2 pi i t / N}, t = 0..N/2, each from its exact integer phase through sincospi (as feat_twiddle)
//   k_stft_frames    block = (frame, clip): the N-point real transform of frame * window as an M = N/2-point complex f64 FFT in LDS,
//                    then the split step to X_0..X_M; |X_k| to the scratch rows (if asked), the frame's centroid to cent[]
//   k_stft_reduce    thread = (clip, bin): the mean over the clip's frames, frames added in ascending order; bin M + 1 = the centroid
//   k_frame_rms      block = (frame, clip): sqrt(sum v^2 / frame_len)
//   k_clip_sum_sq    block = clip: sum v^2 over the whole clip
//
// Numerical contract (openwurli_hip.h, ow_stft_profile): the reference holds float32, so every sample is first rounded to float32
// (after the optional 24-bit quantiser) and the product frame * window is one rounded float32 multiplication; everything after that
// is f64.  Sums run per thread over strided ascending indices and are then joined by a tree whose shape depends only on blockDim;
// no atomics anywhere.
//
// The FFT is an in-place decimation in frequency: one radix-2 pass when log2 M is odd, then radix-4 passes down to L = 4.  A pass over
// blocks of length L takes x[j + q L/r], forms the r-point DFT, multiplies output p by W_L^{jp} = tw[j p N/L] and stores it at
// j + p L/r, so that bin k ends at stft_pos(k), the mixed-radix digit reversal.  LDS holds double2 (one ds_read_b128 / ds_write_b128
// per element); element i lives at slot i + (i >> 4): the 256-byte bank row takes 16 elements, and the skew moves every next row by
// one 16-byte slot, so that the strides 4, 16, 64, .. elements of the late passes spread over the row instead of landing on one slot.
// 8192 real points are 4096 + 256 slots = 68 KiB: two workgroups per CU.
#pragma once
#include "ow_features.h"

namespace owdev {

constexpr uint32_t STFT_MIN_FFT = 64, STFT_MAX_FFT = 8192;      // n_fft: a power of two in this range (the largest: 68 KiB of LDS)

struct OwStftGrid {             // one launch, formed on the host (api_compare.inc)
    uint32_t n_fft, log2_m;     // N; log2(N / 2)
    uint32_t hop;
    uint32_t clip0;             // first clip of this launch
    int wav24_mode;
    int want_mag;               // mags != nullptr
    double freq_val;            // numpy's rfftfreq step 1.0 / (N * (1.0 / sr))
};

__device__ __forceinline__ uint32_t stft_slot(uint32_t i) { return i + (i >> 4); }
inline size_t stft_lds_bytes(uint32_t n_fft) { return sizeof(double2) * ((size_t)(n_fft / 2) + (n_fft / 32)); }

// where bin k of the M-point transform lies after the passes
__device__ __forceinline__ uint32_t stft_pos(uint32_t k, uint32_t log2_m) {
    uint32_t span = 1u << log2_m, pos = 0;
    if (log2_m & 1u) { span >>= 1; pos = (k & 1u) * span; k >>= 1; }
    while (span > 1u) { span >>= 2; pos += (k & 3u) * span; k >>= 2; }
    return pos;
}
// e^{-2 pi i t / N} for t < N from the half table (tw[t + N/2] = -tw[t])
__device__ __forceinline__ double2 stft_tw(const double2* __restrict__ tw, uint32_t t, uint32_t half_n) {
    if (t >= half_n) { const double2 w = tw[t - half_n]; return make_double2(-w.x, -w.y); }
    return tw[t];
}
__device__ __forceinline__ double2 stft_cmul(double2 a, double2 w) { return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
// the float32 the reference analyses: its 24-bit file (or the sample) read as float32
__device__ __forceinline__ float stft_sample(const double* __restrict__ x, uint32_t i, uint32_t len, int wav24_mode) {
    return i < len ? (float)feat_wav24(x[i], wav24_mode) : 0.0f;
}
// joins the threads' partial sums: wavefront butterfly, then the wavefronts' sums in ascending order; every thread gets the total
__device__ __forceinline__ double stft_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                       // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (uint32_t w = 0; w < (blockDim.x + 63) / 64; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(256) void k_stft_twiddles(double2* __restrict__ tw, uint32_t n_fft) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_fft / 2) return;
    double s, c;
    sincospi(-2.0 * ((double)t / (double)n_fft), &s, &c);
    tw[t] = make_double2(c, s);
}

// clips: [n_clips][stride]; lengths, n_frames, frame_off: per clip (frame_off = the clip's first row in mags / cent, relative to the
// launch's chunk); window: [N] (float32 values widened); tw: [N/2 + 1]; mags: [frames of the chunk][M + 1] or nullptr; cent: [frames of
// the chunk].  grid = (most frames of a clip in the launch, clips of the launch); dynamic LDS = stft_lds_bytes(N).  Nothing at or beyond
// lengths[c] is read.
__global__ __launch_bounds__(256) void k_stft_frames(const double* __restrict__ clips, size_t stride, const uint32_t* __restrict__ lengths,
                                                     const uint32_t* __restrict__ n_frames, const uint64_t* __restrict__ frame_off,
                                                     const double* __restrict__ window, const double2* __restrict__ tw, OwStftGrid g,
                                                     double* __restrict__ mags, double* __restrict__ cent) {
    extern __shared__ double2 stft_lds[];
    __shared__ double red[4];
    const uint32_t c = g.clip0 + blockIdx.y, frame = blockIdx.x;
    if (frame >= n_frames[c]) return;                       // uniform over the block
    const uint32_t N = g.n_fft, M = N >> 1, len = lengths[c];
    const double* x = clips + (size_t)c * stride;
    const uint64_t start = (uint64_t)frame * g.hop;
    const uint32_t avail = start < len ? (uint32_t)(len - start) : 0u;       // valid samples of this frame, zero-padded past them
    for (uint32_t n = threadIdx.x; n < M; n += blockDim.x) {
        const float a = stft_sample(x + start, 2 * n, avail, g.wav24_mode) * (float)window[2 * n];
        const float b = stft_sample(x + start, 2 * n + 1, avail, g.wav24_mode) * (float)window[2 * n + 1];
        stft_lds[stft_slot(n)] = make_double2((double)a, (double)b);
    }
    __syncthreads();
    uint32_t L = M;
    if (g.log2_m & 1u) {                                    // radix 2: W_M^j = tw[2 j]
        const uint32_t H = M >> 1;
        for (uint32_t j = threadIdx.x; j < H; j += blockDim.x) {
            const double2 a = stft_lds[stft_slot(j)], b = stft_lds[stft_slot(j + H)];
            stft_lds[stft_slot(j)] = make_double2(a.x + b.x, a.y + b.y);
            stft_lds[stft_slot(j + H)] = stft_cmul(make_double2(a.x - b.x, a.y - b.y), tw[2 * j]);
        }
        __syncthreads();
        L = H;
    }
    for (; L >= 4; L >>= 2) {                               // radix 4 over blocks of length L
        const uint32_t Q = L >> 2, tstep = N / L;
        for (uint32_t i = threadIdx.x; i < (M >> 2); i += blockDim.x) {
            const uint32_t j = i & (Q - 1), base = (i - j) * 4 + j;
            const double2 a = stft_lds[stft_slot(base)], b = stft_lds[stft_slot(base + Q)];
            const double2 cc = stft_lds[stft_slot(base + 2 * Q)], d = stft_lds[stft_slot(base + 3 * Q)];
            const double2 t0 = make_double2(a.x + cc.x, a.y + cc.y), t1 = make_double2(a.x - cc.x, a.y - cc.y);
            const double2 t2 = make_double2(b.x + d.x, b.y + d.y), t3 = make_double2(b.y - d.y, d.x - b.x);       // -i (b - d)
            const uint32_t t = j * tstep;
            stft_lds[stft_slot(base)] = make_double2(t0.x + t2.x, t0.y + t2.y);
            stft_lds[stft_slot(base + Q)] = stft_cmul(make_double2(t1.x + t3.x, t1.y + t3.y), stft_tw(tw, t, M));
            stft_lds[stft_slot(base + 2 * Q)] = stft_cmul(make_double2(t0.x - t2.x, t0.y - t2.y), stft_tw(tw, 2 * t, M));
            stft_lds[stft_slot(base + 3 * Q)] = stft_cmul(make_double2(t1.x - t3.x, t1.y - t3.y), stft_tw(tw, 3 * t, M));
        }
        __syncthreads();
    }
    // split: X_k = E + W_N^k O with E = (Z_k + conj Z_{M-k}) / 2, O = -i (Z_k - conj Z_{M-k}) / 2, Z_M = Z_0
    double* mag_row = g.want_mag ? mags + (frame_off[c] + frame) * (uint64_t)(M + 1) : nullptr;
    double weighted = 0.0, power = 0.0;
    for (uint32_t k = threadIdx.x; k <= M; k += blockDim.x) {
        const double2 zk = stft_lds[stft_slot(stft_pos(k & (M - 1), g.log2_m))];
        const double2 zm = stft_lds[stft_slot(stft_pos((M - k) & (M - 1), g.log2_m))];
        const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
        const double2 o = make_double2(0.5 * (zk.y + zm.y), 0.5 * (zm.x - zk.x));
        const double2 wo = stft_cmul(o, tw[k]);
        const double re = e.x + wo.x, im = e.y + wo.y;
        const double m = sqrt(re * re + im * im);
        if (mag_row) mag_row[k] = m;
        const double p = m * m;
        weighted += ((double)k * g.freq_val) * p;
        power += p;
    }
    weighted = stft_block_sum(weighted, red);
    power = stft_block_sum(power, red);
    if (threadIdx.x == 0) cent[frame_off[c] + frame] = weighted / (power + 1e-10);
}

// mean_mag: [n_clips][M + 1] or nullptr, centroid: [n_clips] or nullptr (both indexed by the call's clip).  grid = (ceil((M + 2) / 256),
// clips of the launch): thread k <= M takes a bin, thread M + 1 the centroid.
__global__ __launch_bounds__(256) void k_stft_reduce(const double* __restrict__ mags, const double* __restrict__ cent,
                                                     const uint32_t* __restrict__ n_frames, const uint64_t* __restrict__ frame_off, uint32_t clip0,
                                                     uint32_t m, double* __restrict__ mean_mag, double* __restrict__ centroid) {
    const uint32_t c = clip0 + blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nf = n_frames[c];
    const uint64_t f0 = frame_off[c];
    if (k <= m && mean_mag) {
        double s = 0.0;
        for (uint32_t f = 0; f < nf; ++f) s += mags[(f0 + f) * (uint64_t)(m + 1) + k];
        mean_mag[(size_t)c * (m + 1) + k] = s / (double)nf;
    } else if (k == m + 1 && centroid) {
        double s = 0.0;
        for (uint32_t f = 0; f < nf; ++f) s += cent[f0 + f];
        centroid[c] = s / (double)nf;
    }
}

// rms: [clips of the launch][frames_stride], written for frame < n_frames[c].  grid = (most frames of a clip in the launch, clips)
__global__ __launch_bounds__(256) void k_frame_rms(const double* __restrict__ clips, size_t stride, const uint32_t* __restrict__ lengths,
                                                   const uint32_t* __restrict__ n_frames, uint32_t clip0, uint32_t frame_len, uint32_t hop,
                                                   int wav24_mode, double* __restrict__ rms, size_t frames_stride) {
    __shared__ double red[4];
    const uint32_t c = clip0 + blockIdx.y, frame = blockIdx.x;
    if (frame >= n_frames[c]) return;
    const uint32_t len = lengths[c];
    const uint64_t start = (uint64_t)frame * hop;
    const uint32_t avail = start < len ? (uint32_t)(len - start < frame_len ? len - start : frame_len) : 0u;
    const double* x = clips + (size_t)c * stride + start;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < avail; i += blockDim.x) {
        const double v = (double)stft_sample(x, i, avail, wav24_mode);
        acc += v * v;
    }
    acc = stft_block_sum(acc, red);
    if (threadIdx.x == 0) rms[(size_t)blockIdx.y * frames_stride + frame] = sqrt(acc / (double)frame_len);
}

// sum_sq: [n_clips] (indexed by the call's clip).  grid = clips of the launch
__global__ __launch_bounds__(256) void k_clip_sum_sq(const double* __restrict__ clips, size_t stride, const uint32_t* __restrict__ lengths,
                                                     uint32_t clip0, int wav24_mode, double* __restrict__ sum_sq) {
    __shared__ double red[4];
    const uint32_t c = clip0 + blockIdx.x, len = lengths[c];
    const double* x = clips + (size_t)c * stride;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) {
        const double v = (double)stft_sample(x, i, len, wav24_mode);
        acc += v * v;
    }
    acc = stft_block_sum(acc, red);
    if (threadIdx.x == 0) sum_sq[c] = acc;
}

}  // namespace owdev
