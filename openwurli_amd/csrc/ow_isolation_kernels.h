// openwurli-hip: recorded-note intake (gfx950, f64): the pairwise isolation sub-scores of ml/score_isolation.py:36-167 (score_temporal,
// score_harmonic_collision, score_energy_dominance) and the clip bounds of ml/extract_notes.py:43-64 (detect_obm_onset / detect_obm_offset).
//
//   k_isolation_score    block = one wavefront = 64 targets of ONE file; lane = target.  Every lane walks the file's notes from the first
//                        to the last in the same loop, so `score -= ...` and `total_energy += ...` run in the reference's list order:
//                        f64 rounding fixes that order, hence no tree reduction and no split of the others across lanes.
//                        The other's record is addressed by the loop counter and by the wave's table entry (blockIdx) alone, so it is
//                        wave-uniform: it arrives through scalar loads and sits in SGPRs; the next record is requested before the
//                        current one is worked on.  The three cases of an other (held, released, neither) diverge per lane: the
//                        compiler predicates the short held case and branches round the released case when no lane of the wavefront is
//                        in it (that case holds the kernel's only transcendental, pow(10.0, x), twice: at window_start for temporal and
//                        collision, at the window's midpoint for dominance).  Accumulations are written with __dmul_rn / __dadd_rn /
//                        __dsub_rn: single rounded operations whatever the build's contraction flag says.
//                        Nothing else is transcendental here: the decay rate 0.26 * exp(0.049 * midi) comes with the other's record (the
//                        host gathers it from the caller's 128-entry table), and harmonic_collision_check depends on the two MIDI
//                        numbers only: a 128 x 128 table of 8-bit masks, BUILT ON THE HOST (api_isolation.inc: iso_collision_table;
//                        multiply, divide, max, min and compare on the caller's 128 frequencies) and read here as table[other][target],
//                        so the lanes of a wavefront read one 128-byte row.  A target's mask is the AND over its energetic others.
//   k_clip_bounds        block = clip, 256 threads, two passes: peak = max |x|, then the first index with |x| > onset_frac * peak and the
//                        last index >= 1 with |x| > offset_frac * peak (-1: none).  Exact: a max and two index reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace owdev {

struct OwIsoNoteDev {            // 64 bytes; read per lane as a target, through scalar loads as an other
    double onset, offset, amp;
    double rate;                 // decay rate of this note as an other, dB / s
    double ws, we;               // analysis window of this note as a target
    int64_t key;                 // equal id strings, equal keys
    int32_t midi;                // 0..127
    int32_t score;               // 0: not a target
};

struct OwIsoWaveDev {            // one per wavefront
    uint32_t first, end;         // the file's notes [first, end)
    uint32_t base;               // targets base .. base + 63, clipped to end
    uint32_t pad;
};

__device__ inline double iso_remaining(double rate, double t) {
    if (t <= 0.0) return 1.0;
    const double decay_db = __dmul_rn(rate, t);
    return pow(10.0, -decay_db / 20.0);
}

__global__ __launch_bounds__(64) void k_isolation_score(const OwIsoNoteDev* __restrict__ notes, const OwIsoWaveDev* __restrict__ waves,
                                                        const uint8_t* __restrict__ table, double* __restrict__ temporal,
                                                        double* __restrict__ dominance, uint8_t* __restrict__ mask_out) {
    const OwIsoWaveDev w = waves[blockIdx.x];                 // wave-uniform
    const uint32_t ti = w.base + threadIdx.x;
    const bool live = ti < w.end;
    const OwIsoNoteDev t = notes[live ? ti : w.first];        // an idle lane follows the file's first note and stores nothing
    const double t_amp = t.amp;
    const double t_floor = 1e-6 > t_amp ? 1e-6 : t_amp;       // max(target["amplitude"], 1e-6)
    const double mid = (t.ws + t.we) / 2.0;
    double score = 1.0, total = t_amp;
    uint32_t mask = 0xFFu;
    OwIsoNoteDev nxt = notes[w.first];
    for (uint32_t j = w.first; j < w.end; ++j) {
        const OwIsoNoteDev o = nxt;
        nxt = notes[j + 1 < w.end ? j + 1 : j];               // uniform address: a scalar request, ahead of the arithmetic below
        const uint32_t m = table[(uint32_t)o.midi * 128u + (uint32_t)t.midi];
        if (o.key == t.key) continue;
        if (o.onset < t.we && o.offset > t.ws) {              // held during the window
            const double rel = o.amp / t_floor;
            if (rel > 0.1) score = __dsub_rn(score, __dmul_rn(0.10, 1.0 < rel ? 1.0 : rel));
            mask &= m;
            total = __dadd_rn(total, o.amp);
        } else if (o.offset < t.ws) {                         // released before the window, still decaying
            const double at_start = iso_remaining(o.rate, t.ws - o.offset);
            const double e = __dmul_rn(at_start, o.amp);
            const double rel = e / t_floor;
            if (rel > 0.1) score = __dsub_rn(score, __dmul_rn(0.10, 1.0 < rel ? 1.0 : rel));
            if (e > 0.05) mask &= m;
            const double at_mid = iso_remaining(o.rate, mid - o.offset);
            total = __dadd_rn(total, __dmul_rn(at_mid, o.amp));
        }
    }
    if (live && t.score) {
        temporal[ti] = score > 0.05 ? score : 0.05;           // max(0.05, score)
        dominance[ti] = total < 1e-10 ? 1.0 : t_amp / total;
        mask_out[ti] = (uint8_t)mask;
    }
}

#define OW_CLIP_THREADS 256

// the block's maximum (IS_MAX) or minimum of v, in every thread
template <bool IS_MAX, class T>
__device__ inline T clip_block_reduce(T v, T* sh) {
    for (int o = 32; o > 0; o >>= 1) {
        const T u = __shfl_xor(v, o);
        v = IS_MAX ? (u > v ? u : v) : (u < v ? u : v);
    }
    __syncthreads();                                          // sh may still be read from the reduction before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = sh[0];
    for (int k = 1; k < OW_CLIP_THREADS / 64; ++k) r = IS_MAX ? (sh[k] > r ? sh[k] : r) : (sh[k] < r ? sh[k] : r);
    return r;
}

// clips: [n_clips][stride], lengths[c] <= stride samples of row c are audio
__global__ __launch_bounds__(OW_CLIP_THREADS) void k_clip_bounds(const double* __restrict__ clips, size_t stride, const uint32_t* __restrict__ lengths,
                                                                 double onset_frac, double offset_frac, double* __restrict__ peak_out,
                                                                 long long* __restrict__ first_out, long long* __restrict__ last_out) {
    __shared__ double sh_d[OW_CLIP_THREADS / 64];
    __shared__ long long sh_i[OW_CLIP_THREADS / 64];
    const double* x = clips + (size_t)blockIdx.x * stride;
    const uint32_t n = lengths[blockIdx.x];
    double pk = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += OW_CLIP_THREADS) {
        const double a = fabs(x[i]);
        pk = a > pk ? a : pk;
    }
    const double peak = clip_block_reduce<true>(pk, sh_d);
    const double on = __dmul_rn(onset_frac, peak), off = __dmul_rn(offset_frac, peak);
    long long first = LLONG_MAX, last = -1;
    for (uint32_t i = threadIdx.x; i < n; i += OW_CLIP_THREADS) {
        const double a = fabs(x[i]);
        if (a > on && (long long)i < first) first = i;
        if (i >= 1 && a > off) last = i;                      // i ascends per thread
    }
    first = clip_block_reduce<false>(first, sh_i);
    last = clip_block_reduce<true>(last, sh_i);
    if (threadIdx.x == 0) {
        peak_out[blockIdx.x] = peak;
        first_out[blockIdx.x] = first == LLONG_MAX ? -1 : first;
        last_out[blockIdx.x] = last;
    }
}

}  // namespace owdev
