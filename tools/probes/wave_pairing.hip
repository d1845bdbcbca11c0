// Where the wavefronts of a one-round launch at two per SIMD land, and when each retires: the launch shape of the chain kernels of a
// full pool (k_preamp_pair, k_post<false, true>: 2 048 wavefronts of ~250 VGPRs on 1 024 SIMDs).
// `hipcc --offload-arch=gfx950 -O2 -I openwurli_amd/csrc tools/probes/wave_pairing.hip -o /tmp/wave_pairing && /tmp/wave_pairing`
// 120 resident doubles, each the carrier of its own dependent f64 FMA chain (VALU-bound, as the chain kernels are), launched as 2 048 x 64 threads, as 256 x 512 threads and as 256 x 512 threads
// with the turn-taking of ow_wave_turns.h.  Every wavefront records its HW_ID, its XCC id and its first and last clock reading.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>
#include "ow_wave_turns.h"

#define NREG 120
#define OUTER 4000
#define HWREG_HW_ID (4 | (0 << 6) | ((32 - 1) << 11))
#define HWREG_XCC_ID (20 | (0 << 6) | ((4 - 1) << 11))

struct WaveRec { unsigned hw_id, xcc, block, wave; long long t0, t1; };

template <int THREADS, bool TURNS>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_pairing(WaveRec* __restrict__ rec, double* __restrict__ out, double seed) {
    __shared__ uint32_t turn_words[OW_TURN_LDS_WORDS];
    owdev::WaveTurns turns;
    if (TURNS) turns.init(turn_words);
    const long long t0 = __builtin_readcyclecounter();
    double a[NREG];
    const double b = seed * 0.9999999, c = seed * 1e-9;
    for (int i = 0; i < NREG; ++i) a[i] = seed + i * 0.125 + threadIdx.x * 1e-3;
#pragma unroll 1
    for (int r = 0; r < OUTER; ++r) {
        if (TURNS) turns.tick((uint32_t)r);
#pragma unroll
        for (int i = 0; i < NREG; ++i) a[i] = __builtin_fma(a[i], b, c);
    }
    if (TURNS) turns.finish();
    double s = 0.0;
    for (int i = 0; i < NREG; ++i) s += a[i];
    out[blockIdx.x * THREADS + threadIdx.x] = s;
    const long long t1 = __builtin_readcyclecounter();
    if ((threadIdx.x & 63) == 0) {
        WaveRec w;
        w.hw_id = __builtin_amdgcn_s_getreg(HWREG_HW_ID);
        w.xcc = __builtin_amdgcn_s_getreg(HWREG_XCC_ID);
        w.block = blockIdx.x; w.wave = threadIdx.x >> 6; w.t0 = t0; w.t1 = t1;
        rec[blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6)] = w;
    }
}

// HW_ID (gfx9): simd_id [5:4], cu_id [11:8], sh_id [12], se_id [15:13]
static unsigned long long simd_key(const WaveRec& w) { return ((unsigned long long)w.xcc << 32) | (w.hw_id & 0xFF30u); }

static void report(const char* what, const std::vector<WaveRec>& recs, int waves_per_block, float ms) {
    std::map<unsigned long long, std::vector<const WaveRec*>> by_simd;
    for (const WaveRec& w : recs) by_simd[simd_key(w)].push_back(&w);
    int two = 0, one = 0, more = 0;
    double frac = 0.0, life = 0.0, span = 0.0, gap = 0.0;
    for (auto& kv : by_simd) {
        auto& v = kv.second;
        if (v.size() == 1) ++one; else if (v.size() > 2) ++more;
        if (v.size() != 2) continue;
        ++two;
        const long long start = std::min(v[0]->t0, v[1]->t0), first = std::min(v[0]->t1, v[1]->t1), last = std::max(v[0]->t1, v[1]->t1);
        frac += (double)(first - start) / (double)(last - start);
        life += 0.5 * (double)((v[0]->t1 - v[0]->t0) + (v[1]->t1 - v[1]->t0));
        span += (double)(last - start);
        gap += (double)(v[0]->t0 > v[1]->t0 ? v[0]->t0 - v[1]->t0 : v[1]->t0 - v[0]->t0);
    }
    printf("%s: %.3f ms, %zu wavefronts on %zu SIMDs; SIMDs with exactly two: %d, with one: %d, with more: %d\n", what, ms, recs.size(),
           by_simd.size(), two, one, more);
    if (two)
        printf("    on the SIMDs with two: the first wavefront retires at %.3f of the pair's span (mean); mean lifetime / span %.3f; "
               "start gap %.0f ticks of a span of %.0f\n", frac / two, life / span, gap / two, span / two);
    if (waves_per_block == 8) {
        std::map<unsigned, std::map<unsigned long long, int>> by_block;
        for (const WaveRec& w : recs) by_block[w.block][simd_key(w)] += 1;
        int good = 0;
        for (auto& kv : by_block) {
            bool ok = kv.second.size() == 4;
            for (auto& s : kv.second) ok = ok && s.second == 2;
            good += ok ? 1 : 0;
        }
        int split = 0;      // partners (w, w + 4)?
        for (auto& kv : by_simd)
            if (kv.second.size() == 2 && kv.second[0]->block == kv.second[1]->block &&
                (kv.second[0]->wave ^ kv.second[1]->wave) == 4u) ++split;
        printf("    workgroups with exactly two of their eight wavefronts on each of four SIMDs: %d of %zu; pairs that are wavefronts (w, w + 4): %d\n",
               good, by_block.size(), split);
    }
}

template <int THREADS, bool TURNS>
static void run(const char* what, WaveRec* d_rec, double* d_out) {
    const int blocks = 2048 * 64 / THREADS, waves = 2048;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float ms = 0.0f;
    for (int rep = 0; rep < 2; ++rep) {      // the second launch counts
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL((k_pairing<THREADS, TURNS>), dim3(blocks), dim3(THREADS), 0, 0, d_rec, d_out, 1.25);
        hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) { printf("%s: launch failed\n", what); exit(1); }
        hipEventElapsedTime(&ms, e0, e1);
    }
    std::vector<WaveRec> recs(waves);
    hipMemcpy(recs.data(), d_rec, waves * sizeof(WaveRec), hipMemcpyDeviceToHost);
    report(what, recs, THREADS / 64, ms);
}

int main() {
    WaveRec* d_rec; double* d_out;
    if (hipMalloc(&d_rec, 2048 * sizeof(WaveRec)) != hipSuccess || hipMalloc(&d_out, 2048 * 64 * sizeof(double)) != hipSuccess) return 1;
    run<64, false>("2048 x 64 threads", d_rec, d_out);
    run<512, false>("256 x 512 threads", d_rec, d_out);
    run<512, true>("256 x 512 threads, taking turns", d_rec, d_out);
    hipFree(d_rec); hipFree(d_out);
    return 0;
}
