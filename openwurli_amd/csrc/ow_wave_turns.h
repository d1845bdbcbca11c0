// The two wavefronts of a SIMD take turns by progress (k_preamp_pair, k_post<false, true>; tools/probes/wave_pairing.hip).
//
// VALU issue between two co-resident wavefronts is arbitrated by priority, then age: at equal priority the older one runs nearly
// unimpeded and the younger gets the leftover slots.  In a launch of exactly one round at two per SIMD the older wavefront therefore
// retires early and the younger finishes alone, at the one-wavefront rate.  Here each wavefront publishes how many host samples it has
// done; the one that is behind raises its priority, the one that is ahead drops it, so both reach the end of the block together.
//
// For workgroups of OW_TURN_WAVES = 8 wavefronts (512 threads, two per SIMD at <= 256 VGPRs): the partner of a wavefront is the one
// other wavefront of its workgroup with the same SIMD id.  Nothing here waits: the helper cannot deadlock and cannot change a result.
// `s_setprio` ignores EXEC, so every decision is made on scalars (readfirstlane) and comes out behind a scalar branch; the builtins,
// not asm statements, which the unroller would price like a call (ow_chain_dev.h, exp_core).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace owdev {

#define OW_TURN_WAVES 8
#define OW_TURN_LDS_WORDS (2 * OW_TURN_WAVES)      // SIMD id per wavefront, then samples done per wavefront
#define OW_TURN_FINISHED 0xFFFFFFFFu
#define OW_HWREG_SIMD_ID (4 | (4 << 6) | ((2 - 1) << 11))      // hwreg(HW_REG_HW_ID, 4, 2)

// Ordering between the lanes of ONE wavefront that exchange data through LDS: what __syncthreads() is for a one-wavefront workgroup.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct WaveTurns {
    uint32_t* mine;            // this wavefront's progress word (LDS)
    const uint32_t* theirs;    // the partner's; the wavefront's own if it has none: then it is never ahead nor behind
    int prio;                  // the level last set

    static __device__ __forceinline__ void put(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ uint32_t get(const uint32_t* p) {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    }

    // `lds`: OW_TURN_LDS_WORDS words of the workgroup.  Holds the kernel's one workgroup barrier: every wavefront of the workgroup
    // calls it, whether it has engines or not.  A wavefront with no other on its SIMD, or with more than one, takes no part.
    __device__ __forceinline__ void init(uint32_t* lds, bool enable = true) {
        const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const uint32_t simd = __builtin_amdgcn_s_getreg(OW_HWREG_SIMD_ID);
        mine = lds + OW_TURN_WAVES + w;
        put(lds + w, simd);
        put(mine, 0u);
        __syncthreads();
        int partner = w, n = 0;
        for (int i = 0; i < OW_TURN_WAVES; ++i) {
            const uint32_t s = get(lds + i);
            if (i != w && s == simd) { partner = i; ++n; }
        }
        if (!enable || n != 1) partner = w;
        theirs = lds + OW_TURN_WAVES + __builtin_amdgcn_readfirstlane(partner);
        prio = 0;
    }

    // once per host sample, `done` = samples finished so far (wave-uniform)
    __device__ __forceinline__ void tick(uint32_t done) {
        put(mine, done);
        const uint32_t other = get(theirs);
        const uint32_t me = (uint32_t)__builtin_amdgcn_readfirstlane((int)done);
        if (me < other) {
            if (prio == 0) { __builtin_amdgcn_s_setprio(1); prio = 1; }
        } else if (me > other) {
            if (prio != 0) { __builtin_amdgcn_s_setprio(0); prio = 0; }
        }
    }

    __device__ __forceinline__ void finish() {
        put(mine, OW_TURN_FINISHED);
        if (prio != 0) { __builtin_amdgcn_s_setprio(0); prio = 0; }
    }
};

}  // namespace owdev
