// pcore_fused_probe.h -- the measurement builds of the fused COST kernel (pcore_fused.hip), kept out of its code.
// Each probe is a struct the kernel calls unconditionally; in the production build its methods are empty and the
// calls compile to nothing.  A measurement build (tools/build_variant.sh NAME -D...) defines one of
//   PCORE_FUSED_PROFILE     FProf: per-phase shader clocks (tools/fused_phase_prof.py)
//   PCORE_FLUSH_STATS       FlushStats: small-triangle flush batches, records, loop trips (tools/flush_stats.py)
//   PCORE_WG_TIMING         WgClock: wall clock at every workgroup's start and end (tools/wg_timeline.py)
//   PCORE_DEBUG_SKIP_RT=1   dbg_skip_bits: the kernel honours PCORE_DEBUG_SKIP (tools/ablate.sh, tools/ablate_sq.sh)
// and exports the probe's reader (pcore_debug_*).
#pragma once
#include "pcore_internal.h"

namespace pcore {

// Per-wave shader clocks of the fused kernel's phases -- [0] setup, [1] vertex stage, [2] triangle windows +
// queueing, [3] fragment batches, [4] wait at the end-of-raster barrier, [5] phase 2 (occlusion, unprojection,
// 1-NN, counts), [6] phase 3 + barriers.  Each wave sums in registers and adds once at exit.
#ifdef PCORE_FUSED_PROFILE
__device__ unsigned long long g_fprof[8];
extern "C" int pcore_debug_fused_profile(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fprof), sizeof(unsigned long long) * 8);
    if (e == hipSuccess && reset) {
        const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_fprof), z, sizeof(z));
    }
    return e == hipSuccess ? 0 : 1;
}
struct FProf {
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last = __builtin_amdgcn_s_memtime();
    __device__ __forceinline__ void mark(int k) {
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        acc[k] += t - last;
        last = t;
    }
    __device__ __forceinline__ void flush() {
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < 8; k++) atomicAdd(&g_fprof[k], acc[k]);
    }
};
#else
struct FProf {
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush() {}
};
#endif

// Counts of the raster's step loop: [0] flush batches, [1] records in them, [2] fragment tests of queued records,
// [3] partial flushes (stream switch, vertex ring about to be overwritten), [4] big triangles, [5] triangles touching
// a sample, [6] triangle slots that are not padding, [7] steps, [8] vertex passes, [9] steps that enter the general
// (more than one sample, NaN vertex) path instead of the one-sample fast path.
#ifdef PCORE_FLUSH_STATS
__device__ unsigned long long pcore_flush_stats[10];
extern "C" int pcore_debug_flush_stats(unsigned long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(pcore_flush_stats), sizeof(unsigned long long) * 10);
}
struct FlushStats {
    static __device__ __forceinline__ void add(int k, unsigned long long v) { atomicAdd(&pcore_flush_stats[k], v); }
    __device__ __forceinline__ void batch(int lane, int records) {
        if (lane == 0) { add(0, 1ull); add(1, (unsigned long long)records); }
    }
    __device__ __forceinline__ void record() { add(2, 1ull); }
    __device__ __forceinline__ void partial_flush(int lane) { if (lane == 0) add(3, 1ull); }
    __device__ __forceinline__ void step(int lane, uint64_t single, uint64_t rest, uint32_t ct) {
        const uint64_t blanes = __ballot(!(ct >> 31));
        if (lane == 0) {
            add(6, (unsigned long long)__popcll(blanes));
            add(7, 1ull);
            if (rest) add(9, 1ull);  // the general path counts the step's touching triangles (slow_step)
            else add(5, (unsigned long long)__popcll(single));
        }
    }
    __device__ __forceinline__ void slow_step(int lane, uint64_t big, int nk) {
        const uint64_t btouch = __ballot(nk > 0);
        if (lane == 0) {
            add(4, (unsigned long long)__popcll(big));
            add(5, (unsigned long long)__popcll(btouch));
        }
    }
    __device__ __forceinline__ void vertex_pass(int lane) { if (lane == 0) add(8, 1ull); }
};
#else
struct FlushStats {
    __device__ __forceinline__ void batch(int, int) {}
    __device__ __forceinline__ void record() {}
    __device__ __forceinline__ void partial_flush(int) {}
    __device__ __forceinline__ void step(int, uint64_t, uint64_t, uint32_t) {}
    __device__ __forceinline__ void slow_step(int, uint64_t, int) {}
    __device__ __forceinline__ void vertex_pass(int) {}
};
#endif

// Wall clock (100 MHz) at the start and end of every fused_cost_kernel workgroup, indexed by pose: the kernel holds
// one WgClock for its lifetime.
#ifdef PCORE_WG_TIMING
__device__ unsigned long long pcore_wg_clock[2 * 1048576];
extern "C" int pcore_debug_wg_clock(unsigned long long* host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(pcore_wg_clock), sizeof(unsigned long long) * 2 * (size_t)n);
}
struct WgClock {
    int pose;
    __device__ explicit WgClock(int p) : pose(p) {
        if (threadIdx.x == 0) pcore_wg_clock[2 * pose] = wall_clock64();
    }
    __device__ ~WgClock() {
        __syncthreads();
        if (threadIdx.x == 0) pcore_wg_clock[2 * pose + 1] = wall_clock64();
    }
};
#else
struct WgClock {
    __device__ explicit WgClock(int) {}
};
#endif

// The PCORE_DEBUG_SKIP ablation mask (FusedArgs::dbg_skip).  The production build reads none: a run-time flag kept as
// a lane-mask boolean across the step loop cost two VALU per test per step, so there the mask is the constant 0 and
// every test of it folds away.
#if PCORE_DEBUG_SKIP_RT
__device__ __forceinline__ int dbg_skip_bits(const FusedArgs& a) { return a.dbg_skip; }
#else
__device__ constexpr int dbg_skip_bits(const FusedArgs&) { return 0; }
#endif

}  // namespace pcore
