// pcore_gicp_probe.h -- the measurement builds of the GICP kernels (pcore_gicp.hip), kept out of their code: the role
// pcore_fused_probe.h plays for the fused kernel.  The kernels use the GPROF_* and GTL_* macros unconditionally; in
// the production build they are empty.  A measurement build defines PCORE_GICP_PROFILE or PCORE_GICP_TIMELINE (tools
// only) and exports the probe's reader (pcore_debug_gicp_*).
#pragma once

#include <hip/hip_runtime.h>

namespace pcore {
namespace {

// PCORE_GICP_PROFILE (tools/gicp_phase_prof.py, tools/c1_phase_prof.py): per-phase shader clocks of gicp_kernel,
// [0] correspondence search, [1] contributions (+ M stores), [2] wave reduction, [3] LM iteration, which splits into [4] damped
// solves, [5] se3_exp + compose, [6] the trials' error sums and their reduction, [7] the decisions; [8] counts the
// iterations that reused a set of the correspondence history instead of searching.
// Each wave sums its clocks in registers and adds them once at exit (no atomics inside the loop); each
// clock read is ordered after its phase's last result by an asm input dependency.
#ifdef PCORE_GICP_PROFILE
constexpr int kGprof = 10;  // [9]: the pose-iterations the sums cover (poses of >= PCORE_GICP_PROF_MIN_NS points)
#ifndef PCORE_GICP_PROF_MIN_NS
#define PCORE_GICP_PROF_MIN_NS 0
#endif
__device__ unsigned long long g_gicp_prof[kGprof];
extern "C" int pcore_debug_gicp_profile(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gicp_prof), sizeof(unsigned long long) * kGprof);
    if (e == hipSuccess && reset) {
        const unsigned long long z[kGprof] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_gicp_prof), z, sizeof(z));
    }
    return e == hipSuccess ? 0 : 1;
}
#define GPROF_DECL unsigned long long gp_acc[kGprof] = {}
#define GPROF_T(v) const unsigned long long v = __builtin_readcyclecounter()
#define GPROF_TD(v, dep)                                                                   \
    unsigned long long v;                                                                  \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "v"(dep) : "memory")
#define GPROF_ADD(k, a, b) gp_acc[k] += (unsigned long long)((b) - (a))
#define GPROF_COUNT(k, n) gp_acc[k] += (n)
// a pose's start: the sums before it (restored at its end if the pose is below the size filter)
#define GPROF_POSE_BEGIN                \
    unsigned long long gp_snap[kGprof]; \
    for (int k_ = 0; k_ < kGprof; k_++) gp_snap[k_] = gp_acc[k_]
#define GPROF_POSE_END(ns, run)         \
    gp_acc[9] += (run);                 \
    if ((ns) < PCORE_GICP_PROF_MIN_NS)  \
        for (int k_ = 0; k_ < kGprof; k_++) gp_acc[k_] = gp_snap[k_]
#define GPROF_FLUSH \
    if (lane == 0)  \
        for (int k_ = 0; k_ < kGprof; k_++) atomicAdd(&g_gicp_prof[k_], gp_acc[k_])
#define GPROF_PARAM , unsigned long long (&gp_acc)[kGprof]
#define GPROF_ARG , gp_acc
#else
#define GPROF_DECL
#define GPROF_T(v)
#define GPROF_TD(v, dep)
#define GPROF_ADD(k, a, b)
#define GPROF_COUNT(k, n)
#define GPROF_POSE_BEGIN
#define GPROF_POSE_END(ns, run)
#define GPROF_FLUSH
#define GPROF_PARAM
#define GPROF_ARG
#endif

// PCORE_GICP_TIMELINE (tools/gicp_timeline.py): gicp_kernel records, per pose, the real-time clock (100 MHz) when a wave dequeues it and when
// it writes the refined pose, and per wave its start and exit.
#ifdef PCORE_GICP_TIMELINE
constexpr int kTlPoses = 1 << 17, kTlWaves = 1 << 14;
__device__ unsigned long long g_tl_pose[2 * kTlPoses];
__device__ unsigned long long g_tl_wave[2 * kTlWaves];
__device__ unsigned int g_tl_nwaves;
__device__ int g_tl_run[kTlPoses];  // iterations each pose executed (fewer than it reports after a cycle exit)
extern "C" int pcore_debug_gicp_timeline_run(int* run) {
    return hipMemcpyFromSymbol(run, HIP_SYMBOL(g_tl_run), sizeof(g_tl_run)) == hipSuccess ? 0 : 1;
}
extern "C" int pcore_debug_gicp_timeline(unsigned long long* poses, unsigned long long* waves, unsigned int* nwaves) {
    hipError_t e = hipMemcpyFromSymbol(poses, HIP_SYMBOL(g_tl_pose), sizeof(g_tl_pose));
    if (e == hipSuccess) e = hipMemcpyFromSymbol(waves, HIP_SYMBOL(g_tl_wave), sizeof(g_tl_wave));
    if (e == hipSuccess) e = hipMemcpyFromSymbol(nwaves, HIP_SYMBOL(g_tl_nwaves), sizeof(unsigned int));
    const unsigned int z = 0;
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_tl_nwaves), &z, sizeof(z));
    return e == hipSuccess ? 0 : 1;
}
// a pose's stamps, by the lane that writes the pose; a wave's, by its lane 0 at exit
__device__ __forceinline__ void tl_stamp_pose(int gp, unsigned long long t0, int run) {
    if (gp >= kTlPoses) return;
    g_tl_pose[2 * gp] = t0;
    g_tl_pose[2 * gp + 1] = __builtin_amdgcn_s_memrealtime();
    g_tl_run[gp] = run;
}
__device__ __forceinline__ void tl_stamp_wave(unsigned long long t0) {
    const unsigned int w = atomicAdd(&g_tl_nwaves, 1u);
    if (w >= (unsigned)kTlWaves) return;
    g_tl_wave[2 * w] = t0;
    g_tl_wave[2 * w + 1] = __builtin_amdgcn_s_memrealtime();
}
#define GTL_NOW(v) const unsigned long long v = __builtin_amdgcn_s_memrealtime()
#define GTL_POSE(gp, t0, run) tl_stamp_pose(gp, t0, run)
#define GTL_WAVE(t0) \
    if (lane == 0) tl_stamp_wave(t0)
#define GTL_PARAM(v) , unsigned long long v
#define GTL_ARG(v) , v
#else
#define GTL_NOW(v)
#define GTL_POSE(gp, t0, run)
#define GTL_WAVE(t0)
#define GTL_PARAM(v)
#define GTL_ARG(v)
#endif

}  // namespace
}  // namespace pcore
