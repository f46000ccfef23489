// pcore_raster.h -- exact-semantics device helpers shared by every stage of the render-and-compare path
// (pcore_fused.hip, pcore_render.hip, pcore_cloud.hip).
//
// Float semantics: every kernel of those files is compiled with -ffp-contract=off (plus the pragma below), IEEE
// f32 division and no fast-math, so each expression is evaluated in the explicit order of the
// reference CUDA code it restates (file:line cited per function).  Integer z-buffers are therefore
// bit-identical to the CPU oracle (oracle/pcore_oracle.cpp), which follows the same order.
#pragma once
#include "pcore_internal.h"
#include "pcore_fdiv.h"

#include <climits>
#include <cfloat>

#pragma clang fp contract(off)

namespace pcore {

constexpr int kWave = 64;
constexpr int64_t PCORE_KEY_NONE_DEV = 0x7fffffffffffffffLL;

// x86 cvttss2si semantics of the host `(int) float` casts (search_env.cpp:2022-2048).
__device__ __forceinline__ int32_t cvt_i32_x86(float f) {
    if (!(f == f) || f >= 2147483648.0f || f < -2147483648.0f) return INT_MIN;
    return (int32_t)f;
}

// CUDA abs() of a wrapped int32 difference (image_renderer.cuh:163-165).
__device__ __forceinline__ int32_t iabs_wrap(int32_t a, int32_t b) {
    int32_t d = (int32_t)((uint32_t)a - (uint32_t)b);
    return d < 0 ? (int32_t)(0u - (uint32_t)d) : d;
}

__device__ __forceinline__ float ref_max(float a, float b) { return (a > b) ? a : b; }  // image_renderer.cuh:14-15
__device__ __forceinline__ float ref_min(float a, float b) { return (a < b) ? a : b; }  // image_renderer.cuh:17-18

// mat_mul_v row (image_renderer.cuh:20-27): ((m0*x + m1*y) + m2*z) + m3
__device__ __forceinline__ float row4(float m0, float m1, float m2, float m3, float x, float y, float z) {
    return m0 * x + m1 * y + m2 * z + m3;
}

// Source-occlusion rule applied to the per-pixel minimum fragment depth.  Equals the reference's
// serial z-test + black-out sequence (image_renderer.cuh:146-196) for every fragment order because the
// black-out predicate is monotone in the stored depth ("Deterministic raster contract").
__device__ __forceinline__ int32_t occlusion_rule(int32_t z, int32_t src, int lab, bool use_seg, int32_t pl,
                                                  float occlusion_threshold) {
    if (z == INT_MAX) return 0;  // no fragment: max2zero (image_renderer.cuh:465-466)
    bool cond;
    if (use_seg) cond = (pl != lab - 1) && ((float)iabs_wrap(z, src) > 0.5f);
    else cond = (float)iabs_wrap(z, src) > occlusion_threshold;
    if (cond && z > src && src > 0) return 0;  // blacked out -> INT_MAX -> max2zero
    return z;
}

// Reference bounding box (image_renderer.cuh:86-107) with its exact NaN behaviour.
__device__ __forceinline__ void bbox_ref(const float (&p)[3][2], float cmax0, float cmax1, float (&bmin)[2],
                                         float (&bmax)[2]) {
    bmin[0] = FLT_MAX; bmin[1] = FLT_MAX;
    bmax[0] = -FLT_MAX; bmax[1] = -FLT_MAX;
    const float cmax[2] = {cmax0, cmax1};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            bmin[j] = ref_max(0.0f, ref_min(bmin[j], p[i][j]));
            bmax[j] = ref_min(cmax[j], ref_max(bmax[j], p[i][j]));
        }
}

// Loop bounds of `for (P = size_t(bmin + 0.5f); P <= bmax; ++P)` (image_renderer.cuh:110-111) with
// NVIDIA float->u64 conversion (NaN/negative -> 0, saturating).  Returns false if the loop is empty.
__device__ __forceinline__ bool loop_bounds(float bmin, float bmax, int& lo, int& hi) {
    if (!(bmax >= 0.0f)) return false;  // NaN or negative upper bound: P (>= 0) <= bmax never holds
    const float st = bmin + 0.5f;
    int start;
    if (!(st > 0.0f)) start = 0;
    else if (st >= 1.0e9f) return false;  // bmax <= width-1, so a start this large never iterates
    else start = (int)st;
    hi = (int)floorf(bmax);
    lo = start;
    return lo <= hi;
}

// One fragment test at raster pixel (P0, P1) (image_renderer.cuh:44-57, 112-129).
// Returns whether the pixel is inside (NaN barycentrics count as inside, as in the reference) and sets the depth
// for inside pixels; every lane runs the same instructions (no branch on the inside test), so a batch of
// fragment tests is one straight-line block plus the depth's rare IEEE fallback.
// BARY = 1: the barycentrics without the reference's three multiplications by 0.5, bit-identical under the bound of a
// fastdiv pose (pcore_fdiv.h); only the depth pass of a fastdiv pose asks for it.  BARY = 2: also the area's
// reciprocal without the division's scaling steps, bit-identical under the bound of an interior pose (pcore_fdiv.h,
// recip_interior); only the depth pass of an interior pose asks for it.
template <int BARY = 0>
__device__ __forceinline__ bool fragment_inside(float A0, float A1, float B0, float B1, float C0, float C1, float P0,
                                                float P1, float& alpha, float& beta, float& gamma) {
    frag_barycentrics<BARY>(A0, A1, B0, B1, C0, C1, P0, P1, beta, gamma);
    alpha = 1.0f - beta - gamma;
    // !(alpha < -0 || beta < -0 || gamma < -0 || alpha > 1 || beta > 1 || gamma > 1) as one v_min3 / v_max3 each:
    // the three are arithmetic results (quiet NaNs at most), on which v_min3 / v_max3 follow IEEE minNum / maxNum
    // -- a NaN operand is skipped, as in the comparisons, and an all-NaN triple gives NaN (inside, as in the
    // reference) -- so the compiler's canonicalising v_max per operand (it cannot know there is no sNaN) is not needed
    float mn, mx;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(mn) : "v"(alpha), "v"(beta), "v"(gamma));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(mx) : "v"(alpha), "v"(beta), "v"(gamma));
    return !(mn < -0.0f) && !(mx > 1.0f);
}
template <int BARY = 0>
__device__ __forceinline__ bool fragment(float A0, float A1, float B0, float B1, float C0, float C1, float z0,
                                         float z1, float z2, float P0, float P1, int32_t& depth, bool z_ok = false) {
    float alpha, beta, gamma;
    const bool inside = fragment_inside<BARY>(A0, A1, B0, B1, C0, C1, P0, P1, alpha, beta, gamma);
    // the depth quotient chain through reciprocal estimates with an error certificate, the IEEE divisions only
    // where the certificate fails (pcore_fdiv.h, frag_depth_certified); outside lanes never take the fallback
    depth = frag_depth_certified(alpha, beta, gamma, z0, z1, z2, z_ok, inside);
    return inside;
}
// The same with the vertices' reciprocal depths rz_i = v_rcp_f32(z_i) in place of the depths (a fastdiv pose's depth
// pass: every z_i in [1, 2^41)); exact_z(z0, z1, z2) fetches the depths themselves for the lanes that take the IEEE
// fallback (pcore_fdiv.h, frag_depth_certified_rz).
template <int BARY, class ExactZ>
__device__ __forceinline__ bool fragment_rz(float A0, float A1, float B0, float B1, float C0, float C1, float rz0,
                                            float rz1, float rz2, float P0, float P1, int32_t& depth,
                                            ExactZ&& exact_z) {
    float alpha, beta, gamma;
    const bool inside = fragment_inside<BARY>(A0, A1, B0, B1, C0, C1, P0, P1, alpha, beta, gamma);
    depth = frag_depth_certified_rz(alpha, beta, gamma, rz0, rz1, rz2, inside, exact_z);
    return inside;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0)); }

__device__ __forceinline__ int mbcnt64(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// select_kernel's per-pose key (search_env.cpp:1987-2051: int conversion, the |target - source| < 30 filter, cost
// -1 / -2 / INT_MAX excluded): ((cost ^ 0x80000000) << 31) | global index, or PCORE_KEY_NONE_DEV
__device__ __forceinline__ int64_t select_key(float rc, float oc, int m, int num_models, int64_t gidx) {
    const int32_t target = cvt_i32_x86(rc);
    const int32_t source = cvt_i32_x86(oc);
    const int32_t cost = (target < 0) ? -1 : cvt_i32_x86(rc + oc);
    const int32_t adiff = iabs_wrap(target, source);
    const bool ok = !(cost == -1 || cost == -2) && adiff < 30 && cost != INT_MAX && m >= 0 && m < num_models;
    if (!ok) return PCORE_KEY_NONE_DEV;
    const uint64_t hi = (uint64_t)((uint32_t)cost ^ 0x80000000u);
    return (int64_t)((hi << 31) | ((uint64_t)gidx & 0x7fffffffull));
}

// Camera-frame point of pixel (px, py) with integer depth Z (compute_point_clouds.cuh:14-22 with depth_factor,
// cm -> m), in the reference's operation order.
__device__ __forceinline__ float3 unproject(int px, int py, int32_t Z, float cx, float cy, float fx, float fy,
                                            float depth_factor) {
    const float zp = (float)Z / depth_factor;
    return make_float3(((float)px - cx) / fx * zp, ((float)py - cy) / fy * zp, zp);
}

// Stride samples of an image: sample (kx, ky) is pixel (kx * stride, ky * stride); x = columns, y = rows.
__device__ __forceinline__ int2 sample_dims(int width, int height, int stride) {
    return make_int2((width + stride - 1) / stride, (height + stride - 1) / stride);
}

// One step of a block-wide ordered compaction / exclusive scan over blockDim.x threads (a multiple of 64, at most
// 1024): a thread passes its exclusive offset within its wave and the wave's total (wave-uniform) and gets its offset
// in thread order, continued from *carry_s, which advances by the block's total.  Every thread of the block calls it;
// wsum holds a word per wave.  The caller sets *carry_s and synchronises before the first step.
__device__ __forceinline__ int block_ordered_offset(int in_wave, int wave_total, int* wsum, int* carry_s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) wsum[wave] = wave_total;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < nw; w++) {
        if (w < wave) woff += wsum[w];
        tot += wsum[w];
    }
    const int carry = *carry_s;
    __syncthreads();
    if (threadIdx.x == 0) *carry_s = carry + tot;
    __syncthreads();
    return carry + woff + in_wave;
}
// The same for a compaction: the offset of a thread among the block's threads with `valid` set.
__device__ __forceinline__ int block_ordered_offset(bool valid, int* wsum, int* carry_s) {
    const uint64_t b = __ballot(valid);
    return block_ordered_offset(mbcnt64(b), __popcll(b), wsum, carry_s);
}

}  // namespace pcore
