// pcore_render.hip -- stage RENDER (parity): the full-resolution z-buffer and colour planes in HBM, bit-exact with
// the reference renderer.  Not on the measured path (stage COST renders its stride samples in LDS, pcore_fused.hip).
//
// Kernels
//   render_full_kernel<false>  depth pass: atomicMin of every fragment's depth.
//   render_full_kernel<true>   colour id pass: the lowest triangle reaching each pixel's minimum depth.
//   render_finalize_kernel     source occlusion + INT_MAX -> 0 on the full z-buffer (+ the colour planes).
//   fill_i32_kernel            z-buffer / id-buffer initialisation.
//   render_scene_kernel        composed state: all poses into one frame of 64-bit (depth, pose, triangle) keys.
//   scene_finalize_kernel      its keys -> depth, owner, colour planes, visible pixels per pose.
#include "pcore_raster.h"

#pragma clang fp contract(off)

namespace pcore {

// One thread per (triangle, pose), as render_triangle_multi (image_renderer.cuh:212-321); the per-pixel
// spin-lock is replaced by atomicMin and the black-out by render_finalize_kernel.
// IDPASS: the colour of stage RENDER (render_triangle_multi's red / green / blue planes, image_renderer.cuh:146-196).
// The serial z-test writes a triangle's colour whenever its fragment is strictly nearer, so the pixel keeps the colour
// of the first triangle (lowest index) whose fragment reaches the minimum depth: a second pass over the same
// fragments keeps, per pixel, the lowest triangle index whose depth equals the z-buffer's minimum (tri_min; depth is
// only read).
template <bool IDPASS>
__global__ void __launch_bounds__(256) render_full_kernel(const float* tris, int num_tris, const int32_t* tri_lo,
                                                          const int32_t* tri_hi, const float* poses,
                                                          const int32_t* pose_model, int width, int height,
                                                          const float* proj, int32_t* depth, int32_t* tri_min) {
    const int pose = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tris) return;
    const int m = pose_model[pose];
    if (!(t >= tri_lo[m] && t < tri_hi[m])) return;
    const float* M = poses + (size_t)16 * pose;
    const float* tp = tris + (size_t)9 * t;
    const float Wf = (float)width, Hf = (float)height;
    float p[3][2], z[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float x = tp[3 * k], y = tp[3 * k + 1], zz = tp[3 * k + 2];
        const float lx = row4(M[0], M[1], M[2], M[3], x, y, zz);
        const float ly = row4(M[4], M[5], M[6], M[7], x, y, zz);
        const float lz = row4(M[8], M[9], M[10], M[11], x, y, zz);
        const float px = row4(proj[0], proj[1], proj[2], proj[3], lx, ly, lz);
        const float py = row4(proj[4], proj[5], proj[6], proj[7], lx, ly, lz);
        p[k][0] = px / lz * Wf / 2.0f + Wf / 2.0f;
        p[k][1] = py / lz * Hf / 2.0f + Hf / 2.0f;
        z[k] = lz;
    }
    float bmin[2], bmax[2];
    bbox_ref(p, (float)(width - 1), (float)(height - 1), bmin, bmax);
    int lo0, hi0, lo1, hi1;
    if (!loop_bounds(bmin[0], bmax[0], lo0, hi0) || !loop_bounds(bmin[1], bmax[1], lo1, hi1)) return;
    const size_t base = (size_t)pose * width * height;
    for (int P1 = lo1; P1 <= hi1; P1++)
        for (int P0 = lo0; P0 <= hi0; P0++) {
            int32_t d;
            if (fragment(p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], z[0], z[1], z[2], (float)P0, (float)P1, d)) {
                const size_t i = base + P0 + (size_t)(height - 1 - P1) * width;
                if constexpr (!IDPASS) atomicMin(&depth[i], d);
                else if (d == depth[i]) atomicMin(&tri_min[i], t);
            }
        }
}

// Source occlusion + max2zero on the full z-buffer (the a6' rule); with `rgb` (packed r | g << 8
// | b << 16 per triangle) also the colour planes (red, green, blue planes of N x H x W each, the reference's
// result_color): the nearest triangle's colour, black where no fragment landed or the source occludes the render.
__global__ void render_finalize_kernel(int32_t* depth, const int32_t* src_depth, const uint8_t* src_mask,
                                       const int32_t* pose_label, int width, int height, float occlusion_threshold,
                                       const int32_t* tri_min, const uint32_t* rgb, uint8_t* color, int num_poses) {
    const int pose = blockIdx.y;
    const size_t npx = (size_t)width * height;
    const bool use_seg = pose_label != nullptr;
    const int32_t pl = use_seg ? pose_label[pose] : 0;
    int32_t* img = depth + npx * pose;
    const size_t plane = npx * (size_t)num_poses;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        const int32_t dmin = img[i];
        const int32_t z = occlusion_rule(dmin, src_depth[i], use_seg ? (int)src_mask[i] : 0, use_seg, pl, occlusion_threshold);
        img[i] = z;
        if (color) {
            // blocked fragments end at INT_MAX (0 after max2zero) and a blocked dmin is > src > 0, so z != dmin
            const bool shown = dmin != INT_MAX && z == dmin;
            const uint32_t c = shown ? rgb[tri_min[npx * pose + i]] : 0u;
            uint8_t* px = color + npx * pose + i;
            px[0] = (uint8_t)(c & 0xff);
            px[plane] = (uint8_t)((c >> 8) & 0xff);
            px[2 * plane] = (uint8_t)((c >> 16) & 0xff);
        }
    }
}

// ---- composed state ("Composed state"): every pose's fragments into ONE H x W frame ----

// A pixel's key: (depth in signed order) << 32 | id; the unsigned minimum is the nearest depth, among equals the lowest id
__device__ __forceinline__ unsigned long long scene_key(int32_t d, uint32_t id) {
    return ((unsigned long long)((uint32_t)d ^ 0x80000000u) << 32) | id;
}
__device__ __forceinline__ int32_t scene_key_depth(unsigned long long key) {
    return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
}
constexpr unsigned long long kSceneNone = ~0ull;

// Triangle t under a pose as render_full_kernel sets it up: the projected corners, their depths and the bounds of
// the two pixel loops; false when a loop is empty.
__device__ __forceinline__ bool scene_triangle(const SceneArgs& a, int t, int pose, float (&p)[3][2], float (&z)[3],
                                               int& lo0, int& hi0, int& lo1, int& hi1) {
    const float* M = a.poses + (size_t)16 * pose;
    const float* tp = a.tris + (size_t)9 * t;
    const float* proj = a.proj;
    const float Wf = (float)a.width, Hf = (float)a.height;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float x = tp[3 * k], y = tp[3 * k + 1], zz = tp[3 * k + 2];
        const float lx = row4(M[0], M[1], M[2], M[3], x, y, zz);
        const float ly = row4(M[4], M[5], M[6], M[7], x, y, zz);
        const float lz = row4(M[8], M[9], M[10], M[11], x, y, zz);
        const float px = row4(proj[0], proj[1], proj[2], proj[3], lx, ly, lz);
        const float py = row4(proj[4], proj[5], proj[6], proj[7], lx, ly, lz);
        p[k][0] = px / lz * Wf / 2.0f + Wf / 2.0f;
        p[k][1] = py / lz * Hf / 2.0f + Hf / 2.0f;
        z[k] = lz;
    }
    float bmin[2], bmax[2];
    bbox_ref(p, (float)(a.width - 1), (float)(a.height - 1), bmin, bmax);
    return loop_bounds(bmin[0], bmax[0], lo0, hi0) && loop_bounds(bmin[1], bmax[1], lo1, hi1);
}

// Whether the pose's own source black-out removes a fragment of depth d (not INT_MAX) at pixel i: the rule answers 0
// for a blocked d > src > 0, so never d itself.
__device__ __forceinline__ bool scene_blocked(const SceneArgs& a, int pose, int32_t d, size_t i) {
    if (!a.occlude) return false;
    const bool use_seg = a.pose_label != nullptr;
    return occlusion_rule(d, a.src_depth[i], use_seg ? (int)a.src_mask[i] : 0, use_seg,
                          use_seg ? a.pose_label[pose] : 0, a.occlusion_threshold) != d;
}

// One thread per (triangle, pose) and the fragment arithmetic of render_full_kernel, so the depths are the same bits.
// A fragment that its own pose's source black-out removes is dropped (occlusion_rule on the fragment: the rule is
// monotone in the depth, so a pose's fragments at a pixel are blocked exactly when its nearest one is); the others meet
// in the pixel's key, id = pose * num_tris + t, by one no-return 64-bit atomic minimum: the nearest depth, among equals
// the lowest pose, inside it the lowest triangle.  keys: H x W, kSceneNone before the launch.
__global__ void __launch_bounds__(256) render_scene_kernel(SceneArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.num_tris) return;
    for (int pose = blockIdx.y; pose < a.num_poses; pose += gridDim.y) {
        const int m = a.pose_model[pose];
        if (m < 0 || m >= a.num_models || !(t >= a.tri_lo[m] && t < a.tri_hi[m])) continue;
        float p[3][2], z[3];
        int lo0, hi0, lo1, hi1;
        if (!scene_triangle(a, t, pose, p, z, lo0, hi0, lo1, hi1)) continue;
        const uint32_t id = (uint32_t)pose * (uint32_t)a.num_tris + (uint32_t)t;
        for (int P1 = lo1; P1 <= hi1; P1++)
            for (int P0 = lo0; P0 <= hi0; P0++) {
                int32_t d;
                if (!fragment(p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], z[0], z[1], z[2], (float)P0,
                              (float)P1, d) || d == INT_MAX)
                    continue;  // a fragment of depth INT_MAX is no fragment (max2zero)
                const size_t i = P0 + (size_t)(a.height - 1 - P1) * a.width;
                if (scene_blocked(a, pose, d, i)) continue;
                (void)__hip_atomic_fetch_min(&a.keys[i], scene_key(d, id), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
    }
}

// The contract where one key per pixel cannot give it.  A pose whose nearest fragment at a pixel has depth 0 -- a NaN
// depth (a degenerate triangle: NaN barycentrics count as inside, and NaN converts to 0) or a surface within a
// centimetre of the camera's plane -- reads 0 there in its own z-buffer, which means "nothing": the pose is absent from
// the pixel with all its fragments, and the poses behind it show.  That takes the pose's own minimum, which the shared
// key does not hold; but the key marks the pixels: a depth 0 is never blocked and beats every positive depth, so a key
// reads depth 0 exactly where some pose is in that case and no pose has a negative depth (where one has, the key is
// right already).  For each such pixel its block evaluates the contract directly: per pose the minimum over its
// triangles' fragments at this one pixel (the same set-up, loop bounds and fragment test: the same bits), dropped when
// it is 0 or blocked; the minimum of the rest replaces the key.  One block per 256 pixels; without such a pixel, as
// good as always, it returns after reading its keys.
__global__ void __launch_bounds__(256) scene_zero_kernel(SceneArgs a) {
    __shared__ int list[256];
    __shared__ int count;
    __shared__ unsigned long long pose_min;
    const size_t npx = (size_t)a.width * a.height;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    const size_t own = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (own < npx) {
        const unsigned long long key = a.keys[own];
        if (key != kSceneNone && scene_key_depth(key) == 0) list[atomicAdd(&count, 1)] = threadIdx.x;
    }
    __syncthreads();
    const int n = count;
    for (int q = 0; q < n; q++) {
        const size_t i = (size_t)blockIdx.x * 256 + list[q];
        const int P0 = (int)(i % a.width), P1 = a.height - 1 - (int)(i / a.width);
        unsigned long long best = kSceneNone;  // thread 0's
        for (int pose = 0; pose < a.num_poses; pose++) {
            const int m = a.pose_model[pose];
            if (m < 0 || m >= a.num_models) continue;
            if (threadIdx.x == 0) pose_min = kSceneNone;
            __syncthreads();
            unsigned long long mine = kSceneNone;
            for (int t = a.tri_lo[m] + threadIdx.x; t < a.tri_hi[m]; t += 256) {
                float p[3][2], z[3];
                int lo0, hi0, lo1, hi1;
                int32_t d;
                if (!scene_triangle(a, t, pose, p, z, lo0, hi0, lo1, hi1) || P0 < lo0 || P0 > hi0 || P1 < lo1 || P1 > hi1)
                    continue;
                if (fragment(p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], z[0], z[1], z[2], (float)P0, (float)P1,
                             d) && d != INT_MAX)
                    mine = std::min(mine, scene_key(d, (uint32_t)t));
            }
            if (mine != kSceneNone)
                (void)__hip_atomic_fetch_min(&pose_min, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            if (threadIdx.x == 0 && pose_min != kSceneNone) {
                const int32_t d = scene_key_depth(pose_min);
                if (d != 0 && !scene_blocked(a, pose, d, i))
                    best = std::min(best, scene_key(d, (uint32_t)pose * (uint32_t)a.num_tris + (uint32_t)pose_min));
            }
        }
        if (threadIdx.x == 0) a.keys[i] = best;
    }
}

constexpr int kSceneHist = 256;  // poses counted in LDS by scene_finalize_kernel; the ones past them count in HBM

// The keys unpacked (after scene_zero_kernel none holds depth 0): the depth image (0 without a key), the owner image
// (the key's pose, -1 without), the colour planes (red, green, blue of H x W each: the key's triangle, black without)
// and the owners' pixel counts (visible, zero before the launch: integer sums, the same in any order).  owner / color /
// visible nullable.
__global__ void __launch_bounds__(256) scene_finalize_kernel(const unsigned long long* keys, int num_tris,
                                                             int num_poses, size_t npx, const uint32_t* rgb,
                                                             int32_t* depth, int32_t* owner, uint8_t* color,
                                                             int32_t* visible) {
    __shared__ int hist[kSceneHist];
    if (visible) {
        for (int k = threadIdx.x; k < kSceneHist; k += blockDim.x) hist[k] = 0;
        __syncthreads();
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const uint32_t id = (uint32_t)key;
        const bool shown = key != kSceneNone;
        const int pose = shown ? (int)(id / (uint32_t)num_tris) : -1;
        depth[i] = shown ? scene_key_depth(key) : 0;
        if (owner) owner[i] = pose;
        if (color) {
            const uint32_t c = shown ? rgb[id - (uint32_t)pose * (uint32_t)num_tris] : 0u;
            color[i] = (uint8_t)(c & 0xff);
            color[npx + i] = (uint8_t)((c >> 8) & 0xff);
            color[2 * npx + i] = (uint8_t)((c >> 16) & 0xff);
        }
        if (visible && shown) {
            if (pose < kSceneHist) atomicAdd(&hist[pose], 1);
            else atomicAdd(&visible[pose], 1);
        }
    }
    if (visible) {
        __syncthreads();
        for (int k = threadIdx.x; k < kSceneHist && k < num_poses; k += blockDim.x)
            if (hist[k]) atomicAdd(&visible[k], hist[k]);
    }
}

hipError_t launch_render_scene(const SceneArgs& a, hipStream_t s) {
    if (a.num_poses <= 0 || a.num_tris <= 0) return hipSuccess;
    dim3 grid((a.num_tris + 255) / 256, std::min(a.num_poses, 65535));
    hipLaunchKernelGGL(render_scene_kernel, grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t npx = (size_t)a.width * a.height;
    hipLaunchKernelGGL(scene_zero_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_scene_finalize(const unsigned long long* keys, int num_tris, int num_poses, int width, int height,
                                 const uint32_t* rgb, int32_t* depth, int32_t* owner, uint8_t* color,
                                 int32_t* visible, hipStream_t s) {
    const size_t npx = (size_t)width * height;
    unsigned bx = (unsigned)((npx + 255) / 256);
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(scene_finalize_kernel, dim3(bx), dim3(256), 0, s, keys, num_tris, num_poses, npx, rgb, depth,
                       owner, color, visible);
    return hipGetLastError();
}

__global__ void fill_i32_kernel(int32_t* p, int32_t v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

hipError_t launch_fill_i32(int32_t* p, int32_t v, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, v, n);
    return hipGetLastError();
}

hipError_t launch_render_full(const float* tris, int num_tris, const int32_t* tri_lo, const int32_t* tri_hi,
                              const float* poses, const int32_t* pose_model, int num_poses, int width, int height,
                              const float* proj, int32_t* depth, hipStream_t s) {
    if (num_poses <= 0 || num_tris <= 0) return hipSuccess;
    dim3 grid((num_tris + 255) / 256, num_poses);
    hipLaunchKernelGGL(render_full_kernel<false>, grid, dim3(256), 0, s, tris, num_tris, tri_lo, tri_hi, poses,
                       pose_model, width, height, proj, depth, (int32_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_render_full_tri(const float* tris, int num_tris, const int32_t* tri_lo, const int32_t* tri_hi,
                                  const float* poses, const int32_t* pose_model, int num_poses, int width, int height,
                                  const float* proj, const int32_t* depth, int32_t* tri_min, hipStream_t s) {
    if (num_poses <= 0 || num_tris <= 0) return hipSuccess;
    dim3 grid((num_tris + 255) / 256, num_poses);
    hipLaunchKernelGGL(render_full_kernel<true>, grid, dim3(256), 0, s, tris, num_tris, tri_lo, tri_hi, poses,
                       pose_model, width, height, proj, const_cast<int32_t*>(depth), tri_min);
    return hipGetLastError();
}

hipError_t launch_render_finalize(int32_t* depth, const int32_t* src_depth, const uint8_t* src_mask,
                                  const int32_t* pose_label, int num_poses, int width, int height,
                                  float occlusion_threshold, hipStream_t s, const int32_t* tri_min,
                                  const uint32_t* rgb, uint8_t* color) {
    if (num_poses <= 0) return hipSuccess;
    const size_t npx = (size_t)width * height;
    unsigned bx = (unsigned)((npx + 255) / 256);
    if (bx > 256) bx = 256;
    hipLaunchKernelGGL(render_finalize_kernel, dim3(bx, num_poses), dim3(256), 0, s, depth, src_depth, src_mask,
                       pose_label, width, height, occlusion_threshold, tri_min, rgb, color, num_poses);
    return hipGetLastError();
}

}  // namespace pcore
