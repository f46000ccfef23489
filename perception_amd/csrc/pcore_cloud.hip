// pcore_cloud.hip -- stage CLOUD / depth2cloud_global on full-resolution z-buffers (compute_point_clouds.cuh:37-184,
// 265-346), the source sampler of stage COST and the host selection.  Not on the measured path.
//
// Kernels
//   cloud_count / cloud_write      stride mask, ordered compaction (block_ordered_offset), unprojection.
//   exclusive_scan_kernel          the per-image offsets of the compaction.
//   cloud_sample_prefix / cloud_dc_index  result_dc_index: cloud points before every pixel.
//   sample_source_kernel           the source depth / mask at the stride grid (read by the fused kernel).
//   select_kernel                  host selection of the reference (int cost, filter, per-model argmin key).
#include "pcore_raster.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace pcore {

__device__ __forceinline__ bool cloud_valid(const int32_t* depth, const uint8_t* label_mask, size_t idx, int x, int y,
                                            const CloudBounds& cb) {
    if (depth[idx] <= 0) return false;                                 // :64, :123
    if (label_mask != nullptr && label_mask[idx] <= 0) return false;  // :74, :127
    if (cb.on) {
        // transform_point with camera_transform (:14-35): camera point, then R p (left to right) + t
        const float3 c = unproject(x, y, depth[idx], cb.cx, cb.cy, cb.fx, cb.fy, cb.depth_factor);
        float w[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            w[r] = cb.m[4 * r] * c.x + cb.m[4 * r + 1] * c.y + cb.m[4 * r + 2] * c.z;
            w[r] = w[r] + cb.m[4 * r + 3];
        }
        if (w[0] > cb.b[0] || w[0] < cb.b[1]) return false;  // :86-88, :130-132
        if (w[1] > cb.b[2] || w[1] < cb.b[3]) return false;
        if (w[2] > cb.b[4] || w[2] < cb.b[5]) return false;
    }
    return true;
}

// Pixel (x, y) of stride sample k (row-major over dims.x columns) and its index in the image that starts at `base`.
__device__ __forceinline__ size_t sample_pixel(int k, int2 dims, int stride, int width, size_t base, int& x, int& y) {
    const int ky = k / dims.x, kx = k - ky * dims.x;
    x = kx * stride;
    y = ky * stride;
    return base + (size_t)x + (size_t)y * width;
}

// one block per image: number of valid stride samples
__global__ void cloud_count_kernel(const int32_t* depth, int width, int height, int stride, const uint8_t* label_mask,
                                   CloudBounds cb, int32_t* counts) {
    const int n = blockIdx.x;
    const int2 dims = sample_dims(width, height, stride);
    const size_t npx = (size_t)width * height;
    int c = 0;
    for (int k = threadIdx.x; k < dims.x * dims.y; k += blockDim.x) {
        int x, y;
        const size_t idx = sample_pixel(k, dims, stride, width, npx * n, x, y);
        c += cloud_valid(depth, label_mask, idx, x, y, cb) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    __shared__ int part[16];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += part[w];
        counts[n] = t;
    }
}

// single-block exclusive scan (n up to millions: chunked)
__global__ void exclusive_scan_kernel(const int32_t* in, int32_t* out, int n, int32_t* total) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n; base += blockDim.x) {
        const int i = base + threadIdx.x;
        const int v = i < n ? in[i] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off);
            if (lane >= off) incl += y;
        }
        const int o = block_ordered_offset(incl - v, __shfl(incl, 63), wsum, &carry_s);
        if (i < n) out[i] = o;
    }
    if (threadIdx.x == 0 && total) *total = carry_s;
}

__global__ void cloud_write_kernel(const int32_t* depth, int width, int height, int stride, float cx, float cy,
                                   float fx, float fy, float depth_factor, const uint8_t* label_mask,
                                   const int32_t* pose_label, const int32_t* offsets, float* xyz, int32_t* pose_out,
                                   int32_t* label_out, int cap, CloudBounds cb, const uint8_t* rgb_in,
                                   uint8_t* rgb_out, const uint8_t* planes_in, uint8_t* planes_out, int num_poses) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int n = blockIdx.x;
    const int2 dims = sample_dims(width, height, stride);
    const size_t npx = (size_t)width * height;
    if (threadIdx.x == 0) carry_s = offsets[n];
    __syncthreads();
    for (int base = 0; base < dims.x * dims.y; base += blockDim.x) {
        const int k = base + threadIdx.x;
        bool v = false;
        int x = 0, y = 0;
        size_t idx = 0;
        if (k < dims.x * dims.y) {
            idx = sample_pixel(k, dims, stride, width, npx * n, x, y);
            v = cloud_valid(depth, label_mask, idx, x, y, cb);
        }
        const int o = block_ordered_offset(v, wsum, &carry_s);
        if (v && o < cap) {
            const float3 p = unproject(x, y, depth[idx], cx, cy, fx, fy, depth_factor);
            xyz[3 * (size_t)o + 0] = p.x;
            xyz[3 * (size_t)o + 1] = p.y;
            xyz[3 * (size_t)o + 2] = p.z;
            if (pose_out) pose_out[o] = n;
            if (rgb_out) {  // depth_to_2d_cloud :155-157, the input image's channels in order
                rgb_out[3 * (size_t)o + 0] = rgb_in[3 * idx + 0];
                rgb_out[3 * (size_t)o + 1] = rgb_in[3 * idx + 1];
                rgb_out[3 * (size_t)o + 2] = rgb_in[3 * idx + 2];
            }
            if (planes_out) {  // depth_to_2d_cloud :163-165: the rendered colour planes into point planes
                const size_t plane = npx * (size_t)num_poses;
                planes_out[o] = planes_in[idx];
                planes_out[(size_t)cap + o] = planes_in[plane + idx];
                planes_out[2 * (size_t)cap + o] = planes_in[2 * plane + idx];
            }
            if (label_out) {
                if (label_mask) label_out[o] = (int32_t)label_mask[idx] - 1;
                else if (pose_label) label_out[o] = pose_label[n];
                else label_out[o] = 0;
            }
        }
    }
}

hipError_t launch_cloud_count(const int32_t* depth, int num_poses, int width, int height, int stride,
                              const uint8_t* label_mask, const CloudBounds& cb, int32_t* counts, hipStream_t s) {
    if (num_poses <= 0) return hipSuccess;
    hipLaunchKernelGGL(cloud_count_kernel, dim3(num_poses), dim3(256), 0, s, depth, width, height, stride, label_mask,
                       cb, counts);
    return hipGetLastError();
}

hipError_t launch_exclusive_scan(const int32_t* in, int32_t* out, int n, int32_t* total, hipStream_t s) {
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, s, in, out, n, total);
    return hipGetLastError();
}

hipError_t launch_cloud_write(const int32_t* depth, int num_poses, int width, int height, int stride, float cx,
                              float cy, float fx, float fy, float depth_factor, const uint8_t* label_mask,
                              const int32_t* pose_label, const int32_t* offsets, float* xyz, int32_t* pose,
                              int32_t* label, int cap, const CloudBounds& cb, const uint8_t* rgb_in,
                              uint8_t* rgb_out, hipStream_t s, const uint8_t* planes_in, uint8_t* planes_out) {
    if (num_poses <= 0) return hipSuccess;
    hipLaunchKernelGGL(cloud_write_kernel, dim3(num_poses), dim3(256), 0, s, depth, width, height, stride, cx, cy, fx,
                       fy, depth_factor, label_mask, pose_label, offsets, xyz, pose, label, cap, cb, rgb_in,
                       rgb_out, planes_in, planes_out, num_poses);
    return hipGetLastError();
}

// result_dc_index (compute_point_clouds.cuh:267-292): the reference scans a 0/1 mask over every pixel of the N
// z-buffers, so a pixel's entry is the number of cloud points (valid stride samples) before it in pose / row / column
// order.  Per pose, the exclusive count at every stride sample and at the pose's end (one block per pose) ...
__global__ void cloud_sample_prefix_kernel(const int32_t* depth, int width, int height, int stride,
                                           const uint8_t* label_mask, const int32_t* offsets, int32_t* pre) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int n = blockIdx.x;
    const int2 dims = sample_dims(width, height, stride);
    const int nsamp = dims.x * dims.y;
    const size_t npx = (size_t)width * height;
    int32_t* P = pre + (size_t)n * (nsamp + 1);
    const CloudBounds cb{};
    if (threadIdx.x == 0) carry_s = offsets[n];
    __syncthreads();
    for (int base = 0; base < nsamp; base += blockDim.x) {
        const int k = base + threadIdx.x;
        bool v = false;
        if (k < nsamp) {
            int x, y;
            const size_t idx = sample_pixel(k, dims, stride, width, npx * n, x, y);
            v = cloud_valid(depth, label_mask, idx, x, y, cb);
        }
        const int o = block_ordered_offset(v, wsum, &carry_s);
        if (k < nsamp) P[k] = o;
    }
    if (threadIdx.x == 0) P[nsamp] = carry_s;
}

// ... then every pixel: the samples before pixel (x, y) are the rows of samples above it and, on a sample row, the
// samples left of it
__global__ void cloud_dc_index_kernel(int num_poses, int width, int height, int stride, const int32_t* pre,
                                      int32_t* dc) {
    const int2 dims = sample_dims(width, height, stride);
    const int ws = dims.x, hs = dims.y;
    const size_t npx = (size_t)width * height, total = npx * num_poses;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const size_t n = p / npx, r = p - n * npx;
        const int y = (int)(r / width), x = (int)(r - (size_t)y * width);
        const int ry = y % stride == 0 ? y / stride : y / stride + 1;
        const int cx = y % stride == 0 ? (x + stride - 1) / stride : 0;
        const int k = min(ry * ws + cx, ws * hs);
        dc[p] = pre[n * (size_t)(ws * hs + 1) + k];
    }
}

hipError_t launch_cloud_dc_index(const int32_t* depth, int num_poses, int width, int height, int stride,
                                 const uint8_t* label_mask, const int32_t* offsets, int32_t* pre, int32_t* dc,
                                 hipStream_t s) {
    if (num_poses <= 0) return hipSuccess;
    hipLaunchKernelGGL(cloud_sample_prefix_kernel, dim3(num_poses), dim3(256), 0, s, depth, width, height, stride,
                       label_mask, offsets, pre);
    const size_t total = (size_t)width * height * num_poses;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 65535);
    hipLaunchKernelGGL(cloud_dc_index_kernel, dim3(blocks), dim3(256), 0, s, num_poses, width, height, stride, pre, dc);
    return hipGetLastError();
}

// sampled copy of the source depth / mask at the stride grid (used by the fused kernel)
__global__ void sample_source_kernel(const int32_t* src_depth, const uint8_t* src_mask, int width, int height,
                                     int stride, int32_t* src_s, uint8_t* lab_s) {
    const int2 dims = sample_dims(width, height, stride);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < dims.x * dims.y; k += gridDim.x * blockDim.x) {
        int x, y;
        const size_t idx = sample_pixel(k, dims, stride, width, 0, x, y);
        src_s[k] = src_depth[idx];
        if (lab_s) lab_s[k] = src_mask ? src_mask[idx] : 0;
    }
}

hipError_t launch_sample_source(const int32_t* src_depth, const uint8_t* src_mask, int width, int height, int stride,
                                int32_t* src_s, uint8_t* lab_s, hipStream_t s) {
    hipLaunchKernelGGL(sample_source_kernel, dim3(64), dim3(256), 0, s, src_depth, src_mask, width, height, stride,
                       src_s, lab_s);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Selection (search_env.cpp:1987-2051, 2542-2583) as per-model int64 argmin keys
// ------------------------------------------------------------------------------------------------

__global__ void select_kernel(const float* rc, const float* oc, const int32_t* pose_model, int num_poses,
                              int64_t index_base, int num_models, int64_t* keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int64_t key = PCORE_KEY_NONE_DEV;
    int m = -1;
    if (i < num_poses) {
        m = pose_model[i];
        key = select_key(rc[i], oc[i], m, num_models, index_base + i);
    }
    // wave-level minimum when the wave's poses share one model (the common case)
    const int m0 = __shfl(m, 0);
    const bool uniform = __all(m == m0 || m < 0);
    if (uniform) {
        int64_t k = key;
        for (int off = 32; off > 0; off >>= 1) {
            const int64_t o = __shfl_xor(k, off);
            k = o < k ? o : k;
        }
        if ((threadIdx.x & 63) == 0 && k != PCORE_KEY_NONE_DEV && m0 >= 0 && m0 < num_models)
            atomicMin((unsigned long long*)&keys[m0], (unsigned long long)k);
    } else if (key != PCORE_KEY_NONE_DEV) {
        atomicMin((unsigned long long*)&keys[m], (unsigned long long)key);
    }
}

hipError_t launch_select(const float* rc, const float* oc, const int32_t* pose_model, int num_poses,
                         int64_t index_base, int num_models, int64_t* keys, hipStream_t s) {
    if (num_poses <= 0) return hipSuccess;
    hipLaunchKernelGGL(select_kernel, dim3((num_poses + 255) / 256), dim3(256), 0, s, rc, oc, pose_model, num_poses,
                       index_base, num_models, keys);
    return hipGetLastError();
}

}  // namespace pcore
