// pcore_topk.hip -- the k best candidates per model (pcore_select_topk): pcore_select's keys, the k smallest of every
// model instead of the minimum alone, so a caller can refine a shortlist without reading N costs back.
//
// A wave holds a candidate list as one key per lane, ascending (lanes the list does not fill hold PCORE_KEY_NONE).  Keys
// carry the global index, so they are distinct and the list of a set of keys is one fixed sequence: the result cannot
// depend on the order in which keys arrive, on how a batch is cut or on scheduling.
//
// Kernels (one wave per workgroup, plain stores, no atomics)
//   topk_partial_kernel   wave (slice, model) streams its slice 64 poses at a time; a step whose keys all lie at or above
//                         the list's k-th (one ballot) costs nothing more, any other step sorts its 64 keys and merges
//                         them into the list.  Writes one partial list per (slice, model).
//   topk_fold_kernel      wave (model) merges the row's previous content and the slices' partial lists, writes the row.
#include "../../include/pcore.h"
#include "pcore_raster.h"
#include "pcore_topk.h"

#include <algorithm>

namespace pcore {

__device__ __forceinline__ int64_t key_min(int64_t a, int64_t b) { return b < a ? b : a; }
__device__ __forceinline__ int64_t key_max(int64_t a, int64_t b) { return b < a ? a : b; }

// bitonic merge of a wave's bitonic sequence (one key per lane) into ascending order: 6 compare-exchange steps
__device__ __forceinline__ int64_t bitonic_merge64(int64_t v, int lane) {
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const int64_t o = __shfl_xor(v, j);
        v = (lane & j) ? key_max(v, o) : key_min(v, o);
    }
    return v;
}

// bitonic sort of a wave's 64 keys into ascending order: 21 compare-exchange steps
__device__ __forceinline__ int64_t bitonic_sort64(int64_t v, int lane) {
#pragma unroll
    for (int k2 = 2; k2 <= kWave; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int64_t o = __shfl_xor(v, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k2) == 0);
            v = keep_min ? key_min(v, o) : key_max(v, o);
        }
    return v;
}

// the 64 smallest of two ascending lists, ascending: list[i] against the other list reversed is a bitonic sequence
// whose lane-wise minimum holds exactly those 64 (the first step of a 128-key bitonic merge)
__device__ __forceinline__ int64_t merge_lists(int64_t list, int64_t other_sorted, int lane) {
    const int64_t rev = __shfl(other_sorted, kWave - 1 - lane);
    return bitonic_merge64(key_min(list, rev), lane);
}

__global__ __launch_bounds__(kWave) void topk_partial_kernel(const float* __restrict__ rc, const float* __restrict__ oc,
                                                             const int32_t* __restrict__ pose_model, int num_poses,
                                                             int64_t index_base, int num_models, int k, int slice_len,
                                                             int64_t* __restrict__ part) {
    const int lane = threadIdx.x;
    const int lo = blockIdx.x * slice_len;  // slices * slice_len < 2^31 + slice_len: see launch_select_topk
    const int hi = (int)min((int64_t)lo + slice_len, (int64_t)num_poses);
    for (int m = blockIdx.y; m < num_models; m += gridDim.y) {
        int64_t list = PCORE_KEY_NONE_DEV;  // this lane's entry
        int64_t kth = PCORE_KEY_NONE_DEV;   // the list's k-th entry (wave-uniform): only smaller keys can enter
        for (int i0 = lo; i0 < hi; i0 += kWave) {
            const int i = i0 + lane;
            int64_t key = PCORE_KEY_NONE_DEV;
            if (i < hi && pose_model[i] == m) key = select_key(rc[i], oc[i], m, num_models, index_base + i);
            if (__ballot(key < kth) == 0) continue;  // wave-uniform
            list = merge_lists(list, bitonic_sort64(key, lane), lane);
            kth = __shfl(list, k - 1);
        }
        if (lane < k) part[((size_t)blockIdx.x * num_models + m) * k + lane] = list;
    }
}

__global__ __launch_bounds__(kWave) void topk_fold_kernel(const int64_t* __restrict__ part, int num_slices, int num_models,
                                                          int k, int64_t* topk) {
    const int lane = threadIdx.x;
    const int m = blockIdx.x;
    // the row as the caller left it: ascending by contract; sorted here all the same, so that a row in any order folds
    // to the same list
    int64_t list = bitonic_sort64(lane < k ? topk[(size_t)m * k + lane] : PCORE_KEY_NONE_DEV, lane);
    int64_t kth = __shfl(list, k - 1);
    for (int s = 0; s < num_slices; s++) {
        const int64_t p = lane < k ? part[((size_t)s * num_models + m) * k + lane] : PCORE_KEY_NONE_DEV;
        if (!(__shfl(p, 0) < kth)) continue;  // the partial list's smallest key cannot enter: none of it can
        list = merge_lists(list, p, lane);
        kth = __shfl(list, k - 1);
    }
    if (lane < k) topk[(size_t)m * k + lane] = list;
}

// Poses per partial list: kTopkSlice, or more for batches above kTopkSlice * kTopkMaxSlices poses, so that the partial
// lists of a batch never exceed kTopkMaxSlices per model.  A multiple of the wave.
constexpr int kTopkSlice = PCORE_TOPK_SLICE;
constexpr int kTopkMaxSlices = 1024;

int topk_slice_len(int num_poses) {
    const int per = (num_poses + kTopkMaxSlices - 1) / kTopkMaxSlices;
    return std::max(kTopkSlice, (per + kWave - 1) / kWave * kWave);
}

int topk_slices(int num_poses) {
    const int len = topk_slice_len(num_poses);
    return (int)(((int64_t)num_poses + len - 1) / len);
}

hipError_t launch_select_topk(const float* rc, const float* oc, const int32_t* pose_model, int num_poses,
                              int64_t index_base, int num_models, int k, int64_t* part, int64_t* topk, hipStream_t s) {
    if (num_poses <= 0) return hipSuccess;
    const int len = topk_slice_len(num_poses), slices = topk_slices(num_poses);
    // (slices - 1) * len < num_poses <= 2^31 - 1, so the kernel's slice start fits an int
    hipLaunchKernelGGL(topk_partial_kernel, dim3(slices, std::min(num_models, 65535)), dim3(kWave), 0, s, rc, oc,
                       pose_model, num_poses, index_base, num_models, k, len, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(topk_fold_kernel, dim3(num_models), dim3(kWave), 0, s, part, slices, num_models, k, topk);
    return hipGetLastError();
}

}  // namespace pcore
