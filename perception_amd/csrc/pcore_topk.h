// pcore_topk.h -- launcher of pcore_topk.hip (the k smallest select keys per model), for pcore_api.hip (pcore_select_topk).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcore {

// partial lists (slices) a batch of num_poses is cut into
int topk_slices(int num_poses);
// part: scratch of topk_slices(num_poses) x num_models x k keys (one partial list per slice and model); topk:
// num_models x k keys, folded in place
hipError_t launch_select_topk(const float* rc, const float* oc, const int32_t* pose_model, int num_poses,
                              int64_t index_base, int num_models, int k, int64_t* part, int64_t* topk, hipStream_t s);

}  // namespace pcore
