// pcore_state_cost.hip -- stage COST of composed states (pcore_evaluate_states; DESIGN.md section 2, "State cost").
// A state is a list of members, indices into a batch of sampled z-buffers (what pcore_evaluate writes to d_dbg_zs).
// Per sample the nearest non-zero depth over the members wins, the lowest list position on ties; the winning samples
// with a positive depth are the state's points, each matched against the observed segment of its owner's label with
// the fused kernel's exact fixed-radius search (pcore_fused.hip, process_points: the same unprojection, box rule,
// (distance, index) minimum and strict radius test, restated here so that the fused kernel's code does not move).
// One workgroup per state; every count is an integer sum, so the result does not depend on scheduling.
#include "pcore_internal.h"

#include <algorithm>
#include <climits>

#include "../../include/pcore.h"

namespace pcore {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kQueue = 2 * kWave;   // point queue entries per wave (< 2 kWave are ever held)
constexpr int kHist = kThreads;     // list positions counted in LDS; the ones beyond go to global atomics
constexpr int kScratchWgsPerCu = 2;  // workgroups per CU of the launch whose explained bitmaps live in context scratch

__device__ __forceinline__ int lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}
// the wave's LDS writes visible to all its lanes
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS_BM: the explained bitmap (one bit per observed point, label-sorted position) in dynamic LDS; otherwise in the
// workgroup's slot of a.scratch_bitmap, written and read with device-scope atomics only (the marks are atomics that
// execute in L2: a plain load could see a line the vector cache kept from the previous state).
template <bool LDS_BM>
__global__ void __launch_bounds__(kThreads) state_cost_kernel(StateCostArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_bitmap[];
    __shared__ int32_t queue_s[kWaves][3 * kQueue];
    __shared__ int32_t hist_vis[kHist], hist_bad[kHist];
    __shared__ int32_t counters[3];  // bad points, explained observed points, points

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nsamp = a.ws * a.hs, ws = a.ws, s = a.stride;
    const bool use_seg = a.pose_label != nullptr;
    uint32_t* const gbm = LDS_BM ? nullptr : a.scratch_bitmap + (size_t)blockIdx.x * a.bitmap_words;
    int32_t* const queue = queue_s[wave];
    constexpr float kBoxRound = 1.0e-6f;  // pcore_fused.hip, process_points
    const float r_eff = sqrtf(a.r2) * 1.0001f + 1e-7f;

    for (int st = blockIdx.x; st < a.num_states; st += gridDim.x) {
        for (int i = tid; i < a.bitmap_words; i += kThreads) {
            if constexpr (LDS_BM) lds_bitmap[i] = 0u;
            else __hip_atomic_store(&gbm[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        hist_vis[tid] = 0;
        hist_bad[tid] = 0;
        if (tid < 3) counters[tid] = 0;
        __syncthreads();

        // the member span; a non-positive one, or one outside the member array, is an empty state
        const int lo = a.state_off[st], hi = a.state_off[st + 1];
        const int M = (lo < 0 || hi > a.num_members || hi <= lo) ? 0 : hi - lo;
        const int32_t* const mem = a.state_member + (M > 0 ? lo : 0);
        int32_t* const mvis = a.out_member_vis && M > 0 ? a.out_member_vis + lo : nullptr;
        int32_t* const mbad = a.out_member_bad && M > 0 ? a.out_member_bad + lo : nullptr;

        int qcount = 0, wave_pts = 0, my_bad = 0;

        auto process_points = [&](int count) {
            wave_lds_fence();
            for (int base = 0; base < count; base += kWave) {
                const int q = base + lane;
                if (q < count) {
                    const int p = queue[3 * q];
                    const int j = queue[3 * q + 1];
                    const int32_t Z = queue[3 * q + 2];
                    const int ky = p / ws, kx = p - ky * ws;
                    // the stage-COST unprojection (compute_point_clouds.cuh:14-22), the fused kernel's expression
                    const float zp = (float)Z / a.depth_factor;
                    const float xp = ((float)(kx * s) - a.cx) / a.fx * zp;
                    const float yp = ((float)(ky * s) - a.cy) / a.fy * zp;
                    const int32_t pl = use_seg ? a.pose_label[mem[j]] : a.num_grids;
                    const bool grid_ok = use_seg ? (pl >= 0 && pl < a.num_grids) : true;
                    float best = INFINITY;
                    int bidx = 0x7fffffff;
                    if (grid_ok) {
                        const LabelGrid g = a.grids[pl];
                        const float rc = r_eff * g.inv_c + kBoxRound * (float)(max(g.nx, max(g.ny, g.nz)) + 2);
                        const float fx0 = (xp - g.ox) * g.inv_c, fy0 = (yp - g.oy) * g.inv_c, fz0 = (zp - g.oz) * g.inv_c;
                        const float lx = fx0 - rc, hx = fx0 + rc, ly = fy0 - rc, hy = fy0 + rc, lz = fz0 - rc, hz = fz0 + rc;
                        if (hx >= 0.0f && lx < (float)g.nx && hy >= 0.0f && ly < (float)g.ny && hz >= 0.0f && lz < (float)g.nz) {
                            const int ix0 = (int)floorf(fmaxf(lx, 0.0f)), ix1 = min(g.nx - 1, (int)floorf(hx));
                            const int iy0 = (int)floorf(fmaxf(ly, 0.0f)), iy1 = min(g.ny - 1, (int)floorf(hy));
                            const int iz0 = (int)floorf(fmaxf(lz, 0.0f)), iz1 = min(g.nz - 1, (int)floorf(hz));
                            // the box spans <= 2 cells per axis while the radius is the observation's (cells >= 2.02 r);
                            // the loops below hold for any span
                            for (int iz = iz0; iz <= iz1; iz++)
                                for (int iy = iy0; iy <= iy1; iy++) {
                                    const int c = g.cell_base + (iz * g.ny + iy) * g.nx + ix0;
                                    const int cb = a.cell_start[c], ce = a.cell_start[c + 1 + (ix1 - ix0)];
                                    for (int pi = cb; pi < ce; pi++) {
                                        const float4 o = a.grid_pts[pi];
                                        const float dx = xp - o.x, dy = yp - o.y, dz = zp - o.z;
                                        const float d = dx * dx + dy * dy + dz * dz;
                                        const int oi = __float_as_int(o.w);
                                        const bool take = d < best || (d == best && oi < bidx);
                                        best = take ? d : best;
                                        bidx = take ? oi : bidx;
                                    }
                                }
                        }
                    }
                    const bool is_bad = best > a.r2;  // strict: a point at the radius is explained
                    if (!is_bad && bidx != 0x7fffffff) {
                        const int bit = a.seg_lo[pl] + bidx;  // label-sorted position of the neighbour
                        if constexpr (LDS_BM) atomicOr(&lds_bitmap[bit >> 5], 1u << (bit & 31));
                        else atomicOr(&gbm[bit >> 5], 1u << (bit & 31));
                    }
                    my_bad += is_bad ? 1 : 0;
                    if (j < kHist) {
                        atomicAdd(&hist_vis[j], 1);
                        if (is_bad) atomicAdd(&hist_bad[j], 1);
                    } else {
                        if (mvis) atomicAdd(&mvis[j], 1);
                        if (mbad && is_bad) atomicAdd(&mbad[j], 1);
                    }
                }
            }
            wave_lds_fence();
        };

        for (int base = wave * kWave; base < nsamp; base += kThreads) {
            const int p = base + lane;
            int32_t best = 0;
            int owner = -1;
            if (p < nsamp) {
                for (int j = 0; j < M; j++) {
                    const int m = mem[j];
                    if (m < 0 || m >= a.num_poses) continue;  // contributes nothing
                    const int32_t z = a.zs[(size_t)m * nsamp + p];
                    // strict '<' over the non-zero depths: the lowest list position attaining the minimum owns the sample
                    if (z != 0 && (owner < 0 || z < best)) {
                        best = z;
                        owner = j;
                    }
                }
            }
            const bool valid = owner >= 0 && best > 0;  // depth_to_mask: a negative minimum hides and yields no point
            const uint64_t bv = __ballot(valid);
            if (valid) {
                const int q = qcount + lanes_below(bv);
                queue[3 * q] = p;
                queue[3 * q + 1] = owner;
                queue[3 * q + 2] = best;
            }
            qcount += __popcll(bv);
            wave_pts += __popcll(bv);
            if (qcount >= kWave) {
                process_points(qcount);
                qcount = 0;
            }
        }
        if (qcount > 0) process_points(qcount);

        for (int off = 32; off > 0; off >>= 1) my_bad += __shfl_xor(my_bad, off);
        if (lane == 0) {
            atomicAdd(&counters[0], my_bad);
            atomicAdd(&counters[2], wave_pts);
        }
        __syncthreads();  // every point counted and marked
        int my_expl = 0;
        for (int w = tid; w < a.bitmap_words; w += kThreads) {
            if constexpr (LDS_BM) my_expl += __popc(lds_bitmap[w]);
            else my_expl += __popc(__hip_atomic_load(&gbm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        for (int off = 32; off > 0; off >>= 1) my_expl += __shfl_xor(my_expl, off);
        if (lane == 0) atomicAdd(&counters[1], my_expl);
        if (tid < M) {  // positions beyond kHist were counted in place (zero before the launch)
            if (mvis) mvis[tid] = hist_vis[tid];
            if (mbad) mbad[tid] = hist_bad[tid];
        }
        __syncthreads();

        // the costs in orc_costs' float order (compute_costs.cuh:362-446), as the fused kernel writes them
        if (tid == 0) {
            const float num = (float)counters[2];
            const float badf = (float)counters[0];
            const float rendered_explained = num - badf;
            float rc = (num == 0.0f) ? -1.0f : badf / num;
            rc = (rc == -1.0f) ? -1.0f : rc * 100.0f;
            a.out_rc[st] = rc;
            if (a.calc_obs) {
                const float expl = (float)counters[1];
                const float tot = a.state_obs_total[st];
                a.out_diff[st] = rendered_explained - expl;
                float oc = tot - expl;
                oc = oc / tot;
                a.out_oc[st] = oc * 100.0f;
            } else {
                if (a.out_oc) a.out_oc[st] = 0.0f;
                if (a.out_diff) a.out_diff[st] = 0.0f;
            }
        }
        __syncthreads();  // the counters are read before the next state clears them
    }
}

}  // namespace

int state_cost_scratch_blocks(int num_states, const DeviceInfo& d) {
    return std::min(num_states, std::max(1, d.num_cus) * kScratchWgsPerCu);
}

hipError_t launch_state_cost(const StateCostArgs& a, const DeviceInfo& d, hipStream_t s) {
    if (a.num_states <= 0) return hipSuccess;
    if (a.scratch_bitmap)
        hipLaunchKernelGGL(state_cost_kernel<false>, dim3(state_cost_scratch_blocks(a.num_states, d)), dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL(state_cost_kernel<true>, dim3(a.num_states), dim3(kThreads),
                           (size_t)a.bitmap_words * sizeof(uint32_t), s, a);
    return hipGetLastError();
}

}  // namespace pcore
