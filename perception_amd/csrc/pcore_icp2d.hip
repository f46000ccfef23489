// pcore_icp2d.hip -- planar (x, y, yaw) ICP of rendered clouds onto the observation ("Planar ICP
// spec"; the arithmetic is pcore_icp2d_math.h's): the reference's GetICPAdjustedPosesCPU loop between the two GPU
// passes of the 3-DoF search (search_env.cpp:1198-1299, 6235-6396), one wave per pose.
//
// A pose is a serial chain of at most max_iterations iterations; an iteration is one nearest-target search per source
// point and a wave reduction of ten sums.  The launch is one one-wave workgroup per pose: the hardware dispatcher is
// the pose queue (a wave whose pose leaves early frees its slot for the next workgroup at once), and no barrier exists
// anywhere in the kernel.  (A persistent wave that fetches its next pose with `if (lane == 0) q = atomicAdd(..)` and
// readfirstlane(q), GICP's queue without its LDS hop, was built first: the compiler threaded the lane-0 branch through
// the readfirstlane, and the lanes other than 0 re-ran pose 0 for ever.)  The source points stream from the pose's slot every iteration (a coalesced 16-byte load per point, small beside the search's scattered
// ones), which serves clouds of any size -- up to the whole sampled image -- with one path.
#include "pcore_internal.h"
#include "pcore_icp2d_math.h"

#include <algorithm>
#include <climits>

namespace pcore {

namespace {

// The cell of a world coordinate along one axis: build_grid's float formula (pcore_prep.h), monotone in v.
__device__ __forceinline__ float cell_coord(float v, float o, float inv_c) { return (v - o) * inv_c; }
__device__ __forceinline__ int cell_clamp(float f, int n) {
    const int i = (int)floorf(fmaxf(f, 0.0f));
    return i < n - 1 ? i : n - 1;
}

// The nearest target of a query among those within the radius: the lexicographic minimum of (float squared distance,
// index as set), so the brute force's first minimum, for every query that has a target with d^2 <= r^2; `best` stays
// above r2 (or +inf) otherwise, and the caller rejects the pair.  Targets farther than r cannot be kept, so only the
// cells the query's radius box touches are read: the box is padded (0.5 % of r and 4 ulp of the coordinate) so that
// float rounding never drops a target within r, and the cell formula is monotone, so a target inside the box lies in
// a cell between the box corners' cells.  The query's own cell goes first; another cell is skipped when its nearest
// face is farther than the best distance so far (the faces pulled outwards by a margin that covers the rounding of
// the cell formula).  A non-finite query has no pair.
__device__ __forceinline__ void planar_nn(const PlanarArgs& a, float qx, float qy, float qz, float& best, float& tx,
                                          float& ty) {
    best = INFINITY;
    tx = 0.0f;
    ty = 0.0f;
    const LabelGrid& G = a.grid;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz)) || G.pt_count <= 0) return;
    const float rb = a.r * 1.005f;
    const float px = rb + fabsf(qx) * 4.8e-7f, py = rb + fabsf(qy) * 4.8e-7f, pz = rb + fabsf(qz) * 4.8e-7f;
    // wholly outside the targets' box: below the minimum (the grid's origin is the targets' exact minimum), or in a
    // cell past the last one (every target's cell coordinate is below n)
    if (qx + px < G.ox || qy + py < G.oy || qz + pz < G.oz) return;
    const float flx = cell_coord(qx - px, G.ox, G.inv_c), fly = cell_coord(qy - py, G.oy, G.inv_c),
                flz = cell_coord(qz - pz, G.oz, G.inv_c);
    if (flx >= (float)G.nx || fly >= (float)G.ny || flz >= (float)G.nz) return;
    const int x0 = cell_clamp(flx, G.nx), x1 = cell_clamp(cell_coord(qx + px, G.ox, G.inv_c), G.nx);
    const int y0 = cell_clamp(fly, G.ny), y1 = cell_clamp(cell_coord(qy + py, G.oy, G.inv_c), G.ny);
    const int z0 = cell_clamp(flz, G.nz), z1 = cell_clamp(cell_coord(qz + pz, G.oz, G.inv_c), G.nz);
    int j = INT_MAX;
    auto visit = [&](int cell) {
        const int b = a.cell_start[cell], e = a.cell_start[cell + 1];
        for (int pi = b; pi < e; pi++) {
            const float4 o = a.grid_pts[pi];
            const float d = icp2d::sqdist(qx, qy, qz, o.x, o.y, o.z);
            const int oi = __float_as_int(o.w);
            if (d < best || (d == best && oi < j)) {
                best = d;
                j = oi;
                tx = o.x;
                ty = o.y;
            }
        }
    };
    const int hx = min(max(cell_clamp(cell_coord(qx, G.ox, G.inv_c), G.nx), x0), x1);
    const int hy = min(max(cell_clamp(cell_coord(qy, G.oy, G.inv_c), G.ny), y0), y1);
    const int hz = min(max(cell_clamp(cell_coord(qz, G.oz, G.inv_c), G.nz), z0), z1);
    visit((hz * G.ny + hy) * G.nx + hx);
    // margins of a cell's faces: 1e-4 of the cell for the cell formula's rounding (below 2e-5 of a cell at 64 cells
    // per axis) and 4 ulp of the largest coordinate for the faces' own
    const float mx = G.cell * 1e-4f + (fabsf(G.ox) + (float)G.nx * G.cell) * 5e-7f;
    const float my = G.cell * 1e-4f + (fabsf(G.oy) + (float)G.ny * G.cell) * 5e-7f;
    const float mz = G.cell * 1e-4f + (fabsf(G.oz) + (float)G.nz * G.cell) * 5e-7f;
    auto gap = [](float q, float o, float cell, int i, float m) {
        const float lo = o + (float)i * cell - m, hi = o + (float)(i + 1) * cell + m;
        return fmaxf(fmaxf(lo - q, q - hi), 0.0f);
    };
    for (int iz = z0; iz <= z1; iz++) {
        const float gz = gap(qz, G.oz, G.cell, iz, mz);
        for (int iy = y0; iy <= y1; iy++) {
            const float gy = gap(qy, G.oy, G.cell, iy, my);
            for (int ix = x0; ix <= x1; ix++) {
                if (ix == hx && iy == hy && iz == hz) continue;
                const float gx = gap(qx, G.ox, G.cell, ix, mx);
                const float g2 = (gx * gx + gy * gy + gz * gz) * 0.9999f;
                if (g2 > fminf(best, a.r2)) continue;  // every target of the cell is farther: neither nearer nor kept
                visit((iz * G.ny + iy) * G.nx + ix);
            }
        }
    }
}

// The 64 lanes' partial sums into every lane: an xor butterfly, masks 32, 16, 8, 4, 2, 1 (both lanes of a pair add the
// same two values, so all lanes end with the same bits).
__device__ __forceinline__ void wave_sum(icp2d::Sums& S) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < icp2d::kSumTerms; k++) S.v[k] = S.v[k] + __shfl_xor(S.v[k], m, 64);
}

__device__ void planar_pose(const PlanarArgs& a, int pose, int lane) {
    float4* slot = a.src + (size_t)pose * a.src_cap;
    const int ns = __builtin_amdgcn_readfirstlane(a.src_count[pose]);
    // the slot into the world frame, in place: lane i mod 64 owns point i here and in every iteration
    for (int i = lane; i < ns; i += 64) {
        const float4 p = slot[i];
        float wx, wy, wz;
        icp2d::to_world(a.m, p.x, p.y, p.z, wx, wy, wz);
        slot[i] = make_float4(wx, wy, wz, 0.0f);
    }
    icp2d::Xform G = {1.0, 0.0, 0.0, 0.0};
    int iters = 0, status = icp2d::kIterationCap;
    double mse = 0.0, prev = icp2d::kDblMax;
    if (ns <= 0) {
        status = icp2d::kEmptyRender;
    } else if (a.max_iter > 0) {
        for (;;) {
            icp2d::Sums S;
#pragma unroll
            for (int k = 0; k < icp2d::kSumTerms; k++) S.v[k] = 0.0;
            for (int i = lane; i < ns; i += 64) {
                const float4 p = slot[i];
                float qx, qy, best, tx, ty;
                icp2d::query(G, p.x, p.y, qx, qy);
                planar_nn(a, qx, qy, p.z, best, tx, ty);
                if (best <= a.r2) icp2d::accumulate(S, qx, qy, tx, ty, best);  // a rejected pair adds nothing
            }
            wave_sum(S);
            if (S.v[0] < (double)icp2d::kMinPairs) {
                status = icp2d::kNoCorrespondences;
                G = {1.0, 0.0, 0.0, 0.0};
                mse = 0.0;
                break;
            }
            const icp2d::Xform d = icp2d::step(S);
            G = icp2d::compose(d, G);
            iters++;
            mse = S.v[9] / S.v[0];
            const int st = icp2d::exit_test(iters, a.max_iter, d, mse, prev, a.eps_t, a.eps_fit);
            prev = mse;
            if (st >= 0) {
                status = st;
                break;
            }
        }
    }
    if (lane == 0) {
        const size_t o = (size_t)a.pose_base + pose;
        a.out_xform[4 * o] = G.c;
        a.out_xform[4 * o + 1] = G.s;
        a.out_xform[4 * o + 2] = G.tx;
        a.out_xform[4 * o + 3] = G.ty;
        a.out_iters[o] = iters;
        a.out_status[o] = status;
        if (a.out_mse) a.out_mse[o] = mse;
    }
}

__global__ void __launch_bounds__(64) planar_icp_kernel(PlanarArgs a, int num_poses) {
    const int pose = blockIdx.x;  // chunk-local
    if (pose < num_poses) planar_pose(a, pose, threadIdx.x);
}

__global__ void __launch_bounds__(64) planar_step_test_kernel(const double* sums, double* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    icp2d::Sums S;
    for (int k = 0; k < icp2d::kSumTerms; k++) S.v[k] = sums[(size_t)icp2d::kSumTerms * i + k];
    const icp2d::Xform d = icp2d::step(S);
    out[4 * (size_t)i] = d.c;
    out[4 * (size_t)i + 1] = d.s;
    out[4 * (size_t)i + 2] = d.tx;
    out[4 * (size_t)i + 3] = d.ty;
}

}  // namespace

hipError_t launch_planar_icp(const PlanarArgs& a, int num_poses, hipStream_t s) {
    if (num_poses <= 0) return hipSuccess;
    hipLaunchKernelGGL(planar_icp_kernel, dim3(num_poses), dim3(64), 0, s, a, num_poses);
    return hipGetLastError();
}

hipError_t launch_planar_step_test(const double* sums, double* out, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(planar_step_test_kernel, dim3((n + 63) / 64), dim3(64), 0, s, sums, out, n);
    return hipGetLastError();
}

}  // namespace pcore
