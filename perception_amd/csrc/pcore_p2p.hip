// pcore_p2p.hip -- point-to-plane ICP of rendered clouds against the projective scene of the observation's depth image
// ("Point-to-plane ICP spec"; the arithmetic is pcore_p2p_math.h's): the reference's
// ICP_Point2Plane (cuda_icp/icp.cu:157-218) with Scene_projective (depth_scene.h) and the linemod normals of
// get_normal (scene/common.cpp:17-107).
//
// scene_kernel: one thread per pixel writes the pixel's point (dep2pcd) and normal, each as a float4, so that a query
// is two 16-byte loads.
//
// p2p_icp_kernel: one one-wave workgroup per pose, as planar_icp_kernel (pcore_icp2d.hip): the hardware dispatcher is
// the pose queue, and there is no barrier, no wait loop and no LDS.  A pose is a serial chain of at most
// max_iterations + 1 passes over its slot; a pass moves every point by the previous pass's increment (stored back in
// place), projects it, gathers the scene point and normal of its pixel -- both loads issued unconditionally at a
// clamped index, the row masked afterwards -- and adds the 29-term row into the lane's sums.  After the xor butterfly
// every lane holds the same sums, and the exit tests, the 6 x 6 LDLT and the increment run uniformly in all lanes.
#include "pcore_internal.h"
#include "pcore_p2p_math.h"

namespace pcore {

namespace {

__global__ void __launch_bounds__(256) scene_kernel(const int32_t* __restrict__ depth, int W, int H, float fx, float fy,
                                                    float cx, float cy, float4* __restrict__ pcd4,
                                                    float4* __restrict__ nrm4, float* __restrict__ pcd3,
                                                    float* __restrict__ nrm3) {
    const size_t npx = (size_t)W * H;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * W);
    const int32_t raw = depth[i];
    // dep2pcd of the CV_32S value read as uint32 (depth_scene.cpp:24-29)
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    const uint32_t dep = (uint32_t)raw;
    if (dep != 0) {
        pz = (float)dep / 100.0f;
        px = ((float)x - cx) / fx * pz;
        py = ((float)y - cy) / fy * pz;
    }
    // get_normal: CV_32S -> CV_16U (saturate), then the linemod normal where it is defined
    auto sat16 = [](int32_t v) { return (long long)(v < 0 ? 0 : (v > 65535 ? 65535 : v)); };
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    constexpr int r = p2p::kLinemodRadius;
    const long long d = sat16(raw);
    if (d < p2p::kLinemodMaxDepth && y >= r && y < H - r - 1 && x >= r && x < W - r - 1) {
        const int32_t* line = depth + i;
        const ptrdiff_t rw = (ptrdiff_t)r * W;
        const long long nb[8] = {sat16(line[-r - rw]), sat16(line[-rw]), sat16(line[r - rw]), sat16(line[-r]),
                                 sat16(line[r]),       sat16(line[-r + rw]), sat16(line[rw]), sat16(line[r + rw])};
        long long det, ddx, ddy;
        p2p::linemod_sums(d, nb, det, ddx, ddy);
        float ax = fx * (float)ddx;
        float ay = fy * (float)ddy;
        float az = (float)(-det * d);
        const float sq = sqrtf(ax * ax + ay * ay + az * az);
        if (sq > 0) {
            const float inv = 1.0f / sq;
            nx = ax * inv;
            ny = ay * inv;
            nz = az * inv;
        }
    }
    if (pcd4) pcd4[i] = make_float4(px, py, pz, 0.0f);
    if (nrm4) nrm4[i] = make_float4(nx, ny, nz, 0.0f);
    if (pcd3) {
        pcd3[3 * i] = px;
        pcd3[3 * i + 1] = py;
        pcd3[3 * i + 2] = pz;
    }
    if (nrm3) {
        nrm3[3 * i] = nx;
        nrm3[3 * i + 1] = ny;
        nrm3[3 * i + 2] = nz;
    }
}

// The 64 lanes' partial sums into every lane: an xor butterfly, masks 32, 16, 8, 4, 2, 1 (both lanes of a pair add the
// same two values, so all lanes end with the same bits).
__device__ __forceinline__ void wave_sum(p2p::Sums& S) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < p2p::kRow; k++) S.v[k] = S.v[k] + __shfl_xor(S.v[k], m, 64);
}

// NN: the query of the nearest-neighbour scene (p2p::nn_query) in the projective one's place; nothing else differs.
template <bool NN>
__device__ void p2p_pose(const P2pArgs& a, int pose, int lane) {
    float4* slot = a.src + (size_t)pose * a.src_cap;
    int n = __builtin_amdgcn_readfirstlane(a.src_count[pose]);
    n = n < 0 ? 0 : (n > a.src_cap ? a.src_cap : n);
    p2p::Mat4 T = p2p::identity(), E = p2p::identity();
    float fitness = 0.0f, rmse = 0.0f;
    int ret = a.max_iter;
    for (int iter = 0; iter <= a.max_iter; iter++) {
        p2p::Sums S;
#pragma unroll
        for (int k = 0; k < p2p::kRow; k++) S.v[k] = 0.0f;
        for (int i = lane; i < n; i += 64) {  // lane i mod 64 owns point i in every pass
            float4 p = slot[i];
            if (iter > 0) {  // the previous pass's increment, in place (transform_pcd)
                float qx, qy, qz;
                p2p::apply(E, p.x, p.y, p.z, qx, qy, qz);
                p = make_float4(qx, qy, qz, p.w);
                slot[i] = p;
            }
            size_t idx;
            bool in;
            float d2 = 0.0f;
            if constexpr (NN) {
                in = p2p::nn_query(a.scene_pcd, a.width, a.height, a.fx, a.fy, a.cx, a.cy, a.window, a.max_dist_diff,
                                   p.x, p.y, p.z, idx, d2);
            } else {
                int x, y;
                const bool okx = p2p::pixel(p.x, p.z, a.fx, a.cx, x);
                const bool oky = p2p::pixel(p.y, p.z, a.fy, a.cy, y);
                in = okx && oky && x >= 0 && x < a.width && y >= 0 && y < a.height;
                idx = in ? (size_t)x + (size_t)y * (size_t)a.width : 0;
            }
            const float4 d = a.scene_pcd[idx];
            const float4 nn = a.scene_normal[idx];
            const bool ok = in && (NN ? d2 < a.max_dist_diff * a.max_dist_diff : p2p::accept(p.z, d.z, a.max_dist_diff));
            float r[p2p::kRow];
            p2p::row(p.x, p.y, p.z, d.x, d.y, d.z, nn.x, nn.y, nn.z, r);
#pragma unroll
            for (int k = 0; k < p2p::kRow; k++) S.v[k] = ok ? S.v[k] + r[k] : S.v[k];  // a rejected point adds nothing
        }
        wave_sum(S);
        const float prev_fit = fitness, prev_rmse = rmse;
        const float count = S.v[28], total = S.v[27];
        if (count == 0) {
            ret = iter;
            break;
        }
        fitness = count / (float)n;
        rmse = sqrtf(total / count);
        if (iter == a.max_iter) {
            ret = iter;
            break;
        }
        const float df = fitness - prev_fit, dr = rmse - prev_rmse;
        if (fabsf(df) < a.rel_fitness && fabsf(dr) < a.rel_rmse) {
            ret = iter;
            break;
        }
        double u[6];
        p2p::ldlt_solve6(S.v, u);
        E = p2p::vec6_to_mat4(u);
        T = p2p::mat4_mul(E, T);
    }
    if (lane == 0) {
        const size_t o = (size_t)a.pose_base + pose;
        float* t = a.out_T + 16 * o;
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) t[4 * r + c] = T.m[r][c];
        a.out_fitness[o] = fitness;
        a.out_rmse[o] = rmse;
        a.out_iters[o] = ret;
        if (a.poses_out) {  // concatenate_transforms (renderer.cu:1412-1429), as pcore_gicp.hip's write_pose
            const float* pin = a.poses_in + 16 * o;
            float A[4][4];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) A[r][c] = r < 3 ? pin[4 * r + c] / 100.0f : pin[4 * r + c];
            float* pout = a.poses_out + 16 * o;
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float v = T.m[r][0] * A[0][c] + T.m[r][1] * A[1][c] + T.m[r][2] * A[2][c] + T.m[r][3] * A[3][c];
                    pout[4 * r + c] = r < 3 ? (float)((double)v * 100) : v;
                }
        }
    }
}

__global__ void __launch_bounds__(64) p2p_icp_kernel(P2pArgs a, int num_poses) {
    const int pose = blockIdx.x;  // chunk-local
    if (pose < num_poses) p2p_pose<false>(a, pose, threadIdx.x);
}

__global__ void __launch_bounds__(64) p2p_icp_nn_kernel(P2pArgs a, int num_poses) {
    const int pose = blockIdx.x;  // chunk-local
    if (pose < num_poses) p2p_pose<true>(a, pose, threadIdx.x);
}

}  // namespace

hipError_t launch_p2p_icp(const P2pArgs& a, int num_poses, hipStream_t s) {
    if (num_poses <= 0) return hipSuccess;
    hipLaunchKernelGGL(p2p_icp_kernel, dim3(num_poses), dim3(64), 0, s, a, num_poses);
    return hipGetLastError();
}

hipError_t launch_p2p_nn_icp(const P2pArgs& a, int num_poses, hipStream_t s) {
    if (num_poses <= 0) return hipSuccess;
    hipLaunchKernelGGL(p2p_icp_nn_kernel, dim3(num_poses), dim3(64), 0, s, a, num_poses);
    return hipGetLastError();
}

hipError_t launch_p2p_scene(const int32_t* depth_cm, int width, int height, float fx, float fy, float cx, float cy,
                            float4* pcd4, float4* normal4, float* pcd3, float* normal3, hipStream_t s) {
    const size_t npx = (size_t)width * height;
    if (npx == 0) return hipSuccess;
    hipLaunchKernelGGL(scene_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, depth_cm, width, height, fx,
                       fy, cx, cy, pcd4, normal4, pcd3, normal3);
    return hipGetLastError();
}

}  // namespace pcore
