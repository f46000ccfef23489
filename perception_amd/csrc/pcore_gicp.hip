// pcore_gicp.hip -- per-pose GICP refinement on gfx950.
//
// Build-owned spec (fast_gicp is an un-vendored fork; see DESIGN.md "GICP spec"): fast_gicp's published
// FastGICP + LsqRegistration algorithm at the reference's settings (renderer.cu:1693-1720): k = 10 covariance
// neighbours with PLANE regularisation, nearest-neighbour correspondences inside the pose's label segment,
// Mahalanobis (C_t + R C_s R^T)^-1, Levenberg-Marquardt steps on SE(3) through the exact se3_exp, <= 150
// iterations, rotation / translation epsilons 2e-3 / 5e-4.  The arithmetic lives in pcore_gicp_math.h; its
// order -- including the reduction tree of the normal equations and of the trial errors -- is fixed, and the
// CPU oracle (oracle/pcore_oracle.cpp, orc_gicp) follows the same order, so the refined transforms are
// reproducible bit for bit.
//
//   covariance_kernel  one wave per segment (a pose's rendered cloud or an observed label): brute-force
//                      k-NN of every point inside its segment (candidates staged through LDS), double
//                      mean / covariance, Jacobi (<= 6 sweeps, thresholded), PLANE regularisation.
//   gicp_kernel        one wave per pose: per-lane sequential partial sums of J^T M J / J^T M e / e^T M e,
//                      the shuffle-down tree in registers (wave_tree_sums), the LM iteration (uniform: the
//                      damped solve by 3x3 block elimination, se3_exp, the trial), the correspondence history, then
//                      concatenate_transforms (renderer.cu:1412-1429).
//   gicp_wide_kernel   small batches: eight waves search a pose's correspondences, wave 0 as gicp_kernel.
//
// Here: the kernels, the per-pose state they iterate on and the launchers.  What they are built from lies beside it:
//   pcore_wave.h        wave primitives: wave_lds_sync, opaque_zero, uniform_d / uniform_f, wave_tree_sums, wave_sum_lane0
//   pcore_nn_grid.h     the exact grid-shell neighbour search: grid_shells, grid_nn, knn_insert_lex, sqdist3
//   pcore_gicp_scan.h   the scalar-cache key scan: scan_quads, scan_quads2 (PCORE_SCAN_UNROLL, PCORE_SCAN2_UNROLL)
//   pcore_gicp_ring.h   float transforms as bit patterns in LDS rings: xform_float, xf_lane_words, ring_match16, CycleExit
//   pcore_gicp_probe.h  the measurement builds: GPROF_* (PCORE_GICP_PROFILE), GTL_* (PCORE_GICP_TIMELINE)
// and pcore_cov.h (the covariances' k-NN rounds), pcore_gicp_math.h (the arithmetic shared with the oracle).
#include "pcore_internal.h"

#include <hipcub/hipcub.hpp>
#include "pcore_cov.h"
#include "pcore_gicp_math.h"
#include "pcore_gicp_probe.h"
#include "pcore_gicp_ring.h"
#include "pcore_gicp_scan.h"
#include "pcore_nn_grid.h"
#include "pcore_wave.h"

#include <algorithm>
#include <cstdlib>
#include <cfloat>
#include <climits>

#pragma clang fp contract(off)

namespace pcore {

namespace {

constexpr int kGThreads = 256;
constexpr int kMaxK = 16;

// se3_exp's series coefficients as the kernels read them: an LDS copy through an address-space-3 pointer offset by an
// opaque zero produced inside the iteration loop, so the loads cannot be hoisted out of it (as literal constants they
// were hoisted into 64 VGPRs for the whole kernel; a generic pointer made them flat loads) but can be issued together
// ahead of the series (a volatile pointer serialised them: one LDS round trip per coefficient, 32 in a row)
typedef __attribute__((address_space(3))) const double lds_cvd;

}  // namespace

// ------------------------------------------------------------------------------------------------
// covariances
// ------------------------------------------------------------------------------------------------
// One wave per segment (a pose's rendered cloud or an observed label), one lane per point in rounds of 64 (pcore_cov.h
// cov_knn_round); a 256-thread workgroup per segment left two of its four waves idle on C3's ~111-point clouds.
// C3: 2.65 -> 2.61 ms per 50 k clouds -- the time is the insertion block, which the wave runs whenever any lane
// inserts (k ln(n / k) + k insertions per point), not the candidate loads.
template <int KMAX, bool KFIXED = false>
__global__ void __launch_bounds__(kCovLanes) covariance_kernel(const float4* pts, const int32_t* seg_off,
                                                               const int32_t* seg_cnt, int seg_stride, int k_arg,
                                                               double* cov_out, int max_n) {
    __shared__ float4 tile[kCovLanes];
    const int sg = blockIdx.x;
    const int off = seg_off ? seg_off[sg] : sg * seg_stride;
    const int n = seg_cnt[sg];
    if (n > max_n) return;  // covariance_grid_kernel's segment
    const int lane = threadIdx.x;
    for (int i0 = 0; i0 < n; i0 += kCovLanes)
        cov_knn_round<KMAX, KFIXED>(pts + off, n, k_arg, i0, lane, tile, cov_out + (size_t)6 * off);
}

// The rendered clouds' covariances (k = 10): the threshold k-NN where the cloud's sample grid allows it, else the brute
// force, round by round (pcore_cov.h); bit-identical either way.  Dynamic LDS: kThrLdsBytes.
#ifndef PCORE_COV_WAVES_PER_EU
#define PCORE_COV_WAVES_PER_EU 8  // 64 VGPRs (7 spilled): 8 waves per SIMD, which the 4-granule LDS allows (pcore_cov.h)
#endif
// One rendered cloud's covariances by one wave: P[0, n) -> C[6 i], thr_lds = kThrLdsBytes of the wave's LDS.
__device__ __forceinline__ void cov_cloud_segment(const float4* P, int n, const CovGrid& cg, int lane,
                                                  unsigned char* thr_lds, double* C) {
    float4* tile = reinterpret_cast<float4*>(thr_lds);  // the global path's tile, or the cloud's points (LDS path)
    float* lpts = reinterpret_cast<float*>(thr_lds);
    unsigned short* map = reinterpret_cast<unsigned short*>(thr_lds + kThrPtsBytes);
    unsigned short* list = map + kThrMap;
    int kx0 = 0, ky0 = 0, wx = 0, wy = 0;
    const bool thr = cov_thr_map(P, n, cg, lane, map, kx0, ky0, wx, wy);
    bool in_lds = thr && n <= kThrLdsPts;
    if (in_lds) {
        for (int j = lane; j < n; j += kCovLanes) {
            const float4 p = P[j];
            lpts[3 * j] = p.x;
            lpts[3 * j + 1] = p.y;
            lpts[3 * j + 2] = p.z;
        }
        wave_lds_sync();
    }
    for (int i0 = 0; i0 < n; i0 += kCovLanes) {
        if (in_lds) {
            if (cov_knn_round_thr<true>(P, lpts, n, i0, lane, cg, map, kx0, ky0, wx, wy, list, tile, C)) continue;
            wave_lds_sync();  // the brute force's tile overwrites the points: every lane is done with them
            in_lds = false;   // the later rounds read the cloud from global memory
        } else if (thr && cov_knn_round_thr<false>(P, lpts, n, i0, lane, cg, map, kx0, ky0, wx, wy, list, tile, C)) {
            continue;
        }
        cov_knn_round<10, true>(P, n, 10, i0, lane, tile, C);
    }
}

__global__ void __launch_bounds__(kCovLanes) __attribute__((amdgpu_waves_per_eu(PCORE_COV_WAVES_PER_EU)))
covariance_cloud_kernel(const float4* pts, const int32_t* seg_cnt, int seg_stride, CovGrid cg, double* cov_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char thr_lds[];
    const int off = blockIdx.x * seg_stride;
    cov_cloud_segment(pts + off, seg_cnt[blockIdx.x], cg, threadIdx.x, thr_lds, cov_out + (size_t)6 * off);
}

hipError_t launch_covariances_cloud(const float4* pts, const int32_t* seg_cnt, int seg_stride, int num_segs,
                                    float fx, float fy, float cx, float cy, int stride, double* cov_out, hipStream_t s) {
    if (num_segs <= 0) return hipSuccess;
    const CovGrid cg{fx, fy, cx, cy, stride};
    hipLaunchKernelGGL(covariance_cloud_kernel, dim3(num_segs), dim3(kCovLanes), kThrLdsBytes, s, pts, seg_cnt,
                       seg_stride, cg, cov_out);
    return hipGetLastError();
}

// Segments above kGridNNMin points: one thread per point, k-NN by the exact grid shell search
template <int KMAX>
__global__ void __launch_bounds__(kGThreads) covariance_grid_kernel(const float4* pts, int off, int n,
                                                                    const LabelGrid* grid, const int32_t* cell_start,
                                                                    const float4* gpts, int k, double* cov_out) {
    const int i = blockIdx.x * kGThreads + threadIdx.x;
    if (i >= n) return;
    const LabelGrid g = *grid;
    const float4* P = pts + off;
    const float4 xi = P[i];
    float nd[KMAX];
    int nb[KMAX];
#pragma unroll
    for (int q = 0; q < KMAX; q++) { nd[q] = 0.0f; nb[q] = 0; }
    int cnt = 0;
    auto visit = [&](int b, int e) {
        for (int pi = b; pi < e; pi++) {
            const float4 o = gpts[pi];
            knn_insert_lex<KMAX>(nd, nb, cnt, k, sqdist3(xi.x, xi.y, xi.z, o.x, o.y, o.z), __float_as_int(o.w));
        }
    };
    const bool ok = isfinite(xi.x) && isfinite(xi.y) && isfinite(xi.z) &&
                    grid_shells(g, cell_start, xi.x, xi.y, xi.z, shell_budget(n), visit,
                                [&] { return cnt == k ? nd[k - 1] : INFINITY; });
    if (!ok) {
        cnt = 0;
        for (int j = 0; j < n; j++) {
            const float4 xj = P[j];
            knn_insert_lex<KMAX>(nd, nb, cnt, k, sqdist3(xi.x, xi.y, xi.z, xj.x, xj.y, xj.z), j);
        }
    }
    cov_from_list<KMAX>(P, nb, cnt, cov_out + (size_t)6 * (off + i));
}

hipError_t launch_covariances(const float4* pts, const int32_t* seg_off, const int32_t* seg_cnt, int seg_stride,
                              int num_segs, int k, double* cov_out, hipStream_t s, int max_n) {
    if (num_segs <= 0) return hipSuccess;
    if (k <= 0 || k > kMaxK) return hipErrorInvalidValue;
    if (k == 10)
        hipLaunchKernelGGL((covariance_kernel<10, true>), dim3(num_segs), dim3(kCovLanes), 0, s, pts, seg_off, seg_cnt,
                           seg_stride, k, cov_out, max_n);
    else if (k < 10)
        hipLaunchKernelGGL(covariance_kernel<10>, dim3(num_segs), dim3(kCovLanes), 0, s, pts, seg_off, seg_cnt,
                           seg_stride, k, cov_out, max_n);
    else
        hipLaunchKernelGGL(covariance_kernel<kMaxK>, dim3(num_segs), dim3(kCovLanes), 0, s, pts, seg_off, seg_cnt,
                           seg_stride, k, cov_out, max_n);
    return hipGetLastError();
}

hipError_t launch_covariances_grid(const float4* pts, const int32_t* seg_off_host, const int32_t* seg_cnt_host,
                                   int num_segs, int first_grid, const LabelGrid* grids, const int32_t* cell_start,
                                   const float4* grid_pts, int k, double* cov_out, hipStream_t s) {
    if (k <= 0 || k > kMaxK) return hipErrorInvalidValue;
    for (int sg = 0; sg < num_segs; sg++) {
        const int n = seg_cnt_host[sg];
        if (n <= kGridNNMin) continue;
        const dim3 blocks((n + kGThreads - 1) / kGThreads);
        if (k <= 10)
            hipLaunchKernelGGL(covariance_grid_kernel<10>, blocks, dim3(kGThreads), 0, s, pts, seg_off_host[sg], n,
                               grids + first_grid + sg, cell_start, grid_pts, k, cov_out);
        else
            hipLaunchKernelGGL(covariance_grid_kernel<kMaxK>, blocks, dim3(kGThreads), 0, s, pts, seg_off_host[sg], n,
                               grids + first_grid + sg, cell_start, grid_pts, k, cov_out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// GICP
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ void load_cov(const double* cov, int i, double (&c)[6]) {
    const double2* c2 = reinterpret_cast<const double2*>(cov + (size_t)6 * i);
    const double2 a = c2[0], b = c2[1], d = c2[2];
    c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y; c[4] = d.x; c[5] = d.y;
}

// the pose's state in double: rotation and translation of the GICP transform (source -> target, metres)
struct Xform {
    double R[3][3];
    double t[3];
};

__device__ __forceinline__ void xform_identity(Xform& x) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) x.R[r][c] = r == c ? 1.0 : 0.0;
        x.t[r] = 0.0;
    }
}

// The first kLdsRounds rounds of source points' inputs to the trials' errors, kept in the wave's LDS (SoA,
// conflict-free): M as three double2 per point, the source point and the correspondence's target (w = 1 when the
// point has one).  Later rounds go through the per-pose scratch slots in HBM / L2.  5 KB per round and wave: two
// rounds cover C3's clouds (111 source points on average), so their trials read no HBM scratch; 10.4 KB per wave at
// 12 waves per CU is 125 KB of the CU's 160 KB.
#ifndef PCORE_GICP_LDS_ROUNDS
#define PCORE_GICP_LDS_ROUNDS 2
#endif
constexpr int kLdsPts = 64 * PCORE_GICP_LDS_ROUNDS;
// the first rounds' source points in LDS as three floats (12 B: the cycle exit's 32-slot ring fits the wave's LDS
// in the same 1,280-byte granules)
struct Pt3 {
    float x, y, z;
};

struct Round0 {
    double2 (*m)[kLdsPts];
    Pt3* s;
    float4* t;
};

// Linearisation of one round of 64 source points (point i on lane i % 64; j: its correspondence, found by the caller,
// or -1), fast_gicp linearize: for points with a correspondence the shared contribution into acc, and M to the wave's
// LDS (r0) or the iteration's scratch (mah[6 i ..]) for the trials' errors.
__device__ __forceinline__ void linearize_round(const Xform& x, const float4* src, const double* scov,
                                                const float4* tgt, const double* tcov, int ns, int i, int j,
                                                double* mah, const Round0& r0,
                                                double (&acc)[gicpm::kTerms] GPROF_PARAM) {
    GPROF_T(t_s0);
    const bool act = i < ns;
    const float4 sp = act ? src[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    GPROF_TD(t_s1, j);
    GPROF_ADD(0, t_s0, t_s1);  // the search is the caller's: its wait for j, if any, counts as search
    const bool first = i < kLdsPts;  // a point of the rounds kept in LDS
    if (first && !(act && j >= 0)) r0.t[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (act && j >= 0) {
        double q[3];
        gicpm::transform_point(x.R, x.t, (double)sp.x, (double)sp.y, (double)sp.z, q);
        double cs[6], ct[6], M6[6];
        load_cov(scov, i, cs);
        load_cov(tcov, j, ct);
        const float4 tj = tgt[j];
        const double t3[3] = {(double)tj.x, (double)tj.y, (double)tj.z};
        gicpm::contrib(x.R, q, cs, t3, ct, acc, M6);
        if (first) {
            r0.m[0][i] = make_double2(M6[0], M6[1]);
            r0.m[1][i] = make_double2(M6[2], M6[3]);
            r0.m[2][i] = make_double2(M6[4], M6[5]);
            r0.s[i] = Pt3{sp.x, sp.y, sp.z};
            r0.t[i] = make_float4(tj.x, tj.y, tj.z, 1.0f);
        } else {
            double2* m2 = reinterpret_cast<double2*>(mah + (size_t)6 * i);
            m2[0] = make_double2(M6[0], M6[1]);
            m2[1] = make_double2(M6[2], M6[3]);
            m2[2] = make_double2(M6[4], M6[5]);
        }
    }
    GPROF_TD(t_s2, acc[gicpm::kErr]);
    GPROF_ADD(1, t_s1, t_s2);
}

// One Levenberg-Marquardt iteration of one wave (LsqRegistration::step_lm) on the reduced system `sys` (28 sums in
// LDS: upper H, b, the error y0 at x): up to kLmMaxTrials solves of (H + lambda I) d = -b, each scored by the error
// at delta * x with the iteration's correspondences and M (point i on lane i % 64, summed by the shuffle-down tree).
// Every lane runs the same uniform arithmetic; the scalars that steer it are moved to SGPRs.
__device__ __forceinline__ int lm_iteration(const double* sys, Xform& x, double& lambda, const float4* src,
                                            const int32_t* corr, const double* mah, const float4* tgt, int ns, int lane,
                                            const Round0& r0, const lds_cvd* se3c, double rot_eps,
                                            double trans_eps, bool& inert GPROF_PARAM) {
    const double y0 = uniform_d(sys[gicpm::kErr]);
    if (lambda < 0.0) lambda = uniform_d(gicpm::lm_init_lambda(sys));
    inert = false;
    double nu = 2.0;
    for (int trial = 0; trial < gicpm::kLmMaxTrials; trial++) {
        GPROF_T(p0);
        double d[6];
        gicpm::lm_solve_schur(sys, lambda, d);
#pragma unroll
        for (int a = 0; a < 6; a++) d[a] = uniform_d(d[a]);
        GPROF_TD(p1, d[5]);
        GPROF_ADD(4, p0, p1);
        if (!gicpm::all_finite6(d)) return gicpm::kLmFailed;  // guard: a non-finite system
        double Rd[3][3], td[3];
        gicpm::se3_exp(d, Rd, td, se3c + opaque_zero());
        Xform xi;
        gicpm::compose(Rd, td, x.R, x.t, xi.R, xi.t);
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) xi.R[r][c] = uniform_d(xi.R[r][c]);
            xi.t[r] = uniform_d(xi.t[r]);
        }
        GPROF_TD(p2, xi.t[2]);
        GPROF_ADD(5, p1, p2);
        // the error at x_i (FastGICP::compute_error: this iteration's correspondences and Mahalanobis matrices)
        auto err_add = [&](const auto& sp, const float4& tj, const double (&M6)[6], double y) {
            double q[3];
            gicpm::transform_point(xi.R, xi.t, (double)sp.x, (double)sp.y, (double)sp.z, q);
            const double e[3] = {(double)tj.x - q[0], (double)tj.y - q[1], (double)tj.z - q[2]};
            return gicpm::mahal_err_add(M6, e, y);
        };
        double ea = 0.0;
        // the first rounds from the wave's LDS copy (written by the linearisation; a round past ns is not read), the
        // later rounds from the scratch slots
#pragma unroll
        for (int i0 = 0; i0 < kLdsPts; i0 += 64) {
            if (i0 > 0 && i0 >= ns) break;
            const int i = i0 + lane;
            const float4 t0 = r0.t[i];
            if (t0.w != 0.0f) {
                const double2 a = r0.m[0][i], b = r0.m[1][i], c = r0.m[2][i];
                const double M6[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
                ea = err_add(r0.s[i], t0, M6, ea);
            }
        }
        for (int i0 = kLdsPts; i0 < ns; i0 += 64) {
            const int i = i0 + lane + opaque_zero();  // per-lane addresses formed here (hoisted, they were spilled)
            const int j = i < ns ? corr[i] : -1;
            if (j >= 0) {
                const double2* m2 = reinterpret_cast<const double2*>(mah + (size_t)6 * i);
                const double2 a = m2[0], b = m2[1], c = m2[2];
                const double M6[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
                ea = err_add(src[i], tgt[j], M6, ea);
            }
        }
        const double yi = uniform_d(wave_sum_lane0(ea));  // lane 0: the tree's sum
        GPROF_TD(p3, yi);
        GPROF_ADD(6, p2, p3);
        const double rho = uniform_d(gicpm::lm_rho(sys, lambda, d, y0, yi));
        GPROF_TD(p4, rho);
        GPROF_ADD(7, p3, p4);
        if (rho < 0.0) {
            if (gicpm::is_converged(Rd, td, rot_eps, trans_eps)) return gicpm::kLmConverged;
            lambda = nu * lambda;
            nu = 2.0 * nu;
            continue;
        }
        x = xi;
        // the cycle exit's condition: accepted at the first trial, lambda not growing and inert on this system
        inert = trial == 0 && rho >= 0.5 && gicpm::lm_lambda_inert(sys, lambda);
        lambda = uniform_d(gicpm::lm_accept_lambda(lambda, rho));
        return gicpm::is_converged(Rd, td, rot_eps, trans_eps) ? gicpm::kLmConverged : gicpm::kLmAccepted;
    }
    return gicpm::kLmFailed;  // LsqRegistration: "lm not converged"
}

// concatenate_transforms (renderer.cu:1412-1429): float(T) * to_eigen(pose, 100), init_from_eigen(., 100)
__device__ __forceinline__ void write_pose(const GicpArgs& g, int gp, const Xform& x, int iters) {
    const float* pin = g.poses_in + (size_t)16 * gp;
    float A[4][4], Tf[4][4];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            A[r][c] = r < 3 ? pin[4 * r + c] / 100.0f : pin[4 * r + c];
            Tf[r][c] = r < 3 ? (float)(c < 3 ? x.R[r][c] : x.t[r]) : (c == 3 ? 1.0f : 0.0f);
        }
    float* pout = g.poses_out + (size_t)16 * gp;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const float p = Tf[r][0] * A[0][c] + Tf[r][1] * A[1][c] + Tf[r][2] * A[2][c] + Tf[r][3] * A[3][c];
            pout[4 * r + c] = r < 3 ? (float)((double)p * 100) : p;
        }
    if (g.iters_out) g.iters_out[gp] = iters;
}

// the launch's iteration counters (GicpArgs::iter_stats): no-return atomics, one lane per pose
__device__ __forceinline__ void count_iterations(const GicpArgs& g, int reported, int run, bool exited) {
    if (!g.iter_stats) return;
    __hip_atomic_fetch_add(g.iter_stats + 0, (unsigned long long)reported, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(g.iter_stats + 1, (unsigned long long)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (exited) __hip_atomic_fetch_add(g.iter_stats + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A pose's end, by one lane: the refined pose with the iterations it reports, the launch's counters and the timeline
// stamp.  iters_run: the iterations executed when a cycle exit stopped the pose (which then reports max_iter), else 0.
__device__ __forceinline__ void finish_pose(const GicpArgs& g, int gp, const Xform& x, int iters,
                                            int iters_run GTL_PARAM(tl_p0)) {
    const int run = iters_run ? iters_run : iters;
    write_pose(g, gp, x, iters);
    count_iterations(g, iters, run, iters_run != 0);
    GTL_POSE(gp, tl_p0, run);
}

// The next pose of the launch's queue (chunk-local; num_poses or more: the queue is empty), by one lane: the queue is
// ordered longest first where the host sorted it (launch_gicp_order).
__device__ __forceinline__ int pop_pose(const GicpArgs& g, int num_poses) {
    const int q = atomicAdd(g.work_counter, 1);
    return (g.pose_order && q < num_poses) ? g.pose_order[q] : q;
}

// the pose a GICP workgroup works on next and its target segment
struct GicpPose {
    int gp, ns, nt, seg;
    const float4* src;
    const double* scov;
    const double* tcov;
    const float4* tgt;
    const float* tquads;
    int32_t* corr;
    double* mah;
    bool use_grid;
};

__device__ __forceinline__ GicpPose gicp_pose(const GicpArgs& g, int pose) {
    GicpPose p;
    p.gp = g.pose_base + pose;
    p.ns = g.src_count[pose];
    p.src = g.src + (size_t)pose * g.src_cap;
    p.scov = g.src_cov + (size_t)6 * pose * g.src_cap;
    p.corr = g.corr + (size_t)pose * g.src_cap;
    p.mah = g.mahal + (size_t)6 * pose * g.src_cap;
    int seg = g.whole_seg;
    if (g.pose_label) {
        const int pl = g.pose_label[p.gp];
        seg = (pl >= 0 && pl < g.num_segs) ? pl : -1;
    }
    seg = __builtin_amdgcn_readfirstlane(seg);
    p.seg = seg;
    const int lo = seg >= 0 ? g.seg_lo[seg] : 0;
    p.nt = seg >= 0 ? g.seg_hi[seg] - lo : 0;
    p.tcov = g.tgt_cov + (size_t)6 * lo;
    p.tgt = g.tgt + lo;
    p.tquads = g.tgt_quads + (seg >= 0 ? (size_t)16 * g.seg_qoff[seg] : 0);
    p.use_grid = seg >= 0 && segment_uses_grid(p.nt, g.grids != nullptr);  // exact grid shell search
    return p;
}

constexpr int kCycleExited = 3;  // coop_pose's flag: wave 0's cycle exit stopped the pose (LmStatus + 1)

// One pose by the NW waves of a workgroup (gicp_wide_kernel's poses): every wave searches
// the iteration's correspondences of rounds r = wave (mod NW) into `corr`, then wave 0 adds the contributions and runs
// the LM iteration exactly as the one-wave path does -- point i on lane i % 64, in point order -- so the refined pose
// is bit-identical; x and the iteration's outcome reach the other waves through LDS (sX, sFlag).  `r0`, `sRed`, `ring`:
// wave 0's LDS.  Every thread of the workgroup calls this; thread 0 writes the pose.
template <int NW>
__device__ __forceinline__ void coop_pose(const GicpArgs& g, const GicpPose& P, int wave, int lane, int32_t* corr,
                                          double* sRed, const Round0& r0, const lds_cvd* se3c, unsigned* ring,
                                          double* sX, int* sFlag GPROF_PARAM) {
    constexpr int NT = 64 * NW;
    const int tid = wave * 64 + lane;
    GTL_NOW(tl_p0);
    LabelGrid G{};
    if (P.use_grid) G = g.grids[P.seg];
    Xform x;
    xform_identity(x);
    double lambda = -1.0;  // wave 0's
    int iters = 0, iters_run = 0;
    CycleExit cyc;  // wave 0's
    cyc.ring = ring;
    if (wave == 0) cyc.start(lane);
    const bool run = P.ns > 0 && P.nt > 0;
    for (int it = 0; run && it < g.max_iter; it++) {
        iters++;
        float Rf[3][3], tf[3];
        xform_float(x.R, x.t, Rf, tf);
        GPROF_T(t_w0);
        // correspondences, all waves
        for (int i0 = wave * 64; i0 < P.ns; i0 += NT) {
            const int i = i0 + lane;
            const bool act = i < P.ns;
            const float4 sp = act ? P.src[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float qf[3];
            gicpm::query_f(Rf, tf, sp.x, sp.y, sp.z, qf);
            int j = -1;
            float best = INFINITY;
            if (P.use_grid) {
                if (act) grid_nn(G, g.cell_start, g.grid_pts, P.tgt, P.nt, qf[0], qf[1], qf[2], best, j);
            } else {
                scan_quads(P.tquads, P.nt, qf[0], qf[1], qf[2], best, j);
            }
            if (act) corr[i] = j;
        }
        __syncthreads();
        GPROF_TD(t_w1, Rf[0][0]);
        GPROF_ADD(0, t_w0, t_w1);
        if (wave == 0) {
            double acc[gicpm::kTerms];
#pragma unroll
            for (int v = 0; v < gicpm::kTerms; v++) acc[v] = 0.0;
            for (int i0 = 0; i0 < P.ns; i0 += 64) {
                const int i = i0 + lane;
                linearize_round(x, P.src, P.scov, P.tgt, P.tcov, P.ns, i, i < P.ns ? corr[i] : -1, P.mah, r0,
                                acc GPROF_ARG);
            }
            GPROF_TD(t_w2, acc[0]);
            const double* sys = wave_tree_sums(acc, sRed, lane);
            GPROF_TD(t_w3, sys[0]);
            bool inert;
            int st = lm_iteration(sys, x, lambda, P.src, corr, P.mah, P.tgt, P.ns, lane, r0, se3c, g.rot_eps,
                                  g.trans_eps, inert GPROF_ARG);
            GPROF_TD(t_w4, st);
            GPROF_ADD(2, t_w2, t_w3);  // [1]: linearize_round's own marks
            GPROF_ADD(3, t_w3, t_w4);
            if (st == gicpm::kLmAccepted && g.cycle_window > 0 && iters < g.max_iter) {
                const int s2 = cyc.step(x.R, x.t, iters, g.max_iter, g.cycle_window, inert, lane);
                if (s2 >= 0) {
                    cyc.member(s2, x.R, x.t);
                    st = kCycleExited;
                }
            }
            if (lane == 0) {
                *sFlag = st;
#pragma unroll
                for (int r = 0; r < 3; r++) {
#pragma unroll
                    for (int c = 0; c < 3; c++) sX[3 * r + c] = x.R[r][c];
                    sX[9 + r] = x.t[r];
                }
            }
        }
        __syncthreads();
        const int flag = __builtin_amdgcn_readfirstlane(*sFlag);
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) x.R[r][c] = uniform_d(sX[3 * r + c]);
            x.t[r] = uniform_d(sX[9 + r]);
        }
        if (flag == kCycleExited) {
            iters_run = iters;
            iters = g.max_iter;
        }
        if (flag != gicpm::kLmAccepted) break;
    }
    __syncthreads();
    if (tid == 0) finish_pose(g, P.gp, x, iters, iters_run GTL_ARG(tl_p0));
}

// One wave per pose; persistent waves pull poses from a counter.  Each iteration linearises in rounds of 64
// source points (point i -> lane i % 64, contributions added in point order), reduces the 28 terms by the
// shuffle-down tree in registers and runs the LM iteration on the wave.  The per-pose iteration chain is
// latency-bound, so the slowest pose sets a chunk's tail (the queue is ordered longest first).
#ifndef PCORE_GICP_WAVES_PER_EU
#define PCORE_GICP_WAVES_PER_EU 3
#endif

// GRID: the kernel holds the exact grid search of large segments (> kGridNNMin targets).  launch_gicp picks the
// instance without it when no segment of the observation is that large (every C2-C5 label): the search's registers
// then weigh on no pose (gicp_kernel 12.1 -> 11.9 ms per C3 call).
template <bool GRID>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PCORE_GICP_WAVES_PER_EU)))
gicp_kernel(GicpArgs g, int num_poses) {
    __shared__ double sRed[gicpm::kTerms];
    __shared__ double2 sM0[3][kLdsPts];
    __shared__ Pt3 sS0[kLdsPts];
    __shared__ float4 sT0[kLdsPts];
    __shared__ int sPose;
    __shared__ double sSe3[4 * gicpm::kSe3Terms];  // se3_exp's series coefficients, read at their use
    __shared__ unsigned sHist[3 * 64];              // the correspondence history's float transforms (below)
    __shared__ unsigned sCyc[kCycleRingWords];      // the cycle exit's last 32 float transforms (CycleExit)
    const int lane = threadIdx.x;
    const Round0 r0{sM0, sS0, sT0};
    if (threadIdx.x < 4 * gicpm::kSe3Terms) sSe3[threadIdx.x] = gicpm::kSe3Coef[threadIdx.x];
    GPROF_DECL;
    GTL_NOW(tl_w0);
    for (;;) {
        wave_lds_sync();  // the previous pose's reads of sPose are done
        if (lane == 0) sPose = pop_pose(g, num_poses);
        wave_lds_sync();
        const int pose = __builtin_amdgcn_readfirstlane(sPose);  // chunk-local, uniform
        if (pose >= num_poses) break;
        const GicpPose P = gicp_pose(g, pose);
        if (!GRID && P.use_grid && lane == 0 && g.iter_stats)  // the host picked the instance without the search
            __hip_atomic_fetch_add(g.iter_stats + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        GTL_NOW(tl_p0);
        GPROF_POSE_BEGIN;
        Xform x;
        xform_identity(x);
        double lambda = -1.0;
        int iters = 0, iters_run = 0, exit_slot = -1;
        CycleExit cyc;
        cyc.ring = sCyc;
        cyc.start(lane);
        // correspondence history: sHist[64 v + l] holds component 3 (l & 3) + v (v = 0, 1, 2) of set l >> 2's float
        // transform (R rows 0..2, then t); `kept` has bit 4e set for every filled set e (the words of unfilled sets
        // are never compared).  In LDS rather than in three VGPRs per lane: the kernel is at its register budget,
        // and a history word held in a VGPR was spilled to scratch and reloaded behind a vmcnt(0) every iteration.
        const bool hist = g.corr_hist != nullptr && P.ns <= g.corr_hist_cap;
        int32_t* const hbase = hist ? g.corr_hist + (size_t)pose * kCorrHist * g.corr_hist_cap : nullptr;
        unsigned long long kept = 0ull;
        int ring = 0;
        const int sub = lane & 3;
        if (P.ns > 0 && P.nt > 0) {
            for (int it = 0; it < g.max_iter; it++) {
                iters++;
                float Rf[3][3], tf[3];
                xform_float(x.R, x.t, Rf, tf);
                int32_t* cset = P.corr;
                bool reuse = false;
                if (hist) {
                    unsigned b0, b1, b2;
                    xf_lane_words(Rf, tf, sub, b0, b1, b2);
                    // bitwise equality (-0 != +0, NaN == NaN): the float queries, and so the correspondences, are
                    // functions of these bits
                    const unsigned hv0 = sHist[lane], hv1 = sHist[64 + lane], hv2 = sHist[128 + lane];
                    const unsigned long long eq = __ballot(b0 == hv0 && b1 == hv1 && b2 == hv2);
                    const unsigned long long full = eq & (eq >> 1) & (eq >> 2) & (eq >> 3) & kept;
                    int e;
                    if (full != 0ull) {
                        e = __builtin_ctzll(full) >> 2;
                        reuse = true;
                    } else {
                        e = ring;
                        ring = ring + 1 == kCorrHist ? 0 : ring + 1;
                        kept |= 1ull << (4 * e);
                        if ((lane >> 2) == e) {  // every lane reads back only the words it wrote itself
                            sHist[lane] = b0;
                            sHist[64 + lane] = b1;
                            sHist[128 + lane] = b2;
                        }
                    }
                    cset = hbase + (size_t)__builtin_amdgcn_readfirstlane(e) * g.corr_hist_cap;
                }
                GPROF_COUNT(8, reuse ? 1ull : 0ull);
                double acc[gicpm::kTerms];
#pragma unroll
                for (int v = 0; v < gicpm::kTerms; v++) acc[v] = 0.0;
                // rounds in pairs: both rounds' correspondences first (one pass over the key quads serves both:
                // scan_quads2), then their contributions in point order -- the sums are those of round-by-round
                // linearisation, bit for bit
                for (int i0 = 0; i0 < P.ns; i0 += 128) {
                    const int ia = i0 + lane, ib = ia + 64;
                    const bool two = i0 + 64 < P.ns;  // uniform
                    GPROF_T(t_s0);
                    int ja = -1, jb = -1;
                    if (reuse) {
                        if (ia < P.ns) ja = cset[ia];
                        if (two && ib < P.ns) jb = cset[ib];
                    } else {
                        const float4 sa = ia < P.ns ? P.src[ia] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        const float4 sb = two && ib < P.ns ? P.src[ib] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        float qa[3], qb[3];
                        gicpm::query_f(Rf, tf, sa.x, sa.y, sa.z, qa);
                        gicpm::query_f(Rf, tf, sb.x, sb.y, sb.z, qb);
                        if (GRID && P.use_grid) {  // segments above kGridNNMin (the grid is read here, not per pose)
                            const LabelGrid Gs = g.grids[P.seg];
                            float best;
                            if (ia < P.ns) grid_nn(Gs, g.cell_start, g.grid_pts, P.tgt, P.nt, qa[0], qa[1], qa[2], best, ja);
                            if (two && ib < P.ns)
                                grid_nn(Gs, g.cell_start, g.grid_pts, P.tgt, P.nt, qb[0], qb[1], qb[2], best, jb);
                        } else if (two) {
                            scan_quads2(P.tquads, P.nt, qa[0], qa[1], qa[2], qb[0], qb[1], qb[2], ja, jb);
                        } else {
                            float best = INFINITY;
                            scan_quads(P.tquads, P.nt, qa[0], qa[1], qa[2], best, ja);
                        }
                        if (ia < P.ns) cset[ia] = ja;
                        if (two && ib < P.ns) cset[ib] = jb;
                    }
                    GPROF_TD(t_s1, ja + jb);
                    GPROF_ADD(0, t_s0, t_s1);
                    linearize_round(x, P.src, P.scov, P.tgt, P.tcov, P.ns, ia, ia < P.ns ? ja : -1, P.mah, r0,
                                    acc GPROF_ARG);
                    if (two)
                        linearize_round(x, P.src, P.scov, P.tgt, P.tcov, P.ns, ib, ib < P.ns ? jb : -1, P.mah, r0,
                                        acc GPROF_ARG);
                }
                GPROF_T(t_b);
                const double* sys = wave_tree_sums(acc, sRed, lane);
                GPROF_TD(t_c, sys[0]);
                bool inert;
                const int st = lm_iteration(sys, x, lambda, P.src, cset, P.mah, P.tgt, P.ns, lane, r0, (const lds_cvd*)sSe3,
                                            g.rot_eps, g.trans_eps, inert GPROF_ARG);
                GPROF_TD(t_d, st);
                GPROF_ADD(2, t_b, t_c);
                GPROF_ADD(3, t_c, t_d);
                if (st != gicpm::kLmAccepted) break;
                if (g.cycle_window > 0 && iters < g.max_iter) {
                    exit_slot = cyc.step(x.R, x.t, iters, g.max_iter, g.cycle_window, inert, lane);
                    if (exit_slot >= 0) {
                        iters_run = iters;
                        iters = g.max_iter;
                        break;
                    }
                }
            }
        }
        if (exit_slot >= 0) cyc.member(exit_slot, x.R, x.t);
        GPROF_POSE_END(P.ns, iters_run ? iters_run : iters);
        if (lane == 0) finish_pose(g, P.gp, x, iters, iters_run GTL_ARG(tl_p0));
    }
    GPROF_FLUSH;
    GTL_WAVE(tl_w0);
}

// Small batches (C1: 128 poses fill 128 of 1024 SIMDs) with large target segments: WPP waves per pose.
// All waves search the correspondences of the iteration's source points (round r -> wave r % WPP), the
// indices go to LDS, and wave 0 then adds the contributions and runs the LM iteration exactly as gicp_kernel
// does -- point i on lane i % 64, in point order -- so the refined poses are bit-identical; only the
// nearest-target searches, the expensive part against a whole-scene target, run in parallel.
template <int WPP>
__global__ void __launch_bounds__(64 * WPP) gicp_wide_kernel(GicpArgs g, int num_poses) {
    extern __shared__ __attribute__((aligned(16))) int32_t jbuf[];  // src_cap correspondences
    __shared__ double sRed[gicpm::kTerms];
    __shared__ double2 sM0[3][kLdsPts];
    __shared__ Pt3 sS0[kLdsPts];
    __shared__ float4 sT0[kLdsPts];
    __shared__ double sX[12];
    __shared__ int sPose, sFlag;
    __shared__ double sSe3[4 * gicpm::kSe3Terms];
    __shared__ unsigned sCyc[kCycleRingWords];  // wave 0's cycle exit ring
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const Round0 r0{sM0, sS0, sT0};  // wave 0's
    if (tid < 4 * gicpm::kSe3Terms) sSe3[tid] = gicpm::kSe3Coef[tid];
    GPROF_DECL;  // wave 0's phases: [0] the searches of all waves (to the barrier), [1] contributions, [2] tree, [3] LM
    for (;;) {
        __syncthreads();
        if (tid == 0) sPose = pop_pose(g, num_poses);
        __syncthreads();
        const int pose = __builtin_amdgcn_readfirstlane(sPose);
        if (pose >= num_poses) break;
        coop_pose<WPP>(g, gicp_pose(g, pose), wave, lane, jbuf, sRed, r0, (const lds_cvd*)sSe3, sCyc, sX,
                       &sFlag GPROF_ARG);
    }
    if (wave == 0) GPROF_FLUSH;
}

constexpr int kGicpWideWpp = 8;
constexpr size_t kGicpWideMaxLds = 96 * 1024;  // correspondence buffer: src_cap <= 24576

// Test hook of the kernels' damped solve (gicpm::lm_solve_schur): one wave per 28-term system.
__global__ void __launch_bounds__(64) lm_solve_test_kernel(const double* sys, const double* lambda, double* out, int n) {
    const int i = blockIdx.x;
    if (i >= n) return;
    double d[6];
    gicpm::lm_solve_schur(sys + (size_t)gicpm::kTerms * i, lambda[i], d);
    if (threadIdx.x == 0)
        for (int a = 0; a < 6; a++) out[(size_t)6 * i + a] = d[a];
}

hipError_t launch_lm_solve_test(const double* sys, const double* lambda, double* out, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lm_solve_test_kernel, dim3(n), dim3(64), 0, s, sys, lambda, out, n);
    return hipGetLastError();
}

// predicted cost of one GICP iteration of a pose: source points x targets of its segment (the scan)
__global__ void gicp_cost_key_kernel(GicpArgs g, int n, uint32_t* keys, int32_t* idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int seg = g.whole_seg;
    if (g.pose_label) {
        const int pl = g.pose_label[g.pose_base + i];
        seg = (pl >= 0 && pl < g.num_segs) ? pl : -1;
    }
    const unsigned long long nt = seg >= 0 ? (unsigned long long)(g.seg_hi[seg] - g.seg_lo[seg]) : 0ull;
    const unsigned long long c = (unsigned long long)max(g.src_count[i], 0) * nt;
    keys[i] = (uint32_t)min(c >> 4, 0xffffffffull);
    idx[i] = i;
}

size_t gicp_order_temp_bytes(int n) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                       (const int32_t*)nullptr, (int32_t*)nullptr, n);
    return bytes;
}

hipError_t launch_gicp_order(const GicpArgs& g, int n, uint32_t* keys_in, uint32_t* keys_out, int32_t* idx_in,
                             int32_t* order_out, void* temp, size_t temp_bytes, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gicp_cost_key_kernel, dim3((n + 255) / 256), dim3(256), 0, s, g, n, keys_in, idx_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairsDescending(temp, temp_bytes, keys_in, keys_out, idx_in, order_out, n, 0,
                                                        32, s);
}

hipError_t gicp_occupancy_per_cu(int* per_cu) {
    *per_cu = 0;
    int other = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, gicp_kernel<true>, 64, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&other, gicp_kernel<false>, 64, 0);
    if (e == hipSuccess) *per_cu = std::min(*per_cu, other);
    return e;
}

hipError_t launch_gicp(const GicpArgs& g, int num_poses, const DeviceInfo& d, hipStream_t s, bool grid) {
    if (num_poses <= 0) return hipSuccess;
    const int resident_wgs = std::max(1, d.gicp_resident_wgs), num_cus = std::max(1, d.num_cus);
    hipError_t e = hipMemsetAsync(g.work_counter, 0, sizeof(int32_t), s);  // the pose queue's counter
    if (e != hipSuccess) return e;
    // a batch too small to give every SIMD a pose: spread each pose's searches over kGicpWideWpp waves
    const size_t wide_lds = (size_t)g.src_cap * sizeof(int32_t);
    bool wide = num_poses <= num_cus * 2 && wide_lds <= kGicpWideMaxLds;
    if (const char* e = getenv("PCORE_GICP_KERNEL")) {  // tests pin either kernel (same results)
        if (e[0] == 'n') wide = false;
        else if (e[0] == 'w' && wide_lds <= kGicpWideMaxLds) wide = true;
    }
    if (wide) {
        const int wgs = std::min(num_poses, num_cus * 2);
        hipLaunchKernelGGL(gicp_wide_kernel<kGicpWideWpp>, dim3(wgs), dim3(64 * kGicpWideWpp), wide_lds, s, g,
                           num_poses);
        return hipGetLastError();
    }
    const dim3 wgs(std::min(resident_wgs, num_poses)), block(64);
    if (grid)
        hipLaunchKernelGGL(gicp_kernel<true>, wgs, block, 0, s, g, num_poses);
    else
        hipLaunchKernelGGL(gicp_kernel<false>, wgs, block, 0, s, g, num_poses);
    return hipGetLastError();
}

}  // namespace pcore
