// pcore_p2p_math.h -- the arithmetic of the point-to-plane projective ICP spec ("Point-to-plane
// ICP spec"): the reference's ICP_Point2Plane loop (cuda_icp/icp.cu:157-218, icp.cpp:116-179) against a
// Scene_projective (depth_scene.h), as oracle/ref_cpu_path.cpp restates it, operation for operation.  One set of
// functions for the HIP kernels (pcore_p2p.hip) and any host-side caller; the numpy restatement the tests hold them to
// (tests/p2p_reference.py) is written independently of this header.  Float arithmetic on float inputs, the 6 x 6 solve
// and the Euler angles in double, one operation per expression node, compiled with -ffp-contract=off.
//
// Per iteration, over the pose's points s (moved in place by every increment):
//   project      v = ((s.x / s.z) * fx + cx) - 0 + 0.5 (and y); rejected when NaN or |v| >= 2^31, else      pixel()
//                truncated toward zero; then 0 <= x < W, 0 <= y < H
//   query        the scene point d and normal n of that pixel; rejected when d.z <= 0 or |s.z - d.z| > max   accept()
//   row          29 floats: the upper triangle of A A^T (21), A b (6), b b, 1 with                           row()
//                A = (n.z s.y - n.y s.z, n.x s.z - n.z s.x, n.y s.x - n.x s.y, n), b = (d - s) . n
//   sums         lane l adds the rows of points l, l + 64, ... in that order; xor butterfly 32 .. 1          (kernel)
//   exits        count == 0; iter == max_iter; |d fitness| < rel_fitness and |d rmse| < rel_rmse             (kernel)
//   solve        Eigen's LDLT with diagonal pivoting, in double                                              ldlt_solve6()
//   increment    R = Rz Ry Rx as the quaternion product, with pcore::dmath's sin / cos, to float             vec6_to_mat4()
//   apply        s <- E s, each row left to right; T <- E T, each dot from index 3 down to 0                 apply(), mat4_mul()
#pragma once

#include "pcore_dmath.h"

#ifdef __HIPCC__
#define PCORE_P2P __host__ __device__ __forceinline__
#else
#include <math.h>
#define PCORE_P2P inline
#endif

namespace pcore {
namespace p2p {

constexpr int kRow = 29;  // 21 + 6 + 1 + 1
constexpr int kLinemodRadius = 5, kLinemodMaxDepth = 2000, kLinemodMaxDiff = 50;  // get_normal (common.cpp:17-107)

struct Sums {
    float v[kRow];
};

struct Mat4 {
    float m[4][4];
};

PCORE_P2P Mat4 identity() {
    Mat4 r;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) r.m[i][j] = i == j ? 1.0f : 0.0f;
    return r;
}

// pcd2dep + the reference's int(float): false where the host conversion gives INT_MIN (NaN, |v| >= 2^31), which the
// range test rejects
PCORE_P2P bool pixel(float num, float z, float f, float c, int& out) {
    const float v = ((num / z) * f + c) - 0.0f + 0.5f;
    out = 0;
    if (!(v == v) || !(__builtin_fabsf(v) < 2147483648.0f)) return false;
    out = (int)v;
    return true;
}

// Scene_projective::query's tests on the gathered scene point's z
PCORE_P2P bool accept(float sz, float dz_scene, float max_dist_diff) {
    const float dz = sz - dz_scene;
    const float adz = (dz > 0) ? dz : -dz;
    return !(dz_scene <= 0 || adz > max_dist_diff);
}

// The nearest-neighbour scene's query ("Nearest-neighbour scene"; the reference's Scene_nn,
// pcd_scene.h:48-137, with the kd-tree replaced by an exact search over a pixel window).  Among the pixels (c, q) of
// the image with |c - x| <= window and |q - y| <= window around the query's own pixel (x, y) whose scene point P has
// P.z > 0, the one with the smallest d2 = (dx dx + dy dy) + dz dz wins, the lowest index q W + c on equal d2; it is
// accepted iff d2 < max_dist_diff^2.
constexpr int kNnMaxWindow = 128;
constexpr int kNnBatch = 8;  // candidates loaded ahead of the comparisons, per row

// One axis of the rectangle that holds every pixel whose scene point can lie within rho of the query: the scene is
// dep2pcd of a depth image in centimetres, P.x = fl(fl((c - cx) / fx) P.z) with P.z >= 0.01, so c - cx is P.x / P.z fx
// to within 2^-21 of its size (0.008 pixel at the largest image) for P.x in [s - rho, s + rho] and P.z in [z_lo, z_hi];
// x / z takes its extremes at the corners.  The range [lo, hi] (the window clipped to the image) shrinks to the
// corners' pixels widened by one; a corner that is not a number leaves its side of the window as it is.
PCORE_P2P void nn_axis_bound(float s, float rho, float z_lo, float z_hi, float f, float c, int& lo, int& hi) {
    const float a = s - rho, b = s + rho;
    const float v0 = (a / z_lo) * f + c, v1 = (a / z_hi) * f + c, v2 = (b / z_lo) * f + c, v3 = (b / z_hi) * f + c;
    const float m01 = v0 < v1 ? v0 : v1, m23 = v2 < v3 ? v2 : v3, M01 = v0 > v1 ? v0 : v1, M23 = v2 > v3 ? v2 : v3;
    const bool num = v0 == v0 && v1 == v1 && v2 == v2 && v3 == v3;
    const float vmin = (m01 < m23 ? m01 : m23) - 2.0f;  // floor + 1 pixel: v - 2 < floor(v) - 1
    const float vmax = (M01 > M23 ? M01 : M23) + 2.0f;
    if (!num) return;
    // |lo|, |hi| <= 16384 + 128: exact as floats, and the conversions below are of values between them
    if (vmin > (float)hi) {
        lo = hi + 1;
        return;
    }
    if (vmax < (float)lo) {
        hi = lo - 1;
        return;
    }
    if (vmin > (float)lo) lo = (int)vmin;  // vmin > lo >= 0: truncation is floor
    if (vmax < (float)hi) hi = (int)vmax + 1;
    if (hi < lo) hi = lo - 1;
}

// The winner's pixel index and d2 (found == false: no candidate).  Pcd4 has float members x, y, z.  Every load is at
// a pixel of the image, whatever s holds; the two loops run over at most (2 window + 1)^2 pixels.
template <class Pcd4>
PCORE_P2P bool nn_query(const Pcd4* pcd, int W, int H, float fx, float fy, float cx, float cy, int window, float r,
                        float sx, float sy, float sz, size_t& best_idx, float& best_d2) {
    best_idx = 0;
    best_d2 = 0.0f;
    int x, y;
    const bool okx = pixel(sx, sz, fx, cx, x);
    const bool oky = pixel(sy, sz, fy, cy, y);
    if (!(okx && oky && sz > 0)) return false;
    // the window clipped to the image, without forming x +- window where it could overflow
    if (x < -window || x > W - 1 + window || y < -window || y > H - 1 + window) return false;
    int c0 = x - window < 0 ? 0 : x - window, c1 = x + window > W - 1 ? W - 1 : x + window;
    int q0 = y - window < 0 ? 0 : y - window, q1 = y + window > H - 1 ? H - 1 : y + window;
    // nothing at or beyond r is accepted (d2 < r r needs |dx|, |dy|, |dz| < r (1 + 2^-22)), so only the pixels that
    // can hold a point within rho = r (1 + 2^-13) need a look; where none of them has a point, no winner is reported,
    // and the winner of the whole window would have been refused
    const float rho = r * 1.0001220703125f;
    const float zl = sz - rho, z_lo = zl > 0.0099f ? zl : 0.0099f, z_hi = sz + rho;
    nn_axis_bound(sx, rho, z_lo, z_hi, fx, cx, c0, c1);
    nn_axis_bound(sy, rho, z_lo, z_hi, fy, cy, q0, q1);
    bool found = false;
    float best = 0.0f;
    size_t bi = 0;
    for (int q = q0; q <= q1; q++) {
        const size_t base = (size_t)q * (size_t)W;
        for (int cb = c0; cb <= c1; cb += kNnBatch) {
            // a batch of independent loads (a lone load per candidate leaves the search waiting on memory), the ones
            // past the row's end repeated at c1 and skipped below; candidates are still taken in index order
            Pcd4 P[kNnBatch];
#pragma unroll
            for (int k = 0; k < kNnBatch; k++) P[k] = pcd[base + (size_t)(cb + k <= c1 ? cb + k : c1)];
#pragma unroll
            for (int k = 0; k < kNnBatch; k++) {
                const float dx = sx - P[k].x, dy = sy - P[k].y, dz = sz - P[k].z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                // index order: the first of equals stays
                const bool better = cb + k <= c1 && P[k].z > 0 && (!found ? d2 == d2 : d2 < best);
                if (better) {
                    found = true;
                    best = d2;
                    bi = base + (size_t)(cb + k);
                }
            }
        }
    }
    best_idx = bi;
    best_d2 = best;
    return found;
}

// thrust__pcd2Ab's row of one accepted pair
PCORE_P2P void row(float sx, float sy, float sz, float dx, float dy, float dz, float nx, float ny, float nz,
                   float (&r)[kRow]) {
    r[28] = 1.0f;
    const float ex = dx - sx, ey = dy - sy, ez = dz - sz;
    const float b = ex * nx + ey * ny + ez * nz;
    r[27] = b * b;
    float A[6];
    A[0] = nz * sy - ny * sz;
    A[1] = nx * sz - nz * sx;
    A[2] = ny * sx - nx * sy;
    A[3] = nx;
    A[4] = ny;
    A[5] = nz;
    int sh = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) r[sh++] = A[i] * A[j];
#pragma unroll
    for (int i = 0; i < 6; i++) r[21 + i] = A[i] * b;
}

PCORE_P2P void swap_d(double& a, double& b) {
    const double t = a;
    a = b;
    b = t;
}

// Eigen 3.3 LDLT<Matrix<double,6,6>, Lower>: the unblocked in-place factorisation with diagonal pivoting (largest
// |diagonal| of the trailing corner, the first on ties), then P^T L^-T D^+ L^-1 P b.  A is the symmetric system from
// the sums' upper triangle (acc[0..20], row by row); only the lower triangle is touched.  Every index below is a
// constant once the loops are unrolled (the pivot row is matched against each candidate in turn), so the matrix stays
// in registers on the device.
PCORE_P2P void ldlt_solve6(const float (&acc)[kRow], double (&x)[6]) {
    double m[6][6];
    {
        int sh = 0;
#pragma unroll
        for (int y = 0; y < 6; y++)
#pragma unroll
            for (int c = y; c < 6; c++) {
                m[c][y] = (double)acc[sh];
                m[y][c] = (double)acc[sh];
                sh++;
            }
    }
    int trans[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int big = k;
        double bigv = __builtin_fabs(m[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; i++)
            if (__builtin_fabs(m[i][i]) > bigv) {
                bigv = __builtin_fabs(m[i][i]);
                big = i;
            }
        trans[k] = big;
#pragma unroll
        for (int B = k + 1; B < 6; B++)
            if (big == B) {
#pragma unroll
                for (int j = 0; j < k; j++) swap_d(m[k][j], m[B][j]);
#pragma unroll
                for (int i = B + 1; i < 6; i++) swap_d(m[i][k], m[i][B]);
                swap_d(m[k][k], m[B][B]);
#pragma unroll
                for (int i = k + 1; i < B; i++) swap_d(m[i][k], m[B][i]);
            }
        if (k > 0) {
            double temp[6];
#pragma unroll
            for (int j = 0; j < k; j++) temp[j] = m[j][j] * m[k][j];
            double dot = 0.0;
#pragma unroll
            for (int j = 0; j < k; j++) dot += m[k][j] * temp[j];
            m[k][k] -= dot;
#pragma unroll
            for (int i = k + 1; i < 6; i++) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < k; j++) s += m[i][j] * temp[j];
                m[i][k] -= s;
            }
        }
        const double akk = m[k][k];
        if (k < 5 && __builtin_fabs(akk) > 0.0) {
#pragma unroll
            for (int i = k + 1; i < 6; i++) m[i][k] /= akk;
        }
    }
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = (double)acc[21 + i];
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
        for (int B = k + 1; B < 6; B++)
            if (trans[k] == B) swap_d(d[k], d[B]);
#pragma unroll
    for (int i = 0; i < 6; i++)  // L (unit lower) forward substitution
#pragma unroll
        for (int j = 0; j < i; j++) d[i] -= m[i][j] * d[j];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = (__builtin_fabs(m[i][i]) > 2.2250738585072014e-308) ? d[i] / m[i][i] : 0.0;
#pragma unroll
    for (int i = 5; i >= 0; i--)  // L^T back substitution
#pragma unroll
        for (int j = i + 1; j < 6; j++) d[i] -= m[j][i] * d[j];
#pragma unroll
    for (int k = 5; k >= 0; k--)
#pragma unroll
        for (int B = k + 1; B < 6; B++)
            if (trans[k] == B) swap_d(d[k], d[B]);
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = d[i];
}

struct Quat {
    double w, x, y, z;
};

PCORE_P2P Quat quat_mul(const Quat& a, const Quat& b) {  // Eigen quat_product
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}

// TransformVector6dToMatrix4d (icp.cpp:7-17) -> .cast<float>()
PCORE_P2P Mat4 vec6_to_mat4(const double (&u)[6]) {
    const Quat qz = {dmath::cos_d(u[2] / 2), 0.0, 0.0, dmath::sin_d(u[2] / 2)};
    const Quat qy = {dmath::cos_d(u[1] / 2), 0.0, dmath::sin_d(u[1] / 2), 0.0};
    const Quat qx = {dmath::cos_d(u[0] / 2), dmath::sin_d(u[0] / 2), 0.0, 0.0};
    const Quat q = quat_mul(quat_mul(qz, qy), qx);
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    Mat4 r = identity();
    r.m[0][0] = (float)(1.0 - (tyy + tzz));
    r.m[0][1] = (float)(txy - twz);
    r.m[0][2] = (float)(txz + twy);
    r.m[1][0] = (float)(txy + twz);
    r.m[1][1] = (float)(1.0 - (txx + tzz));
    r.m[1][2] = (float)(tyz - twx);
    r.m[2][0] = (float)(txz - twy);
    r.m[2][1] = (float)(tyz + twx);
    r.m[2][2] = (float)(1.0 - (txx + tyy));
    r.m[0][3] = (float)u[3];
    r.m[1][3] = (float)u[4];
    r.m[2][3] = (float)u[5];
    return r;
}

// transform_pcd (icp.cpp:38-51): each row summed left to right
PCORE_P2P void apply(const Mat4& E, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = E.m[0][0] * x + E.m[0][1] * y + E.m[0][2] * z + E.m[0][3];
    oy = E.m[1][0] * x + E.m[1][1] * y + E.m[1][2] * z + E.m[1][3];
    oz = E.m[2][0] * x + E.m[2][1] * y + E.m[2][2] * z + E.m[2][3];
}

// geometry.h:292-298: result[i][j] = lhs[i] . rhs.col(j), the dot summed from index 3 down to 0 onto +0
PCORE_P2P Mat4 mat4_mul(const Mat4& a, const Mat4& b) {
    Mat4 r;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 3; k >= 0; k--) acc += a.m[i][k] * b.m[k][j];
            r.m[i][j] = acc;
        }
    return r;
}

// the linemod normal of one pixel from its saturated 16-bit depth d and the eight radius-5 neighbours' nb[] (order:
// rows -5, 0, +5, columns -5, 0, +5 without the centre), before the scaling by the focal lengths: accumBilateral in
// 64-bit integers
PCORE_P2P void linemod_sums(long long d, const long long (&nb)[8], long long& det, long long& ddx, long long& ddy) {
    const int di[8] = {-5, 0, +5, -5, +5, -5, 0, +5};
    const int dj[8] = {-5, -5, -5, 0, 0, +5, +5, +5};
    long long A0 = 0, A1 = 0, A3 = 0, b0 = 0, b1 = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const long long delta = nb[k] - d;
        const long long ad = delta < 0 ? -delta : delta;
        const long long f = ad < kLinemodMaxDiff ? 1 : 0;
        const long long fi = f * di[k], fj = f * dj[k];
        A0 += fi * di[k];
        A1 += fi * dj[k];
        A3 += fj * dj[k];
        b0 += fi * delta;
        b1 += fj * delta;
    }
    det = A0 * A3 - A1 * A1;
    ddx = A3 * b0 - A1 * b1;
    ddy = -A1 * b0 + A0 * b1;
}

}  // namespace p2p

#ifdef __HIPCC__
// pcore_p2p.hip: the projective scene of a depth image and the ICP over a chunk of per-pose slots
struct P2pArgs {
    float4* src;                // chunk-local slots (segment i at src + i * src_cap), moved in place
    const int32_t* src_count;
    int32_t src_cap;
    const float4* scene_pcd;    // one float4 per pixel (x, y, z, 0)
    const float4* scene_normal; // one float4 per pixel (nx, ny, nz, 0)
    int32_t width, height;
    float fx, fy, cx, cy;
    float max_dist_diff, rel_fitness, rel_rmse;
    int32_t max_iter;
    const float* poses_in;      // batch-global N x 16, nullable with poses_out
    float* poses_out;           // nullable
    float* out_T;               // batch-global N x 16
    float* out_fitness;
    float* out_rmse;
    int32_t* out_iters;
    int32_t pose_base;          // first batch index of this chunk
    int32_t window;             // the nearest-neighbour scene's half-width in pixels (launch_p2p_nn_icp only)
};
// one one-wave workgroup per pose of the chunk
hipError_t launch_p2p_icp(const P2pArgs& a, int num_poses, hipStream_t s);
// the same over the nearest-neighbour scene: max_dist_diff is the radius, window the search's half-width
hipError_t launch_p2p_nn_icp(const P2pArgs& a, int num_poses, hipStream_t s);
// one thread per pixel: pcd4 / normal4 (float4 per pixel), and / or the packed 3-float buffers; each nullable
hipError_t launch_p2p_scene(const int32_t* depth_cm, int width, int height, float fx, float fy, float cx, float cy,
                            float4* pcd4, float4* normal4, float* pcd3, float* normal3, hipStream_t s);
#endif

}  // namespace pcore
