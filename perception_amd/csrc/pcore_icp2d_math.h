// pcore_icp2d_math.h -- the arithmetic of the planar (x, y, yaw) ICP spec ("Planar ICP spec"):
// PCL's IterativeClosestPoint loop with TransformationEstimation2D and DefaultConvergenceCriteria, as the reference's
// GetICPAdjustedPose configures it (search_env.cpp:6235-6396), restated so that two implementations agree bit for
// bit.  One set of functions for the HIP kernel (pcore_icp2d.hip) and its host-side callers; the numpy restatement
// the tests hold them to (tests/icp2d_reference.py) is written independently of this header.  Everything is double
// arithmetic on float inputs, one operation per expression node, compiled with -ffp-contract=off; there is no
// trigonometry: the rotation travels as (cos, sin).
//
// Per iteration, with the cumulative transform G = (c, s, tx, ty):
//   query        q = (float(c x - s y + tx), float(s x + c y + ty), z)            query()
//   sums         over the kept pairs, raw moments about the world origin          Sums
//   estimation   a = H00 + H11, b = H01 - H10, h = sqrt(a a + b b), c' = a / h, s' = b / h (1, 0 when h == 0),
//                t' = tbar - R' qbar                                                step()
//   compose      G <- (R', t') o G                                                  compose()
//   exit tests   iteration cap, transform threshold, absolute mse, relative mse    exit_test()
#pragma once

#ifdef __HIPCC__
#define PCORE_I2D __host__ __device__ __forceinline__
#else
#define PCORE_I2D inline
#endif

namespace pcore {
namespace icp2d {

// pcore_icp_planar's status values (include/pcore.h)
constexpr int kIterationCap = 0, kTransform = 1, kAbsMse = 2, kRelMse = 3, kNoCorrespondences = 4, kEmptyRender = 5;
constexpr int kMinPairs = 3;            // fewer kept pairs: the pose stops with kNoCorrespondences
constexpr double kAbsMseEps = 1e-12;    // DefaultConvergenceCriteria's absolute mse threshold
constexpr double kDblMax = 1.7976931348623157e308;

struct Xform {
    double c, s, tx, ty;
};

// The raw sums of one iteration's kept pairs (q = float query, t = float target, both widened to double; every
// product of two floats is exact in double): the record pcore_debug_planar_step takes, in this order.
//   n, sum qx, sum qy, sum tx, sum ty, sum qx tx, sum qx ty, sum qy tx, sum qy ty, sum d^2
constexpr int kSumTerms = 10;
struct Sums {
    double v[kSumTerms];
};

// the world-frame point of a camera-frame one: each row of the float 3 x 4 matrix left to right in float
PCORE_I2D void to_world(const float* m, float x, float y, float z, float& wx, float& wy, float& wz) {
    wx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    wy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    wz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

PCORE_I2D void query(const Xform& g, float x, float y, float& qx, float& qy) {
    const double xd = (double)x, yd = (double)y;
    qx = (float)((g.c * xd - g.s * yd) + g.tx);
    qy = (float)((g.s * xd + g.c * yd) + g.ty);
}

// pcore_count_within's float squared distance: ((0 + dx^2) + dy^2) + dz^2
PCORE_I2D float sqdist(float qx, float qy, float qz, float px, float py, float pz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    float d = dx * dx;
    d = d + dy * dy;
    d = d + dz * dz;
    return d;
}

// one kept pair into a lane's partial sums
PCORE_I2D void accumulate(Sums& a, float qx, float qy, float tx, float ty, float d2) {
    const double qxd = (double)qx, qyd = (double)qy, txd = (double)tx, tyd = (double)ty;
    a.v[0] = a.v[0] + 1.0;
    a.v[1] = a.v[1] + qxd;
    a.v[2] = a.v[2] + qyd;
    a.v[3] = a.v[3] + txd;
    a.v[4] = a.v[4] + tyd;
    a.v[5] = a.v[5] + qxd * txd;
    a.v[6] = a.v[6] + qxd * tyd;
    a.v[7] = a.v[7] + qyd * txd;
    a.v[8] = a.v[8] + qyd * tyd;
    a.v[9] = a.v[9] + (double)d2;
}

// TransformationEstimation2D on the raw sums (n >= 1): the increment (c', s', tx', ty')
PCORE_I2D Xform step(const Sums& S) {
    const double n = S.v[0];
    const double qbx = S.v[1] / n, qby = S.v[2] / n, tbx = S.v[3] / n, tby = S.v[4] / n;
    // H = sum (q - qbar)(t - tbar)^T = sum q t^T - n qbar tbar^T
    const double h00 = S.v[5] - (n * qbx) * tbx;
    const double h01 = S.v[6] - (n * qbx) * tby;
    const double h10 = S.v[7] - (n * qby) * tbx;
    const double h11 = S.v[8] - (n * qby) * tby;
    const double a = h00 + h11, b = h01 - h10;
    const double h = __builtin_sqrt(a * a + b * b);
    Xform d;
    d.c = 1.0;
    d.s = 0.0;
    if (h != 0.0) {  // a NaN h (non-finite sums) divides too and carries the NaN into the exit tests
        d.c = a / h;
        d.s = b / h;
    }
    d.tx = tbx - (d.c * qbx - d.s * qby);
    d.ty = tby - (d.s * qbx + d.c * qby);
    return d;
}

// G <- (R', t') o G
PCORE_I2D Xform compose(const Xform& d, const Xform& g) {
    Xform o;
    o.c = d.c * g.c - d.s * g.s;
    o.s = d.s * g.c + d.c * g.s;
    o.tx = (d.c * g.tx - d.s * g.ty) + d.tx;
    o.ty = (d.s * g.tx + d.c * g.ty) + d.ty;
    return o;
}

// DefaultConvergenceCriteria::hasConverged's tests in its order, after `iters` completed iterations whose last
// increment is d and whose mean squared distance is mse (prev: the one before, kDblMax at first): the status, or -1
// to go on
PCORE_I2D int exit_test(int iters, int max_iterations, const Xform& d, double mse, double prev, double eps_t,
                        double eps_fit) {
    if (iters >= max_iterations) return kIterationCap;
    if (d.c >= 1.0 - eps_t && d.tx * d.tx + d.ty * d.ty <= eps_t) return kTransform;
    const double diff = __builtin_fabs(mse - prev);
    if (diff < kAbsMseEps) return kAbsMse;
    if (diff / prev < eps_fit) return kRelMse;
    return -1;
}

}  // namespace icp2d
}  // namespace pcore
