// pcore_gicp_scan.h -- GICP's correspondence search of segments up to kKeyScanMax targets, a scan of the segment's
// correspondence keys (pcore_gicp_math.h nn_key) through the scalar cache: scan_quads for one query per lane
// (gicp_wide_kernel, odd last rounds), scan_quads2 for two from one pass (gicp_kernel's round pairs).  Both return
// the oracle's first strict minimum, bit for bit.  Knobs: PCORE_SCAN_UNROLL, PCORE_SCAN2_UNROLL.
#pragma once

#include "pcore_gicp_math.h"

namespace pcore {
namespace {

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));

// Nearest of a segment's targets read through the scalar cache: every lane scans the same quads of four targets
// stored as correspondence keys (pcore_gicp_math.h: -2 t'x [4], -2 t'y [4], -2 t'z [4], |t'|^2 [4] about the
// segment's origin, which the header quad before them holds), so the loads are wave-uniform s_loads and the
// targets reach the VALU as SGPR operands -- no LDS traffic (an LDS broadcast read still moves 64 lanes x 16 B
// through the LDS pipe).  A pair of targets costs three packed FMAs.  The index work stays out of the per-quad
// loop: alternate quads feed two chains that keep only their smallest quad minimum and the first quad reaching it
// (strict <); the chains merge by (key, quad), and the winning quad's element is found once at the end by
// recomputing its four keys (the same FMAs, so one of them equals the minimum bit for bit) and taking the first
// equal one -- the lexicographic minimum of (key, index), i.e. the oracle's first strict minimum.  Measured on
// C3's GICP call: a per-quad (distance, index) tournament over x / y / z quads 21.9 ms, the index-free scan of
// float squared distances 21.2 ms.  Keys of finite targets and a finite query are finite, so minNum's NaN
// handling never decides a comparison.
typedef __attribute__((address_space(4))) const f4v cf4v;
#ifndef PCORE_SCAN_UNROLL
#define PCORE_SCAN_UNROLL 4  // quad pairs per loop trip (C3: 2 -> 4: 20.60 -> 20.45 ms per step; 1: 21.25)
#endif
#ifndef PCORE_SCAN2_UNROLL
#define PCORE_SCAN2_UNROLL 2  // scan_quads2: quad pairs per loop trip
#endif

// the smallest of a quad's four keys for the query (x2, y2, z2: its centred coordinates, each twice)
__device__ __forceinline__ float quad_min(const f4v& X, const f4v& Y, const f4v& Z, const f4v& T, f2v x2, f2v y2,
                                          f2v z2) {
    const f2v ka = __builtin_elementwise_fma(X.xy, x2, __builtin_elementwise_fma(Y.xy, y2,
                                              __builtin_elementwise_fma(Z.xy, z2, T.xy)));
    const f2v kb = __builtin_elementwise_fma(X.zw, x2, __builtin_elementwise_fma(Y.zw, y2,
                                              __builtin_elementwise_fma(Z.zw, z2, T.zw)));
    return fminf(fminf(fminf(ka.x, ka.y), kb.x), kb.y);
}

__device__ __forceinline__ void scan_quads(const float* seg_quads, int nt, float qx, float qy, float qz, float& best,
                                           int& j) {
    const int nq = (nt + 3) >> 2;
    const cf4v* hq = (const cf4v*)seg_quads;
    const f4v org = hq[0];
    qx = qx - org.x;
    qy = qy - org.y;
    qz = qz - org.z;
    if (!(__builtin_isfinite(qx) && __builtin_isfinite(qy) && __builtin_isfinite(qz))) return;  // no correspondence
    const cf4v* tq = hq + 4;
    const f2v qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    float bA = INFINITY, bB = INFINITY;
    int oA = -1, oB = -1;
    auto qmin = [&](const cf4v* q) {
        const f4v X = q[0], Y = q[1], Z = q[2], T = q[3];
        return quad_min(X, Y, Z, T, qx2, qy2, qz2);
    };
    int o = 0;
    const cf4v* q = tq;  // wave-uniform: the quads' addresses stay scalar
#pragma unroll PCORE_SCAN_UNROLL
    for (; o + 2 <= nq; o += 2, q += 8) {
        const float ma = qmin(q);
        if (ma < bA) { bA = ma; oA = o; }
        const float mb = qmin(q + 4);
        if (mb < bB) { bB = mb; oB = o + 1; }
    }
    if (o < nq) {
        const float ma = qmin(q);
        if (ma < bA) { bA = ma; oA = o; }
    }
    if (bB < bA || (bB == bA && oB >= 0 && oB < oA)) { bA = bB; oA = oB; }
    if (bA < best) {
        // the winning quad, per lane (a vector load), its first element at the minimum
        const float* Q = seg_quads + 16 + 16 * oA;
        const float4 X = *reinterpret_cast<const float4*>(Q), Y = *reinterpret_cast<const float4*>(Q + 4);
        const float4 Z = *reinterpret_cast<const float4*>(Q + 8), T = *reinterpret_cast<const float4*>(Q + 12);
        const int k = gicpm::nn_key(X.x, Y.x, Z.x, T.x, qx, qy, qz) == bA ? 0
                    : gicpm::nn_key(X.y, Y.y, Z.y, T.y, qx, qy, qz) == bA ? 1
                    : gicpm::nn_key(X.z, Y.z, Z.z, T.z, qx, qy, qz) == bA ? 2 : 3;
        best = bA;
        // one of the four recomputed keys equals bA (same FMAs); the clamp only keeps a broken match (which would
        // pick slot 3, padding in a segment's last quad) inside the segment
        j = min(4 * oA + k, nt - 1);
    }
}

// scan_quads for two queries per lane (the pose's source points i and i + 64): every scalar load of a quad feeds both,
// so a pair of rounds reads the segment's key quads once.  Each query keeps its own two chains (alternate quads) and
// its own winner recovery, so (best, j) of each is scan_quads' bit for bit.
__device__ __forceinline__ void scan_quads2(const float* seg_quads, int nt, float ax, float ay, float az, float bx,
                                            float by, float bz, int& ja, int& jb) {
    const int nq = (nt + 3) >> 2;
    const cf4v* hq = (const cf4v*)seg_quads;
    const f4v org = hq[0];
    ax = ax - org.x; ay = ay - org.y; az = az - org.z;
    bx = bx - org.x; by = by - org.y; bz = bz - org.z;
    const bool fa = __builtin_isfinite(ax) && __builtin_isfinite(ay) && __builtin_isfinite(az);
    const bool fb = __builtin_isfinite(bx) && __builtin_isfinite(by) && __builtin_isfinite(bz);
    const cf4v* tq = hq + 4;
    const f2v ax2 = {ax, ax}, ay2 = {ay, ay}, az2 = {az, az};
    const f2v bx2 = {bx, bx}, by2 = {by, by}, bz2 = {bz, bz};
    float aA = INFINITY, aB = INFINITY, bA = INFINITY, bB = INFINITY;
    int oaA = -1, oaB = -1, obA = -1, obB = -1;
    auto qmin2 = [&](const cf4v* q, float& ma, float& mb) {
        const f4v X = q[0], Y = q[1], Z = q[2], T = q[3];
        ma = quad_min(X, Y, Z, T, ax2, ay2, az2);
        mb = quad_min(X, Y, Z, T, bx2, by2, bz2);
    };
    int o = 0;
    const cf4v* q = tq;
#pragma unroll PCORE_SCAN2_UNROLL
    for (; o + 2 <= nq; o += 2, q += 8) {
        float ma, mb;
        qmin2(q, ma, mb);
        if (ma < aA) { aA = ma; oaA = o; }
        if (mb < bA) { bA = mb; obA = o; }
        qmin2(q + 4, ma, mb);
        if (ma < aB) { aB = ma; oaB = o + 1; }
        if (mb < bB) { bB = mb; obB = o + 1; }
    }
    if (o < nq) {
        float ma, mb;
        qmin2(q, ma, mb);
        if (ma < aA) { aA = ma; oaA = o; }
        if (mb < bA) { bA = mb; obA = o; }
    }
    if (aB < aA || (aB == aA && oaB >= 0 && oaB < oaA)) { aA = aB; oaA = oaB; }
    if (bB < bA || (bB == bA && obB >= 0 && obB < obA)) { bA = bB; obA = obB; }
    auto element = [&](int oq, float m, float qx, float qy, float qz) {  // first key == m in quad oq
        const float* Q = seg_quads + 16 + 16 * oq;
        const float4 X = *reinterpret_cast<const float4*>(Q), Y = *reinterpret_cast<const float4*>(Q + 4);
        const float4 Z = *reinterpret_cast<const float4*>(Q + 8), T = *reinterpret_cast<const float4*>(Q + 12);
        const int k = gicpm::nn_key(X.x, Y.x, Z.x, T.x, qx, qy, qz) == m ? 0
                    : gicpm::nn_key(X.y, Y.y, Z.y, T.y, qx, qy, qz) == m ? 1
                    : gicpm::nn_key(X.z, Y.z, Z.z, T.z, qx, qy, qz) == m ? 2
                    : gicpm::nn_key(X.w, Y.w, Z.w, T.w, qx, qy, qz) == m ? 3 : 4;
        // one of the keys equals m (same FMAs); the clamp only keeps a broken match inside the segment
        return min(4 * oq + min(k, 3), nt - 1);
    };
    ja = fa && aA < INFINITY ? element(oaA, aA, ax, ay, az) : -1;
    jb = fb && bA < INFINITY ? element(obA, bA, bx, by, bz) : -1;
}

}  // namespace
}  // namespace pcore
