"""The point-to-plane projective ICP spec ("Point-to-plane ICP spec") in numpy float32 / Python
float, written independently of perception_amd/csrc/pcore_p2p_math.h: the loop of icp_point2plane in
oracle/ref_cpu_path.cpp, operation for operation, with the build-owned choices as switches.

    order = "wave"   lane l of 64 adds the rows of points l, l + 64, ... in that order; the 64 partial sums are
                     combined by an xor butterfly with masks 32, 16, 8, 4, 2, 1            (the spec, the GPU kernel)
            "index"  every row added in index order                                         (the oracle)
    trig  = "spec"   oracle.sin_d / oracle.cos_d (pcore::dmath)                             (the spec)
            "libm"   math.sin / math.cos                                                    (the oracle)

tests/test_p2p_spec.py holds order="index", trig="libm" to oracle.ref_icp bit for bit, which pins everything but those
choices to the committed oracle; tests/test_gpu_p2p.py holds the GPU kernel to order="wave", trig="spec".

Every float32 operation is one numpy float32 operation (no fused multiply-add); a sequential float32 sum is
np.add.accumulate, which adds in order.  A rejected point adds +0 where the kernel adds nothing: the sums start at +0
and a float sum is never -0 after that, so the bits are the same.
"""
from __future__ import annotations

import math

import numpy as np

import oracle

F = np.float32
MAX_ITER = 30
REL_FITNESS = 1e-5
REL_RMSE = 1e-5
MAX_DIST_DIFF = 0.1
DBL_MIN = 2.2250738585072014e-308


def _pixel(num, z, f, c):
    """((num / z) * f + c) - 0 + 0.5 in float32 -> (convertible, truncated value)."""
    with np.errstate(all="ignore"):
        v = ((num / z) * F(f) + F(c)) - F(0.0) + F(0.5)
        ok = ~np.isnan(v) & (np.abs(v) < F(2147483648.0))
    return ok, np.where(ok, v, F(0.0)).astype(np.int64)  # astype truncates toward zero


def rows_of(pts, pcd, nrm, fx, fy, cx, cy, max_dist_diff):
    """The 29-float rows of every point (n, 29), +0 rows for the rejected ones, and the accepted mask."""
    H, W = pcd.shape[:2]
    sx, sy, sz = pts[:, 0], pts[:, 1], pts[:, 2]
    okx, x = _pixel(sx, sz, fx, cx)
    oky, y = _pixel(sy, sz, fy, cy)
    inside = okx & oky & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    idx = np.where(inside, x + y * W, 0)
    d = pcd.reshape(-1, 3)[idx]
    n = nrm.reshape(-1, 3)[idx]
    with np.errstate(all="ignore"):
        dz = sz - d[:, 2]
        adz = np.where(dz > 0, dz, -dz)
        ok = inside & ~((d[:, 2] <= 0) | (adz > F(max_dist_diff)))
        ex, ey, ez = d[:, 0] - sx, d[:, 1] - sy, d[:, 2] - sz
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        b = ex * nx + ey * ny + ez * nz
        A = [nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz]
        r = np.zeros((len(pts), 29), F)
        sh = 0
        for i in range(6):
            for j in range(i, 6):
                r[:, sh] = A[i] * A[j]
                sh += 1
        for i in range(6):
            r[:, 21 + i] = A[i] * b
        r[:, 27] = b * b
        r[:, 28] = F(1.0)
    return np.where(ok[:, None], r, F(0.0)), ok


def sum_rows(r, order):
    """The 29 sums of the rows in the given order, float32."""
    zero = np.zeros((1, 29), F)
    with np.errstate(all="ignore"):
        if order == "index":
            return np.add.accumulate(np.concatenate([zero, r]), axis=0, dtype=F)[-1]
        assert order == "wave"
        rounds = (len(r) + 63) // 64
        pad = np.zeros((rounds * 64, 29), F)
        pad[:len(r)] = r
        S = np.add.accumulate(np.concatenate([np.zeros((1, 64, 29), F), pad.reshape(rounds, 64, 29)]), axis=0,
                              dtype=F)[-1]
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            S = S + S[lane ^ m]
        assert (S.view(np.uint32) == S[0].view(np.uint32)).all() or np.isnan(S).any()
        return S[0]


def ldlt_solve6(acc):
    """Eigen 3.3 LDLT<Matrix<double,6,6>, Lower> with diagonal pivoting on the sums' system, in Python floats."""
    n = 6
    m = [[0.0] * n for _ in range(n)]
    sh = 0
    for y in range(n):
        for x in range(y, n):
            m[x][y] = m[y][x] = float(acc[sh])
            sh += 1
    trans = [0] * n
    for k in range(n):
        big, bigv = k, abs(m[k][k])
        for i in range(k + 1, n):
            if abs(m[i][i]) > bigv:
                bigv, big = abs(m[i][i]), i
        trans[k] = big
        if k != big:
            for j in range(k):
                m[k][j], m[big][j] = m[big][j], m[k][j]
            for i in range(big + 1, n):
                m[i][k], m[i][big] = m[i][big], m[i][k]
            m[k][k], m[big][big] = m[big][big], m[k][k]
            for i in range(k + 1, big):
                m[i][k], m[big][i] = m[big][i], m[i][k]
        if k > 0:
            temp = [m[j][j] * m[k][j] for j in range(k)]
            dot = 0.0
            for j in range(k):
                dot += m[k][j] * temp[j]
            m[k][k] -= dot
            for i in range(k + 1, n):
                s = 0.0
                for j in range(k):
                    s += m[i][j] * temp[j]
                m[i][k] -= s
        akk = m[k][k]
        if n - k - 1 > 0 and abs(akk) > 0.0:
            for i in range(k + 1, n):
                m[i][k] = _div(m[i][k], akk)
    d = [float(acc[21 + i]) for i in range(n)]
    for k in range(n):
        if trans[k] != k:
            d[k], d[trans[k]] = d[trans[k]], d[k]
    for i in range(n):
        for j in range(i):
            d[i] -= m[i][j] * d[j]
    for i in range(n):
        d[i] = _div(d[i], m[i][i]) if abs(m[i][i]) > DBL_MIN else 0.0
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            d[i] -= m[j][i] * d[j]
    for k in range(n - 1, -1, -1):
        if trans[k] != k:
            d[k], d[trans[k]] = d[trans[k]], d[k]
    return d


def _div(a, b):
    """IEEE double division (Python raises on a zero divisor and on overflow)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def _sincos(x, trig):
    if trig == "libm":
        if math.isinf(x) or math.isnan(x):
            return math.nan, math.nan
        return math.sin(x), math.cos(x)
    assert trig == "spec"
    return oracle.sin_d(x), oracle.cos_d(x)


def vec6_to_mat4(u, trig):
    """TransformVector6dToMatrix4d: R = Rz Ry Rx as Eigen's quaternion product, then .cast<float>()."""
    sz, cz = _sincos(u[2] / 2, trig)
    sy, cy = _sincos(u[1] / 2, trig)
    sx, cx = _sincos(u[0] / 2, trig)
    w, x, y, z = _qmul(_qmul((cz, 0.0, 0.0, sz), (cy, 0.0, sy, 0.0)), (cx, sx, 0.0, 0.0))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    with np.errstate(all="ignore"):
        E = np.eye(4, dtype=F)
        E[:3, :3] = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                              [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], np.float64).astype(F)
        E[:3, 3] = np.array(u[3:6], np.float64).astype(F)
    return E


def mat4_mul(a, b):
    """result[i][j] = the dot of a's row i and b's column j, summed from index 3 down to 0 onto +0."""
    r = np.zeros((4, 4), F)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                acc = F(0.0)
                for k in (3, 2, 1, 0):
                    acc = F(acc + F(a[i, k] * b[k, j]))
                r[i, j] = acc
    return r


def icp(cloud, pcd, nrm, fx, fy, cx, cy, order="wave", trig="spec", max_iterations=MAX_ITER,
        relative_fitness=REL_FITNESS, relative_rmse=REL_RMSE, max_dist_diff=MAX_DIST_DIFF):
    """-> (T (4, 4) float32, fitness float32, rmse float32, iteration, moved cloud)."""
    pts = np.array(cloud, F, copy=True).reshape(-1, 3)
    pcd, nrm = np.ascontiguousarray(pcd, F), np.ascontiguousarray(nrm, F)
    T = np.eye(4, dtype=F)
    fitness, rmse = F(0.0), F(0.0)
    for it in range(max_iterations + 1):
        r, _ = rows_of(pts, pcd, nrm, fx, fy, cx, cy, max_dist_diff)
        acc = sum_rows(r, order)
        prev_fit, prev_rmse = fitness, rmse
        count, total = acc[28], acc[27]
        if count == 0:
            return T, fitness, rmse, it, pts
        with np.errstate(all="ignore"):
            fitness = F(count / F(len(pts)))
            rmse = np.sqrt(F(total / count))
            if it == max_iterations:
                return T, fitness, rmse, it, pts
            df, dr = F(fitness - prev_fit), F(rmse - prev_rmse)
            if np.abs(df) < F(relative_fitness) and np.abs(dr) < F(relative_rmse):
                return T, fitness, rmse, it, pts
            E = vec6_to_mat4(ldlt_solve6(acc), trig)
            x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
            for k in range(3):
                pts[:, k] = E[k, 0] * x + E[k, 1] * y + E[k, 2] * z + E[k, 3]
        T = mat4_mul(E, T)
    return T, fitness, rmse, max_iterations, pts


def run_clouds(clouds, pcd, nrm, fx, fy, cx, cy, **kw):
    """icp over a list of clouds -> (T (N, 16), fitness (N,), rmse (N,), iterations (N,))."""
    n = len(clouds)
    T = np.zeros((n, 16), F)
    fit, rmse, its = np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int32)
    for i, c in enumerate(clouds):
        t, fit[i], rmse[i], its[i], _ = icp(c, pcd, nrm, fx, fy, cx, cy, **kw)
        T[i] = t.reshape(16)
    return T, fit, rmse, its


def same_bits(a, b):
    """Equal float32 bits, any NaN equal to any NaN (a NaN's sign and payload are not part of the spec)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(np.where(na, F(0), a).view(np.uint32), np.where(nb, F(0), b).view(np.uint32))
