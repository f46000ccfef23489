"""The nearest-neighbour scene's query ("Nearest-neighbour scene") in numpy float32, written from
the spec's text and independently of perception_amd/csrc/pcore_p2p_math.h, and the point-to-plane loop over it: the
sums, the solve, the increment and the composition are tests/p2p_reference.py's.

The query of a point s (camera frame) with radius r = max_dist_diff and window half-width w:

    1. centre    (x, y) = the projective spec's pixel of s; no correspondence when a coordinate is not convertible
                 (NaN, |v| >= 2^31) or !(s.z > 0)
    2. candidates every pixel (c, q) of the image with |c - x| <= w and |q - y| <= w whose scene point P has P.z > 0
    3. distance  d2 = (fl(dx dx) + fl(dy dy)) + fl(dz dz), dx = s.x - P.x, ...
    4. winner    the smallest d2; the lowest pixel index q W + c among equals
    5. accepted  iff d2 < fl(r r)

It looks at every pixel of the window: no bound rectangle, no early exit.  `rule` swaps one step for a wrong one, for
the certificates of tests/test_p2p_nn_spec.py (a case that no wrong rule changes tests nothing):

    "spec"        the above
    "inclusive"   accepted iff d2 <= fl(r r)
    "highest"     the highest pixel index among equals
    "centre"      the centre pixel is the only candidate (w = 0)
    "nolimit"     every pixel of the image is a candidate
    "depth0"      pixels with P.z <= 0 are candidates too
    "projective"  the projective scene's association and acceptance (tests/p2p_reference.py)
"""
from __future__ import annotations

import numpy as np

from tests import p2p_reference as ref

F = np.float32
MAX_ITER = ref.MAX_ITER
REL_FITNESS = ref.REL_FITNESS
REL_RMSE = ref.REL_RMSE
MAX_DIST_DIFF = 0.01
WINDOW = 32
RULES = ("spec", "inclusive", "highest", "centre", "nolimit", "depth0", "projective")
_BLOCK = 32  # points per gathered block: 32 x 257^2 candidates at the largest window


def query(pts, pcd, fx, fy, cx, cy, max_dist_diff=MAX_DIST_DIFF, window=WINDOW, rule="spec"):
    """-> (accepted (n,) bool, pixel index of the winner (n,) int64, 0 where there is none, d2 of the winner)."""
    assert rule in RULES and rule != "projective"
    H, W = pcd.shape[:2]
    n = len(pts)
    flat = pcd.reshape(-1, 3)
    sx, sy, sz = pts[:, 0], pts[:, 1], pts[:, 2]
    okx, x = ref._pixel(sx, sz, fx, cx)
    oky, y = ref._pixel(sy, sz, fy, cy)
    with np.errstate(all="ignore"):
        centre = okx & oky & (sz > 0)
    if rule == "centre":
        window = 0
    rr = F(F(max_dist_diff) * F(max_dist_diff))
    ok = np.zeros(n, bool)
    win = np.zeros(n, np.int64)
    best = np.zeros(n, F)
    for b in range(0, n, _BLOCK):
        e = min(n, b + _BLOCK)
        if rule == "nolimit" or (2 * window + 1) ** 2 > W * H:  # the image's pixels, those of the window marked
            c = np.broadcast_to(np.arange(W, dtype=np.int64), (e - b, W))
            q = np.broadcast_to(np.arange(H, dtype=np.int64), (e - b, H))
            lim = np.iinfo(np.int64).max if rule == "nolimit" else window
            cin, qin = np.abs(c - x[b:e, None]) <= lim, np.abs(q - y[b:e, None]) <= lim
        else:                                                   # the window's pixels, those of the image marked
            o = np.arange(-window, window + 1, dtype=np.int64)
            c = x[b:e, None] + o[None, :]  # int64: |x| < 2^31 cannot overflow
            q = y[b:e, None] + o[None, :]
            cin, qin = (c >= 0) & (c < W), (q >= 0) & (q < H)
        idx = np.clip(q, 0, H - 1)[:, :, None] * W + np.clip(c, 0, W - 1)[:, None, :]
        P = flat[idx]
        with np.errstate(all="ignore"):
            dx = sx[b:e, None, None] - P[..., 0]
            dy = sy[b:e, None, None] - P[..., 1]
            dz = sz[b:e, None, None] - P[..., 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            cand = qin[:, :, None] & cin[:, None, :] & ~np.isnan(d2) & centre[b:e, None, None]
            if rule != "depth0":
                cand &= P[..., 2] > 0
        m = e - b
        d2 = d2.reshape(m, -1)
        cand = cand.reshape(m, -1)
        idx = idx.reshape(m, -1)
        has = cand.any(1)
        dmin = np.where(cand, d2, F(np.inf)).min(1)
        hit = cand & (d2 == dmin[:, None])
        # in the window's row-major order the pixel index grows, so the first hit is the lowest index
        j = np.where(has, hit.shape[1] - 1 - hit[:, ::-1].argmax(1) if rule == "highest" else hit.argmax(1), 0)
        r = np.arange(m)
        with np.errstate(all="ignore"):
            acc = (dmin <= rr) if rule == "inclusive" else (dmin < rr)
        ok[b:e] = has & acc
        win[b:e] = np.where(has, idx[r, j], 0)
        best[b:e] = np.where(has, d2[r, j], F(0.0))
    return ok, win, best


def rows_of(pts, pcd, nrm, fx, fy, cx, cy, max_dist_diff=MAX_DIST_DIFF, window=WINDOW, rule="spec"):
    """The 29-float rows of every point against its winner (n, 29), +0 rows for the points without a correspondence,
    and the accepted mask: the row of tests/p2p_reference.py's rows_of, operation for operation."""
    if rule == "projective":
        return ref.rows_of(pts, pcd, nrm, fx, fy, cx, cy, max_dist_diff)
    ok, win, _ = query(pts, pcd, fx, fy, cx, cy, max_dist_diff, window, rule)
    d = pcd.reshape(-1, 3)[win]
    n = nrm.reshape(-1, 3)[win]
    sx, sy, sz = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
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


def icp(cloud, pcd, nrm, fx, fy, cx, cy, order="wave", trig="spec", max_iterations=MAX_ITER,
        relative_fitness=REL_FITNESS, relative_rmse=REL_RMSE, max_dist_diff=MAX_DIST_DIFF, window=WINDOW, rule="spec"):
    """tests/p2p_reference.py's icp with the query above -> (T (4, 4) float32, fitness, rmse, iteration, moved cloud)."""
    pts = np.array(cloud, F, copy=True).reshape(-1, 3)
    pcd, nrm = np.ascontiguousarray(pcd, F), np.ascontiguousarray(nrm, F)
    T = np.eye(4, dtype=F)
    fitness, rmse = F(0.0), F(0.0)
    for it in range(max_iterations + 1):
        r, _ = rows_of(pts, pcd, nrm, fx, fy, cx, cy, max_dist_diff, window, rule)
        acc = ref.sum_rows(r, order)
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
            E = ref.vec6_to_mat4(ref.ldlt_solve6(acc), trig)
            x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
            for k in range(3):
                pts[:, k] = E[k, 0] * x + E[k, 1] * y + E[k, 2] * z + E[k, 3]
        T = ref.mat4_mul(E, T)
    return T, fitness, rmse, max_iterations, pts


def run_clouds(clouds, pcd, nrm, fx, fy, cx, cy, **kw):
    """icp over a list of clouds -> (T (N, 16), fitness (N,), rmse (N,), iterations (N,), moved clouds)."""
    n = len(clouds)
    T = np.zeros((n, 16), F)
    fit, rmse, its = np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int32)
    moved = []
    for i, c in enumerate(clouds):
        t, fit[i], rmse[i], its[i], m = icp(c, pcd, nrm, fx, fy, cx, cy, **kw)
        T[i] = t.reshape(16)
        moved.append(m)
    return T, fit, rmse, its, moved


same_bits = ref.same_bits
