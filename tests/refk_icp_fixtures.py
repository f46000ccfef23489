"""The fixtures of tests/golden/make_reference_icp_goldens.py -- what the reference's own cuda_icp sources compute on
the host (oracle/ref_host/driver_icp.cpp) -- as tests/test_reference_icp_goldens.py (CPU: the oracle and the numpy
specs) and tests/test_gpu_reference_icp_goldens.py (GPU: the kernels) read them.  Only tests/golden/ is read here.

Packing.  A scene's buffers (H x W x 3 floats, twice) and the 29-float rows do not compress, and a fixture has to stay
under 68,947 bytes.  So a large float array R of the reference is stored as `R xor P` on its bits, where P is a
prediction that this module computes in numpy from the other fixture data (scene_np, row_formula, depth2cloud_np
below); load() gives `stored xor P` back, which is R bit for bit whatever P is.  The prediction only makes the stored
words mostly zero.  It is this module's own restatement, never the code under test, and a wrong prediction costs
bytes, not truth.  The generator checks that load() returns every array of the reference unchanged.

The wrong-rule switches (scene_np's and rows_proj's `rule`, icp_loop's `compose` and `extra_turn`) serve the
certificates of tests/test_reference_icp_goldens.py: a fixture that no wrong rule changes tests nothing.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from tests import p2p_reference as ref

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAMERAS = ("tiny", "small")
ROWS_SIZES = (1, 63, 64, 65, 200)          # the wave boundaries of the kernel's sum
RUNS = ("none", "converge", "cap")          # no accepted point; the relative criteria before 30; the extra turn
SCENES = ("proj", "nn")
MAX_DIST_DIFF = 0.1                         # Scene_projective's (depth_scene.h:9); Scene_nn's 0.01 is private to it
NN_RADIUS = 0.01
SCENE_RULES = ("diff<=50", "depth<=2000", "border", "uint32")
ROW_RULES = ("no_half", "ge")


# ---- bits ----------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def pack(reference, prediction):
    assert reference.shape == prediction.shape, (reference.shape, prediction.shape)
    return bits(reference) ^ bits(prediction)


def unpack(stored, prediction):
    return (np.ascontiguousarray(stored, np.uint32) ^ bits(prediction)).view(F)


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype != F or want.dtype != F:
        assert np.array_equal(got, want), (what, got, want)
        return
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} differ; first at {tuple(bad[0])}: got " \
                          f"{got[tuple(bad[0])]!r}, reference {want[tuple(bad[0])]!r}"


def differs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return True
    if a.dtype == F and b.dtype == F:
        return bool((bits(a) != bits(b)).any())
    return not np.array_equal(a, b)


# ---- the predictions: numpy restatements of get_normal, dep2pcd, depth2cloud_cpu and the row ------------------------

def scene_np(depth, fx, fy, cx, cy, rule="spec"):
    """Scene_projective's buffers of an (H, W) int32 cm image in numpy float32 / int64: dep2pcd of the uint32 read, and
    get_normal's linemod normals of the image saturated to uint16.  rule: "spec", or one of SCENE_RULES -- the
    difference test as <= 50, the distance test as <= 2000, the borders as H - r and W - r instead of H - r - 1 and
    W - r - 1, or the normals from the uint32 read instead of the saturated value."""
    assert rule == "spec" or rule in SCENE_RULES
    d = np.ascontiguousarray(depth, np.int32)
    H, W = d.shape
    u = d.astype(np.int64) & 0xFFFFFFFF
    z = u.astype(F) / F(100.0)
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    x = (c.astype(F) - F(cx)) / F(fx) * z
    y = (r.astype(F) - F(cy)) / F(fy) * z
    pcd = np.where((u == 0)[..., None], F(0), np.stack([x, y, z], -1)).astype(F)
    s = u if rule == "uint32" else np.clip(d.astype(np.int64), 0, 65535)
    R = 5
    edge = 0 if rule == "border" else 1
    nrm = np.zeros((H, W, 3), F)
    ys, xs = slice(R, H - R - edge), slice(R, W - R - edge)
    if H - R - edge <= R or W - R - edge <= R:
        return pcd, nrm
    ld = s[ys, xs]
    A0 = np.zeros_like(ld)
    A1 = np.zeros_like(ld)
    A3 = np.zeros_like(ld)
    b0 = np.zeros_like(ld)
    b1 = np.zeros_like(ld)
    for i, j in ((-R, -R), (0, -R), (R, -R), (-R, 0), (R, 0), (-R, R), (0, R), (R, R)):
        delta = s[R + j:H - R - edge + j, R + i:W - R - edge + i] - ld
        f = (np.abs(delta) <= 50) if rule == "diff<=50" else (np.abs(delta) < 50)
        f = f.astype(np.int64)
        A0 += f * i * i
        A1 += f * i * j
        A3 += f * j * j
        b0 += f * i * delta
        b1 += f * j * delta
    det = A0 * A3 - A1 * A1
    ddx = A3 * b0 - A1 * b1
    ddy = -A1 * b0 + A0 * b1
    with np.errstate(all="ignore"):
        nx = F(fx) * ddx.astype(F)
        ny = F(fy) * ddy.astype(F)
        nz = (-det * ld).astype(F)
        root = np.sqrt(nx * nx + ny * ny + nz * nz)
        inv = F(1.0) / root
        n = np.stack([nx * inv, ny * inv, nz * inv], -1)
    near = (ld <= 2000) if rule == "depth<=2000" else (ld < 2000)
    nrm[ys, xs] = np.where((near & (root > 0))[..., None], n, F(0)).astype(F)
    return pcd, nrm


def depth2cloud_np(depth, fx, fy, cx, cy):
    """depth2cloud_cpu<int32_t> at stride 1: the pixels with depth > 0 in row-major order."""
    d = np.ascontiguousarray(depth, np.int32)
    H, W = d.shape
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    z = d.astype(F) / F(100.0)
    x = (c.astype(F) - F(cx)) / F(fx) * z
    y = (r.astype(F) - F(cy)) / F(fy) * z
    return np.stack([x, y, z], -1)[d > 0].astype(F)


def row_formula(src, dst, nrm, valid):
    """thrust__pcd2Ab's 29 floats of every point from what the scene's query returned; zero rows where it returned
    nothing."""
    sx, sy, sz = (src[:, i] for i in range(3))
    nx, ny, nz = (nrm[:, i] for i in range(3))
    with np.errstate(all="ignore"):
        b = (dst[:, 0] - sx) * nx + (dst[:, 1] - sy) * ny + (dst[:, 2] - sz) * nz
        A = [nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz]
        r = np.zeros((len(src), 29), F)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                r[:, k] = A[i] * A[j]
                k += 1
        for i in range(6):
            r[:, 21 + i] = A[i] * b
        r[:, 27] = b * b
        r[:, 28] = F(1.0)
    return np.where(np.asarray(valid, bool)[:, None], r, F(0.0)).astype(F)


def rows_proj(pts, pcd, nrm, fx, fy, cx, cy, max_dist_diff=MAX_DIST_DIFF, rule="spec"):
    """The projective scene's rows and accepted mask.  rule "spec" is tests/p2p_reference.py's rows_of itself;
    "no_half" projects without the + 0.5f of pcd2dep; "ge" refuses |dz| >= max_dist_diff."""
    if rule == "spec":
        return ref.rows_of(pts, pcd, nrm, fx, fy, cx, cy, max_dist_diff)
    assert rule in ROW_RULES
    H, W = pcd.shape[:2]
    sx, sy, sz = pts[:, 0], pts[:, 1], pts[:, 2]
    half = F(0.0) if rule == "no_half" else F(0.5)
    with np.errstate(all="ignore"):
        vx = ((sx / sz) * F(fx) + F(cx)) - F(0.0) + half
        vy = ((sy / sz) * F(fy) + F(cy)) - F(0.0) + half
        fin = np.isfinite(vx) & np.isfinite(vy) & (np.abs(vx) < F(2 ** 31)) & (np.abs(vy) < F(2 ** 31))
        x = np.where(fin, vx, F(0)).astype(np.int64)
        y = np.where(fin, vy, F(0)).astype(np.int64)
    inside = fin & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    idx = np.where(inside, x + y * W, 0)
    d = pcd.reshape(-1, 3)[idx]
    n = nrm.reshape(-1, 3)[idx]
    with np.errstate(all="ignore"):
        dz = sz - d[:, 2]
        adz = np.where(dz > 0, dz, -dz)
        far = (adz >= F(max_dist_diff)) if rule == "ge" else (adz > F(max_dist_diff))
    ok = inside & ~((d[:, 2] <= 0) | far)
    return row_formula(pts, d, n, ok), ok


def icp_loop(rows_fn, cloud, order="index", trig="libm", max_iterations=ref.MAX_ITER, compose="left", extra_turn=True):
    """ICP_Point2Plane_cpu over rows_fn(points) -> (rows, accepted), with tests/p2p_reference.py's sums, solve,
    increment and product.  compose "right" forms T E instead of E T; extra_turn False stops the loop one turn early
    (iter < max_iteration_): both are wrong rules."""
    pts = np.array(cloud, F, copy=True).reshape(-1, 3)
    T = np.eye(4, dtype=F)
    fitness, rmse = F(0.0), F(0.0)
    last = max_iterations if extra_turn else max_iterations - 1
    for it in range(last + 1):
        acc = ref.sum_rows(rows_fn(pts)[0], order)
        prev_fit, prev_rmse = fitness, rmse
        count, total = acc[28], acc[27]
        if count == 0:
            return T, fitness, rmse, it, pts
        with np.errstate(all="ignore"):
            fitness = F(count / F(len(pts)))
            rmse = np.sqrt(F(total / count))
            if extra_turn and it == max_iterations:
                return T, fitness, rmse, it, pts
            if np.abs(F(fitness - prev_fit)) < F(ref.REL_FITNESS) and np.abs(F(rmse - prev_rmse)) < F(ref.REL_RMSE):
                return T, fitness, rmse, it, pts
            E = ref.vec6_to_mat4(ref.ldlt_solve6(acc), trig)
            x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
            for k in range(3):
                pts[:, k] = E[k, 0] * x + E[k, 1] * y + E[k, 2] * z + E[k, 3]
        T = ref.mat4_mul(E, T) if compose == "left" else ref.mat4_mul(T, E)
    return T, fitness, rmse, last + 1, pts


# ---- loading -------------------------------------------------------------------------------------------------------

def camera(fx):
    return tuple(float(v) for v in fx["camera"])


def unpacked(z):
    """The fixture's arrays with the packed ones restored (see the module's text)."""
    out = {k: z[k] for k in z if not k.endswith("_x")}
    cam = tuple(float(v) for v in out["camera"])
    depth = out["depth"]
    ppcd, pnrm = scene_np(depth, *cam)
    out["scene_pcd"] = unpack(z["scene_pcd_x"], ppcd)
    out["scene_normal"] = unpack(z["scene_normal_x"], pnrm)
    out["depth2cloud"] = unpack(z["depth2cloud_x"], depth2cloud_np(depth, *cam))
    flat_p, flat_n = out["scene_pcd"].reshape(-1, 3), out["scene_normal"].reshape(-1, 3)
    for s in SCENES:
        pix = out[f"{s}_pixel"]
        ok = pix >= 0
        at = np.where(ok, pix, 0)
        out[f"{s}_valid"] = ok
        out[f"{s}_dst_pcd"] = np.where(ok[:, None], flat_p[at], F(0)).astype(F)
        out[f"{s}_dst_normal"] = np.where(ok[:, None], flat_n[at], F(0)).astype(F)
        out[f"{s}_rows"] = unpack(z[f"{s}_rows_x"], row_formula(out["rows_cloud"], out[f"{s}_dst_pcd"],
                                                               out[f"{s}_dst_normal"], ok))
    return out


@functools.lru_cache(maxsize=None)
def load(cam):
    """tests/golden/refk_icp_<cam>.npz, unpacked, read-only."""
    with np.load(os.path.join(GOLDEN, f"refk_icp_{cam}.npz")) as z:
        out = unpacked({k: z[k] for k in z.files})
    for v in out.values():
        v.setflags(write=False)
    return out


def rows_clouds(fx):
    """The clouds of ROWS_SIZES as slices of the fixture's rows_cloud: [(start, end), ...]."""
    ends = np.cumsum(fx["rows_cnt"])
    return [(int(e - n), int(e)) for n, e in zip(fx["rows_cnt"], ends)]
