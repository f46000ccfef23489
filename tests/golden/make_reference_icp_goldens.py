"""Golden vectors from the reference's own point-to-plane ICP sources, compiled for the host (oracle/ref_host/).

Run it where the reference is (PCORE_REFERENCE_ROOT, default /root/reference), from the repository root:

    python tests/golden/make_reference_icp_goldens.py

It builds oracle/_ref/ref_icp_san (oracle.build_ref(): cuda_icp's scenes, get_normal, kd-tree, thrust__pcd2Ab and
ICP_Point2Plane_cpu behind a shim cv::Mat, with -fsanitize=address,undefined and without OpenMP), runs it once per
request and writes tests/golden/refk_icp_<camera>.npz for the tiny and small cameras.  A sanitizer report fails the
run.  Every edge case the fixtures are there for is asserted on the reference's own output before anything is written.
tests/test_reference_icp_goldens.py holds the oracle and the numpy specs to the fixtures on the CPU,
tests/test_gpu_reference_icp_goldens.py the kernels on the GPU.

The 6 x 6 solve is NOT the reference's (Eigen is not available): the program calls the oracle's restatement of it.
Everything around the solve is the reference's text.  The large float arrays are stored xor a numpy prediction
(tests/refk_icp_fixtures.py, "Packing"): lossless, checked below.

Besides the reference's results the generator stores three things of its own, all computed with the numpy specs and
all about the fixture, not about the code under test:
  nn_unique, nn_offset   for every nearest-neighbour query, by brute force over the whole image in the spec's distance
                         arithmetic: whether the nearest scene point is unique, and the winner's pixel offset from the
                         point's own pixel (nn_max_offset: the largest over the accepted queries)
  order_trig_dev         for every full run, |(order "index", trig "libm") - (order "wave", trig "spec")| of
                         tests/p2p_reference.py's loop: the largest over T, and for fitness and rmse -- the exact price
                         of the two build-owned choices on that case -- and whether both return at the same iteration
"""
from __future__ import annotations

import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_host as rh  # noqa: E402
from tests import p2p_nn_cases  # noqa: E402
from tests import p2p_nn_reference as nn  # noqa: E402
from tests import p2p_reference as ref  # noqa: E402
from tests import refk_icp_fixtures as fxm  # noqa: E402

F = np.float32
MAX_BYTES = 68947  # the largest fixture committed before the refk_ ones (tests/golden/demo_depth.png)
SEED = 20261021
# tests/golden/make_reference_kernel_goldens.py's cameras
CAMERAS = {
    "tiny": dict(width=96, height=72, fx=88.0, fy=89.25, cx=47.6, cy=35.2),
    "small": dict(width=200, height=150, fx=180.0, fy=181.5, cx=101.3, cy=73.9),
}
PLANE = {"tiny": (80, 0.25, 0.15), "small": (70, 0.12, 0.08)}  # cm at the image centre, cm per column, cm per row
RUN_MAX_ITER = {"none": 30, "converge": 30, "cap": 1}
RUN_SIZES = {"none": 65, "converge": 200, "cap": 129}


def cam_of(name):
    c = CAMERAS[name]
    return tuple(float(F(c[k])) for k in ("fx", "fy", "cx", "cy"))


def run(op, cam_name, depth, **kw):
    c = CAMERAS[cam_name]
    fx, fy, cx, cy = cam_of(cam_name)
    return rh.run(dict(op=op, width=c["width"], height=c["height"], fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy),
                       depth=np.ascontiguousarray(depth, np.int32), **kw), program="ref_icp")


def equality_depth():
    """The smallest depth d (cm) for which a float s.z exists with fl(s.z - fl(d / 100)) == fl(0.1) exactly: the
    projective scene's `> max_dist_diff` and a `>=` differ on that point alone."""
    for d in range(5, 64):                              # not nearer: a point this near would pair with the origin queries
        z = F(d) / F(100.0)
        s = F(z + F(0.1))
        if F(s - z) == F(0.1):
            return d, s
    raise AssertionError("no depth gives |dz| == max_dist_diff exactly")


class Layout:
    """Where the scene's special pixels are, as fractions of the image (the same recipe for both cameras)."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.step = int(0.72 * W)                      # columns from here on lie 70 cm farther
        self.block = (int(0.30 * H), int(0.55 * H), int(0.12 * W), int(0.30 * W))  # rows, columns: 4 cm farther
        self.hole = (int(0.65 * H), int(0.65 * H) + 3, int(0.40 * W), int(0.40 * W) + 6)
        self.diff = {49: (int(0.12 * H), int(0.36 * W)), 50: (int(0.12 * H), int(0.50 * W)),
                     51: (int(0.12 * H) + 7, int(0.43 * W))}   # (row, column) of the centre; the neighbour is 5 to the right
        self.near = {1999: (int(0.80 * H), int(0.15 * W)), 2000: (int(0.80 * H), int(0.25 * W)),
                     2001: (int(0.80 * H), int(0.35 * W))}
        self.negative = (int(0.62 * H), int(0.10 * W))   # -7, with 30 cm five to the right and 40 cm five below
        self.above = (int(0.86 * H), int(0.55 * W))      # 70000
        self.equal = (int(0.22 * H), int(0.58 * W))      # the depth of equality_depth()
        self.centre = None


def scene_depth(cam_name):
    c = CAMERAS[cam_name]
    W, H = c["width"], c["height"]
    L = Layout(W, H)
    z0, sx, sy = PLANE[cam_name]
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    d = np.round(z0 + sx * (x - W // 2) + sy * (y - H // 2)).astype(np.int64)
    d[:, L.step:] += 70
    r0, r1, c0, c1 = L.block
    d[r0:r1, c0:c1] += 4
    r0, r1, c0, c1 = L.hole
    d[r0:r1, c0:c1] = 0
    rng = np.random.default_rng(SEED + W)
    for _ in range(6):                                  # lone holes
        d[rng.integers(8, H - 8), rng.integers(int(0.45 * W), L.step - 8)] = 0
    for k, (r, cc) in L.diff.items():
        d[r, cc + 5] = d[r, cc] + k
    for v, (r, cc) in L.near.items():              # with two neighbours inside the difference threshold
        d[r, cc], d[r, cc + 5], d[r + 5, cc] = v, v - 10, v - 15
    r, cc = L.negative
    d[r, cc], d[r, cc + 5], d[r + 5, cc] = -7, 30, 40
    d[L.above] = 70000
    d[L.equal] = equality_depth()[0]
    return d.astype(np.int32), L


def pixel_point(cam, c, r, z):
    fx, fy, cx, cy = cam
    return np.array([(c - cx) / fx * z, (r - cy) / fy * z, z], np.float64)


def rigid(rng, pts, deg, shift):
    a = np.deg2rad(rng.uniform(-deg, deg, 3))
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    c = pts.mean(0)
    return (pts - c) @ (Rz @ Ry @ Rx).T + c + rng.uniform(-shift, shift, 3)


def plane_pixels(depth, L, rng, n, margin=7):
    """n distinct pixels (column, row) of the near surface or the block, away from the borders."""
    W, H = L.W, L.H
    c, r = np.meshgrid(np.arange(margin, L.step - 2), np.arange(margin, H - margin))
    ok = (depth[r, c] > 50) & (depth[r, c] < 300)
    px = np.stack([c[ok], r[ok]], 1)
    return px[rng.permutation(len(px))[:n]]


def special_points(cam_name, depth, L, pcd):
    """name -> query points (float32) that the rows clouds of 63 points and more carry in front."""
    cam = cam_of(cam_name)
    W, H = L.W, L.H
    g = {}
    zc = float(pcd[H // 2, W // 2, 2])
    g["outside"] = [pixel_point(cam, -3.0, H / 2, zc), pixel_point(cam, W + 2.0, H / 2, zc),
                    pixel_point(cam, W / 2, -2.0, zc), pixel_point(cam, W / 2, H + 1.0, zc)]
    # the last column lies behind the step, the last row on the near surface: 2 mm in front of their pixels' points
    g["last"] = [pixel_point(cam, W - 1, H // 3, float(pcd[H // 3, W - 1, 2]) - 0.002),
                 pixel_point(cam, W // 3, H - 1, float(pcd[H - 1, W // 3, 2]) - 0.002),
                 pixel_point(cam, W - 1, H - 1, float(pcd[H - 1, W - 1, 2]) + 0.002)]
    # |s.z - d.z| one float below max_dist_diff, exactly on it, one float above: the rays through the equality pixel
    r, c = L.equal
    _, s_eq = equality_depth()
    g["max_dist"] = []
    for sz in (np.nextafter(s_eq, F(0)), s_eq, np.nextafter(s_eq, F(1))):
        p = pixel_point(cam, c, r, 1.0).astype(F)
        g["max_dist"].append(np.array([p[0] * sz, p[1] * sz, sz], F))
    # d2 below, on and above fl(r r) of the nearest-neighbour scene, next to the pixel nearest the principal point
    r0, c0 = int(round(cam[3])), int(round(cam[2]))
    L.centre = (r0, c0)
    g["radius"] = p2p_nn_cases.radius_points(pcd[r0, c0], fxm.NN_RADIUS)
    # the 70 cm step: a point 3 mm behind the near surface's last column that projects into the far surface's first
    def beside(r, c, columns, dz):
        """The scene point of pixel (r, c) moved by `columns` of that pixel's own pitch along x and by dz along z."""
        p = pcd[r, c].astype(np.float64)
        return p + (columns * p[2] / cam[0], 0, dz)

    rr = int(0.45 * H)
    g["step"] = [beside(rr, L.step - 1, 0.75, 0.003), beside(rr + 3, L.step, -0.2, -0.004)]
    # the 4 cm block: points next to one surface that project onto the other's pixels, on its left and right edges
    b0, b1, bc0, bc1 = L.block
    rb = (b0 + b1) // 2
    g["block"] = [beside(rb, bc0 - 1, 0.75, 0.002), beside(rb + 2, bc1, -0.75, 0.002), beside(rb - 2, bc0, -0.75, -0.002)]
    # a hole's "point" is the origin: a query within the radius of it, on the ray through the hole block's first pixel
    h0, _, hc0, _ = L.hole
    g["depth0"] = [pixel_point(cam, hc0, h0, 0.005)]
    g["tie"] = [tie_point(depth, L, pcd)]
    return {k: [np.asarray(p, np.float64).astype(F) for p in v] for k, v in g.items()}


def tie_point(depth, L, pcd):
    """A query exactly midway between the points of two neighbouring pixels of one row and one depth, 2 mm behind
    them: both squared distances are the same float.  (The midpoint has to be a float, and both differences exact.)"""
    for r in range(L.H // 2, L.H - 8):
        for c in range(L.W // 3, L.step - 3):
            if depth[r, c] != depth[r, c + 1] or not 50 < depth[r, c] < 300:
                continue
            a, b = pcd[r, c], pcd[r, c + 1]
            m = F((a[0] + b[0]) / F(2))
            if float(m) * 2 == float(a[0]) + float(b[0]) and F(m - a[0]) == F(b[0] - m) and a[1] == b[1]:
                return np.array([m, a[1], F(a[2] + F(0.002))], F)
    raise AssertionError("no exact tie in the scene")


def rows_clouds(cam_name, depth, L, pcd):
    rng = np.random.default_rng(SEED + 7 * L.W)
    sp = special_points(cam_name, depth, L, pcd)
    flat = [(k, p) for k, v in sp.items() for p in v]
    assert len(flat) < 63
    where = {}
    for i, (k, _) in enumerate(flat):
        where.setdefault(k, []).append(i)
    clouds = []
    for n in fxm.ROWS_SIZES:
        px = plane_pixels(depth, L, rng, n)
        pts = pcd[px[:, 1], px[:, 0]].astype(np.float64)
        # a rigid move of a few millimetres (half of the points stay within the nearest-neighbour radius), then a jitter
        pts = rigid(rng, pts, 0.25, 0.004) + rng.normal(0, 0.0004, pts.shape)
        far = rng.random(len(pts)) < 0.2                    # a fifth: beyond the radius, inside max_dist_diff
        pts[far, 2] += rng.uniform(0.012, 0.05, int(far.sum()))
        pts = pts.astype(F)
        if n >= 63:
            for i, (k, p) in enumerate(flat):
                if k != "tie" or n == max(fxm.ROWS_SIZES):   # the tie only once: the other clouds' measures stay comparable
                    pts[i] = p
        clouds.append(pts)
    return clouds, where


def run_clouds(cam_name, depth, L, pcd):
    rng = np.random.default_rng(SEED + 11 * L.W)
    out = {}
    for name in fxm.RUNS:
        px = plane_pixels(depth, L, rng, RUN_SIZES[name], margin=9)
        pts = pcd[px[:, 1], px[:, 0]].astype(np.float64)
        if name == "none":
            pts = pts + (0, 0, 0.5)
        elif name == "converge":
            pts = rigid(rng, pts, 0.2, 0.003) + rng.normal(0, 0.0003, pts.shape)
        else:
            pts = rigid(rng, pts, 0.5, 0.004) + rng.normal(0, 0.0003, pts.shape)
        out[name] = pts.astype(F)
    return out


def brute_nearest(pts, pcd, cam):
    """For every point: (d2 of the nearest scene point over the whole image, how many pixels attain it, the lowest such
    pixel index, the point's own pixel) in the spec's arithmetic (tests/p2p_nn_reference.py steps 1 to 4, no window)."""
    flat = pcd.reshape(-1, 3)
    cand = flat[:, 2] > 0
    best = np.zeros(len(pts), F)
    ties = np.zeros(len(pts), np.int64)
    win = np.zeros(len(pts), np.int64)
    for i, s in enumerate(pts):
        dx, dy, dz = s[0] - flat[:, 0], s[1] - flat[:, 1], s[2] - flat[:, 2]
        d2 = np.where(cand, (dx * dx + dy * dy) + dz * dz, F(np.inf))
        assert d2.dtype == F
        best[i] = d2.min()
        ties[i] = (d2 == best[i]).sum()
        win[i] = int(np.argmax(d2 == best[i]))
    okx, x = ref._pixel(pts[:, 0], pts[:, 2], cam[0], cam[2])
    oky, y = ref._pixel(pts[:, 1], pts[:, 2], cam[1], cam[3])
    assert okx.all() and oky.all()
    return best, ties, win, x, y


def match_pixels(points, normals, valid, pcd, nrm, what):
    """The pixel whose scene point and normal are the given ones, bit for bit (-1 where not valid)."""
    flat_p, flat_n = fxm.bits(pcd).reshape(-1, 3), fxm.bits(nrm).reshape(-1, 3)
    keys = {}
    for i, p in enumerate(flat_p):
        keys.setdefault(p.tobytes(), i)
    out = np.full(len(points), -1, np.int32)
    for i in range(len(points)):
        if not valid[i]:
            continue
        j = keys.get(fxm.bits(points[i]).tobytes())
        assert j is not None, (what, i, "the query returned a point that is no pixel's")
        assert np.array_equal(flat_n[j], fxm.bits(normals[i])), (what, i, "the normal is not that pixel's")
        out[i] = j
    return out


def fixture(cam_name):
    c = CAMERAS[cam_name]
    W, H = c["width"], c["height"]
    cam = cam_of(cam_name)
    depth, L = scene_depth(cam_name)
    out = dict(width=np.int32(W), height=np.int32(H), camera=np.array(cam, F), depth=depth,
               max_dist_diff=F(fxm.MAX_DIST_DIFF), nn_radius=F(fxm.NN_RADIUS))

    # ---- the scenes ----
    s = run(rh.OP_ICP_SCENE, cam_name, depth)
    pcd, nrm = s["proj_pcd"], s["proj_normal"]
    ppcd, pnrm = fxm.scene_np(depth, *cam)
    out["scene_pcd_x"], out["scene_normal_x"] = fxm.pack(pcd, ppcd), fxm.pack(nrm, pnrm)
    has = (fxm.bits(nrm) != 0).any(-1)
    # what the scene is there for, on the reference's own buffers
    assert not has[:5].any() and not has[:, :5].any() and not has[H - 6:].any() and not has[:, W - 6:].any()
    assert has[5, 5:W - 6].any() and has[H - 7, 5:W - 6].any() and has[5:H - 6, 5].any() and has[5:H - 6, W - 7].any()
    assert (depth[H - 6] > 0).all() and (depth[:, W - 6] > 0).all() and (depth[:5] > 0).all() and (depth[:, :5] > 0).all()
    for k, (r, cc) in L.diff.items():
        assert depth[r, cc + 5] - depth[r, cc] == k and has[r, cc]
    for v, (r, cc) in L.near.items():
        assert depth[r, cc] == v and has[r, cc] == (v < 2000)
    r, cc = L.negative
    assert depth[r, cc] < 0 and has[r, cc] and pcd[r, cc, 2] > 4e7     # saturated to 0 for the normal, uint32 for the point
    assert depth[L.above] > 65535 and pcd[L.above][2] == F(depth[L.above]) / F(100) and not has[L.above]
    assert (depth == 0).sum() >= 20 and (np.abs(np.diff(depth.astype(np.int64), axis=1)) > 50).any()
    # Scene_nn's cloud: the points of the image saturated to uint16, reordered by the tree.  They are the projective
    # scene's points (uint32 read) except where the two conversions differ: a negative pixel is no point of the tree,
    # a pixel above 65535 is a point at 655.35 m.
    sat = np.clip(depth.astype(np.int64), 0, 65535)
    assert len(s["nn_pcd"]) == (sat > 0).sum()
    tree = {p.tobytes() for p in fxm.bits(s["nn_pcd"])}
    same = np.array([[fxm.bits(pcd[r, c]).tobytes() in tree for c in range(W)] for r in range(H)])
    assert np.array_equal((sat > 0) != same, depth > 65535) and not same[depth < 0].any()
    assert (s["nn_pcd"][:, 2] == F(65535) / F(100)).sum() == (depth > 65535).sum() >= 1
    out["nn_count"], out["nn_nodes"] = np.int32(len(s["nn_pcd"])), np.int32(s["nn_nodes"][0])
    out["nn_not_shared"] = np.argwhere((depth < 0) | (depth > 65535)).astype(np.int32)  # (row, column)

    d2c = run(rh.OP_ICP_DEPTH2CLOUD, cam_name, depth)["cloud"]
    pred = fxm.depth2cloud_np(depth, *cam)
    assert len(d2c) == (depth > 0).sum() == len(pred)
    out["depth2cloud_x"] = fxm.pack(d2c, pred)

    # ---- rows ----
    clouds, where = rows_clouds(cam_name, depth, L, pcd)
    cloud = np.concatenate(clouds)
    assert (cloud[:, 2] > 0).all() and np.isfinite(cloud).all()
    out["rows_cloud"], out["rows_cnt"] = cloud, np.array([len(x) for x in clouds], np.int32)
    r = run(rh.OP_ICP_ROWS, cam_name, depth, cloud=cloud, max_dist_diff=F(fxm.MAX_DIST_DIFF))
    for sc in fxm.SCENES:
        ok = r[f"{sc}_valid"].astype(bool)
        pix = match_pixels(r[f"{sc}_dst_pcd"], r[f"{sc}_dst_normal"], ok, pcd, nrm, (cam_name, sc))
        out[f"{sc}_pixel"] = pix
        at = np.where(ok, pix, 0)
        out[f"{sc}_rows_x"] = fxm.pack(r[f"{sc}_rows"], fxm.row_formula(
            cloud, np.where(ok[:, None], pcd.reshape(-1, 3)[at], F(0)), np.where(ok[:, None], nrm.reshape(-1, 3)[at], F(0)), ok))
    pv, nv = r["proj_valid"].astype(bool), r["nn_valid"].astype(bool)
    big = int(np.cumsum(out["rows_cnt"])[-2])             # the cloud of 200: where its specials start
    idx = {k: [big + i for i in v] for k, v in where.items()}
    assert not pv[idx["outside"]].any() and pv[idx["last"]].all()
    lastpix = out["proj_pixel"][idx["last"]]
    assert lastpix[0] % W == W - 1 and lastpix[1] // W == H - 1 and lastpix[2] == W * H - 1
    assert list(pv[idx["max_dist"]]) == [True, True, False], pv[idx["max_dist"]]
    sz = cloud[idx["max_dist"], 2]
    assert F(sz[1] - pcd[L.equal][2]) == F(fxm.MAX_DIST_DIFF) and (out["proj_pixel"][idx["max_dist"][:2]] == L.equal[0] * W + L.equal[1]).all()
    assert list(nv[idx["radius"]]) == [False, True, False], nv[idx["radius"]]     # d2 == rr, below, above
    assert (out["nn_pixel"][idx["radius"][1]] == L.centre[0] * W + L.centre[1])
    both = pv & nv
    split = both & (out["proj_pixel"] != out["nn_pixel"])
    assert split[idx["block"]].sum() >= 2 and split.sum() >= 3, "the two scenes pair no point differently"
    assert (nv[idx["step"]] & ~pv[idx["step"]]).any(), "no point that only the nearest-neighbour scene pairs"
    assert (pv & ~nv).sum() >= 20 and nv.sum() >= 100, (pv.sum(), nv.sum())
    assert not nv[idx["depth0"]].any() and float(np.linalg.norm(cloud[idx["depth0"][0]])) < fxm.NN_RADIUS
    # max_iteration_ = 0 on every rows cloud: the measures of the first turn alone, in the reference's index order
    for sc in fxm.SCENES:
        for k in ("fitness", "rmse", "iteration"):
            out[f"rows_run0_{sc}_{k}"] = []
    for cl in clouds:
        g0 = run(rh.OP_ICP_RUN, cam_name, depth, cloud=cl, max_dist_diff=F(fxm.MAX_DIST_DIFF), rel_fitness=F(ref.REL_FITNESS),
                 rel_rmse=F(ref.REL_RMSE), max_iter=0)
        for sc in fxm.SCENES:
            for k in ("fitness", "rmse", "iteration"):
                out[f"rows_run0_{sc}_{k}"].append(g0[f"{sc}_{k}"][0])
    for sc in fxm.SCENES:
        for k in ("fitness", "rmse", "iteration"):
            out[f"rows_run0_{sc}_{k}"] = np.array(out[f"rows_run0_{sc}_{k}"])
    zero_normal = both & ~has.reshape(-1)[np.where(nv, out["nn_pixel"], 0)]
    out["rows_where"] = np.array([f"{k}:{','.join(str(i) for i in v)}" for k, v in idx.items()])

    # ---- the nearest neighbour of the whole image, by brute force in the spec's arithmetic ----
    best, ties, win, x, y = brute_nearest(cloud, pcd, cam)
    rr = F(F(fxm.NN_RADIUS) * F(fxm.NN_RADIUS))
    assert np.array_equal(best < rr, nv), "the tree accepts another set of points than the brute force"
    unique = ties == 1
    assert ties[idx["tie"][0]] == 2 and nv[idx["tie"][0]], "the tie query is no tie"
    off = np.stack([win % W - x, win // W - y], 1)
    out["nn_unique"] = unique
    out["nn_offset"] = np.where(nv[:, None], off, 0).astype(np.int16)
    out["nn_max_offset"] = np.int32(np.abs(off[nv]).max())
    share = unique[nv].mean()
    out["nn_unique_share"] = np.float64(share)
    assert share >= 0.95 and nv.sum() >= 100, (cam_name, share, nv.sum())
    assert (out["nn_pixel"][nv & unique] == win[nv & unique]).all(), "the tree's answer is not the unique nearest point"
    assert out["nn_max_offset"] <= nn.WINDOW

    # ---- full runs ----
    rc = run_clouds(cam_name, depth, L, pcd)
    devs, same_it = [], []
    for name in fxm.RUNS:
        pts = rc[name]
        out[f"run_{name}_cloud"] = pts
        out[f"run_{name}_max_iter"] = np.int32(RUN_MAX_ITER[name])
        g = run(rh.OP_ICP_RUN, cam_name, depth, cloud=pts, max_dist_diff=F(fxm.MAX_DIST_DIFF), rel_fitness=F(ref.REL_FITNESS),
                rel_rmse=F(ref.REL_RMSE), max_iter=RUN_MAX_ITER[name])
        for sc in fxm.SCENES:
            for k in ("T", "fitness", "rmse", "iteration", "exit", "moved", "solver_A", "solver_b", "solver_T"):
                out[f"run_{name}_{sc}_{k}"] = g[f"{sc}_{k}"]
            it, ex = int(g[f"{sc}_iteration"][0]), int(g[f"{sc}_exit"][0])
            assert len(g[f"{sc}_solver_A"]) == it
            if name == "none":
                assert (it, ex) == (0, 0) and g[f"{sc}_fitness"][0] == 0
            elif name == "converge":
                assert ex == 1 and 2 <= it < 30, (cam_name, sc, it, ex)
            else:
                assert ex == 2 and it == RUN_MAX_ITER[name], (cam_name, sc, it, ex)
            kw = dict(max_iterations=RUN_MAX_ITER[name])
            if sc == "proj":
                a = ref.icp(pts, pcd, nrm, *cam, order="index", trig="libm", **kw)
                b = ref.icp(pts, pcd, nrm, *cam, order="wave", trig="spec", **kw)
            else:
                a = nn.icp(pts, pcd, nrm, *cam, order="index", trig="libm", **kw)
                b = nn.icp(pts, pcd, nrm, *cam, order="wave", trig="spec", **kw)
            dev = [np.abs(a[0].astype(np.float64) - b[0].astype(np.float64)).max(), abs(float(a[1]) - float(b[1])),
                   abs(float(a[2]) - float(b[2]))]
            devs.append(dev)
            same_it.append(a[3] == b[3])
            assert a[3] == b[3], (cam_name, name, sc, "the two evaluations return at different iterations", a[3], b[3])
    out["order_trig_dev"] = np.array(devs, np.float64).reshape(len(fxm.RUNS), len(fxm.SCENES), 3)
    out["order_trig_max_dev"] = out["order_trig_dev"].max((0, 1))
    out["order_trig_same_iteration"] = np.array(same_it).reshape(len(fxm.RUNS), len(fxm.SCENES))

    # ---- the packing is lossless ----
    back = fxm.unpacked(out)
    for got, want in ((back["scene_pcd"], pcd), (back["scene_normal"], nrm), (back["depth2cloud"], d2c),
                      (back["proj_rows"], r["proj_rows"]), (back["nn_rows"], r["nn_rows"]),
                      (back["nn_dst_pcd"], r["nn_dst_pcd"]), (back["proj_dst_normal"], r["proj_dst_normal"])):
        assert np.array_equal(fxm.bits(got), fxm.bits(want))
    assert np.array_equal(back["proj_valid"], pv) and np.array_equal(back["nn_valid"], nv)
    print(f"{cam_name}: accepted proj {pv.sum()} nn {nv.sum()} of {len(cloud)}; unique-nearest share {share:.4f}; "
          f"nn_max_offset {int(out['nn_max_offset'])}; zero-normal pairs {int(zero_normal.sum())}; order_trig_max_dev "
          f"{out['order_trig_max_dev']}; iterations "
          f"{[[int(out[f'run_{n}_{sc}_iteration'][0]) for sc in fxm.SCENES] for n in fxm.RUNS]}")
    return out


def packed(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def main():
    import oracle
    oracle.build_ref()
    for cam_name in CAMERAS:
        blob = packed(fixture(cam_name))
        assert len(blob) <= MAX_BYTES, f"refk_icp_{cam_name}: {len(blob)} bytes > {MAX_BYTES}"
        with open(os.path.join(HERE, f"refk_icp_{cam_name}.npz"), "wb") as f:
            f.write(blob)
        print(f"refk_icp_{cam_name}.npz  {len(blob)} bytes")


if __name__ == "__main__":
    main()
