"""Hand-made scenes and slots for the nearest-neighbour scene's tests (tests/test_p2p_nn_spec.py certifies on the CPU
that every adversarial group below changes a result under the matching wrong rule; tests/test_gpu_p2p_nn.py holds the
kernel to the restatement on the same slots).

The 40 x 30 "dyadic" scene: fx = fy = 32, cx = 20, cy = 15 and a plane at 50 cm, so that a scene point is
((c - 20) / 64, (q - 15) / 64, 0.5) exactly and distances between points on the pixel grid are exact -- ties are ties
in float32.  Columns 30 .. 39 lie at 100 cm (a depth edge).  The normals are caller-made (the debug hook takes any):
a different unit vector per pixel, so that every change of a correspondence changes the row; some are zero.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle

F = np.float32
W, H = 40, 30
CAM = (32.0, 32.0, 20.0, 15.0)
G = 1.0 / 64.0  # the grid's pitch on the near plane, metres
SLOT_SIZES = (0, 1, 63, 64, 65, 128, 129)
WINDOWS = (0, 1, 4, 32, 128)
RADII = (0.01, 0.03, 0.1)
# pixels without a scene point
HOLE_TIE4 = (12, 20)                                       # the centre of the four-way tie
HOLE_BLOCK = [(c, q) for c in (9, 10, 11) for q in (7, 8, 9)]  # depth-0 holes around a centre
ZERO_NORMALS = [(c, q) for c in range(22, 26) for q in range(18, 22)]


def P(c, q, z=0.5):
    """The dyadic scene's point of pixel (c, q) at depth z."""
    return np.array([(c - 20) / 32.0 * z, (q - 15) / 32.0 * z, z])


@functools.lru_cache(maxsize=None)
def dyadic_scene():
    d = np.full((H, W), 50, np.int32)
    d[:, 30:] = 100
    d[HOLE_TIE4[1], HOLE_TIE4[0]] = 0
    for c, q in HOLE_BLOCK:
        d[q, c] = 0
    d[7, 13] = 56                                          # a lone pixel 6 cm behind the plane, next to the hole block
    pcd, _ = oracle.ref_scene(d, *CAM)
    assert np.array_equal(pcd[15, 20], F((0, 0, 0.5))) and np.array_equal(pcd[3, 7], P(7, 3).astype(F))
    rng = np.random.default_rng(12)
    nrm = rng.normal(size=(H, W, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    for c, q in ZERO_NORMALS:
        nrm[q, c] = 0
    return d, pcd, nrm


def radius_points(P0, r):
    """Three queries next to the scene point P0 (float32; s.y = P0.y, so dy = 0) whose float32 d2 to it is fl(r r),
    the float below and the float above: dz is 0.999 r, and s.x walks float by float until the sum lands on the
    target.  P0.x has to be small enough for s.x's spacing to reach every float of d2 (asserted)."""
    P0 = np.asarray(P0, F)
    r = F(r)
    rr = F(r * r)
    sz = F(P0[2] + F(0.9999) * r)
    dz = F(sz - P0[2])
    dz2 = F(dz * dz)
    out = []
    for target in (rr, np.nextafter(rr, F(0)), np.nextafter(rr, F(1))):
        sx = F(P0[0] + F(np.sqrt(float(target) - float(dz2))))
        for _ in range(20000):
            dx = F(sx - P0[0])
            d2 = F(F(dx * dx) + dz2)                       # (dx dx + 0 0) + dz dz
            if d2 == target:
                break
            sx = np.nextafter(sx, F(np.inf) if d2 < target else F(-np.inf))
        assert d2 == target, (P0, r, d2, target)
        out.append((sx, P0[1], sz))
    return out


def special_points(r):
    """name -> list of query points of the dyadic scene (float64 / float32 rows of 3)."""
    g = {}
    g["radius"] = radius_points((0, 0, 0.5), r)            # pixel (20, 15)
    g["tie2"] = [tuple(P(5.5, 10)), tuple(P(33, 4.5, 1.0) * 1.0)]      # midway between two pixels: columns, rows
    g["tie4"] = [tuple(P(*HOLE_TIE4)), tuple(P(16.5, 24.5))]          # a hole's four neighbours; a pixel corner
    # the depth edge: the point projects into column 30 (the far surface) and lies next to column 29's point
    g["edge"] = [tuple(P(29, 12) + (0.0100, 0, 0.004)), tuple(P(29, 20) + (0.0062, 0, 0.002))]
    # around the hole block: the lone pixel (13, 7) at 56 cm is the nearest of the window at w = 1 .. 2 for a query at
    # (12, 7.4) lifted toward it, while beyond the window nothing is nearer; at the block's centre w = 1 holds holes only
    g["holes"] = [tuple(P(10, 8)), tuple(P(10, 8) + (0.001, -0.002, 0.003))]
    g["beyond_window"] = [tuple(P(10.2, 8) + (0, 0, 0.004))]  # nearest: column 8 or 12, two pixels away
    g["zero_normal"] = [tuple(P(23, 19) + (0.002, 0.001, 0.003)), tuple(P(24.4, 20.3) + (0, 0, -0.002))]
    # windows clipped at the four corners, centres inside and up to five pixels outside the image
    g["corners"] = [tuple(P(c, q) + (0, 0, 0.002)) for c, q in ((0.2, 0.3), (38.8, 0.1), (0.4, 28.9), (-3, -2),
                                                                  (-5, 10), (10, -5), (20, 33.2))] + \
                   [tuple(P(c, q, 1.0) + (0, 0, 0.002)) for c, q in ((39.3, 29.2), (42, 31), (44.4, 12), (39, -3))]
    # a depth-0 pixel's "point" is the origin: a query within r of it that projects onto the hole (12, 20) itself, and
    # one that projects outside the image with the holes inside its window at w >= 32
    g["depth0"] = [(-0.00125, 0.00078125, 0.005), (0.003, 0.002, 0.004)]
    g["not_a_query"] = [(np.nan, 0, 0.5), (0, np.nan, 0.5), (0, 0, np.nan), (np.inf, 0, 0.5), (0, -np.inf, 0.5),
                        (0, 0, np.inf), (0.01, 0.01, -0.5), (0.01, 0.01, 0.0), (0.01, 0.01, -0.0), (1e30, 0, 1e-30),
                        (0, -1e30, 1e-30), (6.7e7, 0, 1.0), (-6.7e7, 6.7e7, 1.0), (7e7, 0, 1.0), (300.0, 0, 0.5),
                        (0, -300.0, 0.5)]
    return {k: [np.array(p, np.float64).astype(F) for p in v] for k, v in g.items()}


@functools.lru_cache(maxsize=None)
def dyadic_slots(r):
    """The clouds of SLOT_SIZES for radius r: near-plane pixels' points moved by a small rigid transform (a fraction
    of r), with every special point written over the first entries of the clouds of 63 points and more.
    -> dict(clouds, xyzw (S, cap, 4), cnt, pcd, nrm, pcd4, nrm4, cam, where: name -> indices into a large cloud)."""
    _, pcd, nrm = dyadic_scene()
    rng = np.random.default_rng(int(round(r * 1000)))
    sp = special_points(r)
    flat = [(k, p) for k, v in sp.items() for p in v]
    assert len(flat) < 63
    where = {}
    for i, (k, _) in enumerate(flat):
        where.setdefault(k, []).append(i)
    px = np.stack(np.meshgrid(np.arange(1, 29), np.arange(1, 29)), -1).reshape(-1, 2)
    clouds = []
    for n in SLOT_SIZES:
        sel = px[rng.permutation(len(px))[:n]]
        pts = pcd[sel[:, 1], sel[:, 0]].astype(np.float64)
        pts = pts[pts[:, 2] > 0]
        while len(pts) < n:                                # holes drawn: fill up with the first point's pixel mates
            pts = np.concatenate([pts, pts[:n - len(pts)] + (G, 0, 0)])
        a = np.deg2rad(rng.uniform(-0.4, 0.4, 3)) * (r / 0.03)
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        c = pts.mean(0) if n else np.zeros(3)
        pts = ((pts - c) @ (Rz @ Ry @ Rx).T + c + rng.uniform(-0.2, 0.2, 3) * r).astype(F).reshape(-1, 3)
        if n >= 63:
            for i, (_, p) in enumerate(flat):
                pts[i] = p
        clouds.append(pts)
    cap = max(SLOT_SIZES) + 3
    xyzw = np.full((len(clouds), cap, 4), np.nan, F)       # past a slot's count: never read
    for i, c in enumerate(clouds):
        xyzw[i, :len(c), :3] = c
        xyzw[i, :len(c), 3] = 1.0
    cnt = np.array([len(c) for c in clouds], np.int32)
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:2] + (1,), F)], -1)
    return dict(clouds=clouds, xyzw=xyzw, cnt=cnt, pcd=pcd, nrm=nrm, pcd4=pad(pcd), nrm4=pad(nrm), cam=CAM, where=where)


# the 96 x 72 scene of an ordinary camera: a tilted plane with a 12 cm step, holes, and the projective scene's normals
TINY_CAM = (88.0, 89.25, float(F(47.6)), float(F(35.2)))
TINY_SIZES = (1, 64, 129, 301)


@functools.lru_cache(maxsize=None)
def tiny_slots():
    Wt, Ht = 96, 72
    rng = np.random.default_rng(21)
    x, y = np.meshgrid(np.arange(Wt), np.arange(Ht))
    d = np.round(80 + 0.25 * (x - 48) + 0.15 * (y - 36)).astype(np.int32)
    d[:, 62:] += 12
    d[rng.random((Ht, Wt)) < 0.06] = 0
    d[30:34, 20:27] = 0
    pcd, nrm = oracle.ref_scene(d, *TINY_CAM)
    clouds = []
    for n in TINY_SIZES:
        px = np.stack(np.meshgrid(np.arange(6, 90, 2), np.arange(6, 64, 2)), -1).reshape(-1, 2)
        px = px[rng.permutation(len(px))[:n]]
        pts = pcd[px[:, 1], px[:, 0]].astype(np.float64)
        pts[pts[:, 2] == 0] = pcd[40, 50]
        a = np.deg2rad(rng.uniform(-1.0, 1.0, 3))
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        c = pts.mean(0)
        pts = ((pts - c) @ (Rz @ Ry @ Rx).T + c + rng.uniform(-0.005, 0.005, 3)).astype(F)
        if n >= 64:
            pts[3] = (0.1, 0.05, -0.8)
            pts[7] = (np.nan, 0.0, 0.8)
            pts[11] = (3.0, 0.0, 0.8)                      # far right of the image
            pts[12] = pcd[30, 61] + F((0.004, 0.0, 0.01))  # at the step
            pts[13] = pcd[2, 50] + F((0.0, -0.03, 0.0))    # above the first row
            pts[14] = pcd[32, 23 + 40] * F(1.0)            # on the far side of the step
            pts[15] = (1e30, 0.0, 1e-30)
        clouds.append(pts)
    cap = max(TINY_SIZES) + 3
    xyzw = np.full((len(clouds), cap, 4), np.nan, F)
    for i, c in enumerate(clouds):
        xyzw[i, :len(c), :3] = c
        xyzw[i, :len(c), 3] = 1.0
    cnt = np.array([len(c) for c in clouds], np.int32)
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:2] + (1,), F)], -1)
    return dict(clouds=clouds, xyzw=xyzw, cnt=cnt, pcd=pcd, nrm=nrm, pcd4=pad(pcd), nrm4=pad(nrm), cam=TINY_CAM)
