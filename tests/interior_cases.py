"""Cases for the fused raster's pose classes (pose_window and raster_phase in perception_amd/csrc/pcore_fused.hip):
  2  interior  fastdiv, and the proven box of every computed screen coordinate lies inside the image: no clamp of the
               vertices to the image, the area reciprocal without the division's scaling steps
  1  fastdiv   every vertex at least 1 cm in front of the camera plane: the unscaled divisions
  0  general   everything else

A 72 x 48 camera (the width a multiple of both strides, as evaluate requires) at strides 8 and 3 and one hand-made mesh of about 200 triangles on a 0.12 m x 0.09 m sheet (24 x 17
pixels at the sweeps' depth of 0.75 m): sub-pixel triangles, triangles with vertices on whole pixels (edges and
vertices on sample centres), zero-area triangles whose three vertices coincide (X = 0 at every sample: NaN
barycentrics, inside) and with a repeated vertex (Y = 0, X != 0 off the edge's line: infinite barycentrics, outside),
larger triangles over them all, and the two corners of the sheet's box as vertices.

Poses (identity rotation; given as the float32 rows the kernels read, so that the certificates can restate the vertex
pass bit for bit).  For each of the four borders the sheet moves outward across it:
  inside       the box and its margin inside the image                                     class 2
  margin       the box inside the image, its margin (2 pixels and a little) across         class 1
  exact        the box's extreme vertex exactly on the border pixel (0, W-1; 0, H-1)       class 1
  beyond       that vertex one float step beyond the border pixel                          class 1
  astride      the box a third across the border                                           class 1
  near         further out and 1.2 cm from the camera plane (the nearest vertices 0.9 cm)   class 0
and two rolled poses in the middle of the image (class 2).
tests/test_interior_cases.py certifies the classes on a float32 restatement of pose_window;
tests/test_gpu_interior_pose.py runs the cases bit for bit against the oracle."""
from __future__ import annotations

import functools

import numpy as np

from perception_amd.model import compute_proj
from tests import mesh_cases as mc

F32 = np.float32
CAM = dict(mc.CAM, width=72, height=48)  # mesh_cases' intrinsics (MeshCase reads them from there)
STRIDES = (8, 3)
Z0 = 0.75                     # metres: the depth of the sweeps
SHEET = (0.12, 0.09)          # metres: the model's box is [0, SHEET] x [-Z_AMP, Z_AMP]
Z_AMP = 0.003
PIX = (Z0 / CAM["fx"], Z0 / CAM["fy"])  # metres per pixel at Z0
BORDERS = ("left", "right", "bottom", "top")   # of the screen coordinates: sx = 0, sx = W-1, sy = 0, sy = H-1
KINDS = ("inside", "margin", "exact", "beyond", "astride", "near")
EXPECTED_CLASS = dict(inside=2, margin=1, exact=1, beyond=1, astride=1, near=0, rolled=2)


def _tri(a, b, c):
    return np.array([a, b, c], np.float64).reshape(9)


@functools.lru_cache(maxsize=None)
def mesh():
    """(T, 9) float32, metres."""
    rng = np.random.default_rng(29)
    sx, sy = SHEET
    px, py = PIX
    t = []
    # the box's corners as vertices of two thin triangles along the diagonal (the extreme vertices of every sweep)
    t.append(_tri((0, 0, -Z_AMP), (px * 3, 0, 0), (0, py * 3, Z_AMP)))
    t.append(_tri((sx, sy, Z_AMP), (sx - px * 3, sy, 0), (sx, sy - py * 3, -Z_AMP)))
    # sub-pixel triangles: 0.2 to 0.9 pixels across
    for _ in range(70):
        c = np.array([rng.random() * (sx - px), rng.random() * (sy - py), (rng.random() * 2 - 1) * Z_AMP])
        d = (rng.random((3, 3)) * 0.7 + 0.2) * np.array([px, py, 0.0005])
        t.append(_tri(c, c + d[0] * (1, 0, 1), c + d[1] * (0, 1, 1)))
    # vertices at whole pixels from the box's corner, at depth Z0: where the `inside` poses put that corner on a whole
    # pixel, vertices and edges go through sample centres
    for _ in range(40):
        i, j = int(rng.integers(0, 20)), int(rng.integers(0, 14))
        w, h = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        t.append(_tri((i * px, j * py, 0), ((i + w) * px, j * py, 0), (i * px, (j + h) * py, 0)))
    # zero area, the three vertices coincide: X = 0 and Y = 0
    for _ in range(12):
        p = (int(rng.integers(0, 24)) * px, int(rng.integers(0, 17)) * py, (rng.random() * 2 - 1) * Z_AMP)
        t.append(_tri(p, p, p))
    # zero area, a repeated vertex and a third one some pixels away: Y = 0, X != 0 off the line
    for k in range(24):
        a = np.array([rng.random() * sx * 0.7, rng.random() * sy * 0.7, (rng.random() * 2 - 1) * Z_AMP])
        c = a + np.array([(rng.random() * 6 + 1) * px, (rng.random() * 5 + 1) * py, 0.001])
        t.append(_tri(a, a, c) if k % 3 == 0 else _tri(a, c, a) if k % 3 == 1 else _tri(c, a, a))
    # larger triangles (2 to 10 pixels) behind and in front of the rest
    for _ in range(60):
        c = np.array([rng.random() * sx * 0.6, rng.random() * sy * 0.6, (rng.random() * 2 - 1) * Z_AMP])
        w, h = (rng.random(2) * 8 + 2) * np.array([px, py])
        w, h = min(w, sx - c[0]), min(h, sy - c[1])
        z = (rng.random(2) * 2 - 1) * Z_AMP
        t.append(_tri(c, (c[0] + w, c[1], z[0]), (c[0], c[1] + h, z[1])))
    # every vertex inside the sheet's box, whose corners the first two triangles hold
    t = np.clip(np.asarray(t, np.float64).reshape(-1, 3), (0, 0, -Z_AMP), (sx, sy, Z_AMP)).reshape(-1, 9).astype(F32)
    order = np.r_[0, 1, 2 + rng.permutation(len(t) - 2)]
    return mc._frozen(t[order])


def proj(cam=None):
    cam = cam or CAM
    return compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"])


def vertex_pass(pose16, v, cam=None):
    """(sx, sy, lz) float32 of vertices v (n, 3) float32 under the pose rows pose16 (float32[16]): the fused kernel's
    vertex pass of a fastdiv pose restated operation by operation in float32 (row4, the sparse projection, the IEEE
    quotients, q * (W/2) + W/2), for the camera `cam` (this module's by default)."""
    cam = cam or CAM
    m = np.asarray(pose16, F32)
    p = proj(cam)
    x, y, z = (np.asarray(v[:, k], F32) for k in range(3))
    row = lambda r: m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3]
    lx, ly, lz = row(0), row(1), row(2)
    pxx = p[0] * lx + p[2] * lz
    pyy = p[5] * ly + p[6] * lz
    hw, hh = F32(cam["width"]) / F32(2), F32(cam["height"]) / F32(2)
    return (pxx / lz) * hw + hw, (pyy / lz) * hh + hh, lz


def pose_box(pose16, tris, cam=None):
    """pose_window's box restated in float32: (xlo, xhi, ylo, yhi, sx0, sx1, sy0, sy1, fastdiv) -- the corners'
    screen box, widened by the margin, and the fastdiv flag -- or None where the window is the whole image."""
    f = F32
    cam = cam or CAM
    m = np.asarray(pose16, F32)
    p = proj(cam)
    v = np.asarray(tris, F32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ax, ay, az = (np.maximum(np.abs(lo[k]), np.abs(hi[k])) for k in range(3))
    B = [np.abs(m[4 * r]) * ax + np.abs(m[4 * r + 1]) * ay + np.abs(m[4 * r + 2]) * az + np.abs(m[4 * r + 3])
         for r in range(3)]
    cor = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)], F32)
    x, y, z = cor[:, 0], cor[:, 1], cor[:, 2]
    row = lambda r: m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3]
    lx, ly, lz = row(0), row(1), row(2)
    pxx = p[0] * lx + p[1] * ly + p[2] * lz + p[3]
    pyy = p[4] * lx + p[5] * ly + p[6] * lz + p[7]
    Wf, Hf = f(cam["width"]), f(cam["height"])
    sx = pxx / lz * Wf / f(2) + Wf / f(2)
    sy = pyy / lz * Hf / f(2) + Hf / f(2)
    if not ((np.abs(sx) < 1e7).all() and (np.abs(sy) < 1e7).all() and (lz > 0).all()):
        return None
    lzmin = lz.min()
    if not lzmin > f(0.05) * B[2]:
        return None
    eps = f(5.9604645e-8)
    Pbx = np.abs(p[0]) * B[0] + np.abs(p[1]) * B[1] + np.abs(p[2]) * B[2] + np.abs(p[3])
    Pby = np.abs(p[4]) * B[0] + np.abs(p[5]) * B[1] + np.abs(p[6]) * B[2] + np.abs(p[7])
    mgx = f(2) + f(256) * eps * (f(0.5) * Wf) * Pbx / lzmin + f(8) * eps * (max(abs(sx.min()), abs(sx.max())) + Wf)
    mgy = f(2) + f(256) * eps * (f(0.5) * Hf) * Pby / lzmin + f(8) * eps * (max(abs(sy.min()), abs(sy.max())) + Hf)
    fastdiv = bool(lzmin - f(1.0e-5) * B[2] >= 1 and B[2] < 2.0 ** 40 and Pbx < 2.0 ** 40 and Pby < 2.0 ** 40)
    return (sx.min() - mgx, sx.max() + mgx, sy.min() - mgy, sy.max() + mgy, sx.min(), sx.max(), sy.min(), sy.max(),
            fastdiv)


def pose_class(pose16, tris, cam=None):
    """0 / 1 / 2 as fused_pose picks the raster's copy."""
    cam = cam or CAM
    b = pose_box(pose16, tris, cam)
    if b is None or not b[8]:
        return 0
    W, H = cam["width"], cam["height"]
    return 2 if (b[0] >= 0 and b[1] <= W - 1 and b[2] >= 0 and b[3] <= H - 1) else 1


def _rows(R, t_cm):
    m = np.zeros(16, F32)
    m[:12] = np.c_[np.asarray(R, np.float64) * 100.0, np.asarray(t_cm, np.float64)].astype(F32).reshape(-1)
    m[15] = 1
    return m


def _translation_for(u, v, z_cm=Z0 * 100):
    """The translation (cm) under which the model's origin shows at screen (u, v), in double."""
    W, H = CAM["width"], CAM["height"]
    p = proj().astype(np.float64)
    x = ((u - W / 2) / (W / 2) - p[2]) * z_cm / p[0]
    y = ((v - H / 2) / (H / 2) - p[6]) * z_cm / p[5]
    return np.array([x, y, z_cm])


def _neighbours(x, n):
    """The 2 n + 1 consecutive float32 values around x."""
    i = int(np.array([x], F32).view(np.int32)[0])
    return (np.arange(-n, n + 1, dtype=np.int64) + i).astype(np.int32).view(F32)


def _coord(m, vertex, axis, mk):
    """vertex_pass's screen coordinate `axis` of one vertex with the translation component of that axis replaced by
    the float32 array mk."""
    p = proj()
    x, y, z = (F32(c) for c in vertex)
    r = axis
    l = m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + np.asarray(mk, F32)
    lz = m[8] * x + m[9] * y + m[10] * z + m[11]
    num = (p[0] * l + p[2] * lz) if axis == 0 else (p[5] * l + p[6] * lz)
    h = F32(CAM["width"] if axis == 0 else CAM["height"]) / F32(2)
    return (num / lz) * h + h


def _exact(t_cm, axis, vertex, target):
    """Pose rows near translation t_cm (float32 neighbours of its `axis` and z components) under which the vertex pass
    puts `vertex` on screen coordinate `target` exactly."""
    m = _rows(np.eye(3), t_cm)
    k = 3 + 4 * axis
    # the translation that puts this vertex (not the model's origin) there, in double
    pj = proj().astype(np.float64)
    size = CAM["width"] if axis == 0 else CAM["height"]
    lz = 100.0 * float(F32(vertex[2])) + float(m[11])
    ndc = (target - size / 2) / (size / 2)
    m[k] = F32((ndc - pj[2 if axis == 0 else 6]) * lz / pj[0 if axis == 0 else 5] - 100.0 * float(F32(vertex[axis])))
    cand = _neighbours(m[k], 40)
    for mz in _neighbours(m[11], 40):
        m2 = m.copy()
        m2[11] = mz
        hit = np.nonzero(_coord(m2, vertex, axis, cand) == F32(target))[0]
        if len(hit):
            m2[k] = cand[hit[len(hit) // 2]]
            return m2
    raise AssertionError("no pose puts the vertex on the border exactly")


def _beyond(m, axis, vertex, target, sgn):
    """From the pose of _exact: the first float32 step of the translation that moves the vertex past the border."""
    k = 3 + 4 * axis
    cand = _neighbours(m[k], 200)
    c = _coord(m, vertex, axis, cand)
    past = np.nonzero(c > target if sgn > 0 else c < target)[0]
    mid = 200
    j = past[np.argmin(np.abs(past - mid))]
    out = m.copy()
    out[k] = cand[j]
    return out


@functools.lru_cache(maxsize=None)
def poses():
    """(poses (n, 16) float32, kinds: a list of (border or None, kind))."""
    W, H = CAM["width"], CAM["height"]
    tris = mesh()
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    bw, bh = (hi[0] - lo[0]) / PIX[0], (hi[1] - lo[1]) / PIX[1]  # the box in pixels: sx grows with x, sy falls with y
    out, kinds = [], []
    # the origin's screen position with the box centred, on a whole pixel
    mid_u, mid_v = float(round((W - 1 - bw) / 2)), float(round((H - 1 + bh) / 2))
    for border in BORDERS:
        # `ext`: the model vertex that leads across the border; `at(d)`: the origin's screen position that puts the
        # leading side of the box d pixels inside the border (d < 0: beyond)
        if border == "left":
            ext, axis, tgt, sgn = (0.0, 0.0, -Z_AMP), 0, 0.0, -1
            at = lambda d: (d, mid_v)
        elif border == "right":
            ext, axis, tgt, sgn = (hi[0], hi[1], Z_AMP), 0, float(W - 1), +1
            at = lambda d: (W - 1 - d - bw, mid_v)
        elif border == "bottom":  # sy = 0: the box's largest y
            ext, axis, tgt, sgn = (hi[0], hi[1], Z_AMP), 1, 0.0, -1
            at = lambda d: (mid_u, d + bh)
        else:                     # sy = H-1: the box's smallest y
            ext, axis, tgt, sgn = (0.0, 0.0, -Z_AMP), 1, float(H - 1), +1
            at = lambda d: (mid_u, H - 1 - d)
        for kind in KINDS:
            if kind == "inside":
                m = _rows(np.eye(3), _translation_for(*(round(c) for c in at(3.5))))
            elif kind == "margin":
                m = _rows(np.eye(3), _translation_for(*at(1.25)))
            elif kind == "exact":
                m = _exact(_translation_for(*at(0.0)), axis, ext, tgt)
            elif kind == "beyond":
                m = _beyond(_exact(_translation_for(*at(0.0)), axis, ext, tgt), axis, ext, tgt, sgn)
            elif kind == "astride":
                m = _rows(np.eye(3), _translation_for(*at(-(bw if axis == 0 else bh) / 3)))
            else:  # near: the same ray further out, 1.2 cm from the camera plane (the sheet spans the whole image)
                u, w_ = at(-6.0)
                m = _rows(np.eye(3), _translation_for(u, w_, z_cm=1.2))
            out.append(m)
            kinds.append((border, kind))
    for a in (0.4, -1.2):  # rolled about the box's centre, in the middle of the image
        R = mc._rz(a)
        c = np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.0])
        t = _translation_for((W - 1) / 2, (H - 1) / 2) - (R @ c) * 100.0
        out.append(_rows(R, t))
        kinds.append((None, "rolled"))
    p = np.ascontiguousarray(np.stack(out), F32)
    p.setflags(write=False)
    return p, kinds


@functools.lru_cache(maxsize=None)
def bank():
    return mc.Bank("interior", [("sheet", mesh(), None)])


class InteriorCase(mc.MeshCase):
    """mesh_cases.MeshCase (the oracle's renders, clouds, observation and costs, each computed once) over this mesh,
    camera and poses."""

    def __init__(self):
        self.name = "interior"
        self.bank = bank()
        self.cam = CAM
        self.width, self.height = CAM["width"], CAM["height"]
        self.proj = proj()
        self.poses, self.kinds = poses()
        self.poses44 = None
        self.n = len(self.poses)
        self.pose_model = np.zeros(self.n, np.int32)
        self.pose_label = self.pose_model.copy()
        self.pose_kind = np.arange(self.n) % 3  # the observation's block pattern (MeshCase.observation)
        self.src_depth = np.zeros((self.height, self.width), np.int32)
        self.mask = np.zeros((self.height, self.width), np.uint8)
        self.r = mc.R
        self.oracle_count = np.concatenate([self.bank.tris_model_count, [0]]).astype(np.int32)

    def describe(self, pose):
        b, k = self.kinds[pose]
        return f"pose {pose} ({k}{'' if b is None else ' at the ' + b + ' border'})"


@functools.lru_cache(maxsize=None)
def case():
    return InteriorCase()
