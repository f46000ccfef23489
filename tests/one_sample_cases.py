"""Cases for the triangle stage's one-sample fast path (raster_phase in perception_amd/csrc/pcore_fused.hip): a step
whose non-empty sample windows are all exactly one sample queues them at once; a step with any other non-empty lane
(a larger window, a NaN-vertex triangle) takes the general code for all its lanes.

A mesh of isolated right triangles whose bounding boxes, laid out in pixels of the face-on pose, come in sizes from a
pixel and a half to most of the image, on a small camera: at stride 8 and at stride 3 the steps hold empty windows,
one-sample windows, windows of 2, 3 and 4 samples in a row, in a column and as 2 x 2, windows of more than 4 samples
(the cooperative path) and padding slots side by side.  Three models share it:
  whole   the mesh and four tiny triangles beyond the image's corners: the pose window is the whole sampled image,
          so its chunks under a 64-sample tile are known on the CPU (tests/test_one_sample_cases.py)
  nan     `whole` and triangles with a NaN vertex: every pose takes the non-fastdiv copy of the raster
  tight   the mesh alone: pose windows with an offset
tests/test_one_sample_cases.py certifies on the CPU that every class occurs and shares steps;
tests/test_gpu_one_sample_path.py runs the cases bit for bit against the oracle."""
from __future__ import annotations

import functools

import numpy as np

from perception_amd.model import compute_proj, init_from_eigen_batch
from tests import mesh_cases as mc

F32 = np.float32
# mesh_cases' intrinsics (MeshCase reads them from there) on an image whose width is a multiple of both strides
CAM = dict(mc.CAM, width=168)
STRIDES = (8, 3)
Z0 = 0.40          # metres: the depth of the layout's pose
OUTSIDE = 40.0     # pixels beyond the image at which the corner triangles of `whole` lie
TCAP = 64          # the smallest tile the tests force (PCORE_FUSED_TCAP)
# (width, height) of the bounding boxes in pixels of the layout's pose, and how many of each
SHAPES = (((3.0, 3.0), 150), ((5.4, 5.4), 40), ((11.0, 3.0), 12), ((3.0, 11.0), 12),
          ((19.0, 3.0), 10), ((3.0, 19.0), 10), ((27.0, 3.0), 8), ((3.0, 27.0), 8), ((8.0, 2.0), 8), ((2.0, 8.0), 8),
          ((11.0, 2.0), 6), ((2.0, 11.0), 6), ((11.0, 11.0), 10), ((19.0, 11.0), 6), ((30.0, 30.0), 4),
          ((3.0, 45.0), 10), ((45.0, 3.0), 4), ((100.0, 80.0), 2))
# the builder keeps the order of triangles that share no vertex, 21 to a step (a vertex pass loads 64 vertices): the
# model starts with a step of boxes too small to hold two samples at either stride
TINY = ((1.5, 1.5), 21)
N_NAN = 3
NAN_AT = (30, 130, 230)      # where the NaN-vertex triangles of `nan` are inserted
CORNERS_AT = (8, 95, 180, 270)  # and the corner triangles of `whole` and `nan`


def _unproject(u, v, z):
    """The model point (metres) that the layout's pose (identity rotation, depth Z0 + z) shows at pixel (u, v) of the
    kernel's screen coordinates: sx = (p00 x / z + p02) W/2 + W/2, sy = (p11 y / z + p12) H/2 + H/2."""
    W, H = CAM["width"], CAM["height"]
    p = compute_proj(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], W, H).astype(np.float64)
    d = Z0 + z
    x = ((u - W / 2) / (W / 2) - p[2]) * d / p[0]
    y = ((v - H / 2) / (H / 2) - p[6]) * d / p[5]
    return np.stack([x, y, z], -1)


def _right_triangle(u0, v0, w, h, corner, z):
    """The right triangle that lacks `corner` of the box [u0, u0 + w] x [v0, v0 + h], vertex depths Z0 + z."""
    c = np.array([(u0, v0), (u0 + w, v0), (u0 + w, v0 + h), (u0, v0 + h)])
    c = np.delete(c, corner, axis=0)
    return _unproject(c[:, 0], c[:, 1], np.asarray(z))


@functools.lru_cache(maxsize=None)
def layout(seed=5):
    """(T, 9) float32: the mesh -- the TINY boxes, then the SHAPES shuffled."""
    rng = np.random.default_rng(seed)
    W, H = CAM["width"], CAM["height"]

    def place(shapes):
        tris = []
        for (w, h), count in shapes:
            for _ in range(count):
                u0, v0 = rng.random() * (W - 1 - w), rng.random() * (H - 1 - h)
                tris.append(_right_triangle(u0, v0, w, h, int(rng.integers(4)), (rng.random(3) * 2 - 1) * 0.004))
        return np.asarray(tris, F32).reshape(-1, 9)

    tiny, rest = place((TINY,)), place(SHAPES)
    return mc._frozen(np.concatenate([tiny, rest[rng.permutation(len(rest))]]))


@functools.lru_cache(maxsize=None)
def corners():
    W, H = CAM["width"], CAM["height"]
    t = [_right_triangle(u, v, 3.0, 3.0, k, np.zeros(3))
         for k, (u, v) in enumerate(((-OUTSIDE, -OUTSIDE), (W + OUTSIDE, -OUTSIDE), (W + OUTSIDE, H + OUTSIDE),
                                     (-OUTSIDE, H + OUTSIDE)))]
    return mc._frozen(np.asarray(t, F32))


@functools.lru_cache(maxsize=None)
def nan_triangles():
    """Copies of the first N_NAN 3 x 3 pixel triangles of the layout, moved by a pixel, with one coordinate NaN."""
    base = layout().reshape(-1, 3, 3)
    small = [t for t in base[TINY[1]:] if np.ptp(t[:, 0]) < 0.009 and np.ptp(t[:, 1]) < 0.009][:N_NAN]
    out = np.array(small, F32) + F32(0.001)
    for i in range(len(out)):
        out[i, i % 3, i % 2] = np.nan
    return mc._frozen(out)


POSE_KINDS = ("layout", "shift-x", "shift-y", "roll", "closer", "farther", "roll-shift", "tilt")
POSES44 = np.stack([
    mc._posed(np.eye(3), (0.0, 0.0, Z0)),
    mc._posed(np.eye(3), (0.008, 0.0, Z0)),             # three pixels to the right
    mc._posed(np.eye(3), (0.0, 0.0115, Z0)),            # four pixels down
    mc._posed(mc._rz(0.05), (0.0, 0.0, Z0)),
    mc._posed(np.eye(3), (0.0, 0.0, 0.36)),
    mc._posed(np.eye(3), (0.0, 0.0, 0.50)),
    mc._posed(mc._rz(-0.2), (0.004, -0.003, 0.42)),
    mc._posed(mc._rx(0.15), (0.0, 0.0, Z0)),
])
MODELS = ("whole", "nan", "tight")


@functools.lru_cache(maxsize=None)
def bank():
    whole = mc._frozen(np.insert(layout(), CORNERS_AT, corners(), axis=0))
    nan = mc._frozen(np.insert(whole, NAN_AT, nan_triangles(), axis=0))
    return mc.Bank("one_sample", [("whole", whole, None), ("nan", nan, np.nonzero(np.isnan(nan).any(1))[0]),
                                  ("tight", layout(), None)])


class OneSampleCase(mc.MeshCase):
    """mesh_cases.MeshCase (the oracle's renders, clouds, observation and costs, each computed once) over this bank,
    camera and poses: pose i is POSES44[i % 8] of model i // 8."""

    def __init__(self):
        self.name = "one_sample"
        self.bank = bank()
        self.cam = CAM
        self.width, self.height = CAM["width"], CAM["height"]
        self.proj = compute_proj(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], self.width, self.height)
        K, npose = self.bank.K, len(POSES44)
        self.poses44 = np.tile(POSES44, (K, 1, 1))
        self.poses = np.ascontiguousarray(init_from_eigen_batch(self.poses44))
        self.pose_model = np.repeat(np.arange(K), npose).astype(np.int32)
        self.pose_label = self.pose_model.copy()
        self.pose_kind = np.tile(np.arange(npose), K)
        self.n = len(self.poses)
        self.src_depth = np.zeros((self.height, self.width), np.int32)
        self.mask = np.zeros((self.height, self.width), np.uint8)
        self.r = mc.R
        self.oracle_count = np.concatenate([self.bank.tris_model_count, [0]]).astype(np.int32)

    def describe(self, pose):
        m = int(self.pose_model[pose])
        return f"model {m} {MODELS[m]}, pose {pose} ({POSE_KINDS[self.pose_kind[pose]]})"

    # -- the triangles' sample windows, on the CPU ----------------------------------------------------
    def screen(self, pose):
        """(T, 3, 2) float64 screen coordinates and (T, 3) camera depths (cm) of the pose's model, with the kernel's
        expressions in double."""
        m = int(self.pose_model[pose])
        v = self.bank.models[m].reshape(-1, 3, 3).astype(np.float64)
        M = self.poses[pose].astype(np.float64).reshape(4, 4)
        cam = v @ M[:3, :3].T + M[:3, 3]
        p = self.proj.astype(np.float64)
        W, H = self.width, self.height
        sx = (p[0] * cam[..., 0] + p[2] * cam[..., 2]) / cam[..., 2] * (W / 2) + W / 2
        sy = (p[5] * cam[..., 1] + p[6] * cam[..., 2]) / cam[..., 2] * (H / 2) + H / 2
        return np.stack([sx, sy], -1), cam[..., 2]

    def windows(self, pose, stride, clip=None):
        """Per triangle of the pose's model: (kx0, ky0, nx, ny) of its sample window by the reference's bounding box
        (first pixel trunc(max(0, min) + 0.5), last pixel floor(min(size - 1, max)); sample kx is column kx * stride,
        sample ky raster row H - 1 - ky * stride), clipped to `clip` = (x0, y0, x1, y1) inclusive samples when given;
        nx = ny = 0 where empty.  sure: no bound lies within 1e-3 pixels of the value at which its rounding changes,
        so the float32 arithmetic of the renderers cannot give another window; NaN triangles are never sure."""
        s, W, H = stride, self.width, self.height
        scr, _ = self.screen(pose)
        with np.errstate(invalid="ignore"):
            lo, hi = scr.min(1), scr.max(1)
            nan = np.isnan(scr).any((1, 2))
            lo, hi = np.nan_to_num(lo), np.nan_to_num(hi)
            ex = np.stack([np.maximum(0, lo[:, 0]) + 0.5, np.minimum(W - 1, hi[:, 0]),
                           np.maximum(0, lo[:, 1]) + 0.5, np.minimum(H - 1, hi[:, 1])], 1)
            sure = (np.abs(ex - np.round(ex)) > 1e-3).all(1) & ~nan
            px0, px1, py0, py1 = (np.floor(ex[:, k]).astype(np.int64) for k in range(4))
        kx0, kx1 = -(-px0 // s), px1 // s
        ky0, ky1 = -(-(H - 1 - py1) // s), (H - 1 - py0) // s
        if clip is not None:
            kx0, ky0 = np.maximum(kx0, clip[0]), np.maximum(ky0, clip[1])
            kx1, ky1 = np.minimum(kx1, clip[2]), np.minimum(ky1, clip[3])
        nx, ny = kx1 - kx0 + 1, ky1 - ky0 + 1
        empty = (nx <= 0) | (ny <= 0) | (hi[:, 0] < 0) | (hi[:, 1] < 0)
        nx, ny = np.where(empty, 0, nx), np.where(empty, 0, ny)
        return kx0, ky0, nx, ny, sure, nan

    def chunks(self, stride):
        """The chunks (x0, y0, x1, y1 inclusive) of a pose whose window is the whole sampled image under a tile of
        TCAP samples: row bands of whole window rows, blocks of columns when a row exceeds the tile (fused_pose)."""
        ws, hs = self.width // stride, -(-self.height // stride)
        cw = min(ws, TCAP)
        ch = max(1, TCAP // cw)
        return [(c0, r0, min(c0 + cw, ws) - 1, min(r0 + ch, hs) - 1) for r0 in range(0, hs, ch)
                for c0 in range(0, ws, cw)]


CLASSES = ("empty", "1", "2x1", "3x1", "4x1", "1x2", "1x3", "1x4", "2x2", "big")


def classify(nx, ny):
    """The class index (CLASSES) of every window: nx x ny samples, 'big' beyond four."""
    out = np.full(len(nx), CLASSES.index("big"))
    out[(nx == 0) | (ny == 0)] = 0
    for name in CLASSES[1:-1]:
        a, b = (1, 1) if name == "1" else (int(name[0]), int(name[2]))
        out[(nx == a) & (ny == b)] = CLASSES.index(name)
    return out


@functools.lru_cache(maxsize=None)
def case():
    return OneSampleCase()
