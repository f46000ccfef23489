"""Cases for the interior vertex pass's bounds in 16-bit halves (vertex_bounds, STRIDE == 8, INTERIOR, in
perception_amd/csrc/pcore_fused.hip).

packed_bounds() restates the five instructions on numpy integers: the two words are built with 32-bit additions and
subtractions whose low 16 bits land in a half, then each half is shifted as an int16; scalar_bounds() is the scalar form
that every other pass keeps.  tests/test_bounds_cases.py compares the two over every value of every component.

Two cameras reach the top of the int16 range on the device: 16384 x 16 (`wide`) and 24 x 16384 (`tall`), 16384 being
the largest the camera setter accepts, at stride 8, with the sheet mesh of tests/interior_cases.py 1.5 m away (12 x 8.5
pixels: it covers a sample or more wherever it lies, and with its margins just fits 16 rows) and the
principal point near the far corner, so that a small translation puts the sheet there.  The poses step the sheet towards
the last pixel column (wide) and towards screen row 0, the last sample row (tall), to where the interior class ends: its
box needs the margin of 2 pixels and a little inside the image, so the largest converted coordinate of an interior pose
is 16380, in the last sample column / row (2047) all the same.  The unprojection keeps mesh_cases' intrinsics (the
oracle and the context are given the same ones): only the projection matrix puts the image's far corner in view."""
from __future__ import annotations

import functools

import numpy as np

from tests import interior_cases as ic

F32 = np.float32
Z = 1.5            # metres
SHAPES = dict(wide=(16384, 16), tall=(24, 16384))
INSIDE = tuple(2.2 + 0.55 * k for k in range(12))  # pixels between the sheet's leading vertex and the border pixel


def scalar_bounds(lo0, lo1, hi0, hi1, H):
    """vertex_bounds at stride 8, the scalar form: the words (A0 | B0 << 16, A1 | B1 << 16) as uint32."""
    lo0, lo1, hi0, hi1 = (np.asarray(v, np.int64) for v in (lo0, lo1, hi0, hi1))
    A0, A1 = (lo0 + 7) >> 3, hi0 >> 3
    B0, B1 = (H - 1 - hi1 + 7) >> 3, (H - 1 - lo1) >> 3
    word = lambda a, b: ((a & 0xffff) | ((b & 0xffff) << 16)).astype(np.uint32)
    return word(A0, B0), word(A1, B1)


def packed_bounds(lo0, lo1, hi0, hi1, H):
    """The interior pass's form: a 32-bit lo0 + 7 / hi0 in the low half, the low 16 bits of the 32-bit H + 6 - hi1 / H - 1
    - lo1 written to the upper half, then an arithmetic shift by 3 of each int16 half."""
    u32 = lambda v: np.asarray(v, np.int64).astype(np.uint32)
    low0, low1 = u32(np.asarray(lo0, np.int64) + 7), u32(hi0)
    up0, up1 = u32(H + 6 - np.asarray(hi1, np.int64)), u32(H - 1 - np.asarray(lo1, np.int64))
    w0 = (low0 & np.uint32(0xffff)) | ((up0 & np.uint32(0xffff)) << np.uint32(16))
    w1 = (low1 & np.uint32(0xffff)) | ((up1 & np.uint32(0xffff)) << np.uint32(16))

    def shift(w):
        h = np.ascontiguousarray(w).view(np.int16).reshape(-1, 2) >> 3  # little endian: (low, high) halves
        return np.ascontiguousarray(h.astype(np.int16)).view(np.uint32).reshape(-1)

    return shift(w0), shift(w1)


def cam(shape):
    """The camera whose projection matrix the case uses: the principal point 20 pixels inside the far corner, (W - 20,
    8) for `wide` (the last columns), (8, H - 20) for `tall`: screen row 20, near the screen's row 0, whose samples are
    the last sample rows."""
    W, H = SHAPES[shape]
    cx, cy = (W - 20.0, 8.0) if shape == "wide" else (8.0, H - 20.0)
    return dict(ic.CAM, width=W, height=H, cx=cx, cy=cy)


def _translation(u, v, shape):
    """The translation (cm) under which the model's origin shows at screen (u, v) at depth Z, in double."""
    W, H = SHAPES[shape]
    p = ic.proj(cam(shape)).astype(np.float64)
    z = Z * 100
    return np.array([((u - W / 2) / (W / 2) - p[2]) * z / p[0], ((v - H / 2) / (H / 2) - p[6]) * z / p[5], z])


@functools.lru_cache(maxsize=None)
def poses(shape):
    W, H = SHAPES[shape]
    v = ic.mesh().reshape(-1, 3)
    pix = (Z / ic.CAM["fx"], Z / ic.CAM["fy"])
    bw, bh = float(v[:, 0].max()) / pix[0], float(v[:, 1].max()) / pix[1]
    out = []
    for d in INSIDE:
        # sx grows with x, sy falls with y: the sheet's far corner (largest x) leads towards the last column, its
        # largest y towards screen row 0
        u, w = (W - 1 - d - bw, 3.0 + bh) if shape == "wide" else (5.0, d + bh)
        out.append(ic._rows(np.eye(3), _translation(u, w, shape)))
    p = np.ascontiguousarray(np.stack(out), F32)
    p.setflags(write=False)
    return p


def converted(pose16, shape):
    """(lo0, lo1, hi0, hi1) of every vertex: the vertex pass's four conversions."""
    sx, sy, _ = ic.vertex_pass(pose16, ic.mesh().reshape(-1, 3), cam(shape))
    return (np.floor(sx + F32(0.5)).astype(np.int64), np.floor(sy + F32(0.5)).astype(np.int64),
            np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64))


class BoundsCase(ic.InteriorCase):
    def __init__(self, shape):
        super().__init__()
        self.name = shape
        self.cam = cam(shape)
        self.width, self.height = SHAPES[shape]
        self.proj = ic.proj(self.cam)
        self.poses = poses(shape)
        self.kinds = [(None, f"{d:.2f} px inside") for d in INSIDE]
        self.n = len(self.poses)
        self.pose_model = np.zeros(self.n, np.int32)
        self.pose_label = self.pose_model.copy()
        self.pose_kind = np.arange(self.n) % 3
        self.src_depth = np.zeros((self.height, self.width), np.int32)
        self.mask = np.zeros((self.height, self.width), np.uint8)

    def describe(self, pose):
        return f"{self.name} pose {pose} ({self.kinds[pose][1]})"


@functools.lru_cache(maxsize=None)
def case(shape):
    return BoundsCase(shape)
