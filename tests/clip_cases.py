"""Cases for the triangle stage without its clip to the pose window (raster_phase's WHOLE copy, pcore_fused.hip) and
for the tightened interior class (pose_window: no clamp of the window to the sampled image may bind).

The sheet mesh and the 72-pixel-wide camera of tests/interior_cases.py, 48 and 50 rows high (48 a multiple of both
strides, 50 of neither; every entry point refuses a width that is no multiple of the stride, so the width stays 72), at
strides 8 and 3.  This module restates in float32 / integers
  window()        pose_window's sample window before its clamps, (X0, X1, Y0, Y1), and the class under the old rule (the
                  box inside the image) and the new one (and no clamp binds),
  tri_windows()   the triangle stage's unclipped windows from vertex_bounds' four bounds per vertex,
and picks identity-rotation poses from sweeps of the sheet across the image:
  last_col / last_row     interior poses with a non-empty triangle window in the last column / row of the pose window
  first_col / first_row   interior poses with one in the second column / row: the first is out of reach.  With sx = s k
                          + f the lower bound is A0 = ceil(rpi(sx) / s) >= k while the window starts at X0 = floor((sx -
                          margin - 1) / s) <= k - 1 for f < 3 and A0 = k + 1, X0 = k for f > 3 (margin >= 2), and the
                          same for rows: the nearest a triangle window comes to the first column or row is one sample.
  left_band               the sheet against the left border, the box's xlo in [0, 1): X0 = -1 is clamped to 0, so the
                          pose is interior under the old rule and fastdiv only under the new one
  right / bottom          the sheet against the right border and the last image row (the last sample row of the
                          50-row image is row 48, two rows above the border)
tests/test_clip_cases.py certifies all of it on the CPU; tests/test_gpu_clip.py runs the poses bit for bit against the
oracle, whole and in chunks of eight samples."""
from __future__ import annotations

import functools

import numpy as np

from tests import interior_cases as ic
from tests import mesh_cases as mc

F32 = np.float32
HEIGHTS = (48, 50)
STRIDES = ic.STRIDES
KINDS = ("last_col", "last_row", "first_col", "first_row", "left_band", "right", "bottom")
PER_KIND = 3


def cam(height):
    return dict(ic.CAM, height=height)


def window(pose16, tris, c, s):
    """((X0, X1, Y0, Y1) unclamped, old class, new class) of a pose, or None where the window is the whole image."""
    b = ic.pose_box(pose16, tris, c)
    if b is None:
        return None
    xlo, xhi, ylo, yhi = (F32(v) for v in b[:4])
    Hf, sf = F32(c["height"]), F32(s)
    X0, X1 = int(np.floor((xlo - F32(1)) / sf)), int(np.floor(xhi / sf))
    Y0, Y1 = int(np.floor((Hf - F32(1) - yhi) / sf)), int(np.floor((Hf - ylo) / sf))
    ws, hs = c["width"] // s, -(-c["height"] // s)
    old = ic.pose_class(pose16, tris, c)
    new = old if old < 2 or (X0 >= 0 and X1 <= ws - 1 and Y0 >= 0 and Y1 <= hs - 1) else 1
    return (X0, X1, Y0, Y1), old, new


def tri_windows(pose16, tris, c, s):
    """(lo (T, 2), hi (T, 2)) int: the triangles' sample windows [lo, hi] (x, y) before any clip, from the vertex pass's
    screen coordinates (inside the image) and vertex_bounds' integer formulas."""
    H = c["height"]
    sx, sy, _ = ic.vertex_pass(pose16, np.asarray(tris, F32).reshape(-1, 3), c)
    assert sx.min() >= 0 and sx.max() <= c["width"] - 1 and sy.min() >= 0 and sy.max() <= H - 1
    lo0, lo1 = np.floor(sx + F32(0.5)).astype(np.int64), np.floor(sy + F32(0.5)).astype(np.int64)
    hi0, hi1 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    A0, A1 = (lo0 + s - 1) // s, hi0 // s
    B0, B1 = (H - 1 - hi1 + s - 1) // s, (H - 1 - lo1) // s
    lo = np.stack([A0.reshape(-1, 3).min(1), B0.reshape(-1, 3).min(1)], 1)
    hi = np.stack([A1.reshape(-1, 3).max(1), B1.reshape(-1, 3).max(1)], 1)
    return lo, hi


def _translation(u, v, c):
    """The translation (cm) under which the model's origin shows at screen (u, v) at the depth Z0, in double."""
    W, H = c["width"], c["height"]
    p = ic.proj(c).astype(np.float64)
    z = ic.Z0 * 100
    return np.array([((u - W / 2) / (W / 2) - p[2]) * z / p[0], ((v - H / 2) / (H / 2) - p[6]) * z / p[5], z])


def touches(pose16, tris, c, s):
    """The kinds a pose serves at stride s (a set), from window() and tri_windows()."""
    w = window(pose16, tris, c, s)
    out = set()
    if w is None:
        return out
    (X0, X1, Y0, Y1), old, new = w
    if old == 2 and new == 1 and X0 == -1:
        out.add("left_band")
    if new != 2:
        return out
    lo, hi = tri_windows(pose16, tris, c, s)
    ne = (hi >= lo).all(1)
    if (hi[ne, 0] == X1).any():
        out.add("last_col")
    if (hi[ne, 1] == Y1).any():
        out.add("last_row")
    if (lo[ne, 0] == X0 + 1).any():
        out.add("first_col")
    if (lo[ne, 1] == Y0 + 1).any():
        out.add("first_row")
    return out


@functools.lru_cache(maxsize=None)
def poses(height):
    """(poses (n, 16) float32, kinds: a list of names).  Two sweeps of the sheet, along x in the middle rows and along y
    in the middle columns, in steps of 0.37 pixels; of each kind the first PER_KIND poses that serve it at both strides
    (left_band: at either)."""
    c = cam(height)
    W, H = c["width"], c["height"]
    tris = ic.mesh()
    v = tris.reshape(-1, 3)
    bw, bh = float(v[:, 0].max()) / ic.PIX[0], float(v[:, 1].max()) / ic.PIX[1]
    mid_u, mid_v = float(round((W - 1 - bw) / 2)), float(round((H - 1 + bh) / 2))
    sweep = [(u, mid_v) for u in np.arange(2.0, W - 1 - bw - 2.0, 0.37)]
    sweep += [(mid_u, w) for w in np.arange(bh + 2.0, H - 3.0, 0.37)]
    out, kinds = [], []
    count = dict.fromkeys(KINDS, 0)
    for u, w in sweep:
        m = ic._rows(np.eye(3), _translation(u, w, c))
        t8, t3 = touches(m, tris, c, 8), touches(m, tris, c, 3)
        for k in sorted((t8 & t3) | ((t8 | t3) & {"left_band"})):
            if count[k] < PER_KIND:
                count[k] += 1
                out.append(m)
                kinds.append(k)
    # against the right border and the last image row: the extreme vertex 2.3 pixels inside (the margin is 2 and a little)
    for u, w, k in ((W - 1 - bw - 2.3, mid_v, "right"), (mid_u, bh + 2.3, "bottom"), (W - 1 - bw - 2.3, bh + 2.3, "right")):
        out.append(ic._rows(np.eye(3), _translation(u, w, c)))
        kinds.append(k)
    p = np.ascontiguousarray(np.stack(out), F32)
    p.setflags(write=False)
    return p, kinds


class ClipCase(ic.InteriorCase):
    """interior_cases.InteriorCase (the oracle's renders, clouds, observation and costs, each computed once) with this
    module's camera height and poses."""

    def __init__(self, height):
        super().__init__()
        self.name = f"clip{height}"
        self.cam = cam(height)
        self.height = height
        self.proj = ic.proj(self.cam)
        self.poses, self.kinds = poses(height)
        self.n = len(self.poses)
        self.pose_model = np.zeros(self.n, np.int32)
        self.pose_label = self.pose_model.copy()
        self.pose_kind = np.arange(self.n) % 3
        self.src_depth = np.zeros((self.height, self.width), np.int32)
        self.mask = np.zeros((self.height, self.width), np.uint8)

    def describe(self, pose):
        return f"{self.name} pose {pose} ({self.kinds[pose]})"


@functools.lru_cache(maxsize=None)
def case(height):
    return ClipCase(height)
