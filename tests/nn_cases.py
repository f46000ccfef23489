"""Adversarial observed clouds for the fused kernel's fixed-radius 1-NN grid search (phase 2 of fused_cost_kernel).

Every case here is built on the CPU with numpy and the oracle only: a camera and stride, two meshes, 32 to 64 poses
(many of them face-on at a fixed depth, so that whole columns of samples share x and whole rows share y, all at one z),
a zero source depth (nothing is occluded) and an observed cloud whose points are placed RELATIVE TO THE RENDERED POINTS
of those poses -- at distance exactly r, at equal distances, on the first floats beyond a cell face of the neighbour
grid, in a grid whose cell is set by the extent of a segment with a far point -- instead of being unprojected from a
depth image.  tests/test_nn_cases.py certifies on the CPU that each case can tell a wrong search from a right one;
tests/test_gpu_nn_adversarial.py runs them through the C ABI, bit for bit against the oracle's brute force.

The colour family at the end gives three of these geometries a colour per triangle and per observed point (cost type 1:
which triangle colours a sample, and on which side of the CIEDE2000 gate the pair falls, then decide the costs);
tests/test_gpu_colour.py runs it.

The neighbour grid (build_grid, pcore_prep.h) and the radius box of the query (process_points, pcore_fused.hip) are
restated here in float32 numpy with the same formulas, because the placements depend on where the float cell faces lie.
tests/test_prep.py holds the C++ build_grid to build_grid_np on every segment of every case.
"""
from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np

import oracle
from perception_amd import synthetic as syn
from perception_amd.model import compute_proj, init_from_eigen_batch
from tests.helpers import SMALL, TINY

F32 = np.float32
NAMES = ("003_cracker_box", "005_tomato_soup_can")
MODEL_RGB = np.array([(200, 40, 30), (30, 60, 190)], np.uint8)  # uniform mesh colours: the colour of a sample is
OTHER_RGB = np.array([(20, 200, 60), (230, 220, 40)], np.uint8)  # its model's; OTHER_RGB is beyond the colour gate
COLOUR_THR = 15.0
MESH_K = 8
RADII = (0.003, 0.0075, 0.01, 0.05)


# ---------------------------------------------------------------------------------------------
# float32 helpers
# ---------------------------------------------------------------------------------------------

def step(x, k):
    """float32 x moved by k representable floats (k an integer or an integer array), towards +inf for k > 0."""
    x = np.asarray(x, F32)
    i = x.view(np.int32).astype(np.int64)
    o = np.where(i >= 0, i, -(i & 0x7fffffff)) + np.asarray(k, np.int64)
    back = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return back.view(F32) if back.ndim else back.reshape(1).view(F32)[0]


def d2f(q, o):
    """The kernel's and the oracle's squared distance: float32, ((dx dx + dy dy) + dz dz), no contraction."""
    q = np.asarray(q, F32)
    o = np.asarray(o, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = q[..., 0] - o[..., 0], q[..., 1] - o[..., 1], q[..., 2] - o[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def r2_of(r):
    return F32(r) * F32(r)


# ---------------------------------------------------------------------------------------------
# build_grid and the query's radius box, restated
# ---------------------------------------------------------------------------------------------

def grid_params(lo, hi, r):
    """Origin, cell, 1 / cell and cell counts of build_grid for a point set with the finite bounds lo, hi."""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    ext = (hi - lo).max()
    cell = max(F32(2.0) * F32(r) * F32(1.01), ext / F32(64.0))
    if not cell > 0:
        cell = F32(1.0)
    inv_c = F32(1.0) / cell
    n = np.maximum(1, np.floor((hi - lo) * inv_c).astype(np.int64) + 1)
    return SimpleNamespace(o=lo, cell=F32(cell), inv_c=F32(inv_c), n=n)


def cell_coord(g, x, axis):
    """fl(fl(x - o) inv_c) along one axis: the float cell coordinate of build_grid and of the query."""
    return (np.asarray(x, F32) - g.o[axis]) * g.inv_c


def cell_index(g, x, axis):
    f = cell_coord(g, x, axis)
    return np.minimum(np.floor(np.maximum(f, F32(0.0))).astype(np.int64), g.n[axis] - 1)


def build_grid_np(pts, r):
    """build_grid on (n, 3) float32 points in local-index order: the grid, each point's cell (-1: non-finite, not in
    the grid) and its rank in the CSR order (cell, then local index)."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    if len(pts) == 0:
        g = SimpleNamespace(o=np.zeros(3, F32), cell=F32(1), inv_c=F32(1), n=np.ones(3, np.int64))
        g.cxyz, g.cell_of, g.rank = np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
        return g
    lo, hi = np.zeros(3, F32), np.zeros(3, F32)
    for k in range(3):
        c = pts[:, k][np.isfinite(pts[:, k])]
        if len(c):
            lo[k], hi[k] = c.min(), c.max()
    g = grid_params(lo, hi, r)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (pts - g.o[None, :]) * g.inv_c
        fin = np.isfinite(f).all(1)
        c = np.minimum(np.floor(np.maximum(np.where(fin[:, None], f, 0), 0)).astype(np.int64), g.n[None, :] - 1)
    g.cxyz = c
    g.cell_of = np.where(fin, (c[:, 2] * g.n[1] + c[:, 1]) * g.n[0] + c[:, 0], -1)
    order = np.lexsort((np.arange(len(pts)), g.cell_of))
    g.rank = np.empty(len(pts), np.int64)
    g.rank[order] = np.arange(len(pts))
    return g


def parent_pad(r):
    """The radius of the query's box in metres: sqrtf(r2) * 1.0001f + 1e-7f."""
    return np.sqrt(r2_of(r)) * F32(1.0001) + F32(1e-7)


BOX_ROUND = F32(1.0e-6)  # kBoxRound of pcore_fused.hip: cells of slack per cell of the grid's longest axis


def box_of(g, q, r, parent=False):
    """process_points' cell box of the queries q (n, 3): (inside (n,), i0 (n, 3), i1 (n, 3)); the kernel reads the x
    cells i0..i1 of the rows iy0..min(iy1, iy0 + 1) x iz0..min(iz1, iz0 + 1).  parent = True restates the box as it was
    before the rounding bound kBoxRound (max(nx, ny, nz) + 2) was added to its radius."""
    q = np.asarray(q, F32).reshape(-1, 3)
    rc = parent_pad(r) * g.inv_c
    if not parent:
        rc = rc + BOX_ROUND * F32(int(g.n.max()) + 2)
    with np.errstate(invalid="ignore", over="ignore"):
        f0 = (q - g.o[None, :]) * g.inv_c
        lo, hi = f0 - rc, f0 + rc
        nf = g.n.astype(F32)[None, :]
        inside = ((hi >= 0) & (lo < nf)).all(1)
        i0 = np.floor(np.maximum(np.where(inside[:, None], lo, 0), F32(0))).astype(np.int64)
        i1 = np.minimum(g.n[None, :] - 1, np.floor(np.where(inside[:, None], hi, 0)).astype(np.int64))
    i1[:, 1:] = np.minimum(i1[:, 1:], i0[:, 1:] + 1)
    return inside, i0, i1


# ---------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------

ROT_Y = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])  # the cracker box's large face to the camera
TILT = syn._rot_align_z(np.array([0.3, -0.4, 1.0]))


def _posed(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def _bank():
    bank = syn.model_bank(list(NAMES), MESH_K)
    for m, rgb in zip(bank.models, MODEL_RGB):
        m.colors = np.tile(rgb, (m.tris.shape[0], 1)).astype(np.uint8)
    return bank


def pose_set(z_face, z_step=0.2):
    """40 poses: the box face-on at depth z_face on a 4 x 3 lattice of in-plane shifts and at z_face + z_step on 4,
    8 tilted boxes; the can's cap face-on at 6 shifts and 10 tilted cans.  Returns (poses44, pose_model)."""
    P, M = [], []
    for sy in (-0.17, 0.0, 0.17):
        for sx in (-0.3, -0.1, 0.1, 0.3):
            P.append(_posed(ROT_Y, (sx * z_face, sy * z_face, z_face + 0.03)))
            M.append(0)
    z2 = z_face + z_step
    for sx in (-0.3, -0.1, 0.1, 0.3):
        P.append(_posed(ROT_Y, (sx * z2, 0.05 * z2, z2 + 0.03)))
        M.append(0)
    for i in range(8):
        P.append(_posed(TILT @ syn._rot_z(0.7 * i), (0.12 * z_face * np.cos(i), 0.1 * z_face * np.sin(i),
                                                    z_face + 0.08 + 0.013 * i)))
        M.append(0)
    for i in range(6):
        P.append(_posed(np.eye(3), ((-0.25 + 0.1 * i) * z_face, (0.12 if i % 2 else -0.12) * z_face, z_face + 0.0505)))
        M.append(1)
    for i in range(10):
        P.append(_posed(TILT @ syn._rot_z(0.5 * i), (0.2 * z_face * np.cos(2 * i), 0.12 * z_face * np.sin(2 * i),
                                                    z_face + 0.1 + 0.011 * i)))
        M.append(1)
    return np.stack(P), np.array(M, np.int32)


class NNCase:
    """Everything a run needs, in the caller's order (obs_xyz, obs_label, obs_rgb as given to set_observation) and in
    the label-sorted order the oracle takes (obs_sorted, ...).  pose_label is the 6-DoF segment of each pose."""

    def __init__(self, name, cam, stride, r, poses44, pose_model, pose_label=None):
        self.name, self.cam, self.stride, self.r = name, cam, stride, float(r)
        self.bank = _bank()
        self.width, self.height = cam["width"], cam["height"]
        self.proj = compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], self.width, self.height)
        self.poses44 = poses44
        self.poses = init_from_eigen_batch(poses44)
        self.pose_model = np.asarray(pose_model, np.int32)
        self.pose_label = self.pose_model.copy() if pose_label is None else np.asarray(pose_label, np.int32)
        self.n = len(self.poses)
        self.src_depth = np.zeros((self.height, self.width), np.int32)
        self.mask = np.zeros((self.height, self.width), np.uint8)
        self.meta = {}
        self._render()

    def _render(self):
        c, s = self.cam, self.stride
        z = oracle.render_depth(self.bank.tris, self.bank.tris_model_count, self.poses, self.pose_model, None,
                                self.width, self.height, self.proj, self.src_depth, None, 1.0)
        xyz, pose, _ = oracle.depth_to_cloud(z, s, c["cx"], c["cy"], c["fx"], c["fy"], 100.0)
        zs = z[:, ::s, ::s]
        pn, ky, kx = np.nonzero(zs > 0)
        assert np.array_equal(pn, pose)
        # the kernel's expressions, restated: z = Z / depth_factor, x = (kx s - cx) / fx z, in float32
        zz = zs[pn, ky, kx].astype(F32) / F32(100.0)
        xx = ((kx * s).astype(F32) - F32(c["cx"])) / F32(c["fx"]) * zz
        yy = ((ky * s).astype(F32) - F32(c["cy"])) / F32(c["fy"]) * zz
        assert np.array_equal(np.stack([xx, yy, zz], 1).view(np.uint32), xyz.view(np.uint32))
        self.Q, self.q_pose, self.q_kx, self.q_ky, self.q_Z = xyz, pose, kx, ky, zs[pn, ky, kx]

    def unique_queries(self, label):
        """The distinct rendered points of the poses with this 6-DoF label: (Q, kx, ky, Z, a pose of each)."""
        sel = np.nonzero(self.pose_label[self.q_pose] == label)[0]
        _, first = np.unique(self.Q[sel].view(np.uint32), axis=0, return_index=True)
        i = sel[np.sort(first)]
        return SimpleNamespace(Q=self.Q[i], kx=self.q_kx[i], ky=self.q_ky[i], Z=self.q_Z[i], pose=self.q_pose[i])

    def set_observation(self, xyz, label, rgb, seed):
        """Shuffles the observation into the order in which it is given; returns the permutation applied."""
        xyz = np.asarray(xyz, F32).reshape(-1, 3)
        perm = np.random.default_rng(seed).permutation(len(xyz))
        self.obs_xyz = np.ascontiguousarray(xyz[perm])
        self.obs_label = np.ascontiguousarray(np.asarray(label, np.int32)[perm])
        self.obs_rgb = np.ascontiguousarray(np.asarray(rgb, np.uint8)[perm])
        self.finish()
        return perm

    def finish(self):
        lab = self.obs_label
        self.order = np.argsort(lab, kind="stable")
        self.obs_sorted = np.ascontiguousarray(self.obs_xyz[self.order])
        self.lab_sorted = lab[self.order]
        self.rgb_sorted = np.ascontiguousarray(self.obs_rgb[self.order])
        self.num_labels = max(0, int(lab.max()) + 1)
        self.label_start = np.array([np.searchsorted(self.lab_sorted, L, "left") for L in range(self.num_labels)],
                                    np.int32)
        self.label_end = np.array([np.searchsorted(self.lab_sorted, L, "right") for L in range(self.num_labels)],
                                  np.int32)
        cnt = (self.label_end - self.label_start).astype(np.float32)
        pl = self.pose_label
        ok = (pl >= 0) & (pl < self.num_labels)
        self.pose_obs_total = np.maximum(np.where(ok, cnt[np.clip(pl, 0, self.num_labels - 1)], 0), 1).astype(F32)
        self.pose_obs_total0 = np.full(self.n, float(len(lab)), F32)
        assert len(lab) <= 21000, len(lab)

    def segment(self, label):
        """(points, positions in the label-sorted cloud) of a 6-DoF segment; label None: the whole cloud (3-DoF)."""
        if label is None:
            return self.obs_sorted, np.arange(len(self.obs_sorted))
        if not 0 <= label < self.num_labels:
            return np.zeros((0, 3), F32), np.zeros(0, np.int64)
        a, b = self.label_start[label], self.label_end[label]
        return self.obs_sorted[a:b], np.arange(a, b)

    # -- the oracle's side ------------------------------------------------------------------------
    def oracle_costs(self, cost_type, calc_obs=True, colour_thr=COLOUR_THR):
        c = self.cam
        if cost_type == 1:
            return oracle.evaluate_colour(self.bank.tris, self.bank.colors, self.bank.tris_model_count, self.poses,
                                          self.pose_model, self.width, self.height, self.proj, self.src_depth, 1.0,
                                          self.stride, c["cx"], c["cy"], c["fx"], c["fy"], 100.0, self.obs_sorted,
                                          self.rgb_sorted, self.pose_obs_total0, calc_obs, self.r, colour_thr)
        six = cost_type == 2
        return oracle.evaluate(self.bank.tris, self.bank.tris_model_count, self.poses, self.pose_model,
                               self.pose_label if six else None, self.width, self.height, self.proj, self.src_depth,
                               self.mask if six else None, 1.0, self.stride, c["cx"], c["cy"], c["fx"], c["fy"], 100.0,
                               self.obs_sorted, self.label_start if six else None, self.label_end if six else None,
                               self.pose_obs_total if six else self.pose_obs_total0, cost_type, calc_obs, self.r)


def _rgb_for(labels, match):
    """Colours of observed points: the model's own colour (within the gate) where match, else one beyond it."""
    L = np.clip(np.asarray(labels), 0, 1)
    return np.where(np.asarray(match, bool)[:, None], MODEL_RGB[L], OTHER_RGB[L])


def sample_pitch(case, z):
    c = case.cam
    return case.stride / c["fx"] * z, case.stride / c["fy"] * z


# ---------------------------------------------------------------------------------------------
# family: radius edge
# ---------------------------------------------------------------------------------------------

Z_FACE_EDGE = {0.003: 0.5, 0.0075: 0.85, 0.01: 1.1, 0.05: 0.6}
EDGE_CLASSES = ("eq", "above", "below")


def _edge_targets(r):
    r2 = r2_of(r)
    return {"eq": r2, "above": np.nextafter(r2, F32(np.inf)), "below": np.nextafter(r2, F32(0))}


def edge_point(q, r, target, axis, sec, sign, two_axes):
    """An observed point whose float d2 to q is exactly `target`: the floats around q[axis] + sign r alone (one axis),
    or with a small offset of k floats along `sec` as well (two axes).  None when no candidate lands on the target."""
    q = np.asarray(q, F32)
    a = step(q[axis] + F32(sign) * F32(r), np.arange(-12, 13))
    # one float along `axis` moves d2 by 2 r ulp(q[axis]): the offsets along `sec` reach a little beyond that
    span = np.sqrt(4.0 * r * float(np.spacing(np.abs(a[0])))) / float(np.spacing(np.abs(q[sec])))
    ks = np.arange(1, 3000) * max(1, int(np.ceil(1.5 * span / 3000))) if two_axes else np.arange(0, 1)
    b = step(q[sec], ks)
    o = np.empty((len(a), len(b), 3), F32)
    o[...] = q
    o[..., axis] = a[:, None]
    o[..., sec] = b[None, :]
    hit = np.argwhere(d2f(q, o) == target)
    if len(hit) == 0:
        return None
    return o[hit[0][0], hit[0][1]]


def radius_case(r, cam_name="SMALL", stride=4):
    cam = {"SMALL": SMALL, "TINY": TINY}[cam_name]
    zf = Z_FACE_EDGE[r] if cam_name == "SMALL" else 0.45
    P, M = pose_set(zf)
    case = NNCase(f"radius-{cam_name}-s{stride}-r{r}", cam, stride, r, P, M)
    targets = _edge_targets(r)
    sx, sy = sample_pitch(case, zf)
    all_axes = 2 * r < 0.9 * min(sx, sy)  # else a point at q + r e_x is nearer to q's neighbours: z only
    pts, labs, match, made = [], [], [], {k: 0 for k in EDGE_CLASSES}
    for L in (0, 1):
        u = case.unique_queries(L)
        for i, q in enumerate(u.Q[:360]):
            cls = EDGE_CLASSES[i % 3]
            axis = (i // 3) % 3 if all_axes else 2
            sec = (axis + 1 + (i // 9) % 2) % 3
            sign = 1 if (i // 18) % 2 else -1
            o = edge_point(q, r, targets[cls], axis, sec, sign, two_axes=(i // 36) % 2 == 1)
            if o is None:
                o = edge_point(q, r, targets[cls], axis, sec, sign, two_axes=True)
            if o is None:
                continue
            made[cls] += 1
            pts.append(o)
            labs.append(L)
            match.append(i % 2 == 0)
    case.meta["made"] = made
    case.set_observation(np.stack(pts), labs, _rgb_for(labs, match), seed=11)
    return case


# ---------------------------------------------------------------------------------------------
# family: ties
# ---------------------------------------------------------------------------------------------

# (camera, stride, face-on depth, delta): the sample pitch z stride / fx is between delta and delta + r, so that the
# sample next to a tied one sees the nearer candidate within r (the witness) and nothing else nearer
TIE_CONFIG = {0.003: ("TINY", 1, 0.40, 2.0 ** -9), 0.0075: ("SMALL", 4, 0.45, 2.0 ** -8),
              0.01: ("SMALL", 4, 0.60, 2.0 ** -7), 0.05: ("SMALL", 4, 0.60, 2.0 ** -7)}


def tie_case(r):
    """Units of three samples along a face-on sample row (along a column on every second group of three rows): a
    blocker -- the sample itself, twice: exact duplicates at two indices --, a tied sample q with the mirrored pair
    q -+ delta, and a witness, the sample after q, whose unique nearest neighbour is q + delta.  On flipped units the
    order is witness, q, blocker, and the witness sees q - delta.  After the shuffle every pair is oriented so that the
    witnessed candidate has the HIGHER index and the other one is reached only through the tie (the blocker keeps q's
    other neighbour off it): with the lowest index winning both candidates are explained, with any other rule one is.
    On flipped units the lower index is in the higher cell, so the first candidate in CSR cell order is the wrong one
    wherever a face lies between the two.  The candidates of a pair, and the two duplicates, get colours on opposite
    sides of the colour gate."""
    cam_name, stride, zf, delta = TIE_CONFIG[r]
    cam = {"SMALL": SMALL, "TINY": TINY}[cam_name]
    P, M = pose_set(zf)
    case = NNCase(f"ties-r{r}", cam, stride, r, P, M)
    d = F32(delta)
    pts, labs, mate, want_high = [], [], [], []  # mate: the other candidate / duplicate; want_high: must be the higher
    for L in (0, 1):
        u = case.unique_queries(L)
        Zs, cnt = np.unique(u.Z, return_counts=True)
        plane = u.Z == Zs[np.argmax(cnt)]  # the face-on plane
        for q, kx, ky in zip(u.Q[plane], u.kx[plane], u.ky[plane]):
            along_y = (ky // 3) % 2 == 1
            if along_y and kx % 2:
                continue  # units along y on every second column
            if not along_y and ky % 3 == 1:
                continue  # units along x on two rows of three
            ax = 1 if along_y else 0
            ph = int(ky if along_y else kx) % 3
            flip = bool((kx // 2) % 2) if along_y else ky % 3 == 2
            base = len(pts)
            if ph == (2 if flip else 0):
                pts.extend([q.copy(), q.copy()])
                want_high.extend([False, False])
            elif ph == 1:
                lo, hi = q.copy(), q.copy()
                lo[ax], hi[ax] = q[ax] - d, q[ax] + d
                if d2f(q, lo) != d2f(q, hi):
                    continue  # q -+ delta is not exact in float32 here
                pts.extend([lo, hi])
                want_high.extend([flip, not flip])
            else:
                continue
            labs.extend([L, L])
            mate.extend([base + 1, base])
    pts, labs, mate, want_high = np.stack(pts), np.array(labs), np.array(mate), np.array(want_high)
    # the shuffle decides the indices; then the two points of a pair trade places where the witnessed one came lower
    perm = np.random.default_rng(5).permutation(len(pts))
    pos = np.empty(len(pts), np.int64)
    pos[perm] = np.arange(len(pts))  # the position at which each point is given
    for i in np.nonzero(want_high)[0]:
        if pos[i] < pos[mate[i]]:
            pos[i], pos[mate[i]] = pos[mate[i]], pos[i]
    xyz, lab_given, match = np.empty_like(pts), np.empty(len(pts), np.int32), np.zeros(len(pts), bool)
    xyz[pos], lab_given[pos] = pts, labs
    for i in range(0, len(pts), 2):  # the lower index of a pair within the gate on even pairs, beyond it on odd ones
        a, b = sorted((pos[i], pos[i + 1]))
        match[a], match[b] = (i // 2) % 2 == 0, (i // 2) % 2 != 0
    case.obs_xyz, case.obs_label = np.ascontiguousarray(xyz), lab_given
    case.obs_rgb = np.ascontiguousarray(_rgb_for(lab_given, match))
    case.finish()
    case.meta["delta"] = float(delta)
    return case


# ---------------------------------------------------------------------------------------------
# family: cell faces (ordinary grid, cell = 2.02 r) and the stretched grid (cell = extent / 64)
# ---------------------------------------------------------------------------------------------

def find_face(g, axis, k, near):
    """The smallest float32 x with cell coordinate >= k along `axis`, searched around `near`; None if not there."""
    x = step(F32(near), np.arange(-1536, 1537))
    f = np.floor(cell_coord(g, x, axis))
    i = np.nonzero(f >= k)[0]
    if len(i) == 0 or i[0] == 0:
        return None
    return x[i[0]]


def face_case(r):
    """Anchors fix the grid's box a little inside the rendered points' bounds.  Every rendered point, by the third of
    the image it lies in, gets one observed point across the nearest face along x, y or z, on the first 1 to 3 floats
    of the far side, with the other coordinates equal; rendered points outside the box get theirs on the box's first or
    last floats; in the y third, points that are near a z face too get the other (y, z) rows populated."""
    zf = {0.003: 0.5, 0.0075: 0.6, 0.01: 0.6, 0.05: 0.6}[r]
    P, M = pose_set(zf)
    case = NNCase(f"faces-r{r}", SMALL, 4, r, P, M)
    ws = case.width // case.stride
    crowded = 2.02 * r >= min(sample_pitch(case, zf))  # two samples of a row can be within r of one face
    pts, labs, grids = [], [], {}
    rr = F32(r)
    for L in (0, 1):
        u = case.unique_queries(L)
        lo = u.Q.min(0) + np.array([0.6, 0.6, -0.5], F32) * rr
        hi = u.Q.max(0) - np.array([0.6, 0.6, -0.5], F32) * rr
        g = grid_params(lo, hi, r)
        grids[L] = (lo, hi)
        own = [lo, hi]
        for i, (q, kx, ky) in enumerate(zip(u.Q, u.kx, u.ky)):
            axis = min(2, (3 * kx) // ws)
            other = [a for a in range(3) if a != axis]
            if (q[other] < lo[other]).any() or (q[other] > hi[other]).any():
                continue
            j = i % 3

            def across(ax, jj):
                """The coordinate on the far side of the face nearest to q along ax (None: no such face)."""
                if q[ax] < lo[ax]:
                    return step(lo[ax], jj)
                if q[ax] > hi[ax]:
                    return step(hi[ax], -jj)
                k = int(np.rint(float(cell_coord(g, q[ax], ax))))
                if not 1 <= k <= g.n[ax] - 1:
                    return None
                face = find_face(g, ax, k, F32(np.float64(lo[ax]) + k * np.float64(g.cell)))
                if face is None:
                    return None
                below = q[ax] < face
                # a sample row (column) then serves one side of its faces only: points put on the near side for the samples
                # beyond the face would be nearer, by a few floats, than the ones across it
                if ax < 2 and crowded and below != bool((ky if ax == 0 else kx) % 2):
                    return None
                v = step(face, jj) if below else step(face, -1 - jj)
                return v if lo[ax] <= v <= hi[ax] else None

            v = across(axis, j)
            if v is None:
                continue
            o = q.copy()
            o[axis] = v
            own.append(o)
            if axis == 1 and lo[1] <= q[1] <= hi[1]:
                w = across(2, j)
                if w is not None and abs(float(w) - float(q[2])) <= r:
                    o2, o3 = q.copy(), o.copy()
                    o2[2], o3[2] = w, w
                    own.extend([o2, o3])
        own = np.stack(own)
        assert (own >= lo).all() and (own <= hi).all()  # the anchors stay the grid's box
        pts.append(own)
        labs.extend([L] * len(own))
    pts = np.concatenate(pts)
    case.meta["anchors"] = grids
    case.set_observation(pts, labs, _rgb_for(labs, np.arange(len(pts)) % 2 == 0), seed=13)
    return case


def _stretch_search(xq_list, r, far, prefer_miss=True):
    """Far coordinates (F, H) of a segment -- its minimum F about `far` away and its maximum H one cell beyond the
    face -- such that cell = (H - F) / 64 puts the face between cells 62 and 63 within (r (1 - 1e-4), r] of one of
    the candidate coordinates x_q.  The realised face is the float one, found by a scan.  There the cell coordinate
    moves in steps of ulp(63) cells, about 1.8e-6 m for a 0.47 m cell and more than the window, so most candidates
    miss it and the search goes on; it prefers a placement for which the parent commit's box leaves the face's far
    side out.  Returns (x_q, F, H, face, missed) or None."""
    r2 = r2_of(r)
    best = None
    for jitter in range(24):  # other cell sizes: other alignments of the roundings
        for xq in xq_list:
            xq = F32(xq)
            t = float(xq) + r * (1 - 3e-5)
            c = abs(far) * (1 + 1e-3 * jitter) / 63.0
            F = F32(t - 63 * c)
            for dh in range(-8, 9):
                H = step(F32(t + c), dh)
                g = grid_params(np.array([F, 0, 0], F32), np.array([H, 0, 0], F32), r)
                face = find_face(g, 0, 63, F32(t))
                if face is None:
                    continue
                d = xq - face
                if not (d * d <= r2 and float(face) - float(xq) > r * (1 - 1e-4)):
                    continue
                _, _, i1 = box_of(g, np.array([[xq, 0, 0]], F32), r, parent=True)
                missed = bool(i1[0, 0] < 63)
                if best is None or missed:
                    best = (xq, F, H, face, missed)
                if missed:
                    return best
        if best is not None and not prefer_miss:
            return best
    return best


def stretched_case(r, far, axis):
    """One far observed point per segment at `far` metres along x or y (axis 0 / 1) and one a cell beyond the object,
    placed by _stretch_search; along z (axis 2) one far point at z = +far, which only sets the cell.  The rendered
    points of the chosen face-on column (row) get their observed point on the first floats beyond the face; the others
    get one at 0.5 r, 0.99 r or 1.2 r along the other in-plane axis (at r = 0.05 every eighth of them does)."""
    zf = 0.6
    P, M = pose_set(zf)
    case = NNCase(f"stretched-r{r}-far{far}-axis{axis}", SMALL, 4, r, P, M)
    rr = F32(r)
    pts, labs = [], []
    case.meta["search"] = {}
    for L in (0, 1):
        u = case.unique_queries(L)
        mid = np.median(u.Q, axis=0).astype(F32)
        own = []
        chosen = np.zeros(len(u.Q), bool)
        if axis < 2:
            # the coordinates that most rendered points share first (the columns or rows of the face-on planes)
            coords, mult = np.unique(u.Q[:, axis], return_counts=True)
            # H, one cell beyond the face, has to be the segment's maximum: coordinates within 0.9 cell of the top
            top = coords >= u.Q[:, axis].max() - 0.9 * abs(far) / 63.0
            coords, mult = coords[top], mult[top]
            found = _stretch_search(coords[np.argsort(-mult, kind="stable")][:40], r, far, prefer_miss=r < 0.009)
            assert found is not None, "no far placement puts a face within r (1 - 1e-4) of a column"
            xq, F, H, face, missed = found
            case.meta["search"][L] = dict(coord=float(xq), F=float(F), H=float(H), face=float(face), missed=missed)
            for v in (F, H):
                p = mid.copy()
                p[axis] = v
                own.append(p)
            chosen = u.Q[:, axis] == xq
            for i in np.nonzero(chosen)[0]:
                o = u.Q[i].copy()
                o[axis] = step(face, i % 3)
                own.append(o)
        else:
            p = mid.copy()
            p[2] = F32(far)
            own.append(p)
        oth = 1 - axis if axis < 2 else 0
        sparse = r > 0.02  # else every rendered point is within r of some neighbour's point: on every eighth sample
        for i in np.nonzero(~chosen)[0]:
            if sparse and (u.kx[i] % 8 or u.ky[i] % 8):
                continue
            o = u.Q[i].copy()
            o[oth] = o[oth] + rr * F32((0.5, 0.99, 1.2)[i % 3]) * F32(1 if i % 2 else -1)
            own.append(o)
        own = np.stack(own)
        if axis < 2:
            assert own[:, axis].min() == F and own[:, axis].max() == H  # the grid is the planned one
        pts.append(own)
        labs.extend([L] * len(own))
    pts = np.concatenate(pts)
    case.set_observation(pts, labs, _rgb_for(labs, np.arange(len(pts)) % 2 == 0), seed=17)
    return case


# ---------------------------------------------------------------------------------------------
# family: segments and indices
# ---------------------------------------------------------------------------------------------

def segments_case(r=0.01):
    """Labels {0, 2, 3, 4}: segment 1 is empty, segment 3 holds one point, segment 4 five identical points (extent 0);
    poses with labels 1 (the empty segment), 3, 4 and 7 (at or above the number of segments); observed points with
    label -1 on top of rendered points (they match nothing at 6-DoF and are part of the 3-DoF cloud); NaN points and
    points with +inf or -inf in one coordinate interleaved with the others, so that the local indices after them still
    have to line up with the explained bitmap and with the observed colours."""
    P, M = pose_set(0.6)
    pl = np.where(M == 0, 0, 2).astype(np.int32)
    pl[[12, 13]] = 3, 4        # two of the second plane's face-on boxes
    pl[[14, 20]] = 1, 7        # the empty segment; a label at or above the number of segments
    pl[[30, 35]] = 7, 1
    case = NNCase(f"segments-r{r}", SMALL, 4, r, P, M, pose_label=pl)
    rng = np.random.default_rng(23)
    pts, labs = [], []
    for L in (0, 2):
        u = case.unique_queries(L)
        off = rng.normal(size=u.Q.shape)
        off *= (rng.choice([0.3, 0.7, 0.95, 1.05, 1.3], len(off)) * r / np.linalg.norm(off, axis=1))[:, None]
        own = (u.Q + off.astype(F32)).astype(F32)
        pts.append(own)
        labs.extend([L] * len(own))
        neg = u.Q[::7]
        pts.append(neg)
        labs.extend([-1] * len(neg))
        bad = u.Q[3::11].copy()
        kinds = np.arange(len(bad)) % 3
        bad[kinds == 0] = np.nan
        bad[kinds == 1, np.arange((kinds == 1).sum()) % 3] = np.inf
        bad[kinds == 2, np.arange((kinds == 2).sum()) % 3] = -np.inf
        pts.append(bad)
        labs.extend([L] * len(bad))
    u3, u4 = case.unique_queries(3), case.unique_queries(4)
    pts.append(u3.Q[len(u3.Q) // 2][None] + np.array([[0.5 * r, 0, 0]], F32))
    labs.append(3)
    pts.append(np.repeat(u4.Q[len(u4.Q) // 3][None] + np.array([[0, 0.4 * r, 0]], F32), 5, axis=0))
    labs.extend([4] * 5)
    pts = np.concatenate(pts).astype(F32)
    case.set_observation(pts, labs, _rgb_for(labs, rng.random(len(pts)) < 0.5), seed=29)
    return case


# ---------------------------------------------------------------------------------------------
# family: per-triangle colours (cost type 1: the fused kernel's colour id pass and the CIEDE2000 gate)
# ---------------------------------------------------------------------------------------------

COLOUR_BASE = np.array((120, 130, 110))  # every triangle and every observed point: the base + U[-40, 40] per channel,
COLOUR_SPREAD = 40                       # which puts about a third of the random pairs within the gate at 15
COLOUR_GEOMETRIES = ("segments-s4", "segments-s5", "ties-TINY-s1")
COLOUR_VARIANTS = ("plain", "dup", "rev")
DUP_PER_MODEL = 48


@functools.lru_cache(maxsize=None)
def _colour_geometry(geom):
    """The camera, stride, poses and observed points of a colour case: the `segments` case at stride 4, the same
    observation seen at stride 5, and the r = 0.003 tie case (TINY, stride 1).  Built once; no colour case changes it."""
    if geom == "segments-s4":
        return _cover_poses(segments_case())
    if geom == "segments-s5":
        b = _colour_geometry("segments-s4")
        c = NNCase("segments-s5", b.cam, 5, b.r, b.poses44, b.pose_model, b.pose_label)
        c.obs_xyz, c.obs_label, c.obs_rgb = b.obs_xyz, b.obs_label, b.obs_rgb
        c.finish()
        return _cover_poses(c)
    assert geom == "ties-TINY-s1"
    return _cover_poses(tie_case(0.003))


MIN_GATED = 60


def _cover_poses(case):
    """The observations of the depth cases leave some poses (the second plane, the tilted ones, the poses of the small
    segments) with few or no rendered points within r of an observed point, and a pose without gated pairs cannot show
    a wrong colour.  Every pose with fewer than MIN_GATED such points gets, appended to the observation with label -1,
    an observed point 0.4 r beside every second rendered point of its own."""
    d2, idx = oracle.knn1(case.Q, None, case.obs_sorted)
    gated = np.bincount(case.q_pose[(d2 <= r2_of(case.r)) & (idx >= 0)], minlength=case.n)
    num = np.bincount(case.q_pose, minlength=case.n)
    add = [case.Q[case.q_pose == p][::2] + np.array([0.4 * case.r, 0, 0], F32)
           for p in np.nonzero((gated < MIN_GATED) & (num > 0))[0]]
    if add:
        add = np.concatenate(add).astype(F32)
        case.obs_xyz = np.ascontiguousarray(np.concatenate([case.obs_xyz, add]))
        case.obs_label = np.ascontiguousarray(np.concatenate([case.obs_label, np.full(len(add), -1, np.int32)]))
        case.obs_rgb = np.ascontiguousarray(np.concatenate([case.obs_rgb, np.zeros((len(add), 3), np.uint8)]))
        case.finish()
    return case


def _random_rgb(rng, n):
    return (COLOUR_BASE[None, :] + rng.integers(-COLOUR_SPREAD, COLOUR_SPREAD + 1, (n, 3))).astype(np.uint8)


def _with_mesh(base, name, tris, colors, obs_rgb):
    """A shallow copy of the geometry with other meshes (a list of (tris, colours) per model) and observed colours."""
    case = copy.copy(base)
    case.name, case.meta = name, {}
    case.bank = _bank()
    for m, t, c in zip(case.bank.models, tris, colors):
        m.tris = np.ascontiguousarray(t, F32).reshape(-1, 9)
        m.colors = np.ascontiguousarray(c, np.uint8).reshape(-1, 3)
    case.obs_rgb = np.ascontiguousarray(obs_rgb, np.uint8)
    case.finish()
    return case


def sample_triangles(case):
    """The triangle (index into the concatenated mesh) whose colour each rendered point of case.Q has: the oracle's
    colour planes of the mesh with every triangle's index written into its three colour bytes."""
    T = len(case.bank.tris)
    i = np.arange(T)
    code = np.stack([i & 255, (i >> 8) & 255, i >> 16], 1).astype(np.uint8)
    z, col = oracle.render_depth_color(case.bank.tris, code, case.bank.tris_model_count, case.poses, case.pose_model,
                                       None, case.width, case.height, case.proj, case.src_depth, None, 1.0)
    s = case.stride
    assert np.array_equal(z[:, ::s, ::s][case.q_pose, case.q_ky, case.q_kx], case.q_Z)
    b = col[:, :, ::s, ::s][:, case.q_pose, case.q_ky, case.q_kx].astype(np.int64)
    tid = b[0] | (b[1] << 8) | (b[2] << 16)
    hi = np.cumsum(case.bank.tris_model_count)
    lo = hi - case.bank.tris_model_count
    m = case.pose_model[case.q_pose]
    assert ((tid >= lo[m]) & (tid < hi[m])).all()  # a rendered point has a triangle of its pose's model
    return tid


def gated_pairs(case, nn=None):
    """The (observed point, triangle) pairs whose colour distance the cost of type 1 tests: the rendered points with a
    nearest observed point within r.  Returns a namespace of arrays over the pairs: q (index into case.Q), pose, obs
    (position in the label-sorted cloud), tri, d (the oracle's colour distance); and bad_r (n,), the rendered points
    per pose without a neighbour within r.  nn: (d2, index) of each rendered point's nearest observed point of the
    whole cloud (the oracle's brute force when None)."""
    d2, idx = oracle.knn1(case.Q, None, case.obs_sorted) if nn is None else nn
    tid = sample_triangles(case)
    near = d2 <= r2_of(case.r)
    q = np.nonzero(near & (idx >= 0))[0]
    lab_o = oracle.rgb2lab_n(case.rgb_sorted)
    lab_t = oracle.rgb2lab_n(case.bank.colors)
    d = oracle.colour_distance_n(np.concatenate([lab_o[idx[q]], lab_t[tid[q]]], 1))
    return SimpleNamespace(q=q, pose=case.q_pose[q], obs=idx[q].astype(np.int64), tri=tid[q], d=d,
                           bad_r=np.bincount(case.q_pose[~near], minlength=case.n),
                           num=np.bincount(case.q_pose, minlength=case.n))


def colour_costs_np(case, pairs, thr, calc_obs=True):
    """The costs of type 1 from the gated pairs, in the reference's float order: a pair beyond the threshold is bad, a
    pair within it marks its observed point explained."""
    within = ~(pairs.d > np.float64(F32(thr)))
    rc, oc, df = (np.zeros(case.n, F32) for _ in range(3))
    for p in range(case.n):
        mine = pairs.pose == p
        num = F32(pairs.num[p])
        nbad = F32(pairs.bad_r[p] + (mine & ~within).sum())
        expl = F32(len(np.unique(pairs.obs[mine & within])))
        r = F32(-1.0) if num == 0 else nbad / num
        rc[p] = r if r == F32(-1.0) else r * F32(100.0)
        if calc_obs:
            tot = case.pose_obs_total0[p]
            df[p] = (num - nbad) - expl
            oc[p] = (tot - expl) / tot * F32(100.0)
    return rc, oc, df


def _other_side(rng, rgb_o, d, thr):
    """A colour whose distance to the observed colour rgb_o is on the other side of thr than d: the observed colour
    itself (distance 0) for a pair beyond the gate, a random colour beyond the gate for a pair within it."""
    if d > thr:
        return rgb_o.copy()
    lab_o = oracle.rgb2lab(rgb_o)
    for _ in range(200):
        c = rng.integers(0, 256, 3).astype(np.uint8)
        if oracle.colour_distance(lab_o, oracle.rgb2lab(c)) > thr:
            return c
    raise AssertionError("no colour beyond the gate")


@functools.lru_cache(maxsize=None)
def colour_case(geom, variant="plain"):
    """plain: every triangle and every observed point with a random colour of its own.  dup: DUP_PER_MODEL triangles
    per model that colour gated samples are appended to their model once more, each copy with a colour on the other
    side of the gate (from its original, against the observed point of the original's first gated pair): the original,
    with the lower index, has to win every sample.  dup-front: the same copies BEFORE the originals (the certificate's
    counter-example: there the copies win).  rev: the plain mesh with the triangles, and their colours, in reverse
    order within each model: the same depths, the other winner wherever two triangles tie in depth."""
    base = _colour_geometry(geom)
    seed = 101 + COLOUR_GEOMETRIES.index(geom.replace("s5", "s4"))  # both strides of `segments`: the same mesh colours
    rng = np.random.default_rng(seed)
    cnt = base.bank.tris_model_count
    tris = [m.tris for m in base.bank.models]
    cols = np.split(_random_rgb(rng, int(cnt.sum())), np.cumsum(cnt)[:-1])
    obs_rgb = _random_rgb(rng, len(base.obs_xyz))
    name = f"colour-{geom}-{variant}"
    if variant == "plain":
        return _with_mesh(base, name, tris, cols, obs_rgb)
    if variant == "rev":
        return _with_mesh(base, name, [t[::-1] for t in tris], [c[::-1] for c in cols], obs_rgb)
    assert variant in ("dup", "dup-front")
    plain = colour_case(geom, "plain")
    pairs = gated_pairs(plain)
    lo = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    dt, dc, chosen = [], [], []
    for m in range(len(cnt)):
        ids = np.unique(pairs.tri[(pairs.tri >= lo[m]) & (pairs.tri < lo[m] + cnt[m])])
        assert len(ids) >= DUP_PER_MODEL, (m, len(ids))
        ids = ids[np.linspace(0, len(ids) - 1, DUP_PER_MODEL).astype(int)]
        first = [np.nonzero(pairs.tri == t)[0][0] for t in ids]
        dt.append(tris[m][ids - lo[m]])
        dc.append(np.stack([_other_side(rng, plain.rgb_sorted[pairs.obs[k]], pairs.d[k], COLOUR_THR) for k in first]))
        chosen.append(ids)
    if variant == "dup":
        case = _with_mesh(base, name, [np.concatenate([t, d]) for t, d in zip(tris, dt)],
                          [np.concatenate([c, d]) for c, d in zip(cols, dc)], obs_rgb)
    else:
        case = _with_mesh(base, name, [np.concatenate([d, t]) for t, d in zip(tris, dt)],
                          [np.concatenate([d, c]) for c, d in zip(cols, dc)], obs_rgb)
    case.meta["copied"] = chosen
    return case


def queued_records(case, pose):
    """How many (triangle, sample) records raster_phase queues for a pose: over the model's triangles whose sample
    window (the reference's bounding box and loop bounds, restated in float64) holds 1 to kSmallK = 4 samples, the
    samples.  The triangles go to the workgroup's 4 waves by stream, and a wave's ring holds kRecCap = 128 records."""
    m = int(case.pose_model[pose])
    P = case.poses[pose].astype(np.float64).reshape(4, 4)
    v = case.bank.models[m].tris.astype(np.float64).reshape(-1, 3)
    cam = v @ P[:3, :3].T + P[:3, 3]
    pj = case.proj.astype(np.float64).reshape(4, 4)
    W, H, s = case.width, case.height, case.stride
    with np.errstate(all="ignore"):
        sx = ((np.c_[cam, np.ones(len(cam))] @ pj[0]) / cam[:, 2] * W / 2 + W / 2).reshape(-1, 3)
        sy = ((np.c_[cam, np.ones(len(cam))] @ pj[1]) / cam[:, 2] * H / 2 + H / 2).reshape(-1, 3)
    x0 = np.trunc(np.maximum(0, sx.min(1)) + 0.5)
    x1 = np.floor(np.minimum(W - 1, sx.max(1)))
    y0 = np.trunc(np.maximum(0, sy.min(1)) + 0.5)
    y1 = np.floor(np.minimum(H - 1, sy.max(1)))
    nx = np.floor(x1 / s) - np.ceil(x0 / s) + 1
    ny = np.floor((H - 1 - y0) / s) - np.ceil((H - 1 - y1) / s) + 1
    nk = np.where((nx > 0) & (ny > 0), nx * ny, 0)
    small = (nk >= 1) & (nk <= 4)
    return int(small.sum()), int(nk[small].sum())


# ---------------------------------------------------------------------------------------------
# the table of cases
# ---------------------------------------------------------------------------------------------

CASES = {}
for _r in RADII:
    CASES[f"radius-r{_r}"] = functools.partial(radius_case, _r)
    CASES[f"ties-r{_r}"] = functools.partial(tie_case, _r)
    CASES[f"faces-r{_r}"] = functools.partial(face_case, _r)
CASES["radius-TINY-s1-r0.01"] = functools.partial(radius_case, 0.01, "TINY", 1)
for _r, _far, _axis in ((0.0075, -10.0, 0), (0.0075, -30.0, 0), (0.0075, -60.0, 0), (0.0075, -10.0, 1),
                        (0.0075, -30.0, 1), (0.0075, -60.0, 1), (0.003, -30.0, 0), (0.01, -60.0, 0), (0.05, 65.0, 2),
                        (0.0075, 65.0, 2)):
    CASES[f"stretched-r{_r}-far{_far:g}-axis{_axis}"] = functools.partial(stretched_case, _r, _far, _axis)
CASES["segments"] = segments_case
CASE_NAMES = tuple(CASES)
COLOUR_CASES = tuple(n for n in CASE_NAMES if n.startswith("ties")) + ("segments",)


@functools.lru_cache(maxsize=None)
def nn_case(name):
    """A case of the table, built once per process; no test changes it."""
    return CASES[name]()
