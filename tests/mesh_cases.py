"""Mesh and bank shapes for the fused raster's vertex-ring streams (perception_amd/csrc/pcore_streams.h and the walk
of raster_phase in pcore_fused.hip): the pose sweeps vary the pose over a few meshes, these cases vary the mesh and the
bank over a few poses.

Everything here is built on the CPU with numpy, scipy and the oracle only: a small non-square camera, eight poses per
model (face-on, tilted and rolled, one with the camera plane inside the model's box, one partly off screen), meshes
with irregular valence and shuffled faces, models around the stream-count boundaries S = min(4, ceil(T / 64)), a fan
around one hub vertex, triangles that render nothing (degenerate, duplicated, NaN / inf), banks with empty models and
with a one-triangle model last, and an observed cloud made from the oracle's own rendered points so that the costs
move with every sample.  tests/test_mesh_cases.py certifies on the CPU that the cases can fail (nearly every triangle
owns a sample, deleting one changes a depth, a wrong triangle index changes a colour cost);
tests/test_gpu_mesh_shapes.py runs them through the C ABI, bit for bit against the oracle."""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial import Delaunay

import oracle
from perception_amd.model import compute_proj, init_from_eigen_batch

F32 = np.float32
CAM = dict(width=160, height=120, fx=150.0, fy=140.0, cx=81.5, cy=58.25)
STRIDES = (1, 8, 2, 5)  # the templated kernels (1, 8) and the generic ones (2, 5); the width is a multiple of each
R = 0.006               # sensor resolution: the radius of the costs' nearest-neighbour test
MAX_OBS = 6000          # observed points of a (bank, stride) at most: the oracle's search is a brute force
N_DISPLACED = 300
SHEET = (0.24, 0.18)    # metres
Z_AMP = 0.012
COLOUR_A = np.array((200, 40, 30), np.uint8)
COLOUR_B = np.array((30, 60, 190), np.uint8)
COLOUR_THR = 15.0
EMPTY = np.zeros((0, 9), F32)
SIZES = (1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 256, 257)  # around S = min(4, ceil(T / 64))
SIZED_STREAMS = (1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4)


# ---------------------------------------------------------------------------------------------
# meshes: (n, 9) float32, metres, centred on the origin, seeded
# ---------------------------------------------------------------------------------------------

def _frozen(a):
    a = np.ascontiguousarray(a, F32).reshape(-1, 9)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def delaunay_sheet(nv, seed=3):
    """The Delaunay triangulation of nv random (x, y) on the sheet, random z within +-Z_AMP, faces shuffled:
    irregular valence, slivers along the hull, no overlap.  About 2 nv - 16 triangles."""
    rng = np.random.default_rng(seed + nv)
    xy = (rng.random((nv, 2)) - 0.5) * np.array(SHEET)
    z = (rng.random(nv) * 2 - 1) * Z_AMP
    v = np.c_[xy, z].astype(F32)
    faces = Delaunay(v[:, :2].astype(np.float64)).simplices
    return _frozen(v[faces[rng.permutation(len(faces))]])


@functools.lru_cache(maxsize=None)
def heightfield(n, seed=9):
    """A regular n x n grid over the sheet with random heights, two triangles per cell (the diagonal alternates),
    faces shuffled.  A regular grid leaves few samples at which two triangles give the same winning depth; the seed is
    one that leaves some at every tested stride and, in every `sized` model, no triangle whose samples all lie on such
    ties (tests/test_mesh_cases.py asserts both)."""
    rng = np.random.default_rng(seed + n)
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, n + 1) * SHEET[0], np.linspace(-0.5, 0.5, n + 1) * SHEET[1])
    v = np.stack([x, y, (rng.random(x.shape) * 2 - 1) * Z_AMP], -1).astype(F32)
    tris = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = v[i, j], v[i, j + 1], v[i + 1, j + 1], v[i + 1, j]
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 else [(a, b, d), (b, c, d)]
    tris = np.asarray(tris, F32).reshape(-1, 9)
    return _frozen(tris[rng.permutation(len(tris))])


FAN_HUB = np.array((0.0, 0.0, 0.004), F32)


@functools.lru_cache(maxsize=None)
def fan(n, seed=7):
    """n triangles around one hub vertex, shuffled: every triangle names the hub, so the builder has to load it again
    whenever it ages out of the ring.  The rim (radius 0.058 to 0.082 m, heights within +-8 mm) waves smoothly with a
    little noise: its slopes stay below the tilt of the poses, so no wedge hides behind another one."""
    rng = np.random.default_rng(seed + n)
    ang = 2 * np.pi * np.arange(n) / n
    rad = 0.07 + 0.010 * np.sin(5 * ang) + 0.002 * rng.random(n)
    z = 0.008 * np.sin(2 * ang + 0.4) + 0.0001 * rng.random(n)
    rim = np.c_[rad * np.cos(ang), rad * np.sin(ang), z].astype(F32)
    tris = np.stack([np.tile(FAN_HUB, (n, 1)), rim, np.roll(rim, -1, axis=0)], 1).reshape(-1, 9)
    return _frozen(tris[rng.permutation(n)])


def sized(T):
    """The first T faces of the shuffled heightfield: mostly isolated triangles spread over the sheet."""
    return _frozen(heightfield(24)[:T])


@functools.lru_cache(maxsize=None)
def _noisy(kind, arg, seed=11):
    base = {"delaunay": delaunay_sheet, "heightfield": heightfield}[kind](arg)
    rng = np.random.default_rng(seed + len(base))
    T = len(base)
    pick = lambda k: base[rng.choice(T, k, replace=False)].reshape(k, 3, 3).copy()
    extra = []
    t = pick(6)                       # a repeated vertex
    t[:, 1] = t[:, 0]
    extra.append(t)
    t = pick(6)                       # collinear: the second vertex on the edge of the other two
    t[:, 1] = (t[:, 0] + t[:, 2]) * F32(0.5)
    extra.append(t)
    extra.append(pick(6))             # exact duplicates of earlier triangles
    extra.append(pick(6)[:, [0, 2, 1]])  # duplicates with the winding reversed
    t = pick(1)                       # a vertex pair that differs only in the sign of a zero coordinate
    t2 = t.copy()
    t[:, 0, 1], t2[:, 0, 1] = F32(0.0), F32(-0.0)
    extra += [t, t2]
    t = pick(6)                       # NaN, +inf, -inf, twice each, in different coordinates
    for i, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        t[i, i % 3, (i // 3 + i) % 3] = bad
    extra.append(t)
    extra = np.concatenate(extra).reshape(-1, 9).astype(F32)
    assert 10 * len(extra) <= T + len(extra)
    return _frozen(np.concatenate([base, extra])), np.arange(T, T + len(extra))


def noisy(kind, arg):
    """A base mesh followed by triangles that need no witness: (tris, the indices of the additions)."""
    return _noisy(kind, arg)


# ---------------------------------------------------------------------------------------------
# poses (model -> camera, metres; the camera looks along +z)
# ---------------------------------------------------------------------------------------------

def _rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def _posed(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


POSE_KINDS = ("face-on", "tilt-x", "tilt-y", "tilt-xy", "near", "off-screen", "close", "closer")
POSES44 = np.stack([
    _posed(np.eye(3), (0.0, 0.0, 0.40)),
    _posed(_rx(0.35) @ _rz(0.5), (0.01, -0.005, 0.42)),
    _posed(_ry(-0.30) @ _rz(-1.1), (-0.015, 0.01, 0.38)),
    _posed(_rx(-0.2) @ _ry(0.25) @ _rz(2.4), (0.0, 0.0, 0.45)),
    _posed(_rx(0.35), (0.0, 0.0, 0.02)),            # the camera plane cuts the model's box
    _posed(_rz(0.3), (0.13, 0.05, 0.40)),           # a part of the sheet is beyond the right border
    _posed(_rx(0.15) @ _rz(0.1), (0.0, 0.0, 0.30)),
    _posed(_ry(0.1), (-0.004, 0.002, 0.25)),        # about two pixels per triangle of the largest sheet
])
NEAR_POSE, OFF_SCREEN_POSE = POSE_KINDS.index("near"), POSE_KINDS.index("off-screen")


# ---------------------------------------------------------------------------------------------
# banks
# ---------------------------------------------------------------------------------------------

class Bank:
    def __init__(self, name, models):
        """models: a list of (label, tris, exempt local indices or None)."""
        self.name = name
        self.labels = [m[0] for m in models]
        self.models = [m[1] for m in models]
        self.exempt = [np.zeros(0, np.int64) if m[2] is None else np.asarray(m[2], np.int64) for m in models]
        self.surface = [m[0].split("(")[0] in ("delaunay", "heightfield", "fan", "sized", "noisy") and len(m[1]) > 0
                        for m in models]
        self.K = len(models)
        self.tris = np.ascontiguousarray(np.concatenate(self.models), F32)
        self.tris_model_count = np.array([len(m) for m in self.models], np.int32)
        self.hi = np.cumsum(self.tris_model_count)
        self.lo = self.hi - self.tris_model_count

    def local_index(self):
        """Every triangle's index within its model."""
        return np.concatenate([np.arange(c) for c in self.tris_model_count]).astype(np.int64)

    def index_colours(self):
        """Every triangle's global index in its three colour bytes (as nn_cases.sample_triangles does)."""
        i = np.arange(len(self.tris))
        return np.stack([i & 255, (i >> 8) & 255, i >> 16], 1).astype(np.uint8)

    def num_colourings(self):
        return max(1, int(np.ceil(np.log2(max(2, int(self.tris_model_count.max()))))))

    def colouring(self, b):
        """Colour A for the triangles whose index within their model has bit b set, else colour B."""
        bit = (self.local_index() >> b) & 1
        return np.ascontiguousarray(np.where(bit[:, None] == 1, COLOUR_A, COLOUR_B).astype(np.uint8))


def _sized_model(T):
    return (f"sized({T})", sized(T), None)


def _noisy_model(kind, arg):
    t, ex = noisy(kind, arg)
    return (f"noisy({kind} {arg})", t, ex)


_EMPTY_MODEL = ("EMPTY", EMPTY, None)


@functools.lru_cache(maxsize=None)
def bank(name):
    if name == "small_sizes":  # every size a model of its own, shuffled; the one-triangle model is the bank's last
        order = [SIZES[i] for i in np.random.default_rng(13).permutation(len(SIZES)) if SIZES[i] != 1] + [1]
        return Bank(name, [_sized_model(T) for T in order])
    if name in ("with_empty", "empty_first"):
        models = [_sized_model(1), _EMPTY_MODEL, _sized_model(65), _noisy_model("delaunay", 200), _EMPTY_MODEL,
                  _sized_model(3), _EMPTY_MODEL]
        return Bank(name, ([_EMPTY_MODEL] if name == "empty_first" else []) + models)
    if name == "large":
        return Bank(name, [("delaunay(2600)", delaunay_sheet(2600), None), ("fan(300)", fan(300), None),
                           ("heightfield(24)", heightfield(24), None), _noisy_model("delaunay", 800)])
    raise KeyError(name)


BANKS = ("small_sizes", "with_empty", "large")
ALL_BANKS = BANKS + ("empty_first",)


# ---------------------------------------------------------------------------------------------
# the case: a bank, every pose for every model, and the oracle's side
# ---------------------------------------------------------------------------------------------

class MeshCase:
    """A bank with the POSES44 of every model (model-major: pose i is POSES44[i % 8] of model i // 8), a zero source
    depth, and per stride the observed cloud and the oracle's expectations, each computed once and left unchanged."""

    def __init__(self, name):
        self.name = name
        self.bank = bank(name)
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
        self.r = R
        # the oracle indexes pose_model without a range check: it is given the bank with one more, empty model,
        # and a pose whose model is out of range is a pose of that one
        self.oracle_count = np.concatenate([self.bank.tris_model_count, [0]]).astype(np.int32)

    def describe(self, pose):
        m = int(self.pose_model[pose])
        label = self.bank.labels[m] if 0 <= m < self.bank.K else "out of range"
        return f"bank {self.name}, model {m} {label}, pose {pose} ({POSE_KINDS[self.pose_kind[pose]]})"

    def oracle_models(self, pose_model):
        pm = np.asarray(pose_model, np.int32)
        return np.where((pm < 0) | (pm >= self.bank.K), self.bank.K, pm).astype(np.int32)

    # -- renders ----------------------------------------------------------------------------------
    def render(self, tris=None, count=None, poses=None, pose_model=None):
        return oracle.render_depth(self.bank.tris if tris is None else tris,
                                   self.oracle_count if count is None else count,
                                   self.poses if poses is None else poses,
                                   self.oracle_models(self.pose_model if pose_model is None else pose_model), None,
                                   self.width, self.height, self.proj, self.src_depth, None, 1.0)

    @functools.cached_property
    def z_full(self):
        z = self.render()
        z.setflags(write=False)
        return z

    def zs(self, stride):
        return self.z_full[:, ::stride, ::stride]

    def render_colour(self, colours, tris=None):
        """(depth (n, H, W), colour planes (3, n, H, W)) of every pose with a colour per triangle."""
        return oracle.render_depth_color(self.bank.tris if tris is None else tris, colours, self.oracle_count,
                                         self.poses, self.pose_model, None, self.width, self.height, self.proj,
                                         self.src_depth, None, 1.0)

    @functools.cached_property
    def owners(self):
        """(n, H, W) int64: the global index of the triangle that colours each pixel with a positive depth (the pixels
        that become points), -1 elsewhere."""
        z, col = self.render_colour(self.bank.index_colours())
        assert np.array_equal(z, self.z_full)
        c = col.astype(np.int64)
        return np.where(z > 0, c[0] | (c[1] << 8) | (c[2] << 16), -1)

    @functools.cached_property
    def owners_reversed(self):
        """owners with every model's triangles given in reverse order (the same depths; the other winner wherever
        two triangles give the winning depth), mapped back to the indices of the forward order."""
        b = self.bank
        rev = np.concatenate([np.arange(lo, hi)[::-1] for lo, hi in zip(b.lo, b.hi)]).astype(np.int64)
        z, col = self.render_colour(b.index_colours(), tris=np.ascontiguousarray(b.tris[rev]))
        assert np.array_equal(z, self.z_full)
        c = col.astype(np.int64)
        own = c[0] | (c[1] << 8) | (c[2] << 16)
        return np.where(z > 0, rev[np.minimum(own, len(rev) - 1)], -1)

    def cloud(self, stride):
        """The oracle's compaction of its z-buffers at a stride: (xyz (P, 3), pose (P,))."""
        xyz, pose, _ = oracle.depth_to_cloud(self.z_full, stride, CAM["cx"], CAM["cy"], CAM["fx"], CAM["fy"], 100.0)
        return xyz, pose

    # -- observation ------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def observation(self, stride):
        """The union of the rendered points of all poses at this stride, without the points of every third block of
        samples (so that no pose is explained everywhere), labelled with the model of the pose they come from; then
        N_DISPLACED of them once more, moved by more than r; in shuffled order.  Every point has colour B."""
        s = stride
        xyz, pose = self.cloud(s)
        zs = self.zs(s)
        pn, ky, kx = np.nonzero(zs > 0)
        assert np.array_equal(pn, pose)
        blk = max(1, 12 // s)
        keep = ((kx // blk) + (ky // blk) + self.pose_kind[pose]) % 3 != 0
        pts, lab = xyz[keep], self.pose_model[pose][keep]
        # distinct (point, label) pairs: the same point under two labels stays twice (the `sized` models share faces)
        _, first = np.unique(np.c_[pts.view(np.uint32), lab.astype(np.uint32)], axis=0, return_index=True)
        first = np.sort(first)
        if len(first) > MAX_OBS - N_DISPLACED:
            first = first[np.linspace(0, len(first) - 1, MAX_OBS - N_DISPLACED).astype(np.int64)]
        pts, lab = pts[first], lab[first]
        rng = np.random.default_rng(17 + s)
        if len(pts):
            j = rng.choice(len(pts), min(N_DISPLACED, len(pts)), replace=False)
            moved = pts[j] + (np.array([3.0, -2.0, 2.5]) * R).astype(F32)
            pts, lab = np.concatenate([pts, moved]).astype(F32), np.concatenate([lab, lab[j]])
        perm = rng.permutation(len(pts))
        obs = Observation(np.ascontiguousarray(pts[perm]), np.ascontiguousarray(lab[perm].astype(np.int32)), self)
        return obs

    # -- costs ------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def oracle_costs(self, stride, cost_type):
        return self.costs_of(stride, cost_type, self.poses, self.pose_model, self.pose_label)

    def costs_of(self, stride, cost_type, poses, pose_model, pose_label, colours=None):
        """(rc, oc, diff) of a pose batch of this case against the observation of the stride; pose_model may name
        models out of range (the expectation is an empty model's pose)."""
        o = self.observation(stride)
        c = CAM
        pm = self.oracle_models(pose_model)
        n = len(pm)
        tot0 = np.full(n, max(1.0, float(len(o.xyz))), F32)
        if cost_type == 1:
            return oracle.evaluate_colour(self.bank.tris, colours, self.oracle_count, poses, pm, self.width,
                                          self.height, self.proj, self.src_depth, 1.0, stride, c["cx"], c["cy"],
                                          c["fx"], c["fy"], 100.0, o.sorted_xyz, o.sorted_rgb, tot0, True, R,
                                          COLOUR_THR)
        six = cost_type == 2
        return oracle.evaluate(self.bank.tris, self.oracle_count, poses, pm, pose_label if six else None, self.width,
                               self.height, self.proj, self.src_depth, self.mask if six else None, 1.0, stride,
                               c["cx"], c["cy"], c["fx"], c["fy"], 100.0, o.sorted_xyz,
                               o.label_start if six else None, o.label_end if six else None,
                               o.totals(pose_label) if six else tot0, cost_type, True, R)

    @functools.lru_cache(maxsize=None)
    def oracle_colour_costs(self, stride, b):
        return self.costs_of(stride, 1, self.poses, self.pose_model, None, colours=self.bank.colouring(b))


class Observation:
    """The observed cloud in the order in which it is given (xyz, label, rgb) and label-sorted, as the oracle takes
    it (sorted_xyz, ...)."""

    def __init__(self, xyz, label, case):
        self.xyz, self.label = xyz, label
        self.rgb = np.ascontiguousarray(np.tile(COLOUR_B, (len(xyz), 1)))
        order = np.argsort(label, kind="stable")
        self.sorted_xyz = np.ascontiguousarray(xyz[order])
        self.sorted_rgb = np.ascontiguousarray(self.rgb[order])
        lab = label[order]
        self.num_labels = case.bank.K
        self.label_start = np.array([np.searchsorted(lab, L, "left") for L in range(self.num_labels)], np.int32)
        self.label_end = np.array([np.searchsorted(lab, L, "right") for L in range(self.num_labels)], np.int32)
        for a in (self.xyz, self.label, self.rgb, self.sorted_xyz, self.sorted_rgb):
            a.setflags(write=False)

    def totals(self, pose_label):
        cnt = (self.label_end - self.label_start).astype(F32)
        pl = np.asarray(pose_label)
        ok = (pl >= 0) & (pl < self.num_labels)
        return np.maximum(np.where(ok, cnt[np.clip(pl, 0, self.num_labels - 1)], 0), 1).astype(F32)

    def totals0(self, n):
        return np.full(n, max(1.0, float(len(self.xyz))), F32)


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """A case of the table, built once per process; no test changes it."""
    return MeshCase(name)
