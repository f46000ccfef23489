"""Scenes for a context that lives across requests: one PoseCore is given scene after scene (another mesh bank, another
camera, another observation) and must score each as a fresh context would.

Three small scenes and the orders in which the tests walk them:

  A  three objects on the SMALL camera at stride 4: 3 models, 3 label segments;
  B  one wood block on the same camera (the same image size), in front of A's cracker box: 1 model, 1 segment;
  C  the same block on the TINY camera at stride 3 with another sensor resolution: a smaller image;
  F  scene B seen by a camera that differs from SMALL in fx alone.

  SEQUENCES: A -> B -> C -> A, and C -> A -> B on a fresh context, so that every buffer both shrinks and grows as
  a first transition.

Everything here is built on the CPU with numpy and the oracle.  tests/test_context_reuse_cases.py certifies, from the
oracle alone, that every kind of state a context could wrongly keep from the previous scene changes the costs of the
next one; tests/test_gpu_context_reuse.py walks the sequences on the GPU, bit for bit against the references computed
here (once per process; no test changes them).

In B, C and F a few poses are appended whose label is 1 or 2: segments that A has and they have not.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
from perception_amd import synthetic as syn
from perception_amd.model import init_from_eigen_batch
from tests import icp2d_reference as ref2d
from tests import p2p_reference as refp
from tests import topk_reference as reft
from tests.helpers import SMALL, TINY, SceneCase, label_covs

F32 = np.float32
SMALL_FX = dict(SMALL, fx=186.0)  # SMALL but for fx
A_NAMES = ("003_cracker_box", "005_tomato_soup_can", "004_sugar_box")
SCENES = {
    # names, camera, stride, mesh k, centres, seed, poses per object, sensor resolution
    "A": (A_NAMES, SMALL, 4, 8, [(-0.10, -0.02, 0.55), (0.02, 0.0, 0.50), (0.12, 0.02, 0.60)], syn.SEED, 24, 0.01),
    "B": (("036_wood_block",), SMALL, 4, 6, [(-0.08, -0.01, 0.52)], 7, 40, 0.01),
    "C": (("036_wood_block",), TINY, 3, 6, [(-0.03, -0.01, 0.40)], 7, 40, 0.0075),
    "F": (("036_wood_block",), SMALL_FX, 4, 6, [(-0.08, -0.01, 0.52)], 7, 40, 0.01),
}
SEQUENCES = (("A", "B", "C", "A"), ("C", "A", "B"))
TRANSITIONS = tuple(sorted({(s[i], s[i + 1]) for s in SEQUENCES for i in range(len(s) - 1)}))
MAX_LABELS = 3          # the largest label count of any scene
EMPTY_LABELS = (1, 2)   # labels of A that B, C and F do not have
N_EMPTY = 4             # poses appended per such label
COLOUR_THR = 15.0
COLOUR_BASE = np.array((120, 130, 110))  # as tests/nn_cases.py: about a third of the random pairs within the gate
COLOUR_SPREAD = 40
ICP_POSES = 36
PLANAR_POSES = 24
P2P_POSES = 16
RENDER_POSES = 8
TOPK = 16
# two rigid world frames and two radii for the planar ICP
PLANAR_M = (np.array([[0.0, 0.0, 1.0, 0.1], [-1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.9], [0.0, 0.0, 0.0, 1.0]], F32),
            np.array([[0.6, 0.0, 0.8, -0.2], [-0.8, 0.0, 0.6, 0.05], [0.0, -1.0, 0.0, 0.7], [0.0, 0.0, 0.0, 1.0]], F32))
PLANAR_R = (0.05, 0.03)


def _random_rgb(rng, n):
    return (COLOUR_BASE[None, :] + rng.integers(-COLOUR_SPREAD, COLOUR_SPREAD + 1, (n, 3))).astype(np.uint8)


def _spread(n, m):
    """m of n indices, evenly spread."""
    return np.unique(np.linspace(0, n - 1, m).astype(np.int64))


class ContextScene:
    """A SceneCase with a colour per triangle and per observed point, the poses of labels the scene does not have,
    and the CPU references of every call the GPU test makes."""

    def __init__(self, name):
        names, cam, stride, k, centres, seed, n_poses, res = SCENES[name]
        self.name, self.cam, self.stride, self.res = name, cam, stride, res
        case = SceneCase(names, n_poses=n_poses, cam=cam, stride=stride, seed=seed, k=k, gt_centers=centres)
        self.case, self.scene = case, case.scene
        sc = case.scene
        rng = np.random.default_rng(1000 + sorted(SCENES).index(name))
        for m in sc.bank.models:
            m.colors = _random_rgb(rng, m.tris.shape[0])
        self.obs_rgb_raw = _random_rgb(rng, len(case.obs_xyz_raw))  # in the order of the cloud as unprojected
        self.order = np.argsort(case.obs_label_raw, kind="stable")
        self.obs_rgb = np.ascontiguousarray(self.obs_rgb_raw[self.order])  # label-sorted, as the oracle takes them
        self.num_labels = len(case.label_start)
        self.seg_counts = (case.label_end - case.label_start).astype(np.int64)
        self.n_base = len(case.poses)
        base = case.poses
        if len(names) == 1:
            # SceneCase's 40 poses of one object all lie 10 cm in front of it, where no source depth occludes them and
            # few of their points are within the sensor resolution of an observed one: every second pose moves along
            # the viewing ray to the object's depth and up to 6 cm behind it (the ground truth, at an odd index, stays)
            P = case.poses44.copy()
            ray = np.asarray(centres[0]) / np.linalg.norm(centres[0])
            even = np.arange(0, self.n_base, 2)
            P[even, :3, 3] += ray[None, :] * np.linspace(0.09, 0.16, len(even))[:, None]
            base = init_from_eigen_batch(P)
        poses, pm, pl, tot = [base], [case.pose_model], [case.pose_label], [case.pose_obs_total]
        if self.num_labels < MAX_LABELS:
            # the object in its ground-truth rotation where A's object of that label stands, at four depths: with A's
            # segment table still in place these poses would find A's points
            a_centres = SCENES["A"][4]
            for L in EMPTY_LABELS:
                pick = np.full(N_EMPTY, self.n_base // 3)
                P = case.poses44[pick].copy()
                ray = np.asarray(a_centres[L]) / np.linalg.norm(a_centres[L])
                P[:, :3, 3] = np.asarray(a_centres[L])[None, :] + ray[None, :] * np.linspace(-0.03, 0.03, N_EMPTY)[:, None]
                poses.append(init_from_eigen_batch(P))
                pm.append(case.pose_model[pick])
                pl.append(np.full(N_EMPTY, L, np.int32))
                tot.append(np.ones(N_EMPTY, F32))
        self.poses = np.ascontiguousarray(np.concatenate(poses))
        self.pose_model = np.concatenate(pm).astype(np.int32)
        self.pose_label = np.concatenate(pl).astype(np.int32)
        self.pose_obs_total = np.concatenate(tot).astype(F32)
        self.n = len(self.poses)
        self.pose_obs_total0 = np.full(self.n, float(len(case.obs_xyz)), F32)
        self.empty_idx = np.arange(self.n_base, self.n)
        # the batches of the refinements: spread over the objects, the empty-label poses at the end
        self.icp_idx = np.concatenate([_spread(self.n_base, ICP_POSES - len(self.empty_idx)), self.empty_idx])
        self.planar_idx = _spread(self.n_base, PLANAR_POSES)
        self.p2p_idx = np.concatenate([_spread(self.n_base, P2P_POSES - len(self.empty_idx[:2])), self.empty_idx[:2]])
        self.render_idx = np.concatenate([_spread(self.n_base, RENDER_POSES - len(self.empty_idx[:1])),
                                          self.empty_idx[:1]])

    # -- what the scene sizes ---------------------------------------------------------------------
    @property
    def shape(self):
        sc = self.scene
        return dict(labels=self.num_labels, seg=tuple(int(c) for c in self.seg_counts),
                    num_obs=len(self.case.obs_xyz), tris=int(sc.bank.tris.shape[0]),
                    models=len(sc.bank.tris_model_count), image=(sc.width, sc.height),
                    bitmap_words=max(1, (max(int(self.seg_counts.max()), len(self.case.obs_xyz)) + 31) // 32))

    # -- the oracle, with any part of the observation replaced (the certificate's stale states) ----
    def costs(self, cost_type, cloud=None, src=None, rgb=None):
        """(rc, oc, diff) of every pose.  cloud: the ContextScene whose observed cloud and segments are used; src: an
        (H, W) source depth, or a ContextScene for its source depth and mask; rgb: label-sorted observed colours."""
        sc, case = self.scene, self.case
        cl = (cloud or self).case
        depth, mask = sc.src_depth_cm, sc.mask
        if isinstance(src, ContextScene):
            depth, mask = src.scene.src_depth_cm, src.scene.mask
        elif src is not None:
            depth, mask = src
        if cost_type == 1:
            tot = np.full(self.n, float(len(cl.obs_xyz)), F32)
            return oracle.evaluate_colour(sc.bank.tris, sc.bank.colors, sc.bank.tris_model_count, self.poses,
                                          self.pose_model, sc.width, sc.height, sc.proj, depth, 1.0, self.stride,
                                          sc.cx, sc.cy, sc.fx, sc.fy, 100.0, cl.obs_xyz,
                                          self.obs_rgb if rgb is None else rgb, tot, True, self.res, COLOUR_THR)
        six = cost_type == 2
        tot = self.pose_obs_total if six else np.full(self.n, float(len(cl.obs_xyz)), F32)
        return oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, self.poses, self.pose_model,
                               self.pose_label if six else None, sc.width, sc.height, sc.proj, depth,
                               mask if six else None, 1.0, self.stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0, cl.obs_xyz,
                               cl.label_start if six else None, cl.label_end if six else None, tot, cost_type, True,
                               self.res)

    def covs(self, six, k):
        if k == oracle.GICP_K:
            return label_covs(self.case, six)
        c = self.case
        if not six:
            return oracle.covariances(c.obs_xyz, k)
        cov = np.zeros((len(c.obs_xyz), 6))
        for a, b in zip(c.label_start, c.label_end):
            if b > a:
                cov[a:b] = oracle.covariances(c.obs_xyz[a:b], k)
        return cov

    def icp(self, six, k=oracle.GICP_K, cov=None):
        """oracle.evaluate_icp of the ICP batch: (adjusted poses, iterations, rc, oc, diff)."""
        sc, c, i = self.scene, self.case, self.icp_idx
        tot = self.pose_obs_total[i] if six else self.pose_obs_total0[i]
        return oracle.evaluate_icp(sc.bank.tris, sc.bank.tris_model_count, self.poses[i], self.pose_model[i],
                                   self.pose_label[i] if six else None, sc.width, sc.height, sc.proj, sc.src_depth_cm,
                                   sc.mask if six else None, 1.0, self.stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0,
                                   c.obs_xyz, self.covs(six, k) if cov is None else cov,
                                   c.label_start if six else None, c.label_end if six else None, tot,
                                   2 if six else 0, True, self.res, k=k)

    def clouds(self, idx, six):
        """The stride-sample clouds the ICP entry points render for the poses idx, from the oracle."""
        sc = self.scene
        zb = oracle.render_depth(sc.bank.tris, sc.bank.tris_model_count, self.poses[idx], self.pose_model[idx],
                                 self.pose_label[idx] if six else None, sc.width, sc.height, sc.proj,
                                 sc.src_depth_cm, sc.mask if six else None, 1.0)
        xyz, pidx, _ = oracle.depth_to_cloud(zb, self.stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0)
        return [xyz[pidx == i] for i in range(len(idx))]


@functools.lru_cache(maxsize=None)
def scene(name):
    """A scene of the table, built once per process; no test changes it."""
    return ContextScene(name)


# ---------------------------------------------------------------------------------------------
# references, computed once per process and left unchanged
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def want_costs(name, cost_type):
    return scene(name).costs(cost_type)


@functools.lru_cache(maxsize=None)
def want_icp(name, six, k=oracle.GICP_K):
    return scene(name).icp(six, k)


@functools.lru_cache(maxsize=None)
def want_planar(name, m, r):
    """(xform, iterations, status, mse) of the planar batch with world frame PLANAR_M[m] and radius PLANAR_R[r]; the
    observation in the order in which it is set (as unprojected)."""
    s = scene(name)
    out = ref2d.run_poses(s.clouds(s.planar_idx, False), s.case.obs_xyz_raw, PLANAR_M[m],
                          max_correspondence=PLANAR_R[r])
    return out[:4]


@functools.lru_cache(maxsize=None)
def want_scene(name):
    sc = scene(name).scene
    return oracle.ref_scene(sc.src_depth_cm, sc.fx, sc.fy, sc.cx, sc.cy)


@functools.lru_cache(maxsize=None)
def want_p2p(name):
    """evaluate_p2p of the p2p batch: (adjusted poses, iterations, rc, oc, diff, fitness, rmse)."""
    s = scene(name)
    sc, c, i = s.scene, s.case, s.p2p_idx
    pcd, nrm = want_scene(name)
    T, fit, rmse, its = refp.run_clouds(s.clouds(i, True), pcd, nrm, sc.fx, sc.fy, sc.cx, sc.cy)
    adj = np.stack([oracle.concat_pose(T[j].astype(np.float64), s.poses[p]) for j, p in enumerate(i)])
    rc, oc, df = oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, adj, s.pose_model[i], s.pose_label[i],
                                 sc.width, sc.height, sc.proj, sc.src_depth_cm, sc.mask, 1.0, s.stride, sc.cx, sc.cy,
                                 sc.fx, sc.fy, 100.0, c.obs_xyz, c.label_start, c.label_end, s.pose_obs_total[i], 2,
                                 True, s.res)
    return adj, its, rc, oc, df, fit, rmse


@functools.lru_cache(maxsize=None)
def want_render(name):
    """(depth (n, H, W), colour planes (3, n, H, W)) of the render batch, with the 6-DoF source occlusion."""
    s = scene(name)
    sc, i = s.scene, s.render_idx
    return oracle.render_depth_color(sc.bank.tris, sc.bank.colors, sc.bank.tris_model_count, s.poses[i],
                                     s.pose_model[i], s.pose_label[i], sc.width, sc.height, sc.proj, sc.src_depth_cm,
                                     sc.mask, 1.0)


def want_topk(name, index_base=0):
    s = scene(name)
    rc, oc, _ = want_costs(name, 2)
    return reft.topk(rc, oc, s.pose_model, len(s.scene.bank.tris_model_count), TOPK, index_base)


def count_queries(name):
    """Queries for count_within on scene `name`: centred on A's three segments (where a stale segment table would find
    points) and on the scene's own, with labels -1 .. MAX_LABELS.  -> (queries, labels, radius, expected counts)."""
    from tests.test_valid_pose import _pcl_counts

    s, a = scene(name), scene("A")
    rng = np.random.default_rng(40 + sorted(SCENES).index(name))
    centres = [a.case.obs_xyz[lo:hi].mean(0) for lo, hi in zip(a.case.label_start, a.case.label_end)]
    centres += [s.case.obs_xyz[lo:hi].mean(0) for lo, hi in zip(s.case.label_start, s.case.label_end)]
    n = 300
    q = (np.asarray(centres)[rng.integers(0, len(centres), n)] + rng.normal(scale=0.03, size=(n, 3))).astype(F32)
    lab = rng.integers(-1, MAX_LABELS + 1, n).astype(np.int32)
    lab[:MAX_LABELS] = np.arange(MAX_LABELS)
    q[:MAX_LABELS] = np.asarray(centres[:MAX_LABELS], F32)  # on A's segments, with A's labels
    radius = rng.choice([0.02, 0.0566, 0.11], n)
    want = np.zeros(n, np.int64)
    for L in range(s.num_labels):
        seg = s.case.obs_xyz[s.case.label_start[L]:s.case.label_end[L]]
        for r in np.unique(radius):
            sel = (lab == L) & (radius == r)
            if sel.any():
                want[sel] = _pcl_counts(q[sel], seg, r)
    return q, lab, radius, want


# ---------------------------------------------------------------------------------------------
# the stale states of a transition X -> Y (the certificate; the oracle alone)
# ---------------------------------------------------------------------------------------------

def kept_buffer(x, shape):
    """What a grow-only buffer that held the array x gives a reader of `shape`: x's leading elements in the new shape
    (x repeats where the new reader wants more than x holds: such a buffer would have been reallocated)."""
    return np.resize(np.ascontiguousarray(x), shape)


def stale_source(X, Y):
    """X's source depth and mask as Y's image reads them from the buffers X left."""
    shape = Y.scene.src_depth_cm.shape
    return kept_buffer(X.scene.src_depth_cm, shape), kept_buffer(X.scene.mask, shape)


def same_image(X, Y):
    return X.scene.src_depth_cm.shape == Y.scene.src_depth_cm.shape


def differing(a, b, n=None):
    """The poses whose rc or oc differ in their bits."""
    d = (a[0].view(np.uint32) != b[0].view(np.uint32)) | (a[1].view(np.uint32) != b[1].view(np.uint32))
    return int(d[:n].sum())
