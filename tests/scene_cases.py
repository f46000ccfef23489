"""The pose sets of the composed-state tests (tests/test_scene_cases.py certifies them on the oracle,
tests/test_gpu_render_scene.py runs them on the GPU), on one three-object scene with random per-triangle colours:

  candidates  the scene's own 24 candidate poses, eight per object around its ground truth: nearly every covered pixel
              is reached by several poses at the same integer depth, so the owner rule decides everywhere;
  state       six poses: each object at its first candidate, g[m], then each object again behind the NEXT object's
              place (g[(m + 1) % 3]'s translation moved 3 cm sideways and 10 cm away from the camera): renders that the
              observed object in front of them occludes, so the source, and the labels, change the frame;
  lens        the state set with a seventh pose in its middle: the foam brick unrotated with its nearest face 3 mm from
              the camera's plane, over the right half of the image.  Its depth there is int(0.3 + 0.5) = 0, which its own
              z-buffer reads as "nothing": by the contract the pose is absent from those pixels and the poses behind it
              show, although a 0 wins every z-test against them.

Labels equal model ids; the occlusion threshold is 1.0."""
import functools

import numpy as np

from perception_amd.model import init_from_eigen_batch
from tests import scene_reference as ref
from tests.helpers import SceneCase

NAMES = ("003_cracker_box", "005_tomato_soup_can", "061_foam_brick")
THRESHOLD = 1.0
# (occlude, labels): the three ways a frame is composed
MODES = {"plain": (False, False), "threshold": (True, False), "labels": (True, True)}


class PoseSet:
    def __init__(self, poses44, pose_model):
        self.poses = init_from_eigen_batch(np.asarray(poses44))
        self.pose_model = np.ascontiguousarray(pose_model, np.int32)
        self.pose_label = self.pose_model.copy()
        self.n = len(self.poses)


@functools.lru_cache(maxsize=None)
def scene_case():
    """(SceneCase, tri_rgb (T, 3) uint8): built once per process and never changed."""
    case = SceneCase(NAMES, n_poses=8, seed=5)
    rgb = np.random.default_rng(55).integers(0, 256, (len(case.scene.bank.tris), 3), dtype=np.uint8)
    return case, rgb


@functools.lru_cache(maxsize=None)
def pose_set(name):
    case, _ = scene_case()
    if name == "candidates":
        return PoseSet(case.poses44, case.pose_model)
    g = [case.poses44[8 * m] for m in range(3)]
    moved = []
    for m in range(3):
        T = g[m].copy()
        T[:3, 3] = g[(m + 1) % 3][:3, 3] + np.array([0.03, 0.0, 0.10])
        moved.append(T)
    if name == "state":
        return PoseSet(np.stack(g + moved), np.array([0, 1, 2, 0, 1, 2], np.int32))
    assert name == "lens"
    sc = case.scene
    first = int(np.sum(sc.bank.tris_model_count[:2]))
    zmin = float(sc.bank.tris[first:].reshape(-1, 3)[:, 2].min())
    lens = np.eye(4)
    lens[:3, 3] = (0.025, 0.0, 0.003 - zmin)
    return PoseSet(np.stack(g + [lens] + moved), np.array([0, 1, 2, 2, 0, 1, 2], np.int32))


@functools.lru_cache(maxsize=None)
def per_pose(name, mode):
    """The oracle's (D, C) of every pose of a set alone, in the set's order (shared by the tests; read only)."""
    case, rgb = scene_case()
    ps = pose_set(name)
    occlude, labels = MODES[mode]
    D, C = ref.per_pose(case.scene, rgb, ps.poses, ps.pose_model, ps.pose_label if labels else None, occlude, THRESHOLD)
    D.setflags(write=False)
    C.setflags(write=False)
    return D, C


def expected(name, mode, order=None):
    """The contract's (depth, color, owner, visible) of a set, its poses taken in `order` (default: as they are)."""
    D, C = per_pose(name, mode)
    if order is not None:
        D, C = D[order], C[:, order]
    return ref.compose(D, C)
