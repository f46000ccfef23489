"""The composed-state contract ("Composed state") in numpy, on top of the oracle's per-pose
stage RENDER (oracle.render_depth_color, itself held to the reference's own kernels by the refk_* goldens).

With D_i, C_i pose i's own depth image and colour planes:
    depth[p]    = min of D_i[p] over the poses with D_i[p] != 0, else 0
    owner[p]    = the lowest i attaining it, else -1
    color[:, p] = C_owner[:, p], black without an owner
    visible[i]  = the pixels with owner == i
occlude=False renders every pose against an all-zero source (no black-out at all) and takes no labels."""
import numpy as np

import oracle


def per_pose(sc, tri_rgb, poses, pose_model, pose_label=None, occlude=True, occlusion_threshold=1.0):
    """(D (N, H, W) int32, C (3, N, H, W) uint8) of the poses, each alone, on scene `sc` (synthetic.Scene)."""
    n = len(poses)
    if n == 0:
        return np.zeros((0, sc.height, sc.width), np.int32), np.zeros((3, 0, sc.height, sc.width), np.uint8)
    if occlude:
        src, mask = sc.src_depth_cm, (sc.mask if pose_label is not None else None)
    else:
        assert pose_label is None, "labels are only read with occlude"
        src, mask = np.zeros((sc.height, sc.width), np.int32), None
    return oracle.render_depth_color(sc.bank.tris, tri_rgb, sc.bank.tris_model_count, poses, pose_model, pose_label,
                                     sc.width, sc.height, sc.proj, src, mask, occlusion_threshold)


def compose(D, C):
    """(depth (H, W) int32, color (3, H, W) uint8, owner (H, W) int32, visible (N,) int32) of per-pose images."""
    n, h, w = D.shape
    if n == 0:
        return (np.zeros((h, w), np.int32), np.zeros((3, h, w), np.uint8), np.full((h, w), -1, np.int32),
                np.zeros(0, np.int32))
    far = np.int64(1) << 40
    key = np.where(D != 0, D.astype(np.int64), far)
    owner = key.argmin(0).astype(np.int32)  # the first (lowest) index among equal minima
    dmin = key.min(0)
    none = dmin == far
    owner[none] = -1
    depth = np.where(none, 0, dmin).astype(np.int32)
    pick = np.maximum(owner, 0)[None, None]
    color = np.take_along_axis(C, np.broadcast_to(pick, (3, 1, h, w)), 1)[:, 0]
    color = np.where(none[None], 0, color).astype(np.uint8)
    visible = np.bincount(owner[~none], minlength=n).astype(np.int32)
    return depth, color, owner, visible


def render_scene(sc, tri_rgb, poses, pose_model, pose_label=None, occlude=True, occlusion_threshold=1.0):
    return compose(*per_pose(sc, tri_rgb, poses, pose_model, pose_label, occlude, occlusion_threshold))
