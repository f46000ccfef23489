"""Shared scene builders for the CPU and GPU tests (oracle = checker only)."""
from __future__ import annotations

import functools

import numpy as np

import oracle
from perception_amd import synthetic as syn
from perception_amd.model import init_from_eigen_batch


def oracle_render_fn(tris, cnt, p16, pm, W, H, proj):
    return oracle.render_depth(tris, cnt, p16, pm, None, W, H, proj, np.zeros((H, W), np.int32), None, 1.0)


class SceneCase:
    """A scene + candidate poses + the label-sorted observed cloud, built with the oracle."""

    def __init__(self, names=("003_cracker_box",), n_poses=64, cam=None, stride=8, seed=syn.SEED, k=32,
                 gt_centers=None):
        rng = np.random.default_rng(seed)
        cam = cam or syn.CAM_640
        K = len(names)
        centers = gt_centers or [(0.03 + 0.12 * (i - (K - 1) / 2), -0.02, 0.80 + 0.05 * i) for i in range(K)]
        gts = np.stack([syn.default_gt_pose(rng, c) for c in centers])
        self.scene = syn.make_scene(list(names), gts, oracle_render_fn, cam=cam, rng=rng, k=k)
        sc = self.scene
        self.stride = stride
        xyz, _, lab = oracle.depth_to_cloud(sc.depth_raw, stride, sc.cx, sc.cy, sc.fx, sc.fy, sc.depth_factor,
                                            label_mask=sc.mask)
        self.obs_xyz_raw, self.obs_label_raw = xyz, lab
        order = np.argsort(lab, kind="stable")
        self.obs_xyz = xyz[order]
        self.obs_label = lab[order]
        nl = int(lab.max()) + 1 if len(lab) else 0
        self.label_start = np.array([np.searchsorted(self.obs_label, L, "left") for L in range(nl)], np.int32)
        self.label_end = np.array([np.searchsorted(self.obs_label, L, "right") for L in range(nl)], np.int32)
        seg_count = np.bincount(lab, minlength=max(nl, K)).astype(np.float32)
        poses = []
        models = []
        for obj in range(K):
            P = syn.candidate_poses(gts[obj][:3, 3], n_poses, rng, include=gts[obj])
            poses.append(P)
            models.append(np.full(len(P), obj, np.int32))
        self.poses44 = np.concatenate(poses)
        self.poses = init_from_eigen_batch(self.poses44)
        self.pose_model = np.concatenate(models)
        self.pose_label = self.pose_model.copy()
        self.pose_obs_total = seg_count[self.pose_label]
        self.K = K

    def oracle_costs(self, cost_type=2, sensor_resolution=0.01, occlusion_threshold=1.0, nthreads=0):
        sc = self.scene
        six = cost_type == 2
        return oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, self.poses, self.pose_model,
                               self.pose_label if six else None, sc.width, sc.height, sc.proj, sc.src_depth_cm,
                               sc.mask if six else None, occlusion_threshold, self.stride, sc.cx, sc.cy, sc.fx,
                               sc.fy, 100.0, self.obs_xyz, self.label_start if six else None,
                               self.label_end if six else None,
                               self.pose_obs_total if six else np.full(len(self.poses), len(self.obs_xyz), np.float32),
                               cost_type, True, sensor_resolution, nthreads=nthreads)


def label_covs(case, six=True):
    """Target covariances of a case's observed cloud as evaluate_icp takes them: per label segment (6-DoF) or over
    the whole cloud (3-DoF)."""
    if not six:
        return oracle.covariances(case.obs_xyz)
    cov = np.zeros((len(case.obs_xyz), 6))
    for L in range(len(case.label_start)):
        a, b = case.label_start[L], case.label_end[L]
        if b > a:
            cov[a:b] = oracle.covariances(case.obs_xyz[a:b])
    return cov


def oracle_recognizer_pipeline(rec, inp, sc, icp):
    """The oracle's side of ObjectRecognizer.localize_objects_greedy_render on the recognizer's own candidate states
    (after set_input): stage COST (with GICP when icp) and the selection.  -> (adjusted poses (N, 16), best cost and
    best index per model)."""
    K = len(inp.model_names)
    p = rec.params
    states = rec.generate_successor_states(inp)
    mats = rec._pose_in_cam(states)
    pm = np.array([s[0] for s in states], np.int32)
    pl = np.array([s[1] for s in states], np.int32)
    xyz, lab = rec.obs_xyz_host, rec.obs_label_host
    order = np.argsort(lab, kind="stable")
    oxyz, olab = xyz[order], lab[order]
    ls = np.array([np.searchsorted(olab, L, "left") for L in range(K)], np.int32)
    le = np.array([np.searchsorted(olab, L, "right") for L in range(K)], np.int32)
    tot = rec.segmented_count[pl]
    src = sc.src_depth_cm
    if icp:
        ocov = np.zeros((len(oxyz), 6))
        for L in range(K):
            ocov[ls[L]:le[L]] = oracle.covariances(oxyz[ls[L]:le[L]])
        adj, _, rc, oc, df = oracle.evaluate_icp(sc.bank.tris, sc.bank.tris_model_count, mats, pm, pl, sc.width,
                                                 sc.height, sc.proj, src, sc.mask, 1.0, p.gpu_stride, sc.cx, sc.cy,
                                                 sc.fx, sc.fy, 100.0, oxyz, ocov, ls, le, tot, 2, True,
                                                 p.sensor_resolution)
    else:
        rc, oc, df = oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, mats, pm, pl, sc.width, sc.height,
                                     sc.proj, src, sc.mask, 1.0, p.gpu_stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0, oxyz,
                                     ls, le, tot, 2, True, p.sensor_resolution)
        adj = mats
    bc, bi = oracle.select(rc, oc, pm, K)
    return adj, bc, bi


def grid_clouds(cam, s):
    """Clouds unprojected from a stride-s sample grid of the camera (what render_cloud writes): tilted planes, a step
    (a depth discontinuity inside the neighbourhoods), 24 to 1,000 points -- the last one's window (40 x 25 cells) is
    larger than the covariance kernel's LDS map, which sends it to the brute force."""
    rng = np.random.default_rng(9)
    clouds = []
    for (w, h, x0, y0) in ((12, 10, 30, 20), (23, 20, 10, 5), (8, 3, 50, 40), (27, 17, 3, 30), (40, 25, 20, 10)):
        assert (x0 + w) * s <= cam["width"] and (y0 + h - 1) * s < cam["height"]
        kx, ky = np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h))
        u, v = kx * s, ky * s
        z = 0.8 + 0.0004 * (u - cam["cx"]) + 0.0003 * (v - cam["cy"]) + rng.normal(size=u.shape) * 1e-3
        if w == 27:
            z = np.where(kx > x0 + 13, z + 0.05, z)  # a step: the far side's neighbourhoods reach across it
        z = np.round(z * 100) / 100  # the int-centimetre z-buffer's depths
        x = ((u.astype(np.float32) - np.float32(cam["cx"])) / np.float32(cam["fx"]) * z.astype(np.float32))
        y = ((v.astype(np.float32) - np.float32(cam["cy"])) / np.float32(cam["fy"]) * z.astype(np.float32))
        clouds.append(np.stack([x, y, z.astype(np.float32)], -1).reshape(-1, 3).astype(np.float32))
    return clouds


# ---------------------------------------------------------------------------------------------
# Geometry cases: generic sample strides, non-square cameras, H % stride != 0
# (tests/test_geometry_cases.py certifies them on the oracle; tests/test_gpu_geometry.py runs them on the GPU)
# ---------------------------------------------------------------------------------------------

# the reference's roman_camera_config.yaml and camera_config.yaml (Kinect 2 block); two synthetic small cameras
ROMAN_640 = dict(width=640, height=480, fx=619.274, fy=619.361, cx=324.285, cy=238.717)
KINECT2 = dict(width=512, height=424, fx=354.76029132272464, fy=354.49153515383603, cx=253.06754087288363,
               cy=205.37746288838397)
SMALL = dict(width=200, height=150, fx=180.0, fy=181.5, cx=101.3, cy=73.9)
TINY = dict(width=96, height=72, fx=88.0, fy=89.25, cx=47.6, cy=35.2)
# The focal lengths above differ by 1e-4 to 1.4e-2 of their value: fx used where fy belongs moves a point by less than
# the sensor radius and shows only in borderline costs.  With fy = 4/3 fx it moves every point by centimetres.
ANISO = dict(width=200, height=150, fx=180.0, fy=240.0, cx=101.3, cy=73.9)
GEOMETRY_CAMERAS = {"ROMAN_640": ROMAN_640, "KINECT2": KINECT2, "SMALL": SMALL, "TINY": TINY, "ANISO": ANISO}

GEOMETRY_CASES = [("ROMAN_640", 4), ("ROMAN_640", 5), ("ROMAN_640", 20), ("ROMAN_640", 32),
                  ("KINECT2", 4), ("KINECT2", 16), ("KINECT2", 32),
                  ("SMALL", 2), ("SMALL", 4), ("SMALL", 8), ("SMALL", 10), ("SMALL", 25),
                  ("TINY", 1), ("TINY", 3), ("TINY", 16), ("TINY", 32)]
GEOMETRY_ANISO_CASES = [("ANISO", 5), ("ANISO", 8)]  # the generic kernels and the stride-8 ones (150 % 8 = 6)
GEOMETRY_TIER_CASES = [("ROMAN_640", 5), ("SMALL", 4)]
GEOMETRY_GICP_CASES = [("ROMAN_640", 5), ("ROMAN_640", 4), ("KINECT2", 16), ("SMALL", 8), ("TINY", 3)]
GEOMETRY_GICP_POSES = 64  # the first poses of a case: both objects' candidates (32 + 32)
# Poses of the GICP batch that run into the 150-iteration cap, at least (tests/test_geometry_cases.py asserts it on
# the oracle).  SMALL at stride 8 gives 3 of its 64 (61 converge earlier): its clouds of ~20 points settle quickly.
GEOMETRY_GICP_MIN_CAPPED = {("SMALL", 8): 3}
GEOMETRY_NAMES = ("003_cracker_box", "005_tomato_soup_can")


def case_id(cs):
    return f"{cs[0]}-s{cs[1]}"


def _centre_at(cam, u, v, z):
    """The camera-frame point at depth z (metres) that projects to pixel (u, v)."""
    return ((u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z)


def _posed(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


class GeometryCase:
    """One (camera, stride) case: a two-object scene whose objects are centred on sample pixels next to two corners of
    the image -- the cracker box reaches over the first sample row and column, the soup can over the last ones (the
    last row is the one that exists only because of the ceil when H % stride != 0) -- with SceneCase's candidate poses
    (the first 2 * n_poses) and a hand-made list of border and edge poses appended to them.

    border: object centres on the four image borders (straddling them), on the first / last sample row and column,
            and one in the middle of the image;
    edge:   behind the camera, straddling z = 0, out of view, and so close that the window is the whole image."""

    EDGE_KINDS = ("behind", "straddle_z0", "out_of_view", "very_close")

    def __init__(self, cam_name, stride, n_poses=32):
        cam = GEOMETRY_CAMERAS[cam_name]
        s = stride
        W, H = cam["width"], cam["height"]
        assert W % s == 0
        ws, hs = W // s, (H + s - 1) // s
        self.cam_name, self.cam, self.stride, self.ws, self.hs = cam_name, cam, s, ws, hs
        # the cracker box over the first sample row and column, the soup can over the last ones
        kxa, kya = round(0.06 * ws), round(0.06 * hs)
        kxb, kyb = ws - 1 - round(0.03 * ws), hs - 1 - round(0.03 * hs)
        centres = [_centre_at(cam, kxa * s, kya * s, 0.72), _centre_at(cam, kxb * s, kyb * s, 0.62)]
        base = SceneCase(GEOMETRY_NAMES, n_poses=n_poses, cam=cam, stride=s, gt_centers=centres)
        self.base, self.scene = base, base.scene
        self.obs_xyz, self.obs_label = base.obs_xyz, base.obs_label
        self.obs_xyz_raw, self.obs_label_raw = base.obs_xyz_raw, base.obs_label_raw
        self.label_start, self.label_end = base.label_start, base.label_end
        self.K = base.K

        tilt = syn._rot_align_z(np.array([0.3, -0.4, 1.0]))
        xr, yb = (ws - 1) * s, (hs - 1) * s  # the last sample column / row
        xm, ym = (ws // 2) * s, (hs // 2) * s
        border = [
            _posed(tilt @ syn._rot_z(0.7), _centre_at(cam, 0, 0, 0.50)),            # first row and column (corner)
            _posed(tilt @ syn._rot_z(0.2), _centre_at(cam, 0, ym, 0.55)),           # left border
            _posed(tilt @ syn._rot_z(1.1), _centre_at(cam, xm, 0, 0.55)),           # top border
            _posed(tilt @ syn._rot_z(0.4), _centre_at(cam, W - 1, ym, 0.50)),       # right border
            _posed(tilt @ syn._rot_z(1.9), _centre_at(cam, xm, H - 1, 0.50)),       # bottom border
            _posed(tilt @ syn._rot_z(0.9), _centre_at(cam, xr, ym, 0.48)),          # last sample column
            _posed(tilt @ syn._rot_z(2.3), _centre_at(cam, xm, yb, 0.48)),          # last sample row
            _posed(tilt @ syn._rot_z(0.0), _centre_at(cam, xr, yb, 0.52)),          # last row and column (corner)
            _posed(syn._rot_z(0.5), _centre_at(cam, (ws // 4) * s, yb, 0.60)),      # last sample row, face-on
            _posed(tilt @ syn._rot_z(1.4), _centre_at(cam, xm, ym, 0.55)),          # the middle of the image
        ]
        rot_y = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
        edge = [
            _posed(np.eye(3), (0.0, 0.0, -0.5)),          # behind the camera
            _posed(np.eye(3), (0.0, 0.0, 0.02)),          # straddling z = 0
            _posed(np.eye(3), (2.0, 0.0, 0.8)),           # out of view
            _posed(syn._rot_z(0.1) @ rot_y, (0.0, 0.0, 0.14)),  # very close, large face on: a whole-image window
        ]
        extra = np.stack(border + edge)
        n0 = len(base.poses)
        self.border_idx = np.arange(n0, n0 + len(border))
        self.edge_idx = dict(zip(self.EDGE_KINDS, range(n0 + len(border), n0 + len(extra))))
        em = (np.arange(len(extra)) % 2).astype(np.int32)  # alternate the two models (the cracker box first)
        em[len(border):] = 0
        seg_count = np.bincount(base.obs_label_raw, minlength=base.K).astype(np.float32)
        self.poses44 = np.concatenate([base.poses44, extra])
        self.poses = np.concatenate([base.poses, init_from_eigen_batch(extra)])
        self.pose_model = np.concatenate([base.pose_model, em])
        self.pose_label = self.pose_model.copy()
        self.pose_obs_total = np.concatenate([base.pose_obs_total, seg_count[em]])
        self.n = len(self.poses)

    # -- the oracle's side ------------------------------------------------------------------------
    def oracle_costs(self, cost_type=2, stride=None, sensor_resolution=0.01, occlusion_threshold=1.0):
        """(rc, oc, diff) of every pose; `stride` samples the renders at another stride than the case's (the observed
        cloud stays the case's)."""
        sc = self.scene
        six = cost_type == 2
        tot = self.pose_obs_total if six else np.full(self.n, len(self.obs_xyz), np.float32)
        return oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, self.poses, self.pose_model,
                               self.pose_label if six else None, sc.width, sc.height, sc.proj, sc.src_depth_cm,
                               sc.mask if six else None, occlusion_threshold, stride or self.stride, sc.cx, sc.cy,
                               sc.fx, sc.fy, 100.0, self.obs_xyz, self.label_start if six else None,
                               self.label_end if six else None, tot, cost_type, True, sensor_resolution)

    def oracle_render(self, labels=True):
        sc = self.scene
        return oracle.render_depth(sc.bank.tris, sc.bank.tris_model_count, self.poses, self.pose_model,
                                   self.pose_label if labels else None, sc.width, sc.height, sc.proj, sc.src_depth_cm,
                                   sc.mask if labels else None, 1.0)

    def oracle_icp(self, n=GEOMETRY_GICP_POSES):
        sc = self.scene
        return oracle.evaluate_icp(
            sc.bank.tris, sc.bank.tris_model_count, self.poses[:n], self.pose_model[:n], self.pose_label[:n],
            sc.width, sc.height, sc.proj, sc.src_depth_cm, sc.mask, 1.0, self.stride, sc.cx, sc.cy, sc.fx, sc.fy,
            100.0, self.obs_xyz, label_covs(self), self.label_start, self.label_end, self.pose_obs_total[:n], 2, True,
            0.01)


@functools.lru_cache(maxsize=None)
def geometry_case(cam_name, stride):
    """The case of the table, built once per process (neither test module changes it)."""
    return GeometryCase(cam_name, stride)
