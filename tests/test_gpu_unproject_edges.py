"""Edge cases of the unprojection (float)Z / depth_factor, (kx s - cx) / fx, (ky s - cy) / fy in fused_cost_kernel
(phase 2) and render_cloud_kernel, bit for bit against the CPU oracle: small cameras with an integral principal point,
so the two numerators are exactly zero on one sample column and one sample row that the object covers, at strides 1, 3
and 8; and one focal length and one depth factor outside [2^-40, 2^41), the exponent range in which pcore_fdiv.h's
unscaled division steps equal the IEEE quotient (every f32 `a / b` of these expressions must keep IEEE semantics there).

The camera is 64 x 48 (cx 32, cy 24) for strides 1 and 8.  A stride has to divide the width (pcore_evaluate rejects it
otherwise), so stride 3 runs on 63 x 48 with cx 30, cy 24.  24 poses of a smallest proxy (025_mug: the cylinders have the fewest triangles)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd.core import PoseCore
from tests.helpers import SceneCase

pytestmark = pytest.mark.gpu

CAM64 = dict(width=64, height=48, fx=58.0, fy=58.5, cx=32.0, cy=24.0)
CAM63 = dict(width=63, height=48, fx=58.0, fy=58.5, cx=30.0, cy=24.0)
NAME = "025_mug"  # 4,992 triangles (the cylinders are the smallest proxies); wide enough for three stride-8 columns
N_POSES = 24

# (id, camera, stride, unprojection fx or None for the camera's, evaluate's depth_factor)
CASES = [
    ("s1", CAM64, 1, None, 100.0),
    ("s3", CAM63, 3, None, 100.0),
    ("s8", CAM64, 8, None, 100.0),
    ("s8-fx-2p42", CAM64, 8, 2.0 ** 42, 100.0),          # fx above the range: every x quotient through IEEE division
    ("s1-df-2m41", CAM64, 1, None, 2.0 ** -41),          # depth_factor below the range
]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Case:
    def __init__(self, cam, stride, fx, depth_factor):
        base = SceneCase((NAME,), n_poses=N_POSES, cam=cam, stride=stride, gt_centers=[(0.0, 0.0, 0.20)])
        sc = base.scene
        self.base, self.sc, self.stride = base, sc, stride
        self.fx = float(sc.fx if fx is None else fx)
        self.depth_factor = float(depth_factor)
        # the observed cloud with the unprojection's focal length, label-sorted as SceneCase does
        xyz, _, lab = oracle.depth_to_cloud(sc.depth_raw, stride, sc.cx, sc.cy, self.fx, sc.fy, sc.depth_factor,
                                            label_mask=sc.mask)
        order = np.argsort(lab, kind="stable")
        self.obs_xyz_raw, self.obs_lab_raw = xyz, lab
        self.obs_xyz, obs_lab = xyz[order], lab[order]
        nl = int(lab.max()) + 1
        self.label_start = np.array([np.searchsorted(obs_lab, L, "left") for L in range(nl)], np.int32)
        self.label_end = np.array([np.searchsorted(obs_lab, L, "right") for L in range(nl)], np.int32)
        # the oracle's side, once
        self.z_full = oracle.render_depth(sc.bank.tris, sc.bank.tris_model_count, base.poses, base.pose_model,
                                          base.pose_label, sc.width, sc.height, sc.proj, sc.src_depth_cm, sc.mask, 1.0)
        self.costs = oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, base.poses, base.pose_model,
                                     base.pose_label, sc.width, sc.height, sc.proj, sc.src_depth_cm, sc.mask, 1.0,
                                     stride, sc.cx, sc.cy, self.fx, sc.fy, self.depth_factor, self.obs_xyz,
                                     self.label_start, self.label_end, base.pose_obs_total, 2, True, 0.01)
        self.cloud = oracle.depth_to_cloud(self.z_full, stride, sc.cx, sc.cy, self.fx, sc.fy, self.depth_factor,
                                           pose_label=base.pose_label)


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def edge(request):
    _, cam, stride, fx, df = request.param
    case = _Case(cam, stride, fx, df)
    sc, base = case.sc, case.base
    dev = torch.device("cuda", 0)
    core = PoseCore(0)
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, case.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    mask = torch.from_numpy(sc.mask).to(dev)
    xyz, lab = core.observed_cloud(torch.from_numpy(sc.depth_raw).to(dev), mask, stride, sc.depth_factor)
    core.set_observation(torch.from_numpy(sc.src_depth_cm).to(dev), mask, xyz, lab, 0.01)
    t = {"poses": torch.from_numpy(base.poses).to(dev), "pm": torch.from_numpy(base.pose_model).to(dev),
         "pl": torch.from_numpy(base.pose_label).to(dev), "tot": torch.from_numpy(base.pose_obs_total).to(dev),
         "obs_xyz": xyz, "obs_lab": lab}
    yield case, core, t
    core.close()


def test_case_is_not_vacuous(edge):
    """Valid samples lie on the column kx s == cx and on the row ky s == cy (zero numerators), and off them."""
    case, _, t = edge
    sc, s = case.sc, case.stride
    zs = case.z_full[:, ::s, ::s]
    assert sc.cx % s == 0 and sc.cy % s == 0 and sc.width % s == 0
    assert (zs[:, :, int(sc.cx) // s] > 0).any() and (zs[:, int(sc.cy) // s, :] > 0).any()
    assert (zs > 0).sum() > (zs[:, :, int(sc.cx) // s] > 0).sum() + (zs[:, int(sc.cy) // s, :] > 0).sum()
    x0 = case.cloud[0][:, 0]
    assert (x0 == 0.0).any() and (case.cloud[0][:, 1] == 0.0).any()  # the quotients that are exactly zero
    assert np.array_equal(_bits(t["obs_xyz"].cpu().numpy()), _bits(case.obs_xyz_raw))


def test_costs_and_z_samples_equal_the_oracle(edge):
    case, core, t = edge
    s = case.stride
    hs, ws = (case.sc.height + s - 1) // s, case.sc.width // s
    dbg = torch.full((len(case.base.poses), hs, ws), -7, dtype=torch.int32, device=t["poses"].device)
    rc, oc, df = core.evaluate(t["poses"], t["pm"], t["pl"], t["tot"], cost_type=2, stride=s,
                               depth_factor=case.depth_factor, dbg_zs=dbg)
    torch.cuda.synchronize()
    assert np.array_equal(dbg.cpu().numpy(), case.z_full[:, ::s, ::s])
    for got, want, what in zip((rc, oc, df), case.costs, ("rendered", "observed", "diff")):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), what
    assert (case.costs[0] >= 0.0).any()  # poses with rendered points


def test_render_cloud_kernel_clouds_equal_the_oracle(edge):
    case, core, t = edge
    xyzw, cnt = core.render_clouds(t["poses"], t["pm"], t["pl"], stride=case.stride, depth_factor=case.depth_factor)
    torch.cuda.synchronize()
    xyzw, cnt = xyzw.cpu().numpy(), cnt.cpu().numpy()
    oxyz, opose, _ = case.cloud
    assert np.array_equal(cnt, np.bincount(opose, minlength=len(cnt)))
    assert cnt.sum() > 0
    got = np.concatenate([xyzw[i, :cnt[i], :3] for i in range(len(cnt))])
    assert np.array_equal(_bits(got), _bits(oxyz))
    assert (xyzw[..., 3] == 0.0).all()
