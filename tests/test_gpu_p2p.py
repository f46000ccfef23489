"""GPU: the point-to-plane projective ICP (pcore_scene_projective, pcore_icp_point2plane, pcore_debug_p2p_clouds)
against the committed oracle (the scene) and the numpy restatement of its spec in wave order (tests/p2p_reference.py;
tests/test_p2p_spec.py holds that module to the oracle), bit for bit; batch independence; the pose composition and the
re-scoring; the recognizer's icp_type 4; the argument checks."""
import ctypes
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import _native, io, workloads
from perception_amd import synthetic as syn
from perception_amd.core import PoseCore, decode_keys
from perception_amd.model import matrix_to_quat_xyzw
from perception_amd.recognizer import (CameraIntrinsics, ModelMetaData, ObjectRecognizer, PerchParams,
                                       RecognitionInput)
from tests import p2p_reference as ref
from tests.helpers import TINY, geometry_case, oracle_render_fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _assert_same(got, want, what=""):
    T, fit, rmse, it = got
    wT, wfit, wrmse, wit = want
    assert np.array_equal(it, wit), f"{what} iterations differ at {np.nonzero(it != wit)[0][:8]}: {it[it != wit][:8]} " \
                                    f"!= {wit[it != wit][:8]}"
    assert ref.same_bits(fit, wfit), f"{what} fitness differs at {np.nonzero(fit != wfit)[0][:8]}"
    assert ref.same_bits(rmse, wrmse), f"{what} rmse differs at {np.nonzero(rmse != wrmse)[0][:8]}"
    assert ref.same_bits(T, wT), f"{what} T differs at rows {np.nonzero((T != wT).any(1))[0][:8]}"


# -- 1. the scene, bitwise against oracle.ref_scene ---------------------------------------------------------------

def _hand_depth(W, H, seed):
    """A tilted plane with noise, a step above the difference threshold, zeros, values >= 2000 and > 65535, negatives."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    d = np.round(90 + 0.9 * x + 0.6 * y + rng.integers(-3, 4, (H, W))).astype(np.int64)
    d[:, W // 2:] += 70                                    # a step above 50
    for v in (0, 0, 2000, 2500, 65535, 65536, 70000, -1, -40000, 1999, 2 ** 31 - 1, -2 ** 31):
        d[rng.integers(0, H), rng.integers(0, W)] = v      # single pixels: centres and neighbours of others
    if H > 20:
        d[H // 3:H // 3 + 4, 3:12] = 0
        d[H // 2:H // 2 + 3, W - 14:W - 4] = 3000
        d[6:9, W // 2 - 3:W // 2 + 3] = 70000
        d[H - 12:H - 9, 8:14] = -7
    return d.astype(np.int32)


def _scene_check(core, depth, fx, fy, cx, cy):
    want_p, want_n = oracle.ref_scene(depth, fx, fy, cx, cy)
    got_p, got_n = _host(core.scene_projective(_dev(depth), fx, fy, cx, cy))
    assert ref.same_bits(got_p, want_p), f"points differ at {np.argwhere((got_p != want_p).any(-1))[:6]}"
    assert ref.same_bits(got_n, want_n), f"normals differ at {np.argwhere((got_n != want_n).any(-1))[:6]}"
    return want_p, want_n


def test_scene_hand_made_images_bit_for_bit():
    core = PoseCore(0)
    for seed in range(6):  # 12 x 12: the smallest image with one interior pixel
        d = _hand_depth(12, 12, seed)
        d[5, 5] = 100 + seed                               # the interior pixel itself stays below 2000
        _, n = _scene_check(core, d, 9.0, 11.5, 5.3, 6.1)
        assert not np.delete(n.reshape(-1, 3), 5 * 12 + 5, 0).any()
    assert sum(bool(oracle.ref_scene(_hand_depth(12, 12, s), 9.0, 11.5, 5.3, 6.1)[1].any()) for s in range(6)) >= 1
    d = _hand_depth(64, 48, 11)
    p, n = _scene_check(core, d, 61.0, 47.5, 30.7, 25.2)
    inner = n[5:48 - 6, 5:64 - 6]
    assert inner.any(-1).sum() > 1000 and (~inner.any(-1)).sum() > 20  # normals, and interior pixels without one
    assert not n[:5].any() and not n[48 - 6:].any() and not n[:, :5].any() and not n[:, 64 - 6:].any()
    assert (p[..., 2] > 600).any() and (p[d == 0] == 0).all()          # a negative depth read as uint32


def test_scene_c1_depth_bit_for_bit():
    c1 = _c1()
    sc = c1.scene
    _, n = _scene_check(PoseCore(0), c1.src_depth_cm, sc.fx, sc.fy, sc.cx, sc.cy)
    assert n.any(-1).sum() > 100000


@functools.lru_cache(maxsize=None)
def _c1():
    return workloads.c1_tabletop(oracle_render_fn)


# -- 2. the kernel on hand-made slots ---------------------------------------------------------------------------------

SLOT_SIZES = (0, 1, 63, 64, 65, 128, 129, 301)


@functools.lru_cache(maxsize=None)
def _slot_case():
    """A 96 x 72 scene (a tilted plane with a 12 cm step) and clouds cut from it, moved by a small rigid transform;
    the larger clouds carry points behind the camera, NaN points, points outside the image, points farther than
    max_dist_diff from the scene and points on pixels without a normal."""
    cam = TINY
    W, H = cam["width"], cam["height"]
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    d = np.round(80 + 0.25 * (x - 48) + 0.15 * (y - 36)).astype(np.int32)
    d[:, 62:] += 12
    fx, fy, cx, cy = (float(F(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    pcd, nrm = oracle.ref_scene(d, fx, fy, cx, cy)
    rng = np.random.default_rng(4)
    clouds = []
    for k, n in enumerate(SLOT_SIZES):
        # a window of interior pixels (every third), across the step for the larger clouds
        px = np.stack(np.meshgrid(np.arange(8, 88, 3), np.arange(8, 62, 3)), -1).reshape(-1, 2)
        px = px[rng.permutation(len(px))[:n]] if n < len(px) else px[:n]
        pts = pcd[px[:, 1], px[:, 0]].astype(np.float64)
        a = np.deg2rad(rng.uniform(-1.5, 1.5, 3))
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        c = pts.mean(0) if n else np.zeros(3)
        pts = ((pts - c) @ (Rz @ Ry @ Rx).T + c + rng.uniform(-0.006, 0.006, 3)).astype(F)
        if n >= 63:
            pts[3] = (0.1, 0.05, -0.8)                     # behind the camera
            pts[7] = (0.02, 0.01, 0.0)                     # z == 0
            pts[11] = (np.nan, 0.0, 0.8)
            pts[12] = (0.0, 0.1, np.nan)
            pts[20] = (3.0, 0.0, 0.8)                      # right of the image
            pts[21] = (0.0, -3.0, 0.8)                     # above it
            z0 = pcd[0, 0, 2]
            pts[22] = (F(-0.55) * z0, F(-0.4025) * z0, z0)  # v in (-1, 0) on both axes: pixel (0, 0), no normal there
            pts[30] = pcd[30, 40] + F((0.0, 0.0, 0.3))     # farther than max_dist_diff behind the scene
            pts[31] = pcd[30, 40] - F((0.0, 0.0, 0.3))
            pts[40] = pcd[2, 50]                           # border pixels: a point, no normal
            pts[41] = pcd[70, 3]
            pts[50] = (1e30, 0.0, 1e-30)                   # |v| >= 2^31
        clouds.append(pts)
    cap = 304
    xyzw = np.full((len(clouds), cap, 4), np.nan, F)       # past a slot's count: never read
    for i, c in enumerate(clouds):
        xyzw[i, :len(c), :3] = c
        xyzw[i, :len(c), 3] = 1.0
    cnt = np.array([len(c) for c in clouds], np.int32)
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:2] + (1,), F)], -1)
    return dict(clouds=clouds, xyzw=xyzw, cnt=cnt, pcd=pcd, nrm=nrm, pcd4=pad(pcd), nrm4=pad(nrm), cam=(fx, fy, cx, cy))


@pytest.mark.parametrize("max_iterations", [30, 0, 1])
def test_kernel_on_hand_made_slots_bit_for_bit(max_iterations):
    c = _slot_case()
    want = ref.run_clouds(c["clouds"], c["pcd"], c["nrm"], *c["cam"], max_iterations=max_iterations)
    if max_iterations == 30:  # not vacuous: rejected points, several iterations, both kinds of exit
        assert (want[1][2:] < 1.0).all() and (want[1][2:] > 0.5).all()
        assert want[3].max() >= 3 and want[3][0] == 0 and len(set(want[3].tolist())) >= 3
    else:
        assert (want[3][1:] == max_iterations).all()
    core = PoseCore(0)
    xyzw = _dev(c["xyzw"])
    got = _host(core.p2p_clouds(xyzw, _dev(c["cnt"]), _dev(c["pcd4"]), _dev(c["nrm4"]), *c["cam"],
                                max_iterations=max_iterations))
    _assert_same(got, want, f"max_iterations {max_iterations}")
    moved = xyzw.cpu().numpy()
    for i, cl in enumerate(c["clouds"]):  # the slots hold the moved clouds; nothing past a slot's count was written
        w = ref.icp(cl, c["pcd"], c["nrm"], *c["cam"], max_iterations=max_iterations)[4]
        assert ref.same_bits(moved[i, :len(cl), :3], w), i
        assert np.isnan(moved[i, len(cl):]).all()


# -- 3. through the render ------------------------------------------------------------------------------------------------

RENDER_CASES = [("ROMAN_640", 5), ("KINECT2", 16), ("SMALL", 8), ("TINY", 3), ("TINY", 1)]


def _geometry_core(case):
    sc = case.scene
    core = PoseCore(0)
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    xyz, lab = core.observed_cloud(_dev(sc.depth_raw), _dev(sc.mask), case.stride, sc.depth_factor)
    core.set_observation(_dev(sc.src_depth_cm), _dev(sc.mask), xyz, lab, 0.01)
    return core


@functools.lru_cache(maxsize=None)
def _geometry_reference(cs):
    """The module's results on the clouds the oracle makes for every pose of the case, computed once."""
    case = geometry_case(*cs)
    sc = case.scene
    zb = case.oracle_render(labels=True)
    xyz, pidx, _ = oracle.depth_to_cloud(zb, case.stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0)
    clouds = [xyz[pidx == i] for i in range(case.n)]
    pcd, nrm = oracle.ref_scene(sc.src_depth_cm, sc.fx, sc.fy, sc.cx, sc.cy)
    return clouds, ref.run_clouds(clouds, pcd, nrm, sc.fx, sc.fy, sc.cx, sc.cy)


def _run_case(core, case, idx=None, out_poses=None):
    idx = np.arange(case.n) if idx is None else np.asarray(idx)
    return _host(core.icp_point2plane(_dev(case.poses[idx]), _dev(case.pose_model[idx]), _dev(case.pose_label[idx]),
                                      cost_type=_native.COST_DEPTH_6DOF, stride=case.stride, out_poses=out_poses))


@pytest.mark.parametrize("cs", RENDER_CASES, ids=lambda cs: f"{cs[0]}-s{cs[1]}")
def test_through_the_render_bit_for_bit(cs):
    case = geometry_case(*cs)
    assert case.n == 78
    clouds, want = _geometry_reference(cs)
    ns = np.array([len(c) for c in clouds])
    assert (ns == 0).sum() >= 2 and ns.max() > 64          # empty renders, and clouds of more than one round
    assert (want[3][ns == 0] == 0).all() and len(set(want[3].tolist())) >= 3
    assert (want[0] != np.eye(4, dtype=F).reshape(16)).any(1).sum() >= 16
    core = _geometry_core(case)
    got = _run_case(core, case)
    _assert_same(got, want, f"{cs}")
    again = _run_case(core, case)                          # the scene is kept: the same again
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_three_dof_states_without_labels_bit_for_bit():
    c1 = _c1()
    sc = c1.scene
    stride = 4
    idx = np.arange(1, 128, 2)                             # 64 states, the ground truth among them
    assert c1.gt_index in idx
    poses = c1.poses[idx]
    pm = np.zeros(len(idx), np.int32)
    zb = oracle.render_depth(sc.bank.tris, sc.bank.tris_model_count, poses, pm, None, sc.width, sc.height, sc.proj,
                             c1.src_depth_cm, None, 1.0)
    xyz, pidx, _ = oracle.depth_to_cloud(zb, stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0)
    clouds = [xyz[pidx == i] for i in range(len(idx))]
    pcd, nrm = oracle.ref_scene(c1.src_depth_cm, sc.fx, sc.fy, sc.cx, sc.cy)
    want = ref.run_clouds(clouds, pcd, nrm, sc.fx, sc.fy, sc.cx, sc.cy)
    assert min(len(c) for c in clouds) > 64 and len(set(want[3].tolist())) >= 3
    core = PoseCore(0)
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    obs, _ = core.observed_cloud_bounded(_dev(sc.depth_raw), stride, sc.depth_factor)
    core.set_observation(_dev(c1.src_depth_cm), None, obs, None, 0.0075)
    got = _host(core.icp_point2plane(_dev(poses), _dev(pm), None, cost_type=_native.COST_DEPTH_3DOF, stride=stride,
                                     occlusion_threshold=1.0))
    _assert_same(got, want, "3-DoF")


# -- 4. batch independence --------------------------------------------------------------------------------------------

INDEP_CASE = ("SMALL", 8)


def test_order_and_split_invariance():
    case = geometry_case(*INDEP_CASE)
    _, want = _geometry_reference(INDEP_CASE)
    core = _geometry_core(case)
    rev = np.arange(case.n)[::-1]
    got = _run_case(core, case, idx=rev)
    _assert_same(tuple(a[::-1].copy() for a in got), want, "reversed")
    a = _run_case(core, case, idx=np.arange(0, 31))
    b = _run_case(core, case, idx=np.arange(31, case.n))
    _assert_same(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), want, "split")


def test_chunking_by_the_scratch_budget(monkeypatch):
    case = geometry_case(*INDEP_CASE)
    _, want = _geometry_reference(INDEP_CASE)
    nsamp = case.ws * case.hs
    monkeypatch.setenv("PCORE_P2P_SCRATCH_BYTES", str(3 * (nsamp * 16 + 4)))  # three poses per chunk
    _assert_same(_run_case(_geometry_core(case), case), want, "chunked")


# -- 5. composition and re-scoring --------------------------------------------------------------------------------------

def test_out_poses_and_rescoring():
    case = geometry_case(*INDEP_CASE)
    _, want = _geometry_reference(INDEP_CASE)
    core = _geometry_core(case)
    adj = torch.full((case.n, 16), -7.0, dtype=torch.float32, device=DEV)
    got = _run_case(core, case, out_poses=adj)
    _assert_same(got, want, "with out_poses")
    adj_h = adj.cpu().numpy()
    want_adj = np.stack([oracle.concat_pose(got[0][i].astype(np.float64), case.poses[i]) for i in range(case.n)])
    assert ref.same_bits(adj_h, want_adj)
    assert (adj_h != case.poses).any(1).sum() >= 16
    poses, pm, pl, tot = (_dev(a) for a in (case.poses, case.pose_model, case.pose_label, case.pose_obs_total))
    out = _host(core.evaluate_p2p(poses, pm, pl, tot, stride=case.stride))
    assert np.array_equal(out[0].view(np.uint32), adj_h.view(np.uint32)) and np.array_equal(out[1], got[3])
    assert ref.same_bits(out[5], got[1]) and ref.same_bits(out[6], got[2])
    rc, oc, df = _host(core.evaluate(adj, pm, pl, tot, stride=case.stride))
    for a, b in zip(out[2:5], (rc, oc, df)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _write_pose_lists(root, names, gts, rng, n):
    for k, name in enumerate(names):
        P = syn.candidate_poses(gts[k][:3, 3], n, rng, include=gts[k], num_viewpoints=20, inplane=4)
        rows = np.array([np.concatenate([T[:3, 3], matrix_to_quat_xyzw(T[:3, :3])]) for T in P])
        os.makedirs(os.path.join(root, name), exist_ok=True)
        io.write_poses_txt(os.path.join(root, name, "poses.txt"), rows, decimals=6)


def _recognizer_scene(tmp_path):
    names = ["003_cracker_box", "005_tomato_soup_can"]
    rng = np.random.default_rng(5)
    gts = np.stack([syn.default_gt_pose(rng, c) for c in [(-0.10, 0.0, 0.8), (0.08, 0.04, 0.85)]])
    sc = syn.make_scene(names, gts, oracle_render_fn, rng=rng)
    _write_pose_lists(str(tmp_path), names, gts, rng, 40)
    bank = {n: ModelMetaData(n, model=sc.bank.models[i]) for i, n in enumerate(names)}
    cam = CameraIntrinsics(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy)
    inp = RecognitionInput(names, sc.depth_raw, sc.mask, depth_factor=sc.depth_factor,
                           rendered_root_dir=str(tmp_path), use_icp=1)
    return names, bank, cam, inp


@pytest.mark.parametrize("icp_type", [4, 3])
def test_recognizer_icp_type_routes_the_flow(tmp_path, icp_type):
    """icp_type 4 returns what evaluate_p2p + select made by hand return; icp_type 3 still returns what evaluate_icp +
    select return."""
    names, bank, cam, inp = _recognizer_scene(tmp_path)
    rec = ObjectRecognizer(bank, cam, PerchParams(icp_type=icp_type))
    res = rec.localize_objects_greedy_render(inp)
    states = rec.generate_successor_states(inp)
    p = rec.params
    poses = _dev(rec._pose_in_cam(states))
    pm = _dev(np.array([s[0] for s in states], np.int32))
    pl_h = np.array([s[1] for s in states], np.int32)
    pl, tot = _dev(pl_h), _dev(rec.segmented_count[pl_h].astype(F))
    kw = dict(cost_type=_native.COST_DEPTH_6DOF, stride=p.gpu_stride, depth_factor=p.gpu_depth_factor,
              sensor_resolution=p.sensor_resolution, occlusion_threshold=p.gpu_occlusion_threshold)
    if icp_type == 4:
        adj, _, rc, oc, _, fit, _ = rec.core.evaluate_p2p(poses, pm, pl, tot, **kw)
        assert (fit > 0).sum() > len(states) // 2
    else:
        adj, _, rc, oc, _ = rec.core.evaluate_icp(poses, pm, pl, tot, **kw)
    keys = torch.full((len(names),), _native.PCORE_KEY_NONE, dtype=torch.int64, device=DEV)
    rec.core.select(rc, oc, pm, len(names), keys=keys)
    cost, idx = decode_keys(keys)
    found = [m for m in range(len(names)) if idx[m] >= 0]
    assert found and res.indices == [int(idx[m]) for m in found] and res.costs == [int(cost[m]) for m in found]
    adj_h = adj.cpu().numpy()
    assert (adj_h != poses.cpu().numpy()).any(1).sum() > len(states) // 2
    for k, m in enumerate(found):
        assert np.allclose(res.detected_poses[k][:3], adj_h[int(idx[m])].reshape(4, 4)[:3, 3] / 100.0, atol=1e-6)


# -- 6. argument checks -----------------------------------------------------------------------------------------------

def test_argument_checks_reject_before_any_launch():
    case = geometry_case("TINY", 3)
    _, want = _geometry_reference(("TINY", 3))
    core = _geometry_core(case)
    n = 6
    poses, pm, pl = _dev(case.poses[:n]), _dev(case.pose_model[:n]), _dev(case.pose_label[:n])
    T = torch.full((n, 16), -7.0, dtype=torch.float32, device=DEV)
    fit = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    rmse = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    it = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    adj = torch.full((n, 16), -7.0, dtype=torch.float32, device=DEV)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    DEFAULT = (30, 1e-5, 1e-5, 0.1)

    def call(core=core, cost_type=2, stride=3, icp=DEFAULT, poses=poses, pm=pm, pl=pl, T=T, fit=fit, rmse=rmse, it=it,
             params=True, icp_params=True):
        p = _native.EvalParams(cost_type, 0, stride, 100.0, 0.0, 1.0, 0.0)
        ip = _native.P2pIcpParams(*icp)
        return core.lib.pcore_icp_point2plane(core._h, ptr(poses), ptr(pm), ptr(pl), n,
                                              ctypes.byref(p) if params else None,
                                              ctypes.byref(ip) if icp_params else None, ptr(T), ptr(fit), ptr(rmse),
                                              ptr(it), ptr(adj), None)

    bad = _native.PCORE_E_INVALID_ARG
    nan = float("nan")
    assert call(params=False) == bad and call(icp_params=False) == bad
    assert call(poses=None) == bad and call(pm=None) == bad
    assert call(T=None) == bad and call(fit=None) == bad and call(rmse=None) == bad and call(it=None) == bad
    assert call(icp=(-1, 1e-5, 1e-5, 0.1)) == bad
    assert call(icp=(30, nan, 1e-5, 0.1)) == bad and call(icp=(30, -1e-5, 1e-5, 0.1)) == bad
    assert call(icp=(30, 1e-5, nan, 0.1)) == bad and call(icp=(30, 1e-5, -1e-5, 0.1)) == bad
    assert call(icp=(30, 1e-5, 1e-5, nan)) == bad and call(icp=(30, 1e-5, 1e-5, -0.1)) == bad
    assert call(stride=5) == bad                            # 96 % 5 != 0
    assert call(stride=0) == bad
    assert call(cost_type=7) == bad
    # a sampled image that does not fit the LDS: 2048 x 1536 at stride 1
    big = PoseCore(0)
    sc = case.scene
    big.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    big.set_camera(2048, 1536, 1900.0, 1900.0, 1024.0, 768.0, oracle.compute_proj(1900.0, 1900.0, 1024.0, 768.0, 2048, 1536))
    big.set_observation(torch.zeros((1536, 2048), dtype=torch.int32, device=DEV), None,
                        torch.zeros((0, 3), dtype=torch.float32, device=DEV), None, 0.01)
    assert call(core=big, stride=1, pl=None) == bad
    assert call(core=big, stride=8, pl=pl) == bad           # labels without a source mask
    fresh = PoseCore(0)
    assert call(core=fresh) == _native.PCORE_E_STATE        # nothing set up
    torch.cuda.synchronize()
    for t in (T, fit, rmse, adj):
        assert (t == -7.0).all()
    assert (it == -7).all()                                 # nothing was launched
    # the scene hook's checks
    d = torch.zeros((12, 12), dtype=torch.int32, device=DEV)
    o = torch.full((12, 12, 3), -7.0, dtype=torch.float32, device=DEV)
    sp = lambda depth=d, w=12, h=12, a=o, b=o: core.lib.pcore_scene_projective(
        core._h, ptr(depth), w, h, 9.0, 9.0, 6.0, 6.0, ptr(a), ptr(b), None)
    assert sp(depth=None) == bad and sp(w=0) == bad and sp(h=-1) == bad and sp(a=None) == bad and sp(b=None) == bad
    torch.cuda.synchronize()
    assert (o == -7.0).all()
    assert call() == _native.PCORE_OK
    got = _host((T, fit, rmse, it))
    _assert_same(got, tuple(w[:n] for w in want), "after the rejected calls")
