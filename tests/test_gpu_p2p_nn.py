"""GPU: the point-to-plane ICP against the nearest-neighbour scene (pcore_icp_point2plane_nn,
pcore_debug_p2p_nn_clouds) against the numpy restatement of its spec in wave order (tests/p2p_nn_reference.py), bit for
bit: T, fitness, rmse, iteration and the moved cloud.  tests/test_p2p_nn_spec.py certifies on the CPU that the
hand-made slots used here (tests/p2p_nn_cases.py) change under every wrong rule they are meant to catch."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import _native
from perception_amd.core import PoseCore, decode_keys
from perception_amd.recognizer import ObjectRecognizer, PerchParams
from tests import p2p_nn_cases as cs
from tests import p2p_nn_reference as nn
from tests.helpers import geometry_case
from tests.test_gpu_p2p import _assert_same, _c1, _dev, _geometry_core, _host, _recognizer_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


# -- 1. hand-made slots through the debug hook ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _want(kind, r, window, max_iterations):
    c = cs.dyadic_slots(r) if kind == "dyadic" else cs.tiny_slots()
    return nn.run_clouds(c["clouds"], c["pcd"], c["nrm"], *c["cam"], max_dist_diff=r, window=window,
                         max_iterations=max_iterations)


def _run_slots(c, r, window, max_iterations):
    xyzw = _dev(c["xyzw"])
    got = _host(PoseCore(0).debug_p2p_clouds(xyzw, _dev(c["cnt"]), _dev(c["pcd4"]), _dev(c["nrm4"]), *c["cam"],
                                             max_iterations=max_iterations, max_dist_diff=r, scene="nn", window=window))
    return got, xyzw.cpu().numpy()


def _check_slots(kind, r, window, max_iterations):
    c = cs.dyadic_slots(r) if kind == "dyadic" else cs.tiny_slots()
    want = _want(kind, r, window, max_iterations)
    got, moved = _run_slots(c, r, window, max_iterations)
    what = f"{kind} r {r} window {window} max_iterations {max_iterations}"
    _assert_same(got, want[:4], what)
    for i, cl in enumerate(c["clouds"]):  # the slots hold the moved clouds; nothing past a slot's count was written
        assert nn.same_bits(moved[i, :len(cl), :3], want[4][i]), (what, i)
        assert np.isnan(moved[i, len(cl):]).all()
    return want


@pytest.mark.parametrize("window", cs.WINDOWS)
@pytest.mark.parametrize("r", cs.RADII)
def test_dyadic_slots_every_window_and_radius_bit_for_bit(r, window):
    want = _check_slots("dyadic", r, window, 30)
    assert want[3][0] == 0 and want[1][0] == 0             # the empty slot: identity at iteration 0
    assert (want[1][2:] > 0.3).all() and (want[1][2:] < 1.0).all()  # accepted and refused points in every large slot
    if window >= 1:
        assert want[3].max() >= 2


@pytest.mark.parametrize("max_iterations", [0, 1])
def test_dyadic_slots_iteration_caps_bit_for_bit(max_iterations):
    for r, window in ((0.03, 4), (0.1, 32)):
        want = _check_slots("dyadic", r, window, max_iterations)
        assert (want[3][1:] == max_iterations).all()


@pytest.mark.parametrize("r,window,max_iterations", [(0.03, 32, 30), (0.01, 4, 30), (0.1, 128, 30), (0.03, 1, 1),
                                                     (0.03, 0, 0)])
def test_ordinary_camera_slots_bit_for_bit(r, window, max_iterations):
    want = _check_slots("tiny", r, window, max_iterations)
    if max_iterations == 30 and r >= 0.03:
        assert len(set(want[3].tolist())) >= 2 and want[3].max() >= 3


# -- 2. through the render --------------------------------------------------------------------------------------------

RENDER_CASES = [("KINECT2", 16), ("SMALL", 8), ("TINY", 3)]
INDEP_CASE = ("SMALL", 8)
RENDER_R = 0.1  # these cases' poses lie centimetres off the scene: the default 0.01 leaves nearly all of them unmoved


@functools.lru_cache(maxsize=None)
def _render_reference(cs_):
    case = geometry_case(*cs_)
    sc = case.scene
    zb = case.oracle_render(labels=True)
    xyz, pidx, _ = oracle.depth_to_cloud(zb, case.stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0)
    clouds = [xyz[pidx == i] for i in range(case.n)]
    pcd, nrm = oracle.ref_scene(sc.src_depth_cm, sc.fx, sc.fy, sc.cx, sc.cy)
    return clouds, nn.run_clouds(clouds, pcd, nrm, sc.fx, sc.fy, sc.cx, sc.cy, max_dist_diff=RENDER_R)[:4]


def _run_case(core, case, idx=None, out_poses=None):
    idx = np.arange(case.n) if idx is None else np.asarray(idx)
    return _host(core.icp_point2plane(_dev(case.poses[idx]), _dev(case.pose_model[idx]), _dev(case.pose_label[idx]),
                                      cost_type=_native.COST_DEPTH_6DOF, stride=case.stride, out_poses=out_poses,
                                      scene="nn", max_dist_diff=RENDER_R))


@pytest.mark.parametrize("cs_", RENDER_CASES, ids=lambda c: f"{c[0]}-s{c[1]}")
def test_through_the_render_bit_for_bit(cs_):
    case = geometry_case(*cs_)
    assert case.n == 78
    clouds, want = _render_reference(cs_)
    ns = np.array([len(c) for c in clouds])
    assert (ns == 0).sum() >= 2 and ns.max() > 64
    assert (want[3][ns == 0] == 0).all() and len(set(want[3].tolist())) >= 3
    assert (want[0] != np.eye(4, dtype=F).reshape(16)).any(1).sum() >= (4 if cs_[0] == "TINY" else 16)
    core = _geometry_core(case)
    got = _run_case(core, case)
    _assert_same(got, want, f"{cs_}")
    again = _run_case(core, case)                          # the scene is kept: the same again
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_three_dof_states_without_labels_bit_for_bit():
    c1 = _c1()
    sc = c1.scene
    stride = 8
    idx = np.arange(1, 128, 2)                             # 64 states, the ground truth among them
    poses = c1.poses[idx]
    pm = np.zeros(len(idx), np.int32)
    zb = oracle.render_depth(sc.bank.tris, sc.bank.tris_model_count, poses, pm, None, sc.width, sc.height, sc.proj,
                             c1.src_depth_cm, None, 1.0)
    xyz, pidx, _ = oracle.depth_to_cloud(zb, stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0)
    clouds = [xyz[pidx == i] for i in range(len(idx))]
    pcd, nrm = oracle.ref_scene(c1.src_depth_cm, sc.fx, sc.fy, sc.cx, sc.cy)
    # the restatement looks at every pixel of every window: all 64 states at window 8, four at the default 32
    want = nn.run_clouds(clouds, pcd, nrm, sc.fx, sc.fy, sc.cx, sc.cy, window=8)[:4]
    sub = [1, 4, 9, 41]
    want32 = nn.run_clouds([clouds[i] for i in sub], pcd, nrm, sc.fx, sc.fy, sc.cx, sc.cy)[:4]  # r 0.01, window 32
    ns = [len(c) for c in clouds]
    assert min(ns) > 32 and max(ns) > 256 and (want[1] > 0).sum() > 32 and len(set(want[3].tolist())) >= 3
    core = PoseCore(0)
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    obs, _ = core.observed_cloud_bounded(_dev(sc.depth_raw), stride, sc.depth_factor)
    core.set_observation(_dev(c1.src_depth_cm), None, obs, None, 0.0075)
    got = _host(core.icp_point2plane(_dev(poses), _dev(pm), None, cost_type=_native.COST_DEPTH_3DOF, stride=stride,
                                     occlusion_threshold=1.0, scene="nn", window=8))
    _assert_same(got, want, "3-DoF, window 8")
    got = _host(core.icp_point2plane(_dev(poses[sub]), _dev(pm[sub]), None, cost_type=_native.COST_DEPTH_3DOF,
                                     stride=stride, occlusion_threshold=1.0, scene="nn"))
    _assert_same(got, want32, "3-DoF, the defaults")


# -- 3. batch handling --------------------------------------------------------------------------------------------------

def test_order_and_split_invariance():
    case = geometry_case(*INDEP_CASE)
    _, want = _render_reference(INDEP_CASE)
    core = _geometry_core(case)
    rev = np.arange(case.n)[::-1]
    got = _run_case(core, case, idx=rev)
    _assert_same(tuple(a[::-1].copy() for a in got), want, "reversed")
    a = _run_case(core, case, idx=np.arange(0, 31))
    b = _run_case(core, case, idx=np.arange(31, case.n))
    _assert_same(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), want, "split")


def test_chunking_by_the_scratch_budget(monkeypatch):
    case = geometry_case(*INDEP_CASE)
    _, want = _render_reference(INDEP_CASE)
    nsamp = case.ws * case.hs
    monkeypatch.setenv("PCORE_P2P_SCRATCH_BYTES", str(3 * (nsamp * 16 + 4)))  # three poses per chunk
    _assert_same(_run_case(_geometry_core(case), case), want, "chunked")


def test_out_poses_and_rescoring():
    case = geometry_case(*INDEP_CASE)
    _, want = _render_reference(INDEP_CASE)
    core = _geometry_core(case)
    adj = torch.full((case.n, 16), -7.0, dtype=torch.float32, device=DEV)
    got = _run_case(core, case, out_poses=adj)
    _assert_same(got, want, "with out_poses")
    adj_h = adj.cpu().numpy()
    want_adj = np.stack([oracle.concat_pose(got[0][i].astype(np.float64), case.poses[i]) for i in range(case.n)])
    assert nn.same_bits(adj_h, want_adj)
    assert (adj_h != case.poses).any(1).sum() >= 16
    poses, pm, pl, tot = (_dev(a) for a in (case.poses, case.pose_model, case.pose_label, case.pose_obs_total))
    out = _host(core.evaluate_p2p(poses, pm, pl, tot, stride=case.stride, scene="nn", max_dist_diff=RENDER_R))
    assert np.array_equal(out[0].view(np.uint32), adj_h.view(np.uint32)) and np.array_equal(out[1], got[3])
    assert nn.same_bits(out[5], got[1]) and nn.same_bits(out[6], got[2])
    rc, oc, df = _host(core.evaluate(adj, pm, pl, tot, stride=case.stride))
    for a, b in zip(out[2:5], (rc, oc, df)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# -- 4. context reuse ---------------------------------------------------------------------------------------------------

def _set_scene(core, case):
    sc = case.scene
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    xyz, lab = core.observed_cloud(_dev(sc.depth_raw), _dev(sc.mask), case.stride, sc.depth_factor)
    core.set_observation(_dev(sc.src_depth_cm), _dev(sc.mask), xyz, lab, 0.01)


@pytest.mark.parametrize("order", [(("SMALL", 8), ("TINY", 3)), (("TINY", 3), ("SMALL", 8))], ids=["large-small", "small-large"])
def test_one_context_across_two_scenes_has_no_stale_scene(order):
    idx = np.arange(0, 78, 3)
    fresh = {}
    for c_ in order:
        case = geometry_case(*c_)
        fresh[c_] = _run_case(_geometry_core(case), case, idx=idx)
        _assert_same(fresh[c_], tuple(w[idx] for w in _render_reference(c_)[1]), f"fresh {c_}")
    core = PoseCore(0)
    for c_ in order + order[:1]:
        case = geometry_case(*c_)
        _set_scene(core, case)
        got = _run_case(core, case, idx=idx)
        for a, b in zip(got, fresh[c_]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c_


# -- 5. the recognizer ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top_k", [0, 4])
def test_recognizer_icp_type_5(tmp_path, top_k):
    """icp_type 5 returns what evaluate_p2p(scene="nn") + select made by hand return; staged, the refined rows equal
    the full call's rows bit for bit."""
    names, bank, cam, inp = _recognizer_scene(tmp_path)
    params = PerchParams(icp_type=5, nn_max_dist_diff=0.03, nn_window=16, icp_top_k=top_k)
    rec = ObjectRecognizer(bank, cam, params)
    res = rec.localize_objects_greedy_render(inp)
    states = rec.generate_successor_states(inp)
    p = rec.params
    poses = _dev(rec._pose_in_cam(states))
    pm = _dev(np.array([s[0] for s in states], np.int32))
    pl_h = np.array([s[1] for s in states], np.int32)
    pl, tot = _dev(pl_h), _dev(rec.segmented_count[pl_h].astype(F))
    kw = dict(cost_type=_native.COST_DEPTH_6DOF, stride=p.gpu_stride, depth_factor=p.gpu_depth_factor,
              sensor_resolution=p.sensor_resolution, occlusion_threshold=p.gpu_occlusion_threshold)
    adj, _iters, rc, oc, _df, fit, _ = rec.core.evaluate_p2p(poses, pm, pl, tot, scene="nn", max_dist_diff=0.03,
                                                             window=16, **kw)
    assert (fit > 0).sum() > len(states) // 2
    adj_h = adj.cpu().numpy()
    assert (adj_h != poses.cpu().numpy()).any(1).sum() > len(states) // 2
    # not the projective scene's result
    adj4 = rec.core.evaluate_p2p(poses, pm, pl, tot, **kw)[0].cpu().numpy()
    assert (adj4 != adj_h).any(1).sum() > len(states) // 4
    K = len(names)
    if top_k == 0:
        sel_rc, sel_oc = rc, oc
    else:
        pre = rec.core.evaluate(poses, pm, pl, tot, **kw)
        _, members = decode_keys(rec.core.select_topk(pre[0], pre[1], pm, K, top_k))
        members = np.unique(members[members >= 0])
        assert 0 < len(members) <= K * top_k
        sub = _dev(members.astype(np.int64))
        sel_rc = torch.full_like(rc, -1.0)
        sel_oc = torch.full_like(oc, -1.0)
        sel_rc[sub], sel_oc[sub] = rc[sub], oc[sub]        # the full call's rows of the shortlist members
        part = rec.core.evaluate_p2p(poses[sub].contiguous(), pm[sub].contiguous(), pl[sub].contiguous(),
                                     tot[sub].contiguous(), scene="nn", max_dist_diff=0.03, window=16, **kw)
        for a, b in zip(part[:5], (adj, _iters, rc, oc, _df)):  # refined alone or in the full batch: the same bits
            assert torch.equal(a.view(torch.int32), b[sub].view(torch.int32))
    keys = torch.full((K,), _native.PCORE_KEY_NONE, dtype=torch.int64, device=DEV)
    rec.core.select(sel_rc, sel_oc, pm, K, keys=keys)
    cost, idx = decode_keys(keys)
    found = [m for m in range(K) if idx[m] >= 0]
    assert found and res.indices == [int(idx[m]) for m in found] and res.costs == [int(cost[m]) for m in found]
    for k, m in enumerate(found):
        assert np.allclose(res.detected_poses[k][:3], adj_h[int(idx[m])].reshape(4, 4)[:3, 3] / 100.0, atol=1e-6)


# -- 6. argument checks -----------------------------------------------------------------------------------------------

def test_argument_checks_reject_before_any_launch():
    case = geometry_case("TINY", 3)
    _, want = _render_reference(("TINY", 3))
    core = _geometry_core(case)
    n = 6
    poses, pm, pl = _dev(case.poses[:n]), _dev(case.pose_model[:n]), _dev(case.pose_label[:n])
    T = torch.full((n, 16), -7.0, dtype=torch.float32, device=DEV)
    fit = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    rmse = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    it = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    adj = torch.full((n, 16), -7.0, dtype=torch.float32, device=DEV)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    DEFAULT = (30, 1e-5, 1e-5, RENDER_R, 32)

    def call(core=core, cost_type=2, stride=3, icp=DEFAULT, poses=poses, pm=pm, pl=pl, T=T, fit=fit, rmse=rmse, it=it,
             params=True, icp_params=True):
        p = _native.EvalParams(cost_type, 0, stride, 100.0, 0.0, 1.0, 0.0)
        ip = _native.NnIcpParams(*icp)
        return core.lib.pcore_icp_point2plane_nn(core._h, ptr(poses), ptr(pm), ptr(pl), n,
                                                 ctypes.byref(p) if params else None,
                                                 ctypes.byref(ip) if icp_params else None, ptr(T), ptr(fit), ptr(rmse),
                                                 ptr(it), ptr(adj), None)

    bad = _native.PCORE_E_INVALID_ARG
    nan = float("nan")
    assert call(params=False) == bad and call(icp_params=False) == bad
    assert call(poses=None) == bad and call(pm=None) == bad
    assert call(T=None) == bad and call(fit=None) == bad and call(rmse=None) == bad and call(it=None) == bad
    assert call(icp=(30, 1e-5, 1e-5, 0.01, -1)) == bad and call(icp=(30, 1e-5, 1e-5, 0.01, 129)) == bad
    assert call(icp=(30, 1e-5, 1e-5, 0.0, 32)) == bad and call(icp=(30, 1e-5, 1e-5, -0.01, 32)) == bad
    assert call(icp=(30, 1e-5, 1e-5, nan, 32)) == bad
    assert call(icp=(-1, 1e-5, 1e-5, 0.01, 32)) == bad
    assert call(icp=(30, nan, 1e-5, 0.01, 32)) == bad and call(icp=(30, 1e-5, -1e-5, 0.01, 32)) == bad
    assert call(stride=5) == bad and call(cost_type=7) == bad
    assert call(core=PoseCore(0)) == _native.PCORE_E_STATE  # no observation
    # the hook's checks
    c = cs.dyadic_slots(0.03)
    xyzw, cnt, p4, n4 = _dev(c["xyzw"][:n]), _dev(c["cnt"][:n]), _dev(c["pcd4"]), _dev(c["nrm4"])
    before = xyzw.clone()

    def hook(icp=DEFAULT, T=T, w=cs.W, scene=p4):
        ip = _native.NnIcpParams(*icp)
        return core.lib.pcore_debug_p2p_nn_clouds(ptr(xyzw), ptr(cnt), xyzw.shape[1], n, ptr(scene), ptr(n4), w, cs.H,
                                                  *c["cam"], ctypes.byref(ip), ptr(T), ptr(fit), ptr(rmse), ptr(it), None)

    assert hook(icp=(30, 1e-5, 1e-5, 0.03, 129)) == bad and hook(icp=(30, 1e-5, 1e-5, nan, 4)) == bad
    assert hook(icp=(30, 1e-5, 1e-5, 0.0, 4)) == bad and hook(T=None) == bad and hook(w=0) == bad
    assert hook(scene=None) == bad
    torch.cuda.synchronize()
    for t in (T, fit, rmse, adj):
        assert (t == -7.0).all()
    assert (it == -7).all()                                 # nothing was launched
    assert torch.equal(torch.nan_to_num(xyzw), torch.nan_to_num(before))
    assert call() == _native.PCORE_OK
    _assert_same(_host((T, fit, rmse, it)), tuple(w[:n] for w in want), "after the rejected calls")
