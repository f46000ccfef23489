"""GPU: pcore_icp_planar (the planar x / y / yaw ICP of the 3-DoF search) against the numpy restatement of its spec
(tests/icp2d_reference.py; tests/test_icp2d_spec.py shows the cases are not vacuous), bit for bit; its neighbour search
on a hand-made observation; the estimation step's test hook; the recognizer end to end; the argument checks."""
import ctypes
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import _native
from perception_amd.core import PoseCore
from perception_amd.recognizer import CameraIntrinsics, ModelMetaData, States
from perception_amd.tabletop import TableParams, TabletopRecognizer, pr2_gpu_params
from tests import icp2d_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _core(c, obs=None):
    sc = c.scene
    core = PoseCore(0)
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    obs = c.obs_xyz if obs is None else obs
    core.set_observation(torch.from_numpy(c.src_cm).to(DEV), None, torch.from_numpy(np.ascontiguousarray(obs)).to(DEV),
                         None, ref.SENSOR_RESOLUTION)
    return core


def _run(core, c, idx=None, world_from_cam=None, **kw):
    idx = np.arange(c.n) if idx is None else np.asarray(idx)
    poses = torch.from_numpy(np.ascontiguousarray(c.poses[idx])).to(DEV)
    pm = torch.from_numpy(np.ascontiguousarray(c.pose_model[idx])).to(DEV)
    out = core.icp_planar(poses, pm, c.world_from_cam if world_from_cam is None else world_from_cam, stride=c.stride,
                          depth_factor=100.0, occlusion_threshold=ref.OCCLUSION_THRESHOLD, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got, want, what=""):
    xf, it, st, mse = got
    wxf, wit, wst, wmse = want[:4]
    assert np.array_equal(st, wst), f"{what} status: {np.nonzero(st != wst)[0][:8]}"
    assert np.array_equal(it, wit), f"{what} iterations: {np.nonzero(it != wit)[0][:8]}"
    assert np.array_equal(xf.view(np.uint64), np.ascontiguousarray(wxf).view(np.uint64)), \
        f"{what} xform rows {np.nonzero((xf != wxf).any(1))[0][:8]}"
    assert np.array_equal(mse.view(np.uint64), np.ascontiguousarray(wmse).view(np.uint64)), f"{what} mse"


_KW = {"eps_t": "transformation_epsilon", "eps_fit": "fitness_epsilon", "max_iterations": "max_iterations",
       "max_correspondence": "max_correspondence"}


@pytest.mark.parametrize("row", ref.TABLE_ROWS, ids=ref.row_id)
def test_parity_bit_for_bit(row):
    c = ref.planar_case(row[0], row[1])
    want = ref.row_result(*row)
    core = _core(c)
    got = _run(core, c, **{_KW[k]: v for k, v in row[2]})
    _assert_same(got, want, ref.row_id(row))
    # the same case again on the same context: identical output
    again = _run(core, c, **{_KW[k]: v for k, v in row[2]})
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_order_and_split_invariance():
    c = ref.planar_case("SMALL", 2)
    want = (c.xform, c.iters, c.status, c.mse)
    core = _core(c)
    rev = np.arange(c.n)[::-1]
    got = _run(core, c, idx=rev)
    _assert_same(tuple(a[::-1].copy() for a in got), want, "reversed")
    a = _run(core, c, idx=np.arange(0, 23))
    b = _run(core, c, idx=np.arange(23, c.n))
    _assert_same(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), want, "split")


def test_chunking_by_the_scratch_budget(monkeypatch):
    c = ref.planar_case("SMALL", 2)
    sc = c.scene
    nsamp = (sc.width // c.stride) * ((sc.height + c.stride - 1) // c.stride)
    monkeypatch.setenv("PCORE_ICP2D_SCRATCH_BYTES", str(3 * (nsamp * 16 + 4)))  # three poses per chunk
    got = _run(_core(c), c)
    _assert_same(got, (c.xform, c.iters, c.status, c.mse), "chunked")


def test_neighbour_search_on_a_hand_made_observation():
    """Duplicated targets, targets exactly on d^2 == r^2 and queries outside the grid's box: the world frame is the
    camera's (identity matrix) and r = 2^-4 m, so a target 2^-4 m behind a source point (the rendered z is a
    multiple of 1 cm below 1 m: the sum is exact) is at d^2 == r^2 bit for bit.  The targets are one cloud pushed back by
    r (twice: duplicates) and another cloud's own points (twice); every other pose's cloud lies partly or wholly
    outside their box."""
    c = ref.planar_case("TINY", 1)
    r = 0.0625
    ns = np.array([len(x) for x in c.clouds])
    a, b = int(np.argmax(ns * (c.pose_model == 0))), int(np.argmax(ns * (c.pose_model == 1)))
    back = c.clouds[a] + np.array([0.0, 0.0, r], np.float32)
    obs = np.concatenate([back, c.clouds[b], back, c.clouds[b]]).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    d2, _ = ref.nearest(c.clouds[a], obs)
    assert (d2 == np.float32(r) * np.float32(r)).sum() >= 10     # pairs exactly on the radius, kept
    lo, hi = obs.min(0), obs.max(0)
    allq = np.concatenate(c.clouds)
    assert ((allq < lo) | (allq > hi)).any(1).sum() >= 100        # queries outside the grid's box
    want = ref.run_poses(c.clouds, obs, eye, max_correspondence=r)
    assert len(set(int(s) for s in want[2])) >= 3
    got = _run(_core(c, obs), c, world_from_cam=eye, max_correspondence=r)
    _assert_same(got, want, "hand-made")


def test_step_hook_bit_for_bit():
    rng = np.random.default_rng(3)
    rows = []
    for _ in range(2048):  # sums of random pair sets at table-top magnitudes
        n = int(rng.integers(3, 400))
        q = (rng.uniform(-0.1, 0.1, (n, 2)) + rng.uniform(-1.0, 1.0, 2)).astype(np.float32).astype(np.float64)
        th = rng.uniform(-0.5, 0.5)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        t = (q @ R.T + rng.uniform(-0.03, 0.03, 2) + rng.normal(0, 2e-3, (n, 2))).astype(np.float32).astype(np.float64)
        rows.append([n, q[:, 0].sum(), q[:, 1].sum(), t[:, 0].sum(), t[:, 1].sum(), (q[:, 0] * t[:, 0]).sum(),
                     (q[:, 0] * t[:, 1]).sum(), (q[:, 1] * t[:, 0]).sum(), (q[:, 1] * t[:, 1]).sum(),
                     ((q - t) ** 2).sum()])
    for _ in range(2048):  # raw records over many magnitudes
        rec = rng.normal(size=10) * 10.0 ** rng.integers(-12, 12, 10)
        rec[0] = float(rng.integers(1, 20000))
        rows.append(rec)
    rows.append([3.0, 3.0, 0.0, 6.0, 3.0, 6.0, 3.0, 0.0, 0.0, 0.0])            # h == 0: equal pairs
    rows.append([4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])            # h == 0: all zeros
    rows.append([5.0, 1.0, 2.0, 2.0, 1.0, 0.5, 0.25, 0.25, 0.5, 0.0])
    for scale in (5e-324, 1e-310, 1e-300, 1e-160):                              # denormal and tiny rows
        rows.append([7.0] + [scale * k for k in (3, -2, 1, 4, 9, -5, 6, 7, 1)])
    for scale in (1e150, 1e200, 1e300):                                         # huge rows (a a + b b overflows)
        rows.append([9.0] + [scale * k for k in (1.5, -2.5, 1.25, 0.5, 1.0, -0.75, 0.5, 1.0, 1.0)])
    S = np.array(rows, np.float64)
    assert len(S) >= 4096 + 5
    want = np.array([ref.planar_step(r) for r in S], np.float64)
    core = PoseCore(0)
    got = core.planar_step(torch.from_numpy(S).to(DEV))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)  # a NaN's sign and payload are not part of the spec
    assert np.array_equal(np.where(nan, 0.0, got).view(np.uint64), np.where(nan, 0.0, want).view(np.uint64))
    assert (want[4096] == [1.0, 0.0, 1.0, 1.0]).all() and (want[4097] == [1.0, 0.0, 0.0, 0.0]).all()
    assert nan.mean() < 0.05


# -- the recognizer end to end ----------------------------------------------------------------------------------

E2E_STRIDE = 5


def _recognizer():
    sc, _, src_cm = ref.tabletop_scene("SMALL")
    table = TableParams(x_min=0.56, x_max=0.68, y_min=-0.12, y_max=0.14, table_height=ref.TABLE["table_height"],
                        res=0.04, theta_res=0.7853982)
    bank = {n: ModelMetaData(n, model=sc.bank.models[i]) for i, n in enumerate(ref.NAMES)}
    cam = CameraIntrinsics(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy)
    # IsValidPose's neighbour count scales with the cloud's density, 1 / stride^2 (30 at the reference's stride 4)
    rec = TabletopRecognizer(bank, cam, table, pr2_gpu_params(
        use_color_cost=False, gpu_stride=E2E_STRIDE, min_neighbor_points_for_valid_pose=round(30 * 16 / E2E_STRIDE ** 2)))
    return src_cm, sc, rec


def _oracle_selection(src_cm, sc, rec, states):
    mats = rec._pose_in_cam(states)
    tot = rec._obs_totals(states)
    p = rec.params
    rc, oc, _ = oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, mats, states.model, None, sc.width, sc.height,
                                sc.proj, src_cm, None, p.gpu_occlusion_threshold, p.gpu_stride, sc.cx, sc.cy, sc.fx,
                                sc.fy, 100.0, rec.obs_xyz_host, None, None, tot, 0, True, p.sensor_resolution)
    bc, bi = oracle.select(rc, oc, states.model, len(ref.NAMES))
    return mats, rc, oc, bc, bi


def test_localize_with_planar_icp_matches_the_reference_adjusted_search():
    from perception_amd.tabletop import planar_adjusted_states

    src_cm, sc, rec = _recognizer()
    res = rec.localize(ref.NAMES, sc.depth_raw, sc.camera_pose, sc.depth_factor, use_icp=1)
    states = rec.generate_successor_states()
    assert len(states) >= 64
    # the reference's side: oracle clouds of the grid states, the numpy ICP, the host pose update
    p = rec.params
    zb = oracle.render_depth(sc.bank.tris, sc.bank.tris_model_count, rec._pose_in_cam(states), states.model, None,
                             sc.width, sc.height, sc.proj, src_cm, None, p.gpu_occlusion_threshold)
    xyz, pidx, _ = oracle.depth_to_cloud(zb, p.gpu_stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0)
    clouds = [xyz[pidx == i] for i in range(len(states))]
    xf, it, st, mse, _ = ref.run_poses(clouds, rec.obs_xyz_host, rec.transform, max_iterations=p.max_icp_iterations,
                                       max_correspondence=p.icp_max_correspondence)
    assert (st < ref.NO_CORRESPONDENCES).sum() >= 16 and (it >= 2).sum() >= 16
    g_xf, g_st = (t.cpu().numpy() for t in rec.last_planar)
    assert np.array_equal(g_st, st) and np.array_equal(g_xf.view(np.uint64), xf.view(np.uint64))
    adj = States(states.model, states.req, planar_adjusted_states(states.pose, xf, st))
    assert (adj.pose != states.pose).any()
    mats, rc, oc, bc, bi = _oracle_selection(src_cm, sc, rec, adj)
    g_rc, g_oc, _ = rec._last_costs
    assert np.array_equal(g_rc.view(np.uint32), rc.view(np.uint32))
    assert np.array_equal(g_oc.view(np.uint32), oc.view(np.uint32))
    got = {m: (cost, idx, cont) for m, cost, idx, cont in res}
    found = [m for m in range(len(ref.NAMES)) if bi[m] >= 0]
    assert found and sorted(got) == found
    for m in found:
        assert got[m][:2] == (int(bc[m]), int(bi[m]))
        # the ContPose is the adjusted state's: position and yaw quaternion (through the float pose matrix)
        want = rec.adjusted_cont_poses(mats[[bi[m]]], np.array([m], np.int32), 0)[0]
        assert np.array_equal(got[m][2], want)
        x, y, z, yaw = adj.pose[bi[m]]
        assert np.allclose(got[m][2][:3], [x, y, z], atol=1e-5)
        assert np.allclose(np.abs(got[m][2][3:]), np.abs([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]), atol=1e-5)
    assert rec.last_stats.icp_time > 0.0


def test_localize_without_icp_is_the_plain_grid_search():
    """The default (use_icp = 0) returns what it returned before the planar stage existed: the oracle's evaluate +
    select on the grid states themselves."""
    src_cm, sc, rec = _recognizer()
    res = rec.localize(ref.NAMES, sc.depth_raw, sc.camera_pose, sc.depth_factor)
    states = rec.generate_successor_states()
    mats, rc, oc, bc, bi = _oracle_selection(src_cm, sc, rec, states)
    g_rc, g_oc, _ = rec._last_costs
    assert np.array_equal(g_rc.view(np.uint32), rc.view(np.uint32))
    assert np.array_equal(g_oc.view(np.uint32), oc.view(np.uint32))
    got = {m: (cost, idx, cont) for m, cost, idx, cont in res}
    found = [m for m in range(len(ref.NAMES)) if bi[m] >= 0]
    assert sorted(got) == found
    for m in found:
        assert got[m][:2] == (int(bc[m]), int(bi[m]))
        assert np.array_equal(got[m][2], rec.adjusted_cont_poses(mats[[bi[m]]], np.array([m], np.int32), 0)[0])
    assert rec.last_stats.icp_time == 0.0
    if "use_icp" in inspect.signature(rec.localize).parameters:
        res0 = rec.localize(ref.NAMES, sc.depth_raw, sc.camera_pose, sc.depth_factor, use_icp=0)
        assert [(m, cost, idx) for m, cost, idx, _ in res0] == [(m, cost, idx) for m, cost, idx, _ in res]
        assert all(np.array_equal(a[3], b[3]) for a, b in zip(res0, res))


# -- argument checks ------------------------------------------------------------------------------------------------

def test_argument_checks_reject_before_any_launch():
    c = ref.planar_case("TINY", 1)
    core = _core(c)
    n = 4
    poses = torch.from_numpy(np.ascontiguousarray(c.poses[:n])).to(DEV)
    pm = torch.from_numpy(np.ascontiguousarray(c.pose_model[:n])).to(DEV)
    xf = torch.full((n, 4), -7.0, dtype=torch.float64, device=DEV)
    it = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    M = (ctypes.c_float * 16)(*np.asarray(c.world_from_cam, np.float32).reshape(16))

    def call(cost_type=0, stride=1, max_iterations=20, max_corr=0.05, xform=xf, iters=it, status=st, matrix=M):
        p = _native.EvalParams(cost_type, 0, stride, 100.0, 0.0, 1.0, 0.0)
        pp = _native.PlanarIcpParams(max_iterations, max_corr, 1e-8, 1e-5)
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        return core.lib.pcore_icp_planar(core._h, ptr(poses), ptr(pm), n, ctypes.byref(p), matrix, ctypes.byref(pp),
                                         ptr(xform), ptr(iters), ptr(status), None, None)

    bad = _native.PCORE_E_INVALID_ARG
    assert call(cost_type=_native.COST_DEPTH_6DOF) == bad
    assert call(max_iterations=-1) == bad
    assert call(max_corr=float("nan")) == bad and call(max_corr=float("inf")) == bad and call(max_corr=-0.01) == bad
    assert call(xform=None) == bad and call(iters=None) == bad and call(status=None) == bad
    assert call(stride=5) == bad  # 96 % 5 != 0
    assert call(matrix=None) == bad
    torch.cuda.synchronize()
    assert (xf == -7.0).all() and (it == -7).all() and (st == -7).all()  # nothing was launched
    assert call() == _native.PCORE_OK
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == c.status[:n]).all() and (it.cpu().numpy() == c.iters[:n]).all()
