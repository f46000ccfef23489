"""The fused cost kernel's fixed-radius 1-NN grid search (process_points) on observed clouds built to hurt it: the cases
of tests/nn_cases.py (certified on the CPU by tests/test_nn_cases.py: each of them changes some pose's costs under a
wrong radius test, tie rule, candidate set or box padding) through the C ABI, bit for bit against the oracle's brute
force.  Everything is compared for equality: there are no tolerances.

Two more checks put a far point into the observation of the other grid consumers: the GICP correspondence search of
segments above kGridNNMin targets (grid_shells) and the planar ICP's (planar_nn)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import _native
from perception_amd.core import PoseCore, decode_keys
from tests import icp2d_reference as ref2d
from tests import nn_cases as nc
from tests.helpers import SMALL, SceneCase
from tests.nn_cases import nn_case

pytestmark = pytest.mark.gpu


def _assert_costs(got, want, what=""):
    rc, oc, df = (x.cpu().numpy() for x in got)
    orc, ooc, odf = want
    bad = np.nonzero(~((rc.view(np.uint32) == orc.view(np.uint32)) & (oc.view(np.uint32) == ooc.view(np.uint32)) &
                       (df.view(np.uint32) == odf.view(np.uint32))))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(rc)} poses differ, e.g. {bad[:6]}: gpu rc {rc[bad[:6]]} oc "
                           f"{oc[bad[:6]]} diff {df[bad[:6]]}, oracle rc {orc[bad[:6]]} oc {ooc[bad[:6]]} diff "
                           f"{odf[bad[:6]]}")


def _setup(case, colours=False):
    """A context with the case's meshes, camera and observation (given in the case's shuffled order, with labels)."""
    c = case.cam
    core = PoseCore(0)
    core.upload_meshes(case.bank.tris, case.bank.tris_model_count, colors=case.bank.colors if colours else None)
    core.set_camera(case.width, case.height, c["fx"], c["fy"], c["cx"], c["cy"], case.proj)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in (
        ("src", case.src_depth), ("mask", case.mask), ("poses", case.poses), ("pm", case.pose_model),
        ("pl", case.pose_label), ("tot", case.pose_obs_total), ("tot0", case.pose_obs_total0),
        ("xyz", case.obs_xyz), ("lab", case.obs_label), ("rgb", case.obs_rgb))}
    core.set_observation(t["src"], t["mask"], t["xyz"], t["lab"], case.r)
    if colours:
        core.set_observation_colors(t["rgb"])
    return core, t


_ORACLE = {}


def _want(name, cost_type):
    """The oracle's costs of a case, computed once and left unchanged."""
    if (name, cost_type) not in _ORACLE:
        _ORACLE[name, cost_type] = nn_case(name).oracle_costs(cost_type)
    return _ORACLE[name, cost_type]


def _evaluate(core, t, case, cost_type, colour_thr=nc.COLOUR_THR, **kw):
    six = cost_type == 2
    return core.evaluate(t["poses"], t["pm"], t["pl"] if six else None, t["tot"] if six else t["tot0"],
                         cost_type=cost_type, stride=case.stride, sensor_resolution=case.r,
                         color_distance_threshold=colour_thr, **kw)


@pytest.fixture(scope="module", params=nc.CASE_NAMES)
def ctx(request):
    case = nn_case(request.param)
    core, t = _setup(case)
    yield request.param, case, core, t
    core.close()


def test_depth_costs_select_and_second_call(ctx):
    """cost types 2 and 0; evaluate(select=...) against oracle.select; and the same again on the same context, after
    the first calls' tile-tier feedback."""
    name, case, core, t = ctx
    dev = t["poses"].device
    for call in range(2):
        _assert_costs(_evaluate(core, t, case, 2), _want(name, 2), f"{name} 6-DoF call {call}")
        _assert_costs(_evaluate(core, t, case, 0), _want(name, 0), f"{name} 3-DoF call {call}")
    keys = torch.full((2,), _native.PCORE_KEY_NONE, dtype=torch.int64, device=dev)
    got = _evaluate(core, t, case, 2, select=(keys, 1000, 2))
    _assert_costs(got, _want(name, 2), f"{name} evaluate_select")
    cost, idx = decode_keys(keys)
    ocost, oidx = oracle.select(_want(name, 2)[0], _want(name, 2)[1], case.pose_model, 2, 1000)
    assert np.array_equal(cost, ocost) and np.array_equal(idx, oidx), (cost, idx, ocost, oidx)


def test_chunked_path(ctx, monkeypatch):
    """A 64-sample LDS tile: nearly every pose is scored in chunks of the tile, and the explained bitmap accumulates
    across a pose's chunks (a tie's two candidates, a witness and its tied sample can fall into different chunks)."""
    name, case, core0, t0 = ctx
    monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    core, t = _setup(case)
    _assert_costs(_evaluate(core, t, case, 2), _want(name, 2), f"{name} 6-DoF tcap64")
    _assert_costs(_evaluate(core, t, case, 0), _want(name, 0), f"{name} 3-DoF tcap64")
    assert core.tile_info()["tcap"] == 64
    core.close()


@pytest.mark.parametrize("name", nc.COLOUR_CASES)
@pytest.mark.parametrize("tile", ["auto", "tcap64"])
def test_colour_cost(name, tile, monkeypatch):
    """cost type 1 on the tie cases (the two candidates of a tie, and two exact duplicates, are on opposite sides of
    the colour gate: the index that wins decides whether the sample is bad) and on the case with non-finite points
    (the colours of the points after them must still line up)."""
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    case = nn_case(name)
    core, t = _setup(case, colours=True)
    for call in range(2):
        _assert_costs(_evaluate(core, t, case, 1), _want(name, 1), f"{name} colour {tile} call {call}")
    core.close()


def test_no_observed_cost():
    """calc_obs_cost = False: the rendered cost is unchanged, the observed cost and the points diff are exactly 0."""
    name = "ties-r0.01"
    case = nn_case(name)
    core, t = _setup(case)
    for ct in (2, 0):
        rc, oc, df = _evaluate(core, t, case, ct, calc_obs_cost=False)
        assert np.array_equal(rc.cpu().numpy().view(np.uint32), _want(name, ct)[0].view(np.uint32))
        assert not oc.cpu().numpy().view(np.uint32).any() and not df.cpu().numpy().view(np.uint32).any()
        want = case.oracle_costs(ct, calc_obs=False)
        _assert_costs((rc, oc, df), want, f"calc_obs False, type {ct}")
    core.close()


# ---------------------------------------------------------------------------------------------
# the other grid consumers on a stretched observation
# ---------------------------------------------------------------------------------------------

def gicp_far_target_case():
    """One object on the SMALL camera: the observation is unprojected at stride 1 (a segment above kGridNNMin targets),
    one more target of the segment lies 30 m away, and 12 poses are refined from their stride-4 clouds."""
    case = SceneCase(("003_cracker_box",), n_poses=12, cam=SMALL, stride=1, k=8, gt_centers=[(0.01, -0.01, 0.45)])
    obs_xyz = np.concatenate([case.obs_xyz, [[-30.0, 0.02, 0.6]]]).astype(np.float32)  # one label: label-sorted
    obs_lab = np.concatenate([case.obs_label, [0]]).astype(np.int32)
    return case, obs_xyz, obs_lab


def test_gicp_grid_search_with_a_far_target():
    """evaluate_icp with a segment above kGridNNMin = 2,048 targets and a far target: the segment's grid cell is its
    extent / 64 and its origin is 30 m from the object (grid_shells carries its own rounding terms); poses, iteration
    counts and costs bit for bit against the oracle's brute-force scans."""
    case, obs_xyz, obs_lab = gicp_far_target_case()
    sc = case.scene
    n = len(case.poses)
    assert n <= 16 and len(obs_xyz) > 2048 + 1
    ls, le = np.array([0], np.int32), np.array([len(obs_xyz)], np.int32)
    tot = np.full(n, float(len(obs_xyz)), np.float32)
    want = oracle.evaluate_icp(sc.bank.tris, sc.bank.tris_model_count, case.poses, case.pose_model, case.pose_label,
                               sc.width, sc.height, sc.proj, sc.src_depth_cm, sc.mask, 1.0, 4, sc.cx, sc.cy, sc.fx,
                               sc.fy, 100.0, obs_xyz, oracle.covariances(obs_xyz), ls, le, tot, 2, True, 0.01)
    core = PoseCore(0)
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    dev = torch.device("cuda", 0)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    core.set_observation(up(sc.src_depth_cm), up(sc.mask), up(obs_xyz), up(obs_lab), 0.01)
    adj, iters, rc, oc, df = core.evaluate_icp(up(case.poses), up(case.pose_model), up(case.pose_label), up(tot),
                                               cost_type=2, stride=4)
    torch.cuda.synchronize()
    assert np.array_equal(iters.cpu().numpy(), want[1])
    assert np.array_equal(adj.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    _assert_costs((rc, oc, df), want[2:], "GICP with a far target")
    assert len(np.unique(want[1])) > 1  # the poses do not all stop at the same iteration
    core.close()


def planar_far_target_case():
    """The SMALL / stride 5 table-top case of tests/icp2d_reference.py, its first 16 poses, with one more observed
    point 30 m from the table in the world frame (given in the camera frame, as the observation is)."""
    c = ref2d.planar_case("SMALL", 5)
    M = c.world_from_cam.astype(np.float64)
    w = ref2d.to_world(c.world_from_cam, c.obs_xyz[:1]).astype(np.float64)[0] + np.array([-30.0, 0.0, 0.0])
    far = (np.linalg.inv(M) @ np.append(w, 1.0))[:3]
    obs = np.concatenate([c.obs_xyz, far[None]]).astype(np.float32)
    return c, obs, np.arange(16)


def test_planar_icp_with_a_far_target():
    """icp_planar against the numpy reference on a world-frame observation with a far point: planar_nn's grid takes
    its cell from the extent and its origin lies 30 m from the table."""
    c, obs, idx = planar_far_target_case()
    tgt = ref2d.to_world(c.world_from_cam, obs)
    assert tgt[:, 0].max() - tgt[:, 0].min() > 29.0
    want = ref2d.run_poses([c.clouds[i] for i in idx], obs, c.world_from_cam)
    assert (want[1] > 1).any() and len(set(int(s) for s in want[2])) >= 1
    sc = c.scene
    core = PoseCore(0)
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count)
    core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    dev = torch.device("cuda", 0)
    core.set_observation(torch.from_numpy(c.src_cm).to(dev), None, torch.from_numpy(obs).to(dev), None,
                         ref2d.SENSOR_RESOLUTION)
    out = core.icp_planar(torch.from_numpy(np.ascontiguousarray(c.poses[idx])).to(dev),
                          torch.from_numpy(np.ascontiguousarray(c.pose_model[idx])).to(dev), c.world_from_cam,
                          stride=c.stride, depth_factor=100.0, occlusion_threshold=ref2d.OCCLUSION_THRESHOLD)
    torch.cuda.synchronize()
    xf, it, st, mse = (x.cpu().numpy() for x in out)
    assert np.array_equal(st, want[2]) and np.array_equal(it, want[1])
    assert np.array_equal(xf.view(np.uint64), np.ascontiguousarray(want[0]).view(np.uint64))
    assert np.array_equal(mse.view(np.uint64), np.ascontiguousarray(want[3]).view(np.uint64))
    core.close()
