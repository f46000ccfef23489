"""GPU: the 3-DoF table-top search (f4) end to end -- bounded observed cloud, x / y / yaw grid with
IsValidPose, cylinder observed totals, cost_type 0 scoring and selection -- against the oracle on the
same candidate states."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import synthetic as syn
from perception_amd.recognizer import CameraIntrinsics, ModelMetaData, preprocessing_transform
from perception_amd.tabletop import TableParams, TabletopRecognizer, pr2_gpu_params
from tests.helpers import ROMAN_640, oracle_render_fn

pytestmark = pytest.mark.gpu


def _scene(colors=None, cam=syn.CAM_640):
    names = ["003_cracker_box", "005_tomato_soup_can"]
    placements = [(0.60, -0.08, 0.4), (0.64, 0.10, 0.0)]
    bank = syn.model_bank(names)
    pre = [preprocessing_transform(m, six_dof=False) for m in bank.models]
    sc = syn.make_tabletop_scene(names, placements, pre, oracle_render_fn, table_height=0.7, cam=cam,
                                 rng=np.random.default_rng(4), colors=colors)
    return names, placements, sc


@pytest.mark.parametrize("cylinder", [True, False])
def test_tabletop_localization_matches_oracle(cylinder):
    names, placements, sc = _scene()
    table = TableParams(x_min=0.48, x_max=0.76, y_min=-0.2, y_max=0.2, table_height=0.7, res=0.04)
    bank = {n: ModelMetaData(n, model=sc.bank.models[i]) for i, n in enumerate(names)}
    cam = CameraIntrinsics(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy)
    rec = TabletopRecognizer(bank, cam, table, pr2_gpu_params(use_color_cost=False, use_cylinder_observed=cylinder))
    res = rec.localize(names, sc.depth_raw, sc.camera_pose, sc.depth_factor)
    states = rec.generate_successor_states()
    assert len(states) > 100
    mats = rec._pose_in_cam(states)
    pm = np.array([s[0] for s in states], np.int32)
    tot = rec._obs_totals(states)
    obs = rec.obs_xyz_host
    # bounded observed cloud vs the oracle
    oxyz, _ = oracle.depth_to_cloud_bounded(sc.depth_raw, rec.params.gpu_stride, sc.cx, sc.cy, sc.fx, sc.fy,
                                            sc.depth_factor, rec.transform, rec.bounds)
    assert np.array_equal(obs, oxyz)
    src_cm = (sc.depth_raw.astype(np.float32) / (np.float32(sc.depth_factor) / np.float32(100))).astype(np.int32)
    rc, oc, df = oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, mats, pm, None, sc.width, sc.height, sc.proj,
                                 src_cm, None, rec.params.gpu_occlusion_threshold, rec.params.gpu_stride, sc.cx,
                                 sc.cy, sc.fx, sc.fy, 100.0, obs, None, None, tot, 0, True,
                                 rec.params.sensor_resolution)
    g_rc, g_oc, g_df = rec._last_costs
    assert np.array_equal(g_rc.view(np.uint32), rc.view(np.uint32))
    assert np.array_equal(g_oc.view(np.uint32), oc.view(np.uint32))
    bc, bi = oracle.select(rc, oc, pm, len(names))
    got = {m: (cost, idx) for m, cost, idx, _ in res}
    for m in range(len(names)):
        if bi[m] >= 0:
            assert got[m] == (int(bc[m]), int(bi[m]))
    # No accuracy assertion here: with the table inside the bounds the observed totals count thousands
    # of table points, oc saturates near 100 and the reference's |rc - oc| < 30 filter
    # (search_env.cpp:2022-2048) rejects the near-perfect poses -- the selection above is still exactly
    # the reference's rule on exactly the oracle's costs.
    assert len(res) >= 1


@pytest.mark.parametrize("tile,gpu_stride,cam_name", [
    pytest.param("auto", 4, "640", id="auto"), pytest.param("tcap64", 4, "640", id="tcap64"),
    pytest.param("auto", 8, "640", id="auto-s8"), pytest.param("tcap64", 8, "640", id="tcap64-s8"),
    pytest.param("auto", 5, "640", id="auto-s5"), pytest.param("tcap64", 5, "640", id="tcap64-s5"),
    pytest.param("auto", 5, "roman", id="auto-s5-roman")])
def test_tabletop_colour_cost_matches_oracle(tile, gpu_stride, cam_name, monkeypatch):
    """cost_type 1: the colour id pass (nearest fragment's triangle) and the CIEDE2000 gate, bit-exact -- with
    the chosen LDS tile and with a 64-sample tile that scores nearly every pose in chunks of the tile (the colour
    ids are indexed within the chunk).  The colour kernel is the generic-stride instantiation at every stride: the
    reference's stride 4, stride 8 (which the depth costs serve with the constant-stride kernel), stride 5, and
    stride 5 on the reference's 640 x 480 camera with fx != fy."""
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    names, placements, sc = _scene(colors=[(200, 40, 30), (30, 60, 190)],
                                   cam=syn.CAM_640 if cam_name == "640" else ROMAN_640)
    table = TableParams(x_min=0.52, x_max=0.68, y_min=-0.16, y_max=0.16, table_height=0.7, res=0.04)
    bank = {n: ModelMetaData(n, model=sc.bank.models[i]) for i, n in enumerate(names)}
    cam = CameraIntrinsics(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy)
    # IsValidPose's neighbour count scales with the cloud's density, 1 / stride^2 (30 at the reference's stride 4)
    rec = TabletopRecognizer(bank, cam, table, pr2_gpu_params(
        gpu_stride=gpu_stride, min_neighbor_points_for_valid_pose=round(30 * 16 / gpu_stride ** 2)))
    assert rec.params.use_color_cost and rec.params.gpu_stride == gpu_stride
    assert gpu_stride != 4 or rec.params.min_neighbor_points_for_valid_pose == 30
    assert sc.fx == sc.fy if cam_name == "640" else sc.fx != sc.fy
    res = rec.localize(names, sc.depth_raw, sc.camera_pose, sc.depth_factor, rgb=sc.rgb)
    assert rec.use_colour and rec._cost_type() == 1
    states = rec.generate_successor_states()
    assert len(states) >= 16
    mats = rec._pose_in_cam(states)
    pm = np.array([s[0] for s in states], np.int32)
    tot = rec._obs_totals(states)
    src_cm = (sc.depth_raw.astype(np.float32) / (np.float32(sc.depth_factor) / np.float32(100))).astype(np.int32)
    rc, oc, df = oracle.evaluate_colour(sc.bank.tris, sc.bank.colors, sc.bank.tris_model_count, mats, pm, sc.width,
                                        sc.height, sc.proj, src_cm, rec.params.gpu_occlusion_threshold,
                                        rec.params.gpu_stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0, rec.obs_xyz_host,
                                        rec.obs_rgb.cpu().numpy(), tot, True, rec.params.sensor_resolution,
                                        rec.params.color_distance_threshold)
    g_rc, g_oc, g_df = rec._last_costs
    assert np.array_equal(g_rc.view(np.uint32), rc.view(np.uint32))
    assert np.array_equal(g_oc.view(np.uint32), oc.view(np.uint32))
    assert np.array_equal(g_df.view(np.uint32), df.view(np.uint32))
    bc, bi = oracle.select(rc, oc, pm, len(names))
    got = {m: (cost, idx) for m, cost, idx, _ in res}
    for m in range(len(names)):
        if bi[m] >= 0:
            assert got[m] == (int(bc[m]), int(bi[m]))
    if tile != "auto":
        return
    # the colour gate matters: a wrongly coloured model explains nothing near the red box
    rc_depth, _, _ = oracle.evaluate(sc.bank.tris, sc.bank.tris_model_count, mats, pm, None, sc.width, sc.height,
                                     sc.proj, src_cm, None, rec.params.gpu_occlusion_threshold, rec.params.gpu_stride,
                                     sc.cx, sc.cy, sc.fx, sc.fy, 100.0, rec.obs_xyz_host, None, None, tot, 0, True,
                                     rec.params.sensor_resolution)
    assert (rc > rc_depth).any()
