"""The HIP kernels against the reference's own stage kernels.

tests/golden/refk_*.npz hold what the reference's image_renderer.cuh, compute_point_clouds.cuh and compute_costs.cuh
compute when they run serially on the host (tests/golden/make_reference_kernel_goldens.py; tests/
test_reference_goldens.py holds the oracle to the same files).  Only tests/golden/ is read here.  Through the C ABI:
pcore_render (z-buffers and colour planes), pcore_depth_to_cloud_ex, pcore_observed_cloud,
pcore_observed_cloud_bounded, and pcore_evaluate for cost types 0, 1 and 2 with its sampled z-buffer -- all bit for
bit -- and the two colour hooks within the colour spec's bound.  The evaluation runs with the automatic tile and with
PCORE_FUSED_TCAP=64 (the only switch the tile has: every pose then goes through the fused kernel in chunks)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from perception_amd.core import PoseCore
from perception_amd.model import compute_proj
from tests import refk_fixtures as rf
from tests.refk_fixtures import assert_same

pytestmark = pytest.mark.gpu

CAM_TAGS = [(c, t) for c in rf.CAMERAS for t in rf.TAGS]
CASE_TAGS = [(c, s, t) for c, s in rf.CASES for t in rf.TAGS]
CASE_IDS = [rf.case_id(cs) for cs in rf.CASES]


def _ids(v):
    return "-".join(str(x) for x in v)


def _up(a):
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))  # a copy: the fixtures are read-only


def _core(fx, meshes=None):
    """A context with the fixture's camera and, when given, the raster fixture's bank with its triangle colours."""
    core = PoseCore(0)
    fxc, fyc, cx, cy = rf.camera(fx)
    if meshes is not None:
        core.upload_meshes(meshes["tris"], meshes["tris_model_count"], colors=meshes["tri_rgb"])
    W, H = int(fx["width"]), int(fx["height"])
    proj = compute_proj(fxc, fyc, cx, cy, W, H)
    assert "proj" not in fx or np.array_equal(proj, fx["proj"])
    core.set_camera(W, H, fxc, fyc, cx, cy, proj)
    return core


@pytest.mark.parametrize("cam,tag", CAM_TAGS, ids=[_ids(v) for v in CAM_TAGS])
def test_render(cam, tag):
    """pcore_render equals image_render: the z-buffers everywhere, the colour planes wherever the reference's colour
    does not depend on the order in which a pose's triangles arrive."""
    fx = rf.raster(cam, tag)
    six = tag == "6dof"
    core = _core(fx, fx)
    src, mask = _up(fx["src_depth"]), _up(fx["src_mask"]) if six else None
    ob = rf.observation(cam, rf.STRIDES[cam][1])  # the render reads only the source image of the observation
    core.set_observation(src, mask, _up(ob["xyz"]), _up(ob["label"]), 0.01)
    depth, col = core.render(_up(fx["poses"]), _up(fx["pose_model"]), _up(fx["pose_label"]) if six else None,
                             occlusion_threshold=float(fx["occlusion_threshold"]), color=True)
    torch.cuda.synchronize()
    depth, col = depth.cpu().numpy(), col.cpu().numpy()
    core.close()
    assert_same(depth, fx["depth"], f"pcore_render depth {cam} {tag}")
    m = np.broadcast_to(fx["color_agree"][None], col.shape)
    assert_same(col[m], fx["color"][m], f"pcore_render colour planes {cam} {tag}")


@pytest.mark.parametrize("cam,stride,tag", CASE_TAGS, ids=[_ids(v) for v in CASE_TAGS])
def test_depth_to_cloud_ex(cam, stride, tag):
    """pcore_depth_to_cloud_ex over the reference's z-buffers and colour planes equals depth_to_mask + scan +
    depth_to_2d_cloud: points, pose map, labels, point colours, result_dc_index and the count."""
    ras, c = rf.raster(cam, tag), rf.cloud(cam, stride)
    six = tag == "6dof"
    core = _core(ras)
    out = core.depth_to_cloud(_up(ras["depth"]), stride, rf.DEPTH_FACTOR, pose_label=_up(ras["pose_label"]) if six else None,
                              color_planes=_up(ras["color"]), dc_index=True)
    torch.cuda.synchronize()
    xyz, pose, lab, col, dc = (t.cpu().numpy() for t in out)
    core.close()
    assert len(xyz) == int(c[f"count_{tag}"])
    assert_same(xyz, np.ascontiguousarray(c[f"xyz_{tag}"].T), f"cloud xyz {cam} s{stride} {tag}")
    assert_same(pose, c[f"pose_map_{tag}"], f"cloud pose map {cam} s{stride} {tag}")
    if six:
        assert_same(lab, c["label_6dof"], f"cloud label {cam} s{stride}")
    assert_same(np.ascontiguousarray(col), c[f"color_{tag}"], f"cloud colours {cam} s{stride} {tag}")
    assert_same(dc, rf.dc_index(c[f"dc_mask_{tag}"]), f"dc_index {cam} s{stride} {tag}")


@pytest.mark.parametrize("cam,stride", rf.CASES, ids=CASE_IDS)
def test_observed_clouds(cam, stride):
    """pcore_observed_cloud (label mask) and pcore_observed_cloud_bounded (camera_transform + bounds + colours, a kept
    point exactly on each of the six bounds) equal depth2cloud_global's two uses of the cloud kernels."""
    ob = rf.observed(cam)
    core = _core(ob)
    depth = _up(ob["depth"])
    xyz, lab = core.observed_cloud(depth, _up(ob["label_mask"]), stride, float(ob["depth_factor"]))
    bxyz, brgb = core.observed_cloud_bounded(depth, stride, float(ob["depth_factor"]), cam_to_world=ob["camera_transform"],
                                             bounds=ob[f"s{stride}_bounds"], rgb=_up(ob["rgb"]))
    torch.cuda.synchronize()
    xyz, lab, bxyz, brgb = (t.cpu().numpy() for t in (xyz, lab, bxyz, brgb))
    core.close()
    assert_same(xyz, np.ascontiguousarray(ob[f"s{stride}_mask_xyz"].T), f"observed xyz {cam} s{stride}")
    assert_same(lab, ob[f"s{stride}_mask_label"], f"observed label {cam} s{stride}")
    assert_same(bxyz, np.ascontiguousarray(ob[f"s{stride}_bounded_xyz"].T), f"bounded xyz {cam} s{stride}")
    assert_same(brgb, np.ascontiguousarray(ob[f"s{stride}_bounded_color"].T), f"bounded colours {cam} s{stride}")


@pytest.mark.parametrize("tile", ["auto", "tcap64"])
@pytest.mark.parametrize("cam,stride", rf.CASES, ids=CASE_IDS)
def test_evaluate(cam, stride, tile, monkeypatch):
    """pcore_evaluate from the fixtures' inputs (triangles, poses, source image, observed cloud): d_dbg_zs equals the
    reference's z-buffers at the samples, and rc / oc / diff equal compute_costs for cost types 0, 1 and 2, with the
    observed cost and without it."""
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    c, ob = rf.cloud(cam, stride), rf.observation(cam, stride)
    r3, r6 = rf.raster(cam, "3dof"), rf.raster(cam, "6dof")
    core = _core(r6, r6)
    res, thr = float(c["sensor_resolution"]), float(c["color_threshold"])
    core.set_observation(_up(r6["src_depth"]), _up(r6["src_mask"]), _up(ob["xyz"]), _up(ob["label"]), res)
    core.set_observation_colors(_up(ob["rgb"]))
    poses, pm, pl = _up(r6["poses"]), _up(r6["pose_model"]), _up(r6["pose_label"])
    n = len(r6["poses"])
    hs, ws = -(-int(r6["height"]) // stride), int(r6["width"]) // stride
    got = {}
    for cost_type in (0, 1, 2):
        six = cost_type == 2
        tag = "6dof" if six else "3dof"
        tot = _up(c[f"obs_total_{tag}"])
        for calc in (True, False):
            dbg = torch.full((n, hs, ws), -7, dtype=torch.int32, device=poses.device)
            out = core.evaluate(poses, pm, pl if six else None, tot, cost_type=cost_type, calc_obs_cost=calc, stride=stride,
                                depth_factor=rf.DEPTH_FACTOR, sensor_resolution=res,
                                occlusion_threshold=float(r6["occlusion_threshold"]), dbg_zs=dbg,
                                color_distance_threshold=thr)
            torch.cuda.synchronize()
            got[cost_type, calc] = tuple(t.cpu().numpy() for t in out) + (dbg.cpu().numpy(),)
    if tile == "tcap64":
        assert core.tile_info()["tcap"] == min(64, hs * ws)  # the knob is capped at the image's samples (30 at 96x72, stride 16)
    core.close()
    for (cost_type, calc), (rc, oc, df, zs) in got.items():
        t, ras = f"t{cost_type}", r6 if cost_type == 2 else r3
        what = f"{cam} s{stride} type {cost_type} calc_obs {calc} tile {tile}"
        assert_same(zs, np.ascontiguousarray(ras["depth"][:, ::stride, ::stride]), f"sampled z-buffer {what}")
        if calc:
            assert_same(rc, c[f"rc_{t}"], f"rendered cost {what}")
            assert_same(oc, c[f"oc_{t}"], f"observed cost {what}")
            assert_same(df, c[f"diff_{t}"], f"points difference {what}")
        else:
            assert_same(rc, c[f"rc_{t}_noobs"], f"rendered cost {what}")
            assert not oc.any() and not df.any(), what


def test_colour_hooks():
    """pcore_debug_rgb2lab and pcore_debug_colour_distance against the reference's rgb2lab and color_distance, within
    the project's documented 1e-4 to float64 plus the reference-host's own measured distance from float64 (stored in the
    fixture); and the gate's decision at thresholds 10, 20 and 30 wherever the reference's distance is further from the
    threshold than that bound."""
    fx = rf.load("refk_colour_lab")
    lab = PoseCore.rgb2lab(np.ascontiguousarray(fx["rgb"][:, ::-1]))  # the hook takes a colour as the cost passes it: c[2] first
    tol = rf.colour_tolerance(fx["lab_max_dev"])
    err = np.abs(lab.astype(np.float64) - fx["lab"].astype(np.float64)).max()
    print(f"pcore_debug_rgb2lab: largest distance from the reference-host {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    parts = [rf.load(f"refk_colour_distance_{p}") for p in range(2)]
    pairs = np.concatenate([p["lab_pairs"] for p in parts])
    ref = np.concatenate([p["distance"] for p in parts])
    tol = rf.colour_tolerance(parts[0]["distance_max_dev"])
    core = PoseCore(0)
    got = core.colour_distance(_up(pairs))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    core.close()
    err = np.abs(got - ref).max()
    print(f"pcore_debug_colour_distance: largest distance from the reference-host {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    for thr in (10.0, 20.0, 30.0):
        clear = np.abs(ref - thr) > tol
        assert clear.sum() > 4000
        assert np.array_equal(got[clear] > thr, ref[clear] > thr), thr
