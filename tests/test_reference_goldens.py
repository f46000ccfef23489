"""The oracle against the reference's own stage kernels.

tests/golden/refk_*.npz hold what the reference's image_renderer.cuh, compute_point_clouds.cuh and compute_costs.cuh
compute when they are compiled for the host and run serially (oracle/ref_host/, tests/golden/
make_reference_kernel_goldens.py).  The oracle restates those kernels from a reading of their text; the GPU kernels
follow the same reading.  Here the restatement meets the text itself: the inside test with its -0.0f, the size_t
rounding of the bounding box, the y flip, the integer occlusion rules with source_label - 1, the compaction order, the
percentage functors and the colour channel order are all in the fixtures' numbers.  Raster, clouds and costs are compared
bit for bit; the colour arithmetic, which the project defines for itself, within a bound made of
the project's documented distance to float64 and the reference-host's measured one.

The freshness test builds the reference again and requires every fixture to come out as committed; it needs the
reference's sources and is skipped where they are not."""
import importlib.util
import os

import numpy as np
import pytest

import oracle
from oracle import ref_host
from tests import refk_fixtures as rf
from tests.refk_fixtures import assert_same

CAM_TAGS = [(c, t) for c in rf.CAMERAS for t in rf.TAGS]
CASE_TAGS = [(c, s, t) for c, s in rf.CASES for t in rf.TAGS]
CASE_IDS = [rf.case_id(cs) for cs in rf.CASES]


def _ids(v):
    return "-".join(str(x) for x in v)


def _render_args(fx, six):
    return (fx["tris_model_count"], fx["poses"], fx["pose_model"], fx["pose_label"] if six else None, int(fx["width"]),
            int(fx["height"]), fx["proj"], fx["src_depth"], fx["src_mask"] if six else None,
            float(fx["occlusion_threshold"]))


# ---------------------------------------------------------------------------------------------
# raster
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam,tag", CAM_TAGS, ids=[_ids(v) for v in CAM_TAGS])
def test_render_depth(cam, tag):
    """oracle.render_depth equals image_render's z-buffers (after max -> 0): 16 poses -- at and around the source's own
    poses (|render - source| on, one short of and one beyond the threshold on both sides), with the other object's label,
    over each image border, over missing source depth, behind and across the camera plane, in front of and behind the
    other object -- and a bank that ends in two zero-area triangles."""
    fx = rf.raster(cam, tag)
    got = oracle.render_depth(fx["tris"], *_render_args(fx, tag == "6dof"))
    assert_same(got, fx["depth"], f"render_depth {cam} {tag}")


@pytest.mark.parametrize("cam,tag", CAM_TAGS, ids=[_ids(v) for v in CAM_TAGS])
def test_render_depth_color(cam, tag):
    """oracle.render_depth_color: the same z-buffers, and the colour planes wherever the reference's colour does not
    depend on the order in which a pose's triangles arrive (at least 90 % of the rendered pixels, some pixels not)."""
    fx = rf.raster(cam, tag)
    depth, col = oracle.render_depth_color(fx["tris"], fx["tri_rgb"], *_render_args(fx, tag == "6dof"))
    assert_same(depth, fx["depth"], f"render_depth_color depth {cam} {tag}")
    agree, rendered = fx["color_agree"], fx["depth"] > 0
    assert 0.90 * rendered.sum() <= (agree & rendered).sum() < rendered.sum()
    m = np.broadcast_to(agree[None], col.shape)
    assert_same(col[m], fx["color"][m], f"render_depth_color planes {cam} {tag}")
    assert (fx["color"][:, rendered & agree] > 0).any() and not fx["color"][:, fx["depth"] == 0].any()


# ---------------------------------------------------------------------------------------------
# clouds
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam,stride,tag", CASE_TAGS, ids=[_ids(v) for v in CASE_TAGS])
def test_depth_to_cloud(cam, stride, tag):
    """oracle.depth_to_cloud over the rendered z-buffers equals depth_to_mask + scan + depth_to_2d_cloud: points, pose
    map, labels and count, in the reference's order.  The stored stride mask (result_dc_index before its scan) marks
    exactly the sampled pixels with a positive depth."""
    ras, c = rf.raster(cam, tag), rf.cloud(cam, stride)
    fxc, fyc, cx, cy = rf.camera(ras)
    six = tag == "6dof"
    xyz, pose, lab = oracle.depth_to_cloud(ras["depth"], stride, cx, cy, fxc, fyc, rf.DEPTH_FACTOR,
                                           pose_label=ras["pose_label"] if six else None)
    assert len(xyz) == int(c[f"count_{tag}"]) > 0
    assert_same(xyz, np.ascontiguousarray(c[f"xyz_{tag}"].T), f"cloud xyz {cam} s{stride} {tag}")
    assert_same(pose, c[f"pose_map_{tag}"], f"cloud pose map {cam} s{stride} {tag}")
    if six:
        assert_same(lab, c["label_6dof"], f"cloud label {cam} s{stride}")
    want = np.zeros(ras["depth"].shape, np.uint8)
    want[:, ::stride, ::stride] = ras["depth"][:, ::stride, ::stride] > 0
    assert_same(c[f"dc_mask_{tag}"], want, f"stride mask {cam} s{stride} {tag}")
    planes = ras["color"][:, :, ::stride, ::stride][:, ras["depth"][:, ::stride, ::stride] > 0]
    assert_same(c[f"color_{tag}"], planes, f"cloud colours {cam} s{stride} {tag}")


@pytest.mark.parametrize("cam,stride", rf.CASES, ids=CASE_IDS)
def test_observed_cloud_with_label_mask(cam, stride):
    """oracle.depth_to_cloud with a label mask (depth2cloud_global's 6-DoF use): a raw 16-bit image at 10,000 units per
    metre, pixels without depth inside the mask, label = mask - 1."""
    ob = rf.observed(cam)
    fxc, fyc, cx, cy = rf.camera(ob)
    xyz, pose, lab = oracle.depth_to_cloud(ob["depth"], stride, cx, cy, fxc, fyc, float(ob["depth_factor"]),
                                           label_mask=ob["label_mask"])
    assert_same(xyz, np.ascontiguousarray(ob[f"s{stride}_mask_xyz"].T), f"observed xyz {cam} s{stride}")
    assert_same(lab, ob[f"s{stride}_mask_label"], f"observed label {cam} s{stride}")
    assert not pose.any() and set(np.unique(lab)) == {0, 1}


@pytest.mark.parametrize("cam,stride", rf.CASES, ids=CASE_IDS)
def test_observed_cloud_bounded(cam, stride):
    """oracle.depth_to_cloud_bounded (depth2cloud_global's 3-DoF use: camera_transform + bounds + colours): every one
    of the six bounds lies exactly on the world coordinate of a point that the reference keeps."""
    ob = rf.observed(cam)
    fxc, fyc, cx, cy = rf.camera(ob)
    xyz, rgb = oracle.depth_to_cloud_bounded(ob["depth"], stride, cx, cy, fxc, fyc, float(ob["depth_factor"]),
                                             cam_to_world=ob["camera_transform"], bounds=ob[f"s{stride}_bounds"],
                                             rgb=ob["rgb"])
    assert_same(xyz, np.ascontiguousarray(ob[f"s{stride}_bounded_xyz"].T), f"bounded xyz {cam} s{stride}")
    assert_same(rgb, np.ascontiguousarray(ob[f"s{stride}_bounded_color"].T), f"bounded colours {cam} s{stride}")
    everything, _ = oracle.depth_to_cloud_bounded(ob["depth"], stride, cx, cy, fxc, fyc, float(ob["depth_factor"]))
    assert 0 < len(xyz) < len(everything)


# ---------------------------------------------------------------------------------------------
# costs
# ---------------------------------------------------------------------------------------------

def _tag_of(cost_type):
    return "6dof" if cost_type == 2 else "3dof"


@pytest.mark.parametrize("cost_type", [0, 2])
@pytest.mark.parametrize("cam,stride", rf.CASES, ids=CASE_IDS)
def test_costs(cam, stride, cost_type):
    """oracle.costs on the fixture's neighbours equals compute_render_cost + compute_observed_cost + the functor chain:
    with the observed cost, without it (the oracle then reports zeros), and with one pose flagged occluded.  The project
    has no such flag (the reference never sets it: USE_TREE is 0): the flagged pose is scored as a pose without points,
    which gives the reference's -1 and 100; the reference's points difference of the flagged pose is 1, the -1 counted
    as an explained point (compute_costs.cuh:364-368)."""
    c = rf.cloud(cam, stride)
    tag, t = _tag_of(cost_type), f"t{cost_type}"
    n = len(c[f"rc_{t}"])
    d2, idx, pose = c[f"knn_dist_{tag}"], c[f"knn_index_{tag}"], c[f"pose_map_{tag}"]
    num_o, total, res = len(c["obs_xyz"]), c[f"obs_total_{tag}"], float(c["sensor_resolution"])
    rc, oc, df = oracle.costs(n, cost_type, True, res, d2, idx, pose, num_o, total)
    assert_same(rc, c[f"rc_{t}"], f"rendered cost {cam} s{stride} type {cost_type}")
    assert_same(oc, c[f"oc_{t}"], f"observed cost {cam} s{stride} type {cost_type}")
    assert_same(df, c[f"diff_{t}"], f"points difference {cam} s{stride} type {cost_type}")
    assert (rc == -1).any() and (rc >= 0).any()
    rc, oc, df = oracle.costs(n, cost_type, False, res, d2, idx, pose, num_o, total)
    assert_same(rc, c[f"rc_{t}_noobs"], f"rendered cost without the observed cost {cam} s{stride} type {cost_type}")
    assert not oc.any() and not df.any()
    f = int(c["flagged_pose"])
    keep = pose != f
    assert 0 < keep.sum() < len(pose)
    rc, oc, df = oracle.costs(n, cost_type, True, res, d2[keep], idx[keep], pose[keep], num_o, total)
    assert_same(rc, c[f"rc_{t}_flagged"], f"rendered cost, pose {f} flagged, {cam} s{stride} type {cost_type}")
    assert_same(oc, c[f"oc_{t}_flagged"], f"observed cost, pose {f} flagged, {cam} s{stride} type {cost_type}")
    others = np.arange(n) != f
    assert_same(df[others], c[f"diff_{t}_flagged"][others], f"points difference, pose {f} flagged")
    assert rc[f] == -1 and oc[f] == 100 and df[f] == 0 and c[f"diff_{t}_flagged"][f] == 1


@pytest.mark.parametrize("cost_type", [0, 2])
@pytest.mark.parametrize("cam,stride", rf.CASES, ids=CASE_IDS)
def test_evaluate_end_to_end(cam, stride, cost_type):
    """oracle.evaluate from the fixtures' inputs alone (triangles, poses, source image, observed cloud) equals the
    reference's costs: its own raster, compaction and 1-NN search in between."""
    tag, t = _tag_of(cost_type), f"t{cost_type}"
    ras, c, ob = rf.raster(cam, tag), rf.cloud(cam, stride), rf.observation(cam, stride)
    fxc, fyc, cx, cy = rf.camera(ras)
    six = cost_type == 2
    rc, oc, df = oracle.evaluate(ras["tris"], *_render_args(ras, six), stride, cx, cy, fxc, fyc, rf.DEPTH_FACTOR,
                                 ob["sorted_xyz"], ob["label_start"] if six else None, ob["label_end"] if six else None,
                                 c[f"obs_total_{tag}"], cost_type, True, float(c["sensor_resolution"]))
    assert_same(rc, c[f"rc_{t}"], f"evaluate rendered cost {cam} s{stride} type {cost_type}")
    assert_same(oc, c[f"oc_{t}"], f"evaluate observed cost {cam} s{stride} type {cost_type}")
    assert_same(df, c[f"diff_{t}"], f"evaluate points difference {cam} s{stride} type {cost_type}")


@pytest.mark.parametrize("cam,stride", rf.CASES, ids=CASE_IDS)
def test_evaluate_colour_end_to_end(cam, stride):
    """oracle.evaluate_colour (cost type 1) from the fixtures' inputs equals the reference's costs.  The generator makes
    sure that the colour gate decides poses, that the other channel order rgb2lab(c0, c1, c2) would decide differently,
    that no distance is within 0.05 of the gate and that the triangle order of a tie changes nothing."""
    ras, c, ob = rf.raster(cam, "3dof"), rf.cloud(cam, stride), rf.observation(cam, stride)
    fxc, fyc, cx, cy = rf.camera(ras)
    rc, oc, df = oracle.evaluate_colour(ras["tris"], ras["tri_rgb"], ras["tris_model_count"], ras["poses"],
                                        ras["pose_model"], int(ras["width"]), int(ras["height"]), ras["proj"],
                                        ras["src_depth"], float(ras["occlusion_threshold"]), stride, cx, cy, fxc, fyc,
                                        rf.DEPTH_FACTOR, ob["xyz"], ob["rgb"], c["obs_total_3dof"], True,
                                        float(c["sensor_resolution"]), float(c["color_threshold"]))
    assert_same(rc, c["rc_t1"], f"colour rendered cost {cam} s{stride}")
    assert_same(oc, c["oc_t1"], f"colour observed cost {cam} s{stride}")
    assert_same(df, c["diff_t1"], f"colour points difference {cam} s{stride}")
    if stride != max(rf.STRIDES[cam]):
        assert (c["rc_t1"] != c["rc_t0"]).any()  # the gate decided something


# ---------------------------------------------------------------------------------------------
# colour arithmetic
# ---------------------------------------------------------------------------------------------

def test_rgb2lab():
    """oracle.rgb2lab_n against the reference's rgb2lab on every grey and 4,096 colours.  The fixture's colours are the
    reference function's arguments (r, g, b); the oracle takes a colour as the cost stage passes it on, c[2] first."""
    fx = rf.load("refk_colour_lab")
    got = oracle.rgb2lab_n(np.ascontiguousarray(fx["rgb"][:, ::-1]))
    tol = rf.colour_tolerance(fx["lab_max_dev"])
    err = np.abs(got.astype(np.float64) - fx["lab"].astype(np.float64)).max()
    print(f"rgb2lab: largest distance from the reference-host {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    assert len(fx["rgb"]) == 256 + 4096 and (fx["rgb"][:256] == np.arange(256)[:, None]).all()


def test_colour_distance():
    """oracle.colour_distance_n against the reference's color_distance on 4,096 Lab pairs (equal pairs, a = b = 0, hue
    differences around 180 degrees), and the gate's decision at thresholds 10, 20 and 30 wherever the reference's
    distance is further from the threshold than the bound."""
    parts = [rf.load(f"refk_colour_distance_{p}") for p in range(2)]
    pairs = np.concatenate([p["lab_pairs"] for p in parts])
    ref = np.concatenate([p["distance"] for p in parts])
    assert len(pairs) == 4096 and parts[0]["distance_max_dev"] == parts[1]["distance_max_dev"]
    tol = rf.colour_tolerance(parts[0]["distance_max_dev"])
    got = oracle.colour_distance_n(pairs)
    err = np.abs(got - ref).max()
    print(f"colour distance: largest distance from the reference-host {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    for thr in (10.0, 20.0, 30.0):
        clear = np.abs(ref - thr) > tol
        assert clear.sum() > 4000 and (ref[clear] > thr).any() and (ref[clear] <= thr).any()
        assert np.array_equal(got[clear] > thr, ref[clear] > thr), thr


# ---------------------------------------------------------------------------------------------
# freshness
# ---------------------------------------------------------------------------------------------

@pytest.mark.skipif(not ref_host.have_reference(),
                    reason=f"the reference's sources are not at {ref_host.reference_root()} (PCORE_REFERENCE_ROOT): the "
                           "fixtures cannot be regenerated here")
def test_fixtures_are_fresh():
    """Build the reference's kernels for the host again, regenerate every fixture under the sanitizers and require the
    arrays of the committed files: same names, types, shapes and bits."""
    oracle.build_ref()
    path = os.path.join(rf.GOLDEN, "make_reference_kernel_goldens.py")
    spec = importlib.util.spec_from_file_location("make_reference_kernel_goldens", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    made = gen.fixtures()
    # refk_icp_*.npz are make_reference_icp_goldens.py's, checked by tests/test_reference_icp_goldens.py
    committed = sorted(f[:-4] for f in os.listdir(rf.GOLDEN)
                       if f.startswith("refk_") and f.endswith(".npz") and not f.startswith("refk_icp_"))
    assert committed == sorted(made)
    for name, make in made.items():
        new, old = make(), rf.load(name)
        assert sorted(new) == sorted(old), name
        for k in new:
            assert_same(np.asarray(new[k]), old[k], f"{name}.npz: {k}")
        assert len(gen.packed(new)) <= gen.MAX_BYTES, name
