"""The geometry cases of tests/helpers.py (generic sample strides, fx != fy cameras, H % stride != 0) are not vacuous:
built with the oracle alone, every case has an observed cloud, mostly valid poses with several distinct costs, poses
whose sampled z-buffer reaches the first and the last sample row and column, edge poses with the in-band invalid cost,
and -- the GICP cases -- poses that converge early and poses that run into the iteration cap.  tests/test_gpu_geometry.py
runs the same table on the GPU, so a case that passes there passes on something."""
import numpy as np
import pytest

from tests import helpers
from tests.helpers import GEOMETRY_CAMERAS, GEOMETRY_CASES, GEOMETRY_GICP_CASES, case_id, geometry_case


def test_case_table_is_the_specified_one():
    want = {"ROMAN_640": (640, 480, {4, 5, 20, 32}), "KINECT2": (512, 424, {4, 16, 32}),
            "SMALL": (200, 150, {2, 4, 8, 10, 25}), "TINY": (96, 72, {1, 3, 16, 32})}
    assert len(GEOMETRY_CASES) == len(set(GEOMETRY_CASES)) == 16
    for name, (w, h, strides) in want.items():
        cam = GEOMETRY_CAMERAS[name]
        assert (cam["width"], cam["height"]) == (w, h) and cam["fx"] != cam["fy"]
        assert {s for c, s in GEOMETRY_CASES if c == name} == strides
    assert set(helpers.GEOMETRY_TIER_CASES) == {("ROMAN_640", 5), ("SMALL", 4)}
    assert set(GEOMETRY_GICP_CASES) == {("ROMAN_640", 5), ("ROMAN_640", 4), ("KINECT2", 16), ("SMALL", 8), ("TINY", 3)}
    assert set(helpers.GEOMETRY_TIER_CASES) | set(GEOMETRY_GICP_CASES) <= set(GEOMETRY_CASES)
    assert 32 <= helpers.GEOMETRY_GICP_POSES <= 64
    # H % stride != 0 is in the table, with the remainders the table was chosen for
    rem = {(c, s): GEOMETRY_CAMERAS[c]["height"] % s for c, s in GEOMETRY_CASES}
    assert rem[("KINECT2", 16)] == rem[("KINECT2", 32)] == rem[("TINY", 16)] == rem[("TINY", 32)] == 8
    assert rem[("SMALL", 4)] == 2 and rem[("SMALL", 8)] == 6


def test_anisotropic_cases_move_points_by_more_than_the_sensor_radius():
    """With fx in fy's place the lowest sample row of an ANISO case lands > 1 cm (the sensor radius of the costs) away
    at the objects' depth: every cost that depends on the unprojection changes."""
    for cs in helpers.GEOMETRY_ANISO_CASES:
        case = geometry_case(*cs)
        cam = case.cam
        v = (case.hs - 1) * case.stride - cam["cy"]
        assert abs(v / cam["fy"] - v / cam["fx"]) * 0.5 > 0.01
        adj, iters, *_ = case.oracle_icp()
        assert ((iters > 1) & (iters < 150)).sum() >= 5


@pytest.fixture(scope="module", params=GEOMETRY_CASES + helpers.GEOMETRY_ANISO_CASES, ids=case_id)
def built(request):
    case = geometry_case(*request.param)
    s = case.stride
    zs = case.oracle_render()[:, ::s, ::s].copy()
    return case, zs, case.oracle_costs(2), case.oracle_costs(0)


def test_case_shape_and_size(built):
    case, zs, (rc, oc, df), _ = built
    sc, s = case.scene, case.stride
    assert sc.width % s == 0 and sc.fx != sc.fy
    assert zs.shape == (case.n, case.hs, case.ws) and case.hs == -(-sc.height // s)
    assert case.ws * case.hs <= 19200  # the whole sampled image fits the fused kernel's LDS tile
    assert 64 <= case.n <= 80
    assert len(case.obs_xyz) > 0 and (np.bincount(case.obs_label_raw, minlength=2) > 0).all()
    assert (rc >= 0).sum() * 2 >= case.n
    assert len(np.unique(rc)) >= (3 if case.ws * case.hs >= 64 else 2)
    # the observed cost tells poses apart too (a kernel that explained nothing would not pass)
    assert len(np.unique(oc[rc >= 0])) >= 2 and (rc[rc >= 0] < 100).any()


def test_case_reaches_every_border(built):
    case, zs, (rc, _, _), _ = built
    nz = zs > 0
    hit = {"row0": nz[:, 0, :].any(1), "col0": nz[:, :, 0].any(1), "rowL": nz[:, -1, :].any(1),
           "colL": nz[:, :, -1].any(1)}
    for k, v in hit.items():
        assert v.any(), k
    assert (hit["row0"] & hit["col0"]).any()
    if case.scene.height % case.stride != 0:
        assert hit["rowL"].sum() >= 3
    # the hand-made border poses do it on their own, and so do the candidate poses (whose costs are not all 100)
    b = case.border_idx
    cand = np.arange(case.n) < b[0]
    for k, v in hit.items():
        assert v[b].any() and (v & cand & (rc >= 0) & (rc < 100)).any(), k


def test_case_edge_poses(built):
    case, zs, (rc, oc, df), (rc0, oc0, df0) = built
    e = case.edge_idx
    for kind in ("behind", "straddle_z0", "out_of_view"):
        assert not (zs[e[kind]] > 0).any(), kind
        assert rc[e[kind]] == -1.0 and rc0[e[kind]] == -1.0, kind  # the in-band invalid cost
    assert (zs[e["very_close"]] > 0).all()  # a whole-image window
    assert rc[e["very_close"]] >= 0 and rc0[e["very_close"]] >= 0


@pytest.mark.parametrize("cs", GEOMETRY_GICP_CASES, ids=case_id)
def test_gicp_case_converges_and_hits_the_cap(cs):
    case = geometry_case(*cs)
    n = helpers.GEOMETRY_GICP_POSES
    adj, iters, rc, oc, df = case.oracle_icp()
    assert len(iters) == n
    assert ((iters > 1) & (iters < 150)).sum() >= 5
    want = helpers.GEOMETRY_GICP_MIN_CAPPED.get(cs)
    if want is None:
        assert (iters == 150).sum() >= 5
    else:
        assert (iters == 150).sum() == want  # the count this case gives (stated in helpers.py)
    assert (adj != case.poses[:n]).any(1).sum() >= n // 2 and (rc >= 0).sum() >= n // 2
