"""CPU: the oracle's restatement of cuda_icp (oracle/ref_cpu_path.cpp) and the two numpy specs (tests/p2p_reference.py,
tests/p2p_nn_reference.py) against what the reference's own sources computed on the host: tests/golden/refk_icp_*.npz
(tests/golden/make_reference_icp_goldens.py).  Bit for bit.  Only tests/golden/ is read.

Everything around the 6 x 6 solve is the reference's text; the solve is the oracle's (Eigen is not available where the
fixtures are made), so a run pins the loop, the scenes, the rows and the composition, not LDLT.

The nearest-neighbour scene.  The reference searches a kd-tree over the whole cloud, the project a window around the
point's own pixel, with the lowest pixel index on equal distances.  Where the nearest scene point is unique the two
must give the same point; where two points tie (the fixture holds such queries on purpose: nn_unique) the tree keeps
whichever it visits first, an artefact of its build order, and only the acceptance is compared.

Certificates (a fixture that no wrong rule changes tests nothing): every wrong rule of p2p_nn_reference.RULES and of
tests/refk_icp_fixtures.py must change a fixture value.  Two rules of RULES cannot, by what they are, and are held to
what they can show instead:
  "nolimit"  is the reference's own rule (its tree has no window); it must AGREE with the fixture, and the window
             tests show that a window one pixel narrower than nn_max_offset does not
  "highest"  changes only tied queries, which the comparison leaves out; on the fixture's tied queries it must give
             another winner than the spec, both of them nearest points, one of them the reference's pick
"""
import importlib.util
import os

import numpy as np
import pytest

import oracle
from oracle import ref_host
from tests import p2p_nn_reference as nn
from tests import p2p_reference as ref
from tests import refk_icp_fixtures as fxm

F = np.float32
CAMS = fxm.CAMERAS


def _scene(cam):
    fx = fxm.load(cam)
    return fx, fx["scene_pcd"], fx["scene_normal"], fxm.camera(fx)


def _run_case(fx, name, sc):
    return tuple(fx[f"run_{name}_{sc}_{k}"] for k in ("T", "fitness", "rmse", "iteration", "moved"))


def _assert_run(got, fx, name, sc, what):
    T, fit, rmse, it, moved = got
    wT, wfit, wrmse, wit, wmoved = _run_case(fx, name, sc)
    assert int(it) == int(wit[0]), (what, "iteration", int(it), int(wit[0]))
    fxm.assert_same(np.asarray(T, F).reshape(16), wT, f"{what} T")
    fxm.assert_same(np.asarray([fit], F), wfit, f"{what} fitness")
    fxm.assert_same(np.asarray([rmse], F), wrmse, f"{what} rmse")
    fxm.assert_same(np.asarray(moved, F), wmoved, f"{what} moved cloud")


# ---- the scenes and depth2cloud --------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", CAMS)
def test_oracle_scene_equals_scene_projective(cam):
    fx, pcd, nrm, c = _scene(cam)
    got_p, got_n = oracle.ref_scene(fx["depth"], *c)
    fxm.assert_same(got_p, pcd, "points")
    fxm.assert_same(got_n, nrm, "normals")


@pytest.mark.parametrize("cam", CAMS)
def test_scene_nn_shares_the_projective_points_except_where_the_conversions_differ(cam):
    """Scene_nn builds its cloud from the image saturated to uint16 (pcd_scene.cpp:11-31), Scene_projective reads the
    int32 image as uint32 (depth_scene.cpp:26).  The project searches the projective buffer in both ICPs.  The
    generator found the tree's points to be the projective points of every pixel except the ones listed here, which
    are exactly the negative pixels (no point in the tree, a point 42,949 km off in the buffer) and the pixels above
    65535 (a point at 655.35 m in the tree, at depth / 100 in the buffer): no query of a real scene reaches either."""
    fx = fxm.load(cam)
    d = fx["depth"].astype(np.int64)
    odd = (d < 0) | (d > 65535)
    assert odd.sum() >= 2 and np.array_equal(np.argwhere(odd), fx["nn_not_shared"])
    assert int(fx["nn_count"]) == (np.clip(d, 0, 65535) > 0).sum()
    assert int(fx["nn_nodes"]) % 2 == 1 and int(fx["nn_nodes"]) > int(fx["nn_count"]) // 10


@pytest.mark.parametrize("cam", CAMS)
def test_oracle_depth2cloud_equals_depth2cloud_cpu(cam):
    fx = fxm.load(cam)
    fxm.assert_same(oracle.ref_depth2cloud(fx["depth"], *fxm.camera(fx)), fx["depth2cloud"], "depth2cloud")


# ---- rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", CAMS)
def test_projective_rows_equal_thrust_pcd2ab(cam):
    fx, pcd, nrm, c = _scene(cam)
    rows, ok = ref.rows_of(fx["rows_cloud"], pcd, nrm, *c, fxm.MAX_DIST_DIFF)
    assert np.array_equal(ok, fx["proj_valid"]), np.nonzero(ok != fx["proj_valid"])[0]
    fxm.assert_same(rows, fx["proj_rows"], "rows")
    assert 0.5 < ok.mean() < 1.0


@pytest.mark.parametrize("cam", CAMS)
def test_window_query_equals_the_tree(cam):
    fx, pcd, nrm, c = _scene(cam)
    ok, win, _ = nn.query(fx["rows_cloud"], pcd, *c, fxm.NN_RADIUS, nn.WINDOW)
    assert np.array_equal(ok, fx["nn_valid"]), np.nonzero(ok != fx["nn_valid"])[0]
    cmp = ok & fx["nn_unique"]
    assert cmp.sum() >= 100 and cmp.sum() >= 0.95 * ok.sum()
    fxm.assert_same(pcd.reshape(-1, 3)[win][cmp], fx["nn_dst_pcd"][cmp], "the winner's scene point")
    rows, ok2 = nn.rows_of(fx["rows_cloud"], pcd, nrm, *c, fxm.NN_RADIUS, nn.WINDOW)
    keep = fx["nn_unique"] | ~ok                            # every row but the tied queries'
    assert np.array_equal(ok2, ok)
    fxm.assert_same(rows[keep], fx["nn_rows"][keep], "rows")


@pytest.mark.parametrize("cam", CAMS)
def test_window_claim(cam):
    """include/pcore.h: the window search is the nearest neighbour of the whole image whenever every pixel that can
    hold a point within the radius lies inside the window.  nn_max_offset is the farthest the tree's answer lies from
    a point's own pixel: a window of that size agrees with the tree, one pixel less does not."""
    fx, pcd, _, c = _scene(cam)
    w = int(fx["nn_max_offset"])
    assert 1 <= w <= nn.WINDOW
    assert np.abs(fx["nn_offset"][fx["nn_valid"]]).max() == w
    cmp = fx["nn_valid"] & fx["nn_unique"]
    ok, win, _ = nn.query(fx["rows_cloud"], pcd, *c, fxm.NN_RADIUS, w)
    assert np.array_equal(ok, fx["nn_valid"])
    fxm.assert_same(pcd.reshape(-1, 3)[win][cmp], fx["nn_dst_pcd"][cmp], "window = nn_max_offset")
    ok, win, _ = nn.query(fx["rows_cloud"], pcd, *c, fxm.NN_RADIUS, w - 1)
    assert not np.array_equal(ok, fx["nn_valid"]) or fxm.differs(pcd.reshape(-1, 3)[win][cmp], fx["nn_dst_pcd"][cmp])


# ---- the loop --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", CAMS)
def test_first_turn_measures_equal_the_reference(cam):
    fx, pcd, nrm, c = _scene(cam)
    for i, (a, b) in enumerate(fxm.rows_clouds(fx)):
        cl = fx["rows_cloud"][a:b]
        for sc, run in (("proj", lambda: ref.icp(cl, pcd, nrm, *c, order="index", trig="libm", max_iterations=0)),
                        ("nn", lambda: nn.icp(cl, pcd, nrm, *c, order="index", trig="libm", max_iterations=0))):
            _, fit, rmse, it, _ = run()
            assert it == fx[f"rows_run0_{sc}_iteration"][i] == 0
            fxm.assert_same(np.asarray([fit], F), fx[f"rows_run0_{sc}_fitness"][i:i + 1], (sc, i, "fitness"))
            if sc == "nn" and (fx["nn_valid"] & ~fx["nn_unique"])[a:b].any():
                assert b - a == max(fxm.ROWS_SIZES)          # the tied query's cloud: the rmse depends on the tree's pick
                continue
            fxm.assert_same(np.asarray([rmse], F), fx[f"rows_run0_{sc}_rmse"][i:i + 1], (sc, i, "rmse"))


@pytest.mark.parametrize("name", fxm.RUNS)
@pytest.mark.parametrize("cam", CAMS)
def test_full_runs_equal_icp_point2plane_cpu(cam, name):
    fx, pcd, nrm, c = _scene(cam)
    cl, mi = fx[f"run_{name}_cloud"], int(fx[f"run_{name}_max_iter"])
    _assert_run(oracle.ref_icp(cl, pcd, nrm, *c, max_iter=mi), fx, name, "proj", "oracle.ref_icp")
    _assert_run(ref.icp(cl, pcd, nrm, *c, order="index", trig="libm", max_iterations=mi), fx, name, "proj", "p2p_reference")
    _assert_run(nn.icp(cl, pcd, nrm, *c, order="index", trig="libm", max_iterations=mi), fx, name, "nn", "p2p_nn_reference")
    want_exit = {"none": 0, "converge": 1, "cap": 2}[name]
    for sc in fxm.SCENES:
        assert int(fx[f"run_{name}_{sc}_exit"][0]) == want_exit
    if name == "converge":
        assert all(2 <= int(fx[f"run_{name}_{sc}_iteration"][0]) < 30 for sc in fxm.SCENES)


@pytest.mark.parametrize("cam", CAMS)
def test_solver_trace_is_the_sums_in_index_order(cam):
    """What the reference's loop handed to the solver on its first call is the index-order sum of the rows of the cloud;
    what came back is the spec's LDLT and increment with libm's trigonometry (the solve is the oracle's, so this holds
    the numpy spec to the oracle, not to Eigen)."""
    fx, pcd, nrm, c = _scene(cam)
    for name in ("converge", "cap"):
        cl = fx[f"run_{name}_cloud"]
        for sc, rows_of in (("proj", lambda p: ref.rows_of(p, pcd, nrm, *c, fxm.MAX_DIST_DIFF)),
                            ("nn", lambda p: nn.rows_of(p, pcd, nrm, *c, fxm.NN_RADIUS, nn.WINDOW))):
            A, b, E = (fx[f"run_{name}_{sc}_solver_{k}"] for k in ("A", "b", "T"))
            assert len(A) == int(fx[f"run_{name}_{sc}_iteration"][0]) >= 1
            acc = ref.sum_rows(rows_of(cl)[0], "index")
            full = np.zeros((6, 6), F)
            full[np.triu_indices(6)] = acc[:21]
            full = np.where(np.tri(6, k=-1, dtype=bool), full.T, full)
            fxm.assert_same(full.reshape(36), A[0], (name, sc, "A"))
            fxm.assert_same(acc[21:27], b[0], (name, sc, "b"))
            fxm.assert_same(ref.vec6_to_mat4(ref.ldlt_solve6(acc), "libm").reshape(16), E[0], (name, sc, "increment"))


# ---- certificates ----------------------------------------------------------------------------------------------------

def _nn_changes(rule):
    """Whether the nearest-neighbour rows or acceptance under `rule` differ from the fixture on the compared queries of
    some camera."""
    for cam in CAMS:
        fx, pcd, nrm, c = _scene(cam)
        rows, ok = nn.rows_of(fx["rows_cloud"], pcd, nrm, *c, fxm.NN_RADIUS, nn.WINDOW, rule)
        keep = fx["nn_unique"] | ~fx["nn_valid"]
        if not np.array_equal(ok, fx["nn_valid"]) or fxm.differs(rows[keep], fx["nn_rows"][keep]):
            return True
    return False


@pytest.mark.parametrize("rule", [r for r in nn.RULES if r not in ("spec", "nolimit", "highest")])
def test_certificate_wrong_nearest_neighbour_rule_changes_a_fixture_value(rule):
    assert not _nn_changes("spec")
    assert _nn_changes(rule)


def test_certificate_nolimit_is_the_reference():
    assert not _nn_changes("nolimit")


@pytest.mark.parametrize("cam", CAMS)
def test_certificate_tied_queries(cam):
    fx, pcd, _, c = _scene(cam)
    tied = fx["nn_valid"] & ~fx["nn_unique"]
    assert 1 <= tied.sum() <= 0.05 * fx["nn_valid"].sum()
    pts = fx["rows_cloud"][tied]
    _, low, d_low = nn.query(pts, pcd, *c, fxm.NN_RADIUS, nn.WINDOW)
    _, high, d_high = nn.query(pts, pcd, *c, fxm.NN_RADIUS, nn.WINDOW, "highest")
    assert (low < high).all() and np.array_equal(d_low.view(np.uint32), d_high.view(np.uint32))
    flat = pcd.reshape(-1, 3)
    picked = fxm.bits(fx["nn_dst_pcd"][tied])
    assert ((picked == fxm.bits(flat[low])).all(1) | (picked == fxm.bits(flat[high])).all(1)).all()


def test_certificate_wrong_scene_rule_changes_a_normal():
    for rule in ("spec",) + fxm.SCENE_RULES:
        changed = False
        for cam in CAMS:
            fx, pcd, nrm, c = _scene(cam)
            p, n = fxm.scene_np(fx["depth"], *c, rule=rule)
            fxm.assert_same(p, pcd, f"{rule} points")
            changed |= fxm.differs(n, nrm)
        assert changed == (rule != "spec"), rule


def test_certificate_wrong_projective_rule_changes_a_row():
    for rule in ("spec",) + fxm.ROW_RULES:
        changed = False
        for cam in CAMS:
            fx, pcd, nrm, c = _scene(cam)
            rows, ok = fxm.rows_proj(fx["rows_cloud"], pcd, nrm, *c, rule=rule)
            changed |= fxm.differs(rows, fx["proj_rows"]) or not np.array_equal(ok, fx["proj_valid"])
        assert changed == (rule != "spec"), rule


@pytest.mark.parametrize("wrong", [dict(), dict(compose="right"), dict(extra_turn=False)], ids=["spec", "T E", "no extra turn"])
def test_certificate_wrong_loop_changes_a_run(wrong):
    changed = False
    for cam in CAMS:
        fx, pcd, nrm, c = _scene(cam)
        for name in fxm.RUNS:
            got = fxm.icp_loop(lambda p: ref.rows_of(p, pcd, nrm, *c, fxm.MAX_DIST_DIFF), fx[f"run_{name}_cloud"],
                               max_iterations=int(fx[f"run_{name}_max_iter"]), **wrong)
            want = _run_case(fx, name, "proj")
            changed |= any(fxm.differs(np.asarray(g, w.dtype).reshape(w.shape), w) for g, w in zip(got, want))
    assert changed == bool(wrong)


# ---- freshness -------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not (ref_host.have_reference() and os.path.isdir(os.path.join(ref_host.reference_root(), "cuda_icp"))),
                    reason=f"the reference's sources are not at {ref_host.reference_root()} (PCORE_REFERENCE_ROOT): the "
                           "fixtures cannot be regenerated here")
def test_fixtures_are_fresh():
    """Build the reference's ICP sources for the host again, regenerate both fixtures under the sanitizers and require
    the committed files byte for byte."""
    oracle.build_ref()
    path = os.path.join(fxm.GOLDEN, "make_reference_icp_goldens.py")
    spec = importlib.util.spec_from_file_location("make_reference_icp_goldens", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    committed = sorted(f for f in os.listdir(fxm.GOLDEN) if f.startswith("refk_icp_") and f.endswith(".npz"))
    assert committed == sorted(f"refk_icp_{c}.npz" for c in gen.CAMERAS)
    for cam in gen.CAMERAS:
        blob = gen.packed(gen.fixture(cam))
        assert len(blob) <= gen.MAX_BYTES, cam
        with open(os.path.join(fxm.GOLDEN, f"refk_icp_{cam}.npz"), "rb") as f:
            assert f.read() == blob, f"refk_icp_{cam}.npz is not what the generator writes"
