"""CPU: the nearest-neighbour scene's numpy restatement (tests/p2p_nn_reference.py) -- known answers in wave order, the
bound rectangle's certificate against a whole-image brute force, and the certificates that the hand-made slots of
tests/p2p_nn_cases.py (which tests/test_gpu_p2p_nn.py runs on the GPU) change under every wrong rule they are meant to
catch: a case that no wrong rule changes tests nothing."""
import ctypes
import os

import numpy as np
import pytest

import oracle
from tests import p2p_nn_cases as cs
from tests import p2p_nn_reference as nn
from tests.helpers import SMALL, TINY

F = np.float32
I16 = np.eye(4, dtype=F)


def test_library_and_header_carry_the_entry_points():
    from perception_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pcore.h")).read()
    lib = _native.load()
    for name in ("pcore_icp_point2plane_nn", "pcore_debug_p2p_nn_clouds"):
        assert f"int {name}(" in header and name in _native.EXPORTED_SYMBOLS_WITH_DIGITS, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is not None, name
    assert lib.pcore_abi_version() == 9
    assert "typedef struct pcore_nn_icp_params" in header
    assert ctypes.sizeof(_native.NnIcpParams) == 20
    assert (_native.NN_MAX_DIST_DIFF, _native.NN_WINDOW) == (nn.MAX_DIST_DIFF, nn.WINDOW) == (0.01, 32)


def test_python_layers_route_icp_type_5():
    from perception_amd import perch_fat, staged
    from perception_amd.recognizer import PerchParams
    p = PerchParams()
    assert (p.nn_max_dist_diff, p.nn_window) == (0.01, 32)
    assert staged.ICP_P2P_NN == 5
    ps = perch_fat.ParamServer([{"perch_params": {"icp_type": 5, "nn_max_dist_diff": 0.02, "nn_window": 8}}])
    keys = {k: v[0] for k, v in perch_fat.PERCH_PARAM_DEFAULTS.items()}
    assert keys["nn_max_dist_diff"] == "nn_max_dist_diff" and keys["nn_window"] == "nn_window"
    assert perch_fat.PERCH_PARAM_DEFAULTS["nn_window"][1] == 32 and perch_fat.PERCH_PARAM_DEFAULTS["nn_max_dist_diff"][1] == 0.01
    assert ps.get("/perch_params/nn_window", 32) == 8


# -- 1. known answers in wave order -----------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [0, 4, 32])
def test_the_scenes_own_points_give_identity_at_iteration_1(window):
    _, pcd, nrm = cs.dyadic_scene()
    cloud = pcd[pcd[..., 2] > 0]
    assert len(cloud) > 1000
    T, fit, rmse, it, moved = nn.icp(cloud, pcd, nrm, *cs.CAM, window=window)
    assert np.array_equal(T, I16) and fit == 1 and rmse == 0 and it == 1
    assert nn.same_bits(moved, cloud)


def test_clouds_without_a_correspondence_give_identity_at_iteration_0():
    _, pcd, nrm = cs.dyadic_scene()
    behind = pcd[pcd[..., 2] > 0][:100] * F((1, 1, -1))
    out_of_window = (cs.P(20, 15)[None, :] + np.array([[3.0, 0, 0], [0, -3.0, 0]])).astype(F)  # 192 pixels off
    far = pcd[pcd[..., 2] > 0][:100] + F((0, 0, 0.02))     # in the window, 2 cm off at r = 1 cm
    for cloud in (np.zeros((0, 3), F), behind, out_of_window, far):
        T, fit, rmse, it, moved = nn.icp(cloud, pcd, nrm, *cs.CAM, window=128)
        assert np.array_equal(T, I16) and fit == 0 and rmse == 0 and it == 0
        assert nn.same_bits(moved, cloud)
    assert nn.icp(far, pcd, nrm, *cs.CAM, max_dist_diff=0.03)[1] == 1


def test_max_iterations_0_scores_and_leaves_the_cloud():
    c = cs.dyadic_slots(0.03)
    cloud = c["clouds"][4]
    T, fit, rmse, it, moved = nn.icp(cloud, c["pcd"], c["nrm"], *c["cam"], max_dist_diff=0.03, max_iterations=0)
    assert np.array_equal(T, I16) and it == 0 and 0 < fit < 1 and rmse > 0 and nn.same_bits(moved, cloud)
    ok, _, _ = nn.query(cloud, c["pcd"], *c["cam"], max_dist_diff=0.03)
    assert fit == F(F(ok.sum()) / F(len(cloud)))


# -- 2. the bound rectangle -----------------------------------------------------------------------------------------------

def _bound_rectangle(s, rho, fx, fy, cx, cy):
    """The rectangle of DESIGN.md section 5 in Python floats: every pixel that can hold a point within rho of s."""
    z_lo, z_hi = max(s[2] - rho, 0.01), s[2] + rho
    out = []
    for v, f, c in ((s[0], fx, cx), (s[1], fy, cy)):
        e = [f * a / z + c for a in (v - rho, v + rho) for z in (z_lo, z_hi)]
        out += [int(np.floor(min(e))) - 1, int(np.ceil(max(e))) + 1]
    return out  # c_lo, c_hi, q_lo, q_hi


@pytest.mark.parametrize("cam", [TINY, SMALL], ids=["96x72", "200x150"])
@pytest.mark.parametrize("r", [0.01, 0.03, 0.1])
def test_window_that_holds_the_bound_rectangle_is_the_whole_image_search(cam, r):
    Wc, Hc = cam["width"], cam["height"]
    fx, fy, cx, cy = (float(F(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    rng = np.random.default_rng(Wc + int(r * 1000))
    x, y = np.meshgrid(np.arange(Wc), np.arange(Hc))
    d = np.round(85 + 0.2 * (x - Wc / 2) + 0.12 * (y - Hc / 2) + rng.integers(-1, 2, (Hc, Wc))).astype(np.int32)
    d[:, Wc // 2 + 7:] += 14
    d[rng.random((Hc, Wc)) < 0.05] = 0
    ax, ay, half = int(round(cx)), int(round(cy)), int(r / 0.85 * fx) + 4
    d[ay - half:ay + half + 1, ax - half:ax + half + 1] = 85  # level around the axis: the nearest there is the lateral one
    pcd, _ = oracle.ref_scene(d, fx, fy, cx, cy)
    n = 300
    px = np.stack([rng.integers(0, Wc, n), rng.integers(0, Hc, n)], 1)
    base = pcd[px[:, 1], px[:, 0]].astype(np.float64)
    base[base[:, 2] == 0] = pcd[Hc // 2, Wc // 2 - 3]
    scale = rng.choice([0.0, 0.4, 0.9, 0.999999, 1.0, 1.000001, 1.2, 4.0], n) * r  # on the surface ... far off
    dirs = rng.normal(size=(n, 3))
    pts = (base + dirs / np.linalg.norm(dirs, axis=1)[:, None] * scale[:, None]).astype(F)
    pts[::23, 2] = 0.012                                   # near the camera plane
    pts[::29, 2] *= -1                                     # behind it
    # exactly at r and one float either side, next to the pixel nearest the optical axis
    axis = pcd[ay, ax]
    pts[:3] = cs.radius_points(axis, r)
    window = 0
    for s in pts[pts[:, 2] > 0]:
        c_lo, c_hi, q_lo, q_hi = _bound_rectangle([float(v) for v in s], r, fx, fy, cx, cy)
        xc, yc = int(s[0] / s[2] * fx + cx + 0.5), int(s[1] / s[2] * fy + cy + 0.5)
        need = max(xc - max(c_lo, 0), min(c_hi, Wc - 1) - xc, yc - max(q_lo, 0), min(q_hi, Hc - 1) - yc)
        window = max(window, need)
    assert window > 4                                      # the certificate is not about the centre pixel
    ok_w, idx_w, d2_w = nn.query(pts, pcd, fx, fy, cx, cy, r, window)
    ok_b, idx_b, d2_b = nn.query(pts, pcd, fx, fy, cx, cy, r, 0, rule="nolimit")
    assert np.array_equal(ok_w, ok_b) and np.array_equal(idx_w[ok_b], idx_b[ok_b])
    assert ok_b.sum() > n // 8 and (~ok_b).sum() > n // 8
    assert ok_b[:3].tolist() == [False, True, False] and d2_b[0] == F(F(r) * F(r))  # strict at fl(r r) itself
    ok_s, idx_s, _ = nn.query(pts, pcd, fx, fy, cx, cy, r, 0)  # and the centre pixel alone is not enough
    assert not (np.array_equal(ok_s, ok_b) and np.array_equal(idx_s[ok_b], idx_b[ok_b]))


# -- 3. the hand-made slots can fail --------------------------------------------------------------------------------------

# wrong rule -> (radius, window) at which it has to change the named groups' queries
CERTIFICATES = {
    "inclusive": [((r, w), ("radius",)) for r in cs.RADII for w in cs.WINDOWS],
    "highest": [((0.03, 1), ("tie2", "tie4")), ((0.1, 32), ("tie2", "tie4")), ((0.01, 4), ("tie2",))],
    "centre": [((0.03, 4), ("tie2", "tie4", "edge", "holes", "beyond_window")), ((0.1, 32), ("corners",))],
    "nolimit": [((0.03, 1), ("beyond_window", "holes")), ((0.1, 1), ("corners",)), ((0.03, 0), ("edge", "tie4"))],
    "depth0": [((r, w), ("depth0",)) for r in cs.RADII for w in (0, 4, 128)],
    "projective": [((0.03, 4), ("edge", "holes", "beyond_window", "tie4")), ((0.1, 32), ("corners",))],
}


@pytest.mark.parametrize("rule", sorted(CERTIFICATES))
def test_every_adversarial_group_changes_under_its_wrong_rule(rule):
    for (r, w), groups in CERTIFICATES[rule]:
        c = cs.dyadic_slots(r)
        for slot in (2, 4, 6):                             # 63, 65 and 129 points
            cloud = c["clouds"][slot]
            args = (cloud, c["pcd"], c["nrm"], *c["cam"])
            spec_rows, spec_ok = nn.rows_of(*args, r, w)
            bad_rows, bad_ok = nn.rows_of(*args, r, w, rule=rule)
            for g in groups:                               # the group's own queries change ...
                i = c["where"][g]
                assert (spec_ok[i] != bad_ok[i]).any() or (spec_rows[i] != bad_rows[i]).any(), (rule, r, w, g)
            good = nn.icp(*args, max_dist_diff=r, window=w, max_iterations=2)  # ... and so does the pose's result
            bad = nn.icp(*args, max_dist_diff=r, window=w, max_iterations=2, rule=rule)
            assert not (nn.same_bits(good[0], bad[0]) and nn.same_bits(good[1], bad[1]) and
                        nn.same_bits(good[2], bad[2])), (rule, r, w, slot)


def test_the_slots_hold_what_they_claim():
    _, pcd, nrm = cs.dyadic_scene()
    for r in cs.RADII:
        c = cs.dyadic_slots(r)
        assert [len(x) for x in c["clouds"]] == list(cs.SLOT_SIZES)
        cloud = c["clouds"][4]
        ok, idx, d2 = nn.query(cloud, pcd, *cs.CAM, r, 32)
        i = c["where"]["radius"]
        rr = F(F(r) * F(r))
        assert d2[i].tolist() == [rr, np.nextafter(rr, F(0)), np.nextafter(rr, F(1))] and ok[i].tolist() == [False, True, False]
        assert (idx[i] == 15 * cs.W + 20).all()
        assert not ok[c["where"]["not_a_query"]].any() and not ok[c["where"]["depth0"]].any()
        if r >= 0.03:
            t2, t4 = c["where"]["tie2"], c["where"]["tie4"]
            assert ok[t2].all() and ok[t4].all()
            assert idx[t2].tolist() == [10 * cs.W + 5, 4 * cs.W + 33]                 # the lower column; the upper row
            assert idx[t4].tolist() == [19 * cs.W + 12, 24 * cs.W + 16]               # the lowest index of four
            z = c["where"]["zero_normal"]
            assert ok[z].all() and not nrm.reshape(-1, 3)[idx[z]].any()               # counted, with a zero row
            rows, _ = nn.rows_of(cloud, pcd, nrm, *cs.CAM, r, 32)
            assert (rows[z, :28] == 0).all() and (rows[z, 28] == 1).all()
            e = c["where"]["edge"]
            assert ok[e].all() and (idx[e] % cs.W == 29).all()                        # not the projected column 30
        # one pixel beyond the window is not taken: the nearest of the whole image lies two pixels from the centre
        b = c["where"]["beyond_window"]
        ok1, idx1, _ = nn.query(cloud, pcd, *cs.CAM, r, 1)
        okn, idxn, _ = nn.query(cloud, pcd, *cs.CAM, r, 0, rule="nolimit")
        if r >= 0.03:
            assert okn[b].all() and (not ok1[b].any() or (idx1[b] != idxn[b]).all())
    sizes = sorted({int(k) for k in map(len, cs.tiny_slots()["clouds"])})
    assert sizes == sorted(cs.TINY_SIZES)
