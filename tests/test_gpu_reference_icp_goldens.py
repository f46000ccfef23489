"""GPU: the scene kernel and the two point-to-plane ICP kernels against what the reference's own cuda_icp sources
computed on the host: tests/golden/refk_icp_*.npz (tests/golden/make_reference_icp_goldens.py; the CPU side is
tests/test_reference_icp_goldens.py).  Only tests/golden/ is read.

The kernel adds its rows in wave order with the spec's trigonometry, the reference in index order with libm's: two
build-owned choices.  So the first turn is held to the reference's own rows, summed in wave order
by tests/p2p_reference.py -- the per-point arithmetic is then the reference's and only the order is ours -- and the
full runs to the reference's results within order_trig_dev, the measured price of exactly those two choices on each
case, with no margin: the kernel equals the (wave, spec) evaluation bit for bit by tests/test_gpu_p2p.py and
tests/test_gpu_p2p_nn.py, so its distance from the reference is the stored one.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from perception_amd.core import PoseCore
from tests import p2p_nn_reference as nn
from tests import p2p_reference as ref
from tests import refk_icp_fixtures as fxm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CAMS = fxm.CAMERAS
HOOK = {"proj": dict(scene="projective", max_dist_diff=fxm.MAX_DIST_DIFF),
        "nn": dict(scene="nn", max_dist_diff=fxm.NN_RADIUS, window=nn.WINDOW)}


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)  # the fixtures are read-only


def _pad(a):
    return np.concatenate([a, np.zeros(a.shape[:2] + (1,), F)], -1)


def _slots(clouds):
    cap = max(len(c) for c in clouds) + 3
    xyzw = np.full((len(clouds), cap, 4), np.nan, F)       # past a slot's count: never read
    for i, c in enumerate(clouds):
        xyzw[i, :len(c), :3] = c
        xyzw[i, :len(c), 3] = 1.0
    return xyzw, np.array([len(c) for c in clouds], np.int32)


def _run(fx, clouds, sc, max_iterations):
    xyzw, cnt = _slots(clouds)
    out = PoseCore(0).p2p_clouds(_dev(xyzw), _dev(cnt), _dev(_pad(fx["scene_pcd"])), _dev(_pad(fx["scene_normal"])),
                                 *fxm.camera(fx), max_iterations=max_iterations, **HOOK[sc])
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _reference_rows(fx, sc):
    """The reference's rows of the rows clouds.  A tied nearest-neighbour query (the fixture holds one on purpose) has
    two nearest points; the reference's tree keeps the one it visits first, the project the lowest pixel index, a
    documented difference: that query's row is the spec's."""
    rows = fx[f"{sc}_rows"]
    if sc == "nn":
        tied = fx["nn_valid"] & ~fx["nn_unique"]
        assert 1 <= tied.sum() <= 2
        spec, _ = nn.rows_of(fx["rows_cloud"], fx["scene_pcd"], fx["scene_normal"], *fxm.camera(fx), fxm.NN_RADIUS, nn.WINDOW)
        rows = np.where(tied[:, None], spec, rows)
    return rows


@pytest.mark.parametrize("cam", CAMS)
def test_scene_kernel_equals_scene_projective(cam):
    fx = fxm.load(cam)
    pcd, nrm = PoseCore(0).scene_projective(_dev(fx["depth"]), *fxm.camera(fx))
    torch.cuda.synchronize()
    fxm.assert_same(pcd.cpu().numpy(), fx["scene_pcd"], "points")
    fxm.assert_same(nrm.cpu().numpy(), fx["scene_normal"], "normals")


@pytest.mark.parametrize("sc", fxm.SCENES)
@pytest.mark.parametrize("cam", CAMS)
def test_first_turn_on_the_references_rows(cam, sc):
    fx = fxm.load(cam)
    spans = fxm.rows_clouds(fx)
    clouds = [fx["rows_cloud"][a:b] for a, b in spans]
    rows = _reference_rows(fx, sc)
    sums = [ref.sum_rows(rows[a:b], "wave") for a, b in spans]
    assert [b - a for a, b in spans] == list(fxm.ROWS_SIZES) and all(s[28] > 0 for s in sums[1:])
    T, fit, rmse, it = _run(fx, clouds, sc, 0)
    assert np.array_equal(it, fx[f"rows_run0_{sc}_iteration"]) and not it.any()
    fxm.assert_same(fit, fx[f"rows_run0_{sc}_fitness"], "fitness")
    with np.errstate(all="ignore"):
        want = np.array([np.sqrt(F(s[27] / s[28])) if s[28] > 0 else F(0) for s in sums], F)
    fxm.assert_same(rmse, want, "rmse = sqrt(S27 / S28) of the reference's rows in wave order")
    fxm.assert_same(T, np.tile(np.eye(4, dtype=F).reshape(16), (len(clouds), 1)), "T")
    # one iteration: the spec's solve of those sums
    T1, _, _, it1 = _run(fx, clouds, sc, 1)
    eye = np.eye(4, dtype=F)
    want_T = np.stack([ref.mat4_mul(ref.vec6_to_mat4(ref.ldlt_solve6(s), "spec"), eye).reshape(16) if s[28] > 0
                       else eye.reshape(16) for s in sums])
    assert np.array_equal(it1, np.array([1 if s[28] > 0 else 0 for s in sums], np.int32))
    assert ref.same_bits(T1, want_T), np.nonzero((T1 != want_T).any(1))[0]


@pytest.mark.parametrize("sc", fxm.SCENES)
@pytest.mark.parametrize("cam", CAMS)
def test_full_runs_within_the_price_of_order_and_trigonometry(cam, sc, capsys):
    fx = fxm.load(cam)
    j = fxm.SCENES.index(sc)
    for i, name in enumerate(fxm.RUNS):
        T, fit, rmse, it = _run(fx, [fx[f"run_{name}_cloud"]], sc, int(fx[f"run_{name}_max_iter"]))
        assert int(it[0]) == int(fx[f"run_{name}_{sc}_iteration"][0]), (name, it)
        bound = fx["order_trig_dev"][i, j]
        dist = [np.abs(T[0].astype(np.float64) - fx[f"run_{name}_{sc}_T"].astype(np.float64)).max(),
                abs(float(fit[0]) - float(fx[f"run_{name}_{sc}_fitness"][0])),
                abs(float(rmse[0]) - float(fx[f"run_{name}_{sc}_rmse"][0]))]
        with capsys.disabled():
            print(f"\n[refk_icp] {cam} {sc} {name}: |T|, |fitness|, |rmse| from the reference "
                  f"{[float(d) for d in dist]}, bound {[float(b) for b in bound]}")
        assert all(d <= b for d, b in zip(dist, bound)), (name, dist, list(bound))
