"""The triangle stage without its clip to the pose window (raster_phase's WHOLE copy of an interior pose,
pcore_fused.hip) and the tightened interior class, on the poses of tests/clip_cases.py, certified on the CPU by
tests/test_clip_cases.py: triangle windows in the last column and row of the pose window and next to its first, poses the
new rule moves out of the interior class at the left border, and the sheet against the right border and the last row,
on a 72 x 48 and a 72 x 50 image at strides 8 and 3.  Whole windows (the copy without the clip) and chunks of eight
samples (the copy that keeps it) through evaluate's costs (types 2 and 0) and debug z-samples, pcore_debug_render_clouds
and the colour cost (type 1), bit for bit against the oracle: there are no tolerances."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import clip_cases as cc
from tests.test_gpu_mesh_shapes import Ctx, _assert_costs, _check_depth_costs

pytestmark = pytest.mark.gpu

TILES = ("auto", "tcap8")


def _tile(tile, monkeypatch):
    if tile == "tcap8":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "8")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", cc.STRIDES)
@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_z_samples_and_costs(height, stride, tile, monkeypatch):
    """evaluate(..., dbg_zs): the z-samples equal the oracle's render at the sample grid and rc / oc / diff of cost
    types 2 and 0 equal the oracle's, twice (the second call runs after the first one's tile feedback)."""
    _tile(tile, monkeypatch)
    case = cc.case(height)
    ctx = Ctx(case)
    ctx.observe(stride)
    _check_depth_costs(ctx, f"clip cases, height {height}, tile {tile}", calls=2)
    if tile == "tcap8":
        assert ctx.core.tile_info()["tcap"] == 8
    ctx.close()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", cc.STRIDES)
@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_rendered_clouds(height, stride, tile, monkeypatch):
    """render_clouds (render_cloud_kernel: the same copies of the raster) equals the oracle's compaction of the oracle's
    z-buffers, counts and points."""
    _tile(tile, monkeypatch)
    case = cc.case(height)
    ctx = Ctx(case)
    ctx.observe(stride)
    xyzw, cnt = ctx.core.render_clouds(ctx.poses, ctx.pm, None, stride=stride)
    torch.cuda.synchronize()
    xyzw, cnt = xyzw.cpu().numpy(), cnt.cpu().numpy()
    oxyz, opose = case.cloud(stride)
    ocnt = np.bincount(opose, minlength=case.n)
    bad = np.nonzero(cnt != ocnt)[0]
    assert len(bad) == 0, f"counts differ; first: {case.describe(int(bad[0]))}: gpu {cnt[bad[0]]}, oracle {ocnt[bad[0]]}"
    assert (ocnt > 0).all()
    start = np.cumsum(ocnt) - ocnt
    for p in range(case.n):
        g, w = xyzw[p, :cnt[p], :3], oxyz[start[p]:start[p] + ocnt[p]]
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"points differ, {case.describe(p)}"
    ctx.close()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", cc.STRIDES)
@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_colour_cost(height, stride, tile, monkeypatch):
    """Cost type 1 (its depth pass is the same raster; the colour id pass keeps the clip) with colour A on the
    triangles of odd index: rc / oc / diff equal oracle.evaluate_colour."""
    _tile(tile, monkeypatch)
    case = cc.case(height)
    ctx = Ctx(case, colours=case.bank.colouring(0))
    ctx.observe(stride)
    got, _ = ctx.evaluate(1)
    _assert_costs(case, got, case.oracle_colour_costs(stride, 0), f"clip cases, height {height}, tile {tile}, colour")
    ctx.close()
