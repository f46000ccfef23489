"""The fused raster's three pose classes (pose_window / raster_phase, pcore_fused.hip: interior, fastdiv, general) on
the cases of tests/interior_cases.py, certified on the CPU by tests/test_interior_cases.py: a sheet of sub-pixel,
on-sample and zero-area triangles that moves outward across each border of a 72 x 48 image -- interior, its margin
alone across the border, a vertex exactly on the border pixel and one float step beyond it, astride, and close to the
camera plane.  evaluate's costs (types 2 and 0) and debug z-samples, and pcore_debug_render_clouds, at stride 8 and
at the generic stride 3, with the automatic tile and a 64-sample tile, bit for bit against the oracle: there are no
tolerances."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import interior_cases as ic
from tests.test_gpu_mesh_shapes import Ctx, _check_depth_costs

pytestmark = pytest.mark.gpu

TILES = ("auto", "tcap64")


def _tile(tile, monkeypatch):
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", ic.STRIDES)
def test_z_samples_and_costs(stride, tile, monkeypatch):
    """evaluate(..., dbg_zs): the z-samples equal the oracle's render at the sample grid and rc / oc / diff of cost
    types 2 and 0 equal the oracle's, twice (the second call runs after the first one's tile feedback)."""
    _tile(tile, monkeypatch)
    case = ic.case()
    ctx = Ctx(case)
    ctx.observe(stride)
    _check_depth_costs(ctx, f"interior cases, tile {tile}", calls=2)
    if tile == "tcap64":  # the tile is the whole sampled image where that is smaller (stride 8: 9 x 6 samples)
        assert ctx.core.tile_info()["tcap"] == min(64, (case.width // stride) * (-(-case.height // stride)))
    ctx.close()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", ic.STRIDES)
def test_rendered_clouds(stride, tile, monkeypatch):
    """render_clouds (render_cloud_kernel picks among the same three copies of the raster) equals the oracle's
    compaction of the oracle's z-buffers, counts and points."""
    _tile(tile, monkeypatch)
    case = ic.case()
    ctx = Ctx(case)
    ctx.observe(stride)
    xyzw, cnt = ctx.core.render_clouds(ctx.poses, ctx.pm, None, stride=stride)
    torch.cuda.synchronize()
    xyzw, cnt = xyzw.cpu().numpy(), cnt.cpu().numpy()
    oxyz, opose = case.cloud(stride)
    ocnt = np.bincount(opose, minlength=case.n)
    bad = np.nonzero(cnt != ocnt)[0]
    assert len(bad) == 0, f"counts differ; first: {case.describe(int(bad[0]))}: gpu {cnt[bad[0]]}, oracle {ocnt[bad[0]]}"
    assert (ocnt > 0).sum() >= case.n - 4
    start = np.cumsum(ocnt) - ocnt
    for p in range(case.n):
        g, w = xyzw[p, :cnt[p], :3], oxyz[start[p]:start[p] + ocnt[p]]
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"points differ, {case.describe(p)}"
    ctx.close()
