"""The triangle stage's one-sample fast path (raster_phase, pcore_fused.hip) on the cases of tests/one_sample_cases.py,
certified on the CPU by tests/test_one_sample_cases.py: steps of one-sample and empty windows only, and steps that
hold empty, one-sample, 2- to 4-sample (rows, columns, 2 x 2) and larger windows, padding slots and NaN-vertex
triangles side by side, one-sample windows that only the clip to a chunk of a 64-sample tile makes, fastdiv and
non-fastdiv poses.  Through evaluate (z-samples and the
three costs of types 2 and 0), the colour cost (the id pass; a wrong colour id changes a cost in the colouring of a bit
in which the two triangle indices differ) and pcore_debug_render_clouds, at stride 8 and at the generic stride 3, bit
for bit against the oracle: there are no tolerances."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import one_sample_cases as oc
from tests.test_gpu_mesh_shapes import Ctx, _assert_costs, _check_depth_costs

pytestmark = pytest.mark.gpu

TILES = ("auto", "tcap64")


def _tile(tile, monkeypatch):
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", str(oc.TCAP))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", oc.STRIDES)
def test_z_samples_and_costs(stride, tile, monkeypatch):
    """evaluate(..., dbg_zs): the z-samples equal the oracle's render at the sample grid and rc / oc / diff of cost
    types 2 and 0 equal the oracle's, twice (the second call runs after the first one's tile feedback)."""
    _tile(tile, monkeypatch)
    case = oc.case()
    ctx = Ctx(case)
    ctx.observe(stride)
    _check_depth_costs(ctx, f"one-sample cases, tile {tile}", calls=2)
    if tile == "tcap64":
        assert ctx.core.tile_info()["tcap"] == oc.TCAP
    ctx.close()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", oc.STRIDES)
def test_colour_costs(stride, tile, monkeypatch):
    """Cost type 1 under every colouring of the bank (colour A on the triangles whose index within their model has bit
    b set, the observed points colour B, beyond the gate): rc / oc / diff equal oracle.evaluate_colour."""
    _tile(tile, monkeypatch)
    case = oc.case()
    for b in range(case.bank.num_colourings()):
        ctx = Ctx(case, colours=case.bank.colouring(b))
        ctx.observe(stride)
        got, _ = ctx.evaluate(1)
        _assert_costs(case, got, case.oracle_colour_costs(stride, b), f"stride {stride}, colouring {b}, tile {tile}")
        ctx.close()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stride", oc.STRIDES)
def test_rendered_clouds(stride, tile, monkeypatch):
    """render_clouds (render_cloud_kernel shares the raster) equals the oracle's compaction of the oracle's z-buffers,
    counts and points."""
    _tile(tile, monkeypatch)
    case = oc.case()
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
