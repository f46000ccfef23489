"""The certified fragment depth's IEEE fallback where the vertex ring holds reciprocal depths (the depth pass of
fastdiv and interior poses, raster_phase in pcore_fused.hip), on the cases of tests/fallback_ring_cases.py, certified on
the CPU by tests/test_fallback_ring_cases.py: fronto-parallel patches at depths k + 0.5 cm, whose every covered sample
takes the fallback and computes its depths again from the vertex stream -- in one stream whose ring wraps, in eight
streams with the flush at the stream switch, and for one triangle; at an interior and at a border pose.  evaluate's
debug z-samples and costs (types 2 and 0) and render_clouds at stride 8 and at the generic stride 2, bit for bit
against the oracle: there are no tolerances."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import fallback_ring_cases as fc
from tests.test_gpu_mesh_shapes import Ctx, _check_depth_costs

pytestmark = pytest.mark.gpu


def _ctx(name, monkeypatch):
    case = fc.case(name)
    if case.streams is not None:
        monkeypatch.setenv("PCORE_MODEL_STREAMS", str(case.streams))  # read by upload_meshes
    return case, Ctx(case)


@pytest.mark.parametrize("stride", fc.STRIDES)
@pytest.mark.parametrize("name", list(fc.MODELS))
def test_z_samples_and_costs(name, stride, monkeypatch):
    case, ctx = _ctx(name, monkeypatch)
    ctx.observe(stride)
    _check_depth_costs(ctx, f"fallback ring, model {name}", calls=2)
    ctx.close()


@pytest.mark.parametrize("stride", fc.STRIDES)
@pytest.mark.parametrize("name", list(fc.MODELS))
def test_rendered_clouds(name, stride, monkeypatch):
    case, ctx = _ctx(name, monkeypatch)
    ctx.observe(stride)
    xyzw, cnt = ctx.core.render_clouds(ctx.poses, ctx.pm, None, stride=stride)
    torch.cuda.synchronize()
    xyzw, cnt = xyzw.cpu().numpy(), cnt.cpu().numpy()
    oxyz, opose = case.cloud(stride)
    ocnt = np.bincount(opose, minlength=case.n)
    assert np.array_equal(cnt, ocnt) and (ocnt > 0).all(), (cnt, ocnt)
    start = np.cumsum(ocnt) - ocnt
    for p in range(case.n):
        g, w = xyzw[p, :cnt[p], :3], oxyz[start[p]:start[p] + ocnt[p]]
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"points differ, {case.describe(p)}"
    ctx.close()
