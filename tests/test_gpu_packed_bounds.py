"""The interior vertex pass's bounds in 16-bit halves (vertex_bounds, STRIDE == 8, INTERIOR, pcore_fused.hip) at the
top of their range on the device: the 16384 x 16 and 24 x 16384 cameras of tests/bounds_cases.py (certified on the CPU by
tests/test_bounds_cases.py: every pose interior, converted coordinates up to 16380, bounds in the last sample column /
row, 2047) and the 72 x 48 poses of tests/clip_cases.py, at stride 8.  evaluate's costs (types 2 and 0) and debug
z-samples and pcore_debug_render_clouds, bit for bit against the oracle: there are no tolerances."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import bounds_cases as bc
from tests import clip_cases as cc
from tests.test_gpu_mesh_shapes import Ctx, _check_depth_costs

pytestmark = pytest.mark.gpu

CASES = ("wide", "tall", "small")


def _case(name):
    return cc.case(48) if name == "small" else bc.case(name)


@pytest.mark.parametrize("name", CASES)
def test_z_samples_and_costs(name):
    case = _case(name)
    ctx = Ctx(case)
    ctx.observe(8)
    _check_depth_costs(ctx, f"packed bounds, {name}", calls=2)
    ctx.close()


@pytest.mark.parametrize("name", CASES)
def test_rendered_clouds(name):
    case = _case(name)
    ctx = Ctx(case)
    ctx.observe(8)
    xyzw, cnt = ctx.core.render_clouds(ctx.poses, ctx.pm, None, stride=8)
    torch.cuda.synchronize()
    xyzw, cnt = xyzw.cpu().numpy(), cnt.cpu().numpy()
    oxyz, opose = case.cloud(8)
    ocnt = np.bincount(opose, minlength=case.n)
    bad = np.nonzero(cnt != ocnt)[0]
    assert len(bad) == 0, f"counts differ; first: {case.describe(int(bad[0]))}: gpu {cnt[bad[0]]}, oracle {ocnt[bad[0]]}"
    assert (ocnt > 0).sum() >= case.n - 2  # (the sheet has gaps: a pose may miss every sample)
    start = np.cumsum(ocnt) - ocnt
    for p in range(case.n):
        g, w = xyzw[p, :cnt[p], :3], oxyz[start[p]:start[p] + ocnt[p]]
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"points differ, {case.describe(p)}"
    ctx.close()
