"""The interior vertex pass's bounds in 16-bit halves (vertex_bounds, STRIDE == 8, INTERIOR, pcore_fused.hip) against
the scalar formulas, on the numpy restatements of tests/bounds_cases.py, and the CPU certificates of that module's two
cameras: the GPU tests of tests/test_gpu_packed_bounds.py could fail.

Each of the four converted values enters one half of one word and nothing else, so sweeping one component over all of
[0, 16383] with the others held (at both ends of their range) is exhaustive; the heights are 8, 48, 480 and 16384."""
import numpy as np
import pytest

from tests import bounds_cases as bc
from tests import clip_cases as cc
from tests import interior_cases as ic

ALL = np.arange(16384, dtype=np.int64)


@pytest.mark.parametrize("H", (8, 48, 480, 16384))
def test_packed_halves_equal_the_scalar_formulas(H):
    for held in (0, 16383, 4097):
        h = np.full_like(ALL, held)
        for comp in range(4):
            args = [h, h, h, h]
            args[comp] = ALL
            p0, p1 = bc.packed_bounds(*args, H)
            s0, s1 = bc.scalar_bounds(*args, H)
            assert np.array_equal(p0, s0) and np.array_equal(p1, s1), (H, held, comp)


def test_in_range_halves_do_not_wrap():
    """What the kernel's comment states for an interior pose: with lo0, hi0 in [0, W-1] and lo1, hi1 in [0, H-1] every
    half before the shift lies in [0, H + 6], inside int16, for the largest image."""
    H = 16384
    for v in (ALL + 7, H + 6 - ALL, ALL, H - 1 - ALL):
        assert v.min() >= 0 and v.max() <= H + 6 < 32768


@pytest.mark.parametrize("shape", tuple(bc.SHAPES))
def test_the_cameras_reach_the_top_of_the_range(shape):
    """Every pose is interior (under the old rule and the tightened one), the converted values of the nearest poses
    come within 4 of the largest an interior pose can have (the margin keeps the box 2 pixels and a little inside), and
    the bounds reach the last sample column (wide) / row (tall), 2047."""
    W, H = bc.SHAPES[shape]
    c, tris = bc.cam(shape), ic.mesh()
    top = 0
    for i, m in enumerate(bc.poses(shape)):
        (X0, X1, Y0, Y1), old, new = cc.window(m, tris, c, 8)
        assert old == new == 2
        lo0, lo1, hi0, hi1 = bc.converted(m, shape)
        assert lo0.min() >= 0 and hi0.max() <= W - 1 and lo1.min() >= 0 and hi1.max() <= H - 1
        p, s = bc.packed_bounds(lo0, lo1, hi0, hi1, H), bc.scalar_bounds(lo0, lo1, hi0, hi1, H)
        assert np.array_equal(p[0], s[0]) and np.array_equal(p[1], s[1])
        if shape == "wide":
            top = max(top, int(hi0.max()))
            last = int((s[1] & 0xffff).max())   # A1
        else:
            top = max(top, int((H + 6 - hi1).max()))
            last = int((s[1] >> 16).max())      # B1
        assert last <= 2047
        if i == 0:
            assert last == 2047
    assert top >= (16380 if shape == "wide" else 16386), top


@pytest.mark.parametrize("shape", tuple(bc.SHAPES))
def test_every_pose_renders(shape):
    case = bc.case(shape)
    assert case.z_full.shape == (case.n, case.height, case.width)
    # the sheet's triangles leave gaps, so a pose may miss every sample: most hit one or two, and several poses put a
    # fragment into the last sample column (wide) / row (tall), whose bounds are the largest
    hit = case.zs(8) > 0
    assert (hit.reshape(case.n, -1).sum(1) >= 1).sum() >= case.n - 2
    edge = hit[:, :, -1] if shape == "wide" else hit[:, -1, :]
    assert hit.shape[1:] == ((2, 2048) if shape == "wide" else (2048, 3)) and (edge.sum(1) >= 1).sum() >= 4
