"""CPU certificates of tests/clip_cases.py: the GPU tests of tests/test_gpu_clip.py could fail.  On the float32
restatements of pose_window and of the vertex pass (no GPU):
  - every triangle window of every interior pose lies inside the pose's unclamped window -- what lets the un-chunked
    interior copy of the triangle stage drop its clip -- and some reach the window's last column and last row and the
    column and row next to its first (the first themselves are out of reach: clip_cases' docstring);
  - a clip would matter if the window were one sample smaller on any of those sides;
  - poses against the left border are interior under the old rule (the box inside the image) and not under the new one
    (and no clamp of the window binds), at both image heights;
  - chunks of eight samples split every pose's window, so the chunked copy, which keeps the clip, runs too."""
import numpy as np
import pytest

from tests import clip_cases as cc
from tests import interior_cases as ic


@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_the_cases_are_the_ones_described(height):
    case = cc.case(height)
    assert (case.width, case.height) == (72, height) and set(cc.STRIDES) == {8, 3}
    assert all(case.width % s == 0 for s in cc.STRIDES)  # every entry point requires it
    assert [48 % s for s in cc.STRIDES] == [0, 0] and all(50 % s for s in cc.STRIDES)
    assert case.n <= 24 and len(case.kinds) == case.n
    for k in cc.KINDS:
        assert case.kinds.count(k) >= 1, k
    assert case.proj.shape == ic.proj(cc.cam(height)).shape and case.z_full.shape == (case.n, height, 72)


@pytest.mark.parametrize("s", cc.STRIDES)
@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_triangle_windows_lie_inside_the_unclamped_window_and_reach_its_sides(height, s):
    c, tris = cc.cam(height), ic.mesh()
    poses, kinds = cc.poses(height)
    seen = set()
    interior = 0
    for m, kind in zip(poses, kinds):
        (X0, X1, Y0, Y1), old, new = cc.window(m, tris, c, s)
        if new != 2:
            continue
        interior += 1
        ws, hs = c["width"] // s, -(-height // s)
        assert 0 <= X0 <= X1 <= ws - 1 and 0 <= Y0 <= Y1 <= hs - 1
        lo, hi = cc.tri_windows(m, tris, c, s)
        # every bound, of empty windows too: the clip changes no bit
        assert (lo[:, 0] >= X0).all() and (hi[:, 0] <= X1).all() and (lo[:, 1] >= Y0).all() and (hi[:, 1] <= Y1).all()
        # and the first column and row stay out of reach
        assert (lo[:, 0] >= X0 + 1).all() and (lo[:, 1] >= Y0 + 1).all()
        seen |= cc.touches(m, tris, c, s)
    assert interior >= 12
    # a window one sample smaller on any of these sides would clip a non-empty triangle window
    assert {"last_col", "last_row", "first_col", "first_row"} <= seen, seen


@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_the_tightened_rule_moves_poses_at_the_left_border_out_of_the_class(height):
    c, tris = cc.cam(height), ic.mesh()
    poses, kinds = cc.poses(height)
    moved = 0
    for m, kind in zip(poses, kinds):
        for s in cc.STRIDES:
            (X0, X1, Y0, Y1), old, new = cc.window(m, tris, c, s)
            assert new <= old and old >= 1
            if kind == "left_band":
                assert (old, new, X0) == (2, 1, -1), (kind, s, old, new, X0)
                xlo = ic.pose_box(m, tris, c)[0]
                assert 0 <= xlo < 1
                moved += 1
            else:
                assert old == new == 2, (kind, s, old, new)
    assert moved >= 2


@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_border_poses_fill_the_last_sample_column_and_row(height):
    """`right`: the window ends in the last sample column of the image at both strides; `bottom`: in the last sample
    row -- where the window's clamps to ws - 1 and hs - 1 would bind first."""
    c, tris = cc.cam(height), ic.mesh()
    poses, kinds = cc.poses(height)
    for m, kind in zip(poses, kinds):
        for s in cc.STRIDES:
            (X0, X1, Y0, Y1), _, _ = cc.window(m, tris, c, s)
            if kind == "right":
                assert X1 == 72 // s - 1
            if kind == "bottom":
                assert Y1 == -(-height // s) - 1


@pytest.mark.parametrize("s", cc.STRIDES)
@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_an_eight_sample_tile_chunks_every_window(height, s):
    c, tris = cc.cam(height), ic.mesh()
    for m in cc.poses(height)[0]:
        (X0, X1, Y0, Y1), _, _ = cc.window(m, tris, c, s)
        assert (min(X1, 72 // s - 1) - max(X0, 0) + 1) * (Y1 - Y0 + 1) > 8


@pytest.mark.parametrize("height", cc.HEIGHTS)
def test_every_pose_renders(height):
    case = cc.case(height)
    for s in cc.STRIDES:
        assert ((case.zs(s) > 0).reshape(case.n, -1).sum(1) >= 2).all(), s  # (the sheet spans 3 x 2 samples at stride 8)
