"""No GPU: the composed-state cases (tests/scene_cases.py) can fail -- certified on the oracle alone -- and the entry
point exists.  Each count is what the GPU test of the same name relies on: a rule that no pixel exercised would pass
whatever the kernel did."""
import ctypes

import numpy as np

from perception_amd import _native
from tests import scene_cases as sc
from tests import scene_reference as ref


def _diff(a, b):
    """Pixels where two composed frames differ in depth, owner or colour."""
    return int(((a[0] != b[0]) | (a[2] != b[2]) | (a[1] != b[1]).any(0)).sum())


def test_candidates_exercise_the_owner_rule_everywhere():
    D, _ = sc.per_pose("candidates", "plain")
    depth, _, owner, visible = sc.expected("candidates", "plain")
    covered = depth != 0
    attained = ((D == depth[None]) & (D != 0)).sum(0)
    ties = int((covered & (attained >= 2)).sum())
    print(f"candidates: {ties} of {int(covered.sum())} covered pixels have two or more poses at the minimum")
    assert ties >= 10000
    assert int(visible.sum()) == int(covered.sum()) and (owner[~covered] == -1).all()
    # more than one object owns pixels, and not only the first pose of each
    assert len(np.unique(owner[covered] // 8)) == 3 and (visible > 0).sum() > 3


def test_state_source_and_labels_change_the_frame():
    plain, thr, lab = (sc.expected("state", m) for m in ("plain", "threshold", "labels"))
    d_lab, d_thr, d_lt = _diff(plain, lab), _diff(plain, thr), _diff(thr, lab)
    print(f"state: with / without source differ on {d_lab} (labels) and {d_thr} (threshold) pixels; "
          f"labels / no labels on {d_lt}")
    assert d_lab >= 100 and d_thr >= 100
    assert d_lt >= 20


def test_reversed_order_keeps_depth_and_changes_owner():
    for name in ("candidates", "state"):
        n = sc.pose_set(name).n
        rev = np.arange(n)[::-1]
        a, b = sc.expected(name, "plain"), sc.expected(name, "plain", rev)
        assert np.array_equal(a[0], b[0])
        back = np.where(b[2] >= 0, rev[np.maximum(b[2], 0)], -1)  # the reversed frame's owners as original indices
        assert (back != a[2]).sum() > 0, name


def test_lens_pose_is_absent_where_its_own_depth_reads_zero():
    """The pose 3 mm from the camera's plane reads depth 0 (with a colour) in its own frame on half the image; there the
    contract shows the poses behind it, on more pixels than a z-test in which the 0 won would leave any."""
    for mode in sc.MODES:
        D, C = sc.per_pose("lens", mode)
        zero = (D[3] == 0) & C[:, 3].any(0)
        depth, _, owner, visible = sc.expected("lens", mode)
        behind = int((zero & (depth > 0)).sum())
        print(f"lens, {mode}: {int(zero.sum())} pixels of depth 0, {behind} of them show a pose behind")
        assert zero.sum() >= 100000 and behind >= 5000
        assert visible[3] == 0 and (depth >= 0).all()
        rest = [0, 1, 2, 4, 5, 6]
        state = sc.expected("state", mode)  # the same frame as without the pose, the owners past it moved up
        assert np.array_equal(depth, state[0])
        assert np.array_equal(owner, np.where(state[2] >= 3, state[2] + 1, state[2]))
        assert np.array_equal(visible[rest], state[3])


def test_empty_set_composes_the_empty_frame():
    depth, color, owner, visible = ref.compose(np.zeros((0, 4, 5), np.int32), np.zeros((3, 0, 4, 5), np.uint8))
    assert not depth.any() and not color.any() and (owner == -1).all() and visible.shape == (0,)


def test_render_scene_is_exported_and_refuses_a_null_context():
    lib = _native.load()
    assert "pcore_render_scene" in _native.EXPORTED_SYMBOLS
    assert isinstance(lib.pcore_render_scene, ctypes._CFuncPtr)
    rc = lib.pcore_render_scene(None, None, None, None, 0, 0, 1.0, None, None, None, None, None)
    assert rc == _native.PCORE_E_INVALID_ARG
