"""CPU: the planar ICP spec on its numpy restatement alone -- the table-top cases the GPU parity
tests run (tests/test_gpu_icp2d.py) reach every exit of the loop, iterate, reject pairs and cover the kernel's lane
remainders -- and the host pose update of the recognizer against hand-computed cases."""
import math

import numpy as np
import pytest

from perception_amd.tabletop import planar_adjusted_states
from tests import icp2d_reference as ref


@pytest.mark.parametrize("cs", ref.CASES, ids=ref.case_id)
def test_case_is_not_vacuous(cs):
    c = ref.planar_case(*cs)
    ns = np.array([len(x) for x in c.clouds])
    assert c.n == 64 and len(c.status) == 64
    # the classes of the 64 states: 40 perturbed ground truths, 18 grid neighbours, 4 far, 2 empty
    assert [int((c.kind == k).sum()) for k in ("perturbed", "neighbour", "far", "empty")] == [40, 18, 4, 2]
    assert (c.status[c.kind == "far"] == ref.NO_CORRESPONDENCES).all() and (ns[c.kind == "far"] > 0).all()
    assert (c.status[c.kind == "empty"] == ref.EMPTY_RENDER).all() and (ns[c.kind == "empty"] == 0).all()
    # at least half the poses run three or more iterations
    assert int((c.iters >= 3).sum()) >= 32
    # some converging pose has rejected pairs
    conv = [i for i in range(c.n) if c.status[i] < ref.NO_CORRESPONDENCES and any(r > 0 for _, r in c.traces[i])]
    assert len(conv) >= 1
    # lane remainders: a cloud of more than one round whose count is no multiple of 64; on TINY one below a round
    assert ((ns > 64) & (ns % 64 != 0)).any()
    if cs[0] == "TINY":
        assert ((ns > 0) & (ns < 64)).any()
    # the grid search, not a fallback, is what runs: pcore_icp_planar has no brute-force path at all
    # (GRID_MIN_POINTS = 1), and the observation spans several grid cells
    assert len(c.obs_xyz) >= ref.GRID_MIN_POINTS and len(c.obs_xyz) >= 100
    w = ref.to_world(c.world_from_cam, c.obs_xyz)
    assert ((w.max(0) - w.min(0))[:2] > 2 * 2.02 * ref.MAX_CORR).all()  # more than two cells across in x and y


def test_every_exit_occurs_over_the_table():
    seen = set()
    for row in ref.TABLE_ROWS:
        seen |= set(int(s) for s in ref.row_result(*row)[2])
    assert seen == {0, 1, 2, 3, 4, 5}
    assert len(set(int(s) for s in ref.planar_case("SMALL", 2).status)) >= 4
    # the mse exits come from the row with transformation_epsilon = 0 (icp2d_reference.TABLE_ROWS says why)
    st = ref.row_result(*ref.TABLE_ROWS[-1])[2]
    assert (st == ref.ABS_MSE).sum() >= 1 and (st == ref.REL_MSE).sum() >= 1 and (st == ref.TRANSFORM).sum() == 0


@pytest.mark.parametrize("cs", ref.CASES, ids=ref.case_id)
def test_refinement_improves_the_perturbed_ground_truths(cs):
    """Sanity of the spec: over the perturbed ground-truth poses the median planar error and the median yaw error
    after the refinement are below those before."""
    c = ref.planar_case(*cs)
    adj = planar_adjusted_states(c.states, c.xform, c.status)
    sel = np.nonzero(c.kind == "perturbed")[0]
    gt = np.array([ref.PLACEMENTS[m] for m in c.pose_model[sel]])

    def errors(st):
        d = np.hypot(st[sel, 0] - gt[:, 0], st[sel, 1] - gt[:, 1])
        a = np.abs((st[sel, 3] - gt[:, 2] + math.pi) % (2 * math.pi) - math.pi)
        return np.median(d), np.median(a)

    d0, a0 = errors(c.states)
    d1, a1 = errors(adj)
    print(f"{ref.case_id(cs)}: median planar error {d0 * 1e3:.2f} -> {d1 * 1e3:.2f} mm, "
          f"median yaw error {math.degrees(a0):.2f} -> {math.degrees(a1):.2f} deg")
    assert d1 < d0 and a1 < a0


def test_step_degenerate_rows():
    """h == 0 gives the identity rotation; three collinear, equal pairs give a pure shift."""
    S = np.array([3.0, 3.0, 0.0, 6.0, 3.0, 6.0, 3.0, 0.0, 0.0, 0.0])  # q = (1, 0) x 3, t = (2, 1) x 3
    c, s, tx, ty = ref.planar_step(S)
    assert (c, s, tx, ty) == (1.0, 0.0, 1.0, 1.0)


def test_planar_adjusted_states_hand_cases():
    st = np.array([[0.5, -0.1, 0.7, 0.25],      # identity
                   [0.5, -0.1, 0.7, 0.25],      # pure shift
                   [0.0, 0.0, 0.7, 6.0],        # yaw wrap across 2 pi
                   [0.3, 0.2, 0.7, 1.0],        # a quarter turn about the origin
                   [0.5, -0.1, 0.7, 0.25],      # status 4: passes through
                   [0.5, -0.1, 0.7, 7.0]])      # status 5: passes through, untouched
    xf = np.array([[1.0, 0.0, 0.0, 0.0],
                   [1.0, 0.0, 0.125, -0.25],
                   [math.cos(0.5), math.sin(0.5), 0.0, 0.0],
                   [0.0, 1.0, 0.0, 0.0],
                   [0.0, 1.0, 9.0, 9.0],
                   [0.0, 1.0, 9.0, 9.0]])
    status = np.array([1, 0, 2, 3, 4, 5])
    out = planar_adjusted_states(st, xf, status)
    f = np.float32
    assert np.array_equal(out[0, :3], [float(f(0.5)), float(f(-0.1)), float(f(0.7))]) and abs(out[0, 3] - 0.25) < 1e-15
    assert np.array_equal(out[1, :3], [float(f(0.5) + f(0.125)), float(f(-0.1) + f(-0.25)), float(f(0.7))])
    assert abs(out[1, 3] - 0.25) < 1e-15
    yaw2 = math.atan2(float(f(math.sin(0.5))), float(f(math.cos(0.5))))
    want = math.atan2(math.sin(6.0 + yaw2), math.cos(6.0 + yaw2))  # 6.5 - 2 pi
    assert abs(out[2, 3] - want) < 1e-15 and abs(want - (6.5 - 2 * math.pi)) < 1e-7 and 0.0 <= out[2, 3] < 2 * math.pi
    assert np.array_equal(out[3, :2], [float(-f(0.2)), float(f(0.3))])
    assert abs(out[3, 3] - (1.0 + math.pi / 2)) < 1e-14
    assert np.array_equal(out[4], st[4]) and np.array_equal(out[5], st[5])
