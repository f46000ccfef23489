"""No GPU: the case sets of tests/state_cost_cases.py separate the state-cost contract from every wrong rule of
tests/state_cost_reference.py (at least one state's outputs differ for each), and the joint-search scene does what the
GPU test relies on.  Everything here runs on the oracle alone."""
import numpy as np
import pytest

from tests import state_cost_cases as cases
from tests import state_cost_reference as ref


def _differs(a, b):
    return any(not np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def _totals_differ(a, b):
    return _differs(a[:3], b[:3])


@pytest.fixture(scope="module")
def scene_want():
    return cases.scene().case.expected()


@pytest.mark.parametrize("rule", ["alone", "last_wins", "expl_sum", "label0"])
def test_scene_separates_the_rule(scene_want, rule):
    got = cases.scene().case.expected(rule)
    assert _differs(got, scene_want), rule
    if rule != "last_wins":  # the owner of a tie moves points between members, not the totals
        assert _totals_differ(got, scene_want), rule


def test_scene_state_is_not_the_sum_of_its_members(scene_want):
    sc = cases.scene()
    c = sc.case
    rc, oc, df, vis, bad = scene_want
    alone = c.expected("alone")
    n0 = len(c.states[0])
    assert vis[:n0].sum() < alone[3][:n0].sum()  # copies inside each other hide one another's points
    # a one-member state is the pose alone
    one = ref.evaluate_states(c.Z, [[i] for i in range(len(c.Z))], c.pose_label, sc.pose_obs_total, c.cam, c.stride,
                              c.obs_sorted, c.label_start, c.label_end, c.r)
    want = sc.base.oracle_costs()
    n = len(want[0])
    for g, w in zip(one[:3], want):
        assert np.array_equal(g[:n].view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("rule", ["clamp", "negative", "ge"])
def test_hand_made_cases_separate_the_rule(rule):
    c = cases.hand()
    assert _differs(c.expected(rule), c.expected()), rule


def test_hand_made_values():
    c = cases.hand()
    rc, oc, df, vis, bad = c.expected()
    off = np.concatenate([[0], np.cumsum([len(s) for s in c.states])])
    assert vis[off[0]:off[1]].tolist() == [9, 0] and bad[off[0]:off[1]].tolist() == [0, 0]  # [0, 9]: 9 is skipped
    assert vis[off[1]:off[2]].tolist() == [0, 6]  # [2, 1]: the negative column hides pose 1's and yields no point
    assert vis[off[2]:off[3]].tolist() == [6, 0]
    assert vis[off[3]:off[4]].tolist() == [1] and bad[off[3]:off[4]].tolist() == [0] and rc[3] == 0.0  # d^2 = r^2


@pytest.mark.parametrize("labelled", [True, False])
def test_fuzz_separates_the_composition_rules(labelled):
    # the composition rules; the union rule (c) needs two members' points within the radius of one observed point, which
    # the scene has and these samples, 3.6 cm apart, have not
    c = cases.fuzz("TINY", 8, labelled)
    want = c.expected()
    for rule in ("alone", "last_wins", "clamp", "negative") + (("label0",) if labelled else ()):
        assert _differs(c.expected(rule), want), rule
    assert cases.fuzz("TINY", 8, labelled).Z[0].size == 108


@pytest.mark.parametrize("cam,stride", [("TINY", 8), ("SMALL", 1), ("SMALL", 5)])
@pytest.mark.parametrize("labelled", [True, False])
def test_fuzz_has_owners_beyond_list_position_256(cam, stride, labelled):
    """Per-member counts beyond the kernel's LDS histogram: some state's owners sit at list positions >= 256 with
    non-zero vis and bad there, so a kernel that drops or misplaces those counts differs."""
    c = cases.fuzz(cam, stride, labelled)
    _, _, _, vis, bad = c.expected()
    deep = cases.deep_positions(c.states)
    assert len(deep) > 0 and vis[deep].sum() > 0 and bad[deep].sum() > 0
    straddle = c.states[-2]
    assert len(straddle) > cases.DEEP and 0 <= straddle[cases.DEEP - 1] < len(c.Z) and 0 <= straddle[cases.DEEP] < len(c.Z)


def test_joint_search_scene():
    b = cases.boxes()
    r = cases.boxes_reference()
    sl = r.shortlists
    assert (sl[:, 0] >= 0).all()
    left = lambda i: b.poses[i][3] < 0  # noqa: E731  (tx of the scaled row-major pose)
    assert left(sl[0, 0]) == left(sl[1, 0]), "greedy puts both models on the same box"
    res = r.result
    end = [int(sl[m, res.slot[m]]) for m in range(2)]
    assert left(end[0]) != left(end[1]), "the joint search ends with one model on each box"
    greedy = r.score([[int(sl[0, 0]), int(sl[1, 0])]], np.array([len(b.obs)], np.float32))
    import oracle
    gc = int(oracle.select(greedy[0], greedy[1], np.zeros(1, np.int32), 1)[0][0])
    assert res.cost < gc, (res.cost, gc)
    assert res.trace[0]["adopted"] and not res.trace[-1]["adopted"]


def test_library_sweep_and_totals_equal_the_reference():
    """perception_amd.joint builds the sweep's states and their observed totals as the numpy joint search does."""
    from perception_amd import joint

    rng = np.random.default_rng(11)
    for _ in range(20):
        K, k = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        sl = rng.integers(0, 40, (K, k))
        for m in range(K):
            sl[m, int(rng.integers(0, k + 1)):] = -1  # a model may have fewer candidates, or none
        slot = [int(rng.integers(0, max(1, (sl[m] >= 0).sum()))) if sl[m][0] >= 0 else -1 for m in range(K)]
        assert joint.sweep_states(sl, slot) == ref.sweep_states(sl, slot)
        labels = rng.integers(-1, 5, 40)
        counts = rng.integers(0, 100, 4)
        for st in ref.sweep_states(sl, slot)[0]:
            assert joint.state_obs_total(st, labels, counts) == ref.state_obs_total(st, labels, counts)
            assert joint.state_obs_total(st, None, 321) == ref.state_obs_total(st, None, 321) == 321
