"""CPU certificate of the scene sequences of tests/context_cases.py.  No kernel runs here.

tests/test_gpu_context_reuse.py gives one context scene after scene and compares every result with the oracle.  That
only proves something if a context that wrongly kept a part of the previous scene would score the next one differently.
For every transition X -> Y of the sequences this file computes, with the oracle alone, what Y's poses cost under each
kind of stale state, and asserts that the costs (the bits of rc or oc) differ from Y's own on at least a quarter of Y's
poses, for cost type 2 or for cost type 0:

  stale state                                 what it stands for in struct pcore_ctx
  X's whole observation (equal image sizes)   a set_observation that changed nothing
  X's cloud and segments, Y's source depth    grids / cell_start / grid_pts / seg_* / num_grids kept
  Y's cloud, X's source depth and mask        src_depth / src_mask, or the sampled src_s / lab_s, kept
  X's target covariances on Y's cloud         cov_k_label / cov_k_all not reset: at least a quarter of the refined poses
  X's observed colours on Y's points          obs_lab kept (cost type 1)

A buffer that grew is read through kept_buffer: the old contents' leading elements in the new shape.  The quarter is a
condition on the scenes, not a measurement: a scene that misses it is changed, not the bar.  The last test asserts that
the transitions shrink and grow what they are meant to.
"""
import numpy as np
import pytest

from tests import context_cases as cc

QUARTER = 0.25


def _reaches(counts, n):
    return max(counts) >= QUARTER * n


@pytest.mark.parametrize("x,y", cc.TRANSITIONS, ids=lambda v: v)
def test_stale_observation_changes_a_quarter_of_the_costs(x, y):
    X, Y = cc.scene(x), cc.scene(y)
    good = {ct: cc.want_costs(y, ct) for ct in (2, 0)}
    stale = {"X's cloud, Y's source": lambda ct: Y.costs(ct, cloud=X),
             "Y's cloud, X's source": lambda ct: Y.costs(ct, src=cc.stale_source(X, Y))}
    if cc.same_image(X, Y):
        stale["X's whole observation"] = lambda ct: Y.costs(ct, cloud=X, src=X)
    for what, costs in stale.items():
        counts = [cc.differing(costs(ct), good[ct]) for ct in (2, 0)]
        print(f"{x} -> {y}, {what}: {counts[0]} (type 2), {counts[1]} (type 0) of {Y.n} poses differ")
        assert _reaches(counts, Y.n), (x, y, what, counts, Y.n)


def test_the_same_image_transition_is_in_the_sequences():
    """X's whole observation can only be kept where the image sizes agree: A -> B is such a transition."""
    assert ("A", "B") in cc.TRANSITIONS and cc.same_image(cc.scene("A"), cc.scene("B"))
    assert not cc.same_image(cc.scene("B"), cc.scene("C")) and not cc.same_image(cc.scene("C"), cc.scene("A"))


@pytest.mark.parametrize("six", [True, False], ids=["6dof", "3dof"])
@pytest.mark.parametrize("x,y", cc.TRANSITIONS, ids=lambda v: v)
def test_stale_target_covariances_change_a_quarter_of_the_refined_poses(x, y, six):
    X, Y = cc.scene(x), cc.scene(y)
    good = cc.want_icp(y, six)
    stale = Y.icp(six, cov=cc.kept_buffer(X.covs(six, 10), (len(Y.case.obs_xyz), 6)))
    moved = int((good[0].view(np.uint32) != stale[0].view(np.uint32)).any(1).sum())
    print(f"{x} -> {y}, six {six}: {moved} of {len(Y.icp_idx)} refined poses differ")
    assert len(Y.icp_idx) >= 32 and moved >= QUARTER * len(Y.icp_idx)
    assert len(np.unique(good[1])) > 2  # the poses do not all stop at the same iteration


@pytest.mark.parametrize("name", sorted(cc.SCENES))
def test_covariances_depend_on_k(name):
    """k = 10, 5, 10 on one observation: a context that kept the covariances of the other k would refine differently."""
    s = cc.scene(name)
    for six in (True, False):
        a, b = cc.want_icp(name, six, 10), cc.want_icp(name, six, 5)
        assert (a[0].view(np.uint32) != b[0].view(np.uint32)).any(1).sum() >= QUARTER * len(s.icp_idx)


@pytest.mark.parametrize("x,y", cc.TRANSITIONS, ids=lambda v: v)
def test_stale_observed_colours_change_a_quarter_of_the_costs(x, y):
    X, Y = cc.scene(x), cc.scene(y)
    stale = Y.costs(1, rgb=cc.kept_buffer(X.obs_rgb, (len(Y.case.obs_xyz), 3)))
    n = cc.differing(stale, cc.want_costs(y, 1))
    print(f"{x} -> {y}: {n} of {Y.n} poses differ under X's colours")
    assert n >= QUARTER * Y.n


@pytest.mark.parametrize("x,y", cc.TRANSITIONS, ids=lambda v: v)
def test_stale_mesh_bank_changes_the_costs(x, y):
    """Y's poses scored on X's triangles (the models Y's poses name, taken from X's bank; its last model where X has
    fewer)."""
    import oracle

    X, Y = cc.scene(x), cc.scene(y)
    sx, sy = X.scene, Y.scene
    pm = np.minimum(Y.pose_model, len(sx.bank.tris_model_count) - 1).astype(np.int32)
    stale = oracle.evaluate(sx.bank.tris, sx.bank.tris_model_count, Y.poses, pm, Y.pose_label, sy.width,
                            sy.height, sy.proj, sy.src_depth_cm, sy.mask, 1.0, Y.stride, sy.cx, sy.cy, sy.fx, sy.fy,
                            100.0, Y.case.obs_xyz, Y.case.label_start, Y.case.label_end, Y.pose_obs_total, 2, True,
                            Y.res)
    if np.array_equal(sx.bank.tris, sy.bank.tris):
        assert cc.differing(stale, cc.want_costs(y, 2)) == 0  # B and C share the block
    else:
        assert cc.differing(stale, cc.want_costs(y, 2)) >= QUARTER * Y.n


def test_the_other_references_can_tell_the_scenes_apart():
    """The planar ICP, the point-to-plane ICP, count_within and the top-K lists each give another result on every scene
    of a transition, and within a scene the planar ICP's result depends on the radius and on the matrix."""
    for x, y in cc.TRANSITIONS + (("B", "F"),):
        assert not np.array_equal(cc.want_planar(x, 0, 0)[0], cc.want_planar(y, 0, 0)[0])
        assert not np.array_equal(cc.want_p2p(x)[0], cc.want_p2p(y)[0])
        assert not np.array_equal(cc.want_topk(x), cc.want_topk(y))
    for name in sorted(cc.SCENES):
        a, b, c = (cc.want_planar(name, m, r)[0] for m, r in ((0, 0), (0, 1), (1, 1)))
        assert not np.array_equal(a, b) and not np.array_equal(b, c)
        s = cc.scene(name)
        p = cc.want_p2p(name)
        assert (p[0] != s.poses[s.p2p_idx]).any(1).sum() >= len(s.p2p_idx) // 2 and len(np.unique(p[1])) >= 3
    # a camera that differs in fx alone: another scene (the x of every point), other refined poses
    assert not np.array_equal(cc.want_scene("B")[0], cc.want_scene("F")[0])
    assert {k: v for k, v in cc.SCENES["F"][1].items() if k != "fx"} == \
        {k: v for k, v in cc.SCENES["B"][1].items() if k != "fx"}


@pytest.mark.parametrize("name", ["B", "C", "F"])
def test_a_stale_segment_table_would_count_points(name):
    """count_within: the queries with labels 1 and 2 count 0 in a scene with one segment, and would count points of
    A's segments 1 and 2 if A's seg_lo / seg_hi entries were still read; the poses of those labels get the costs of
    an empty segment, which differ from the costs of the segment A has there."""
    from tests.test_valid_pose import _pcl_counts

    s, a = cc.scene(name), cc.scene("A")
    q, lab, radius, want = cc.count_queries(name)
    assert s.num_labels == 1 and want[lab >= 1].sum() == 0 and want[lab < 0].sum() == 0 and (want[lab == 0] > 0).any()
    assert lab.max() == cc.MAX_LABELS and lab.min() == -1
    for L in cc.EMPTY_LABELS:
        seg = a.case.obs_xyz[a.case.label_start[L]:a.case.label_end[L]]
        sel = lab == L
        assert sum(int(_pcl_counts(q[sel][radius[sel] == r], seg, r).sum()) for r in np.unique(radius)) > 0
    rc, oc, _ = cc.want_costs(name, 2)
    assert (s.pose_label[s.empty_idx] >= 1).all() and len(s.empty_idx) == 2 * cc.N_EMPTY
    assert (rc[s.empty_idx] == 100.0).all() and (oc[s.empty_idx] == 100.0).all()
    stale = s.costs(2, cloud=a)  # A's cloud and segment table under this scene's poses
    assert cc.differing(tuple(v[s.empty_idx] for v in stale), (rc[s.empty_idx], oc[s.empty_idx])) > 0


def test_the_sequences_shrink_and_grow_every_size():
    A, B, C = (cc.scene(n).shape for n in "ABC")
    assert A == dict(labels=3, seg=(142, 49, 48), num_obs=239, tris=6528, models=3, image=(200, 150), bitmap_words=8)
    assert B == dict(labels=1, seg=(134,), num_obs=134, tris=432, models=1, image=(200, 150), bitmap_words=5)
    assert C == dict(labels=1, seg=(97,), num_obs=97, tris=432, models=1, image=(96, 72), bitmap_words=4)
    for s in (A, B, C):
        assert s["bitmap_words"] == -(-max(s["seg"] + (s["num_obs"],)) // 32)
    assert [cc.scene(n).n for n in "ABC"] == [72, 48, 48]
    # A -> B: fewer labels, points, triangles and models on the same image; B -> C: a smaller image and fewer points;
    # C -> A: everything grows.  One sequence begins with a shrinking transition, the other with a growing one.
    assert cc.SEQUENCES[0][:2] == ("A", "B") and cc.SEQUENCES[1][:2] == ("C", "A")
    for k in ("labels", "num_obs", "tris", "models", "bitmap_words"):
        assert A[k] > B[k] >= C[k]
    assert max(A["seg"]) > max(B["seg"]) > max(C["seg"]) and len(A["seg"]) > len(B["seg"])
    assert A["image"] == B["image"] and C["image"][0] < B["image"][0] and C["image"][1] < B["image"][1]
    assert B["num_obs"] > C["num_obs"] and B["bitmap_words"] > C["bitmap_words"]
    assert cc.scene("C").res != cc.scene("B").res  # one transition changes the sensor resolution
    assert cc.scene("C").stride != cc.scene("B").stride
