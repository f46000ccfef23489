"""CPU certificate of the adversarial 1-NN cases of tests/nn_cases.py.  No kernel runs here.

A numpy restatement of phase 2 and 3 of the fused cost kernel -- float32 brute-force distances, a pluggable candidate
set, tie rule and radius test, the costs in the reference's float order -- equals oracle.evaluate and
oracle.evaluate_colour bit for bit under the true rules.  Under each wrong rule ("mutant") it must change the costs of
at least one pose of the case built against that rule: a case that cannot tell a wrong search from a right one fails
here, not silently on the GPU.  The conditions the builders are asked for (how many rendered points have a neighbour at
exactly r, a tie, a neighbour across a cell face) are asserted on the oracle's nearest neighbours.

  mutant                                   killed by
  d2 >= r2 is bad                          radius-*
  the highest index wins ties              ties-*
  the first candidate in CSR order wins    ties-*
  candidates from the query's cell only    faces-*
  candidates from the first x cell only    faces-*
  the box without its rounding bound       stretched-r0.0075-far-30-axis0, -far-60-axis0, -far-30-axis1, -far-60-axis1,
                                           stretched-r0.003-far-30-axis0

The colour cases (cost type 1, a colour per triangle) are certified at the end, from the oracle alone:
  a colour table rolled by one triangle    colour-*-plain: at least 90 % of the poses change
  the highest index wins a depth tie       colour-*-dup (copies in front of their originals change costs), colour-*-rev
  an id ring that goes stale when it wraps colour-*: more records queued than 4 waves' rings hold
"""
import numpy as np
import pytest

import oracle
from tests import nn_cases as nc
from tests.nn_cases import F32, nn_case

def _segment(case, label):
    """(points, positions in the label-sorted cloud, build_grid restated) of a segment, computed once."""
    cache = case.meta.setdefault("segments", {})
    if label not in cache:
        seg, where = case.segment(label)
        cache[label] = (seg, where, nc.build_grid_np(seg, case.r))
    return cache[label]


def _candidates(g, keep, Q, r, rule):
    """(n_q, n_kept) bool: which of the kept points of the segment the rule lets the query see."""
    cxyz = g.cxyz[keep]
    ingrid = g.cell_of[keep] >= 0
    if rule == "own_cell":
        m = np.repeat(ingrid[None, :], len(Q), axis=0)
        for a in range(3):
            m &= nc.cell_index(g, Q[:, a], a)[:, None] == cxyz[None, :, a]
        return m
    inside, i0, i1 = nc.box_of(g, Q, r, parent=rule == "parent_box")
    if rule == "first_x_cell":
        i1 = i1.copy()
        i1[:, 0] = i0[:, 0]
    m = inside[:, None] & ingrid[None, :]
    for a in range(3):
        m &= (cxyz[None, :, a] >= i0[:, a, None]) & (cxyz[None, :, a] <= i1[:, a, None])
    return m


def nearest(case, label, Q, cand="all", tie="low"):
    """(d2, position in the label-sorted cloud or -1) of each query's nearest candidate of the segment, brute force in
    float32.  Only the points within 1.5 r of the queries' bounds are looked at: that keeps every point within r of a
    query, so d2 is exact wherever it is at most r2 and some value above r2 (or inf) elsewhere, which is all the costs
    read."""
    seg, where, g = _segment(case, label)
    none = np.full(len(Q), np.inf, F32), np.full(len(Q), -1, np.int64)
    if len(seg) == 0 or len(Q) == 0:
        return none
    m = F32(1.5 * case.r)
    with np.errstate(invalid="ignore"):
        keep = np.nonzero(((seg >= Q.min(0) - m) & (seg <= Q.max(0) + m)).all(1))[0]
    if len(keep) == 0:
        return none
    D = nc.d2f(Q[:, None, :], seg[keep][None, :, :])
    D = np.where(np.isnan(D), F32(np.inf), D)
    if cand != "all":
        D = np.where(_candidates(g, keep, Q, case.r, cand), D, F32(np.inf))
    dmin = D.min(1)
    tied = (D == dmin[:, None]) & np.isfinite(dmin)[:, None]
    if tie == "low":
        j = tied.argmax(1)
    elif tie == "high":
        j = tied.shape[1] - 1 - tied[:, ::-1].argmax(1)
    else:  # the first in CSR order: by cell, then by index
        j = np.where(tied, g.rank[keep][None, :], np.iinfo(np.int64).max).argmin(1)
    return dmin, np.where(np.isfinite(dmin), where[keep[j]], -1)


_GATE = {}


def _within_gate(case):
    """(2, n_obs) bool: is the observed point's colour within the gate of model m's colour."""
    if case.name not in _GATE:
        cols, inv = np.unique(case.rgb_sorted, axis=0, return_inverse=True)
        ok = np.array([[oracle.colour_distance(oracle.rgb2lab(c), oracle.rgb2lab(m)) <= nc.COLOUR_THR for c in cols]
                       for m in nc.MODEL_RGB])
        _GATE[case.name] = ok[:, inv.reshape(-1)]
    return _GATE[case.name]


def costs_np(case, cost_type, cand="all", tie="low", bad="gt", calc_obs=True):
    r2 = nc.r2_of(case.r)
    rc, oc, df = (np.zeros(case.n, F32) for _ in range(3))
    tot = case.pose_obs_total if cost_type == 2 else case.pose_obs_total0
    for p in range(case.n):
        Q = case.Q[case.q_pose == p]
        d2, idx = nearest(case, int(case.pose_label[p]) if cost_type == 2 else None, Q, cand, tie)
        is_bad = d2 >= r2 if bad == "ge" else d2 > r2
        marks = ~is_bad & (idx >= 0)
        if cost_type == 1:
            gate = _within_gate(case)[case.pose_model[p], np.maximum(idx, 0)]
            is_bad = is_bad | (marks & ~gate)
            marks = marks & gate
        num, nbad = F32(len(Q)), F32(is_bad.sum())
        expl = F32(len(np.unique(idx[marks])))
        r = F32(-1.0) if num == 0 else nbad / num
        rc[p] = r if r == F32(-1.0) else r * F32(100.0)
        if calc_obs:
            df[p] = (num - nbad) - expl
            with np.errstate(invalid="ignore", divide="ignore"):
                oc[p] = (tot[p] - expl) / tot[p] * F32(100.0)
    return rc, oc, df


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


_ORACLE = {}


def oracle_costs(name, cost_type):
    if (name, cost_type) not in _ORACLE:
        _ORACLE[name, cost_type] = nn_case(name).oracle_costs(cost_type)
    return _ORACLE[name, cost_type]


def _changed(name, cost_type, **rule):
    """Poses whose costs the rule changes."""
    a, b = costs_np(nn_case(name), cost_type, **rule), oracle_costs(name, cost_type)
    return np.nonzero(~np.all([x.view(np.uint32) == y.view(np.uint32) for x, y in zip(a, b)], axis=0))[0]


# ---------------------------------------------------------------------------------------------
# the restatement is the oracle; the box as committed loses no neighbour
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_case_shape_and_restatement_equals_oracle(name):
    case = nn_case(name)
    assert 32 <= case.n <= 64 and len(case.obs_xyz) <= 21000
    assert not case.src_depth.any()
    for ct in (2, 0):
        want = oracle_costs(name, ct)
        assert _same(costs_np(case, ct), want), ct
        assert len(np.unique(want[0])) > 3 and len(np.unique(want[1])) > 3  # the costs are not all alike
    if name in nc.COLOUR_CASES:
        want = oracle_costs(name, 1)
        assert _same(costs_np(case, 1), want)
        assert not _same(want, oracle_costs(name, 0))  # the gate matters


@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_committed_box_restated_loses_no_neighbour(name):
    """process_points' box with its rounding bound, restated on build_grid restated: the oracle's costs."""
    case = nn_case(name)
    for ct in (2, 0):
        assert _same(costs_np(case, ct, cand="kernel_box"), oracle_costs(name, ct)), ct


def test_grid_restatement_on_a_stretched_segment():
    """The extent sets the cell (not 2.02 r) and an axis gets 64 or 65 cells: floor(64.0) + 1 when the float quotient
    reaches 64."""
    for name in ("stretched-r0.0075-far-30-axis0", "stretched-r0.05-far65-axis2"):
        case = nn_case(name)
        g = nc.build_grid_np(case.segment(0)[0], case.r)
        assert g.cell > 2.02 * case.r * 5 and g.n.max() in (64, 65), (g.cell, g.n)


# ---------------------------------------------------------------------------------------------
# conditions on the oracle's nearest neighbours
# ---------------------------------------------------------------------------------------------

def _unique_nn(case, label):
    u = case.unique_queries(label)
    seg, where = case.segment(label)
    d2, idx = oracle.knn1(u.Q, None, seg)
    return u, seg, d2, idx


@pytest.mark.parametrize("name", [n for n in nc.CASE_NAMES if n.startswith("radius")])
def test_radius_classes_are_populated(name):
    case = nn_case(name)
    r2 = nc.r2_of(case.r)
    targets = {"eq": r2, "above": np.nextafter(r2, F32(np.inf)), "below": np.nextafter(r2, F32(0))}
    got = {k: 0 for k in targets}
    for L in (0, 1):
        _, _, d2, _ = _unique_nn(case, L)
        for k, t in targets.items():
            got[k] += int((d2 == t).sum())
    assert min(got.values()) >= 50, got


@pytest.mark.parametrize("name", [n for n in nc.CASE_NAMES if n.startswith("ties")])
def test_ties_are_populated(name):
    """Rendered points whose smallest d2 is reached by two observed points: at least 200, at least 20 of them with the
    two in different cells, at least 20 with two exact duplicates; and ties show in the costs of the true rule: some
    pose explains both candidates of a tie."""
    case = nn_case(name)
    ties = cross = dups = 0
    for L in (0, 1):
        u, seg, d2, idx = _unique_nn(case, L)
        g = nc.build_grid_np(seg, case.r)
        D = nc.d2f(u.Q[:, None, :], seg[None, :, :])
        tied = (D == d2[:, None]) & (d2 <= nc.r2_of(case.r))[:, None]
        for row in np.nonzero(tied.sum(1) >= 2)[0]:
            j = np.nonzero(tied[row])[0]
            ties += 1
            cross += len(np.unique(g.cell_of[j])) > 1
            dups += len(np.unique(seg[j].view(np.uint32), axis=0)) == 1
    assert ties >= 200 and cross >= 20 and dups >= 20, (ties, cross, dups)


@pytest.mark.parametrize("name", [n for n in nc.CASE_NAMES if n.startswith("faces")])
def test_cross_face_neighbours_are_populated(name):
    """Per axis, at least 200 rendered points whose nearest neighbour is within r and in another cell along that axis;
    neighbours in the first and in the last cell of an axis; queries outside the grid's box with a neighbour; and a
    rendered point whose box touches four (y, z) rows, each of them populated."""
    case = nn_case(name)
    r2 = nc.r2_of(case.r)
    per_axis = np.zeros(3, int)
    first = last = outside = four = 0
    for L in (0, 1):
        u, seg, d2, idx = _unique_nn(case, L)
        g = nc.build_grid_np(seg, case.r)
        near = d2 <= r2
        f = np.stack([nc.cell_coord(g, u.Q[:, a], a) for a in range(3)], 1)
        qc = np.stack([nc.cell_index(g, u.Q[:, a], a) for a in range(3)], 1)
        oc = g.cxyz[idx]
        out = ((f < 0) | (f >= g.n[None, :].astype(F32))).any(1)
        for a in range(3):
            per_axis[a] += int((near & ~out & (oc[:, a] != qc[:, a])).sum())
        first += int((near & (oc == 0).any(1) & (qc != 0).any(1)).sum())
        last += int((near & (oc == g.n[None, :] - 1).any(1)).sum())
        outside += int((near & out).sum())
        inside, i0, i1 = nc.box_of(g, u.Q, case.r)
        rows = set(map(tuple, g.cxyz[g.cell_of >= 0]))
        cells = {}
        for c in rows:
            cells.setdefault((c[1], c[2]), set()).add(c[0])
        for k in np.nonzero(inside & (i1[:, 1] > i0[:, 1]) & (i1[:, 2] > i0[:, 2]))[0]:
            xs = set(range(i0[k, 0], i1[k, 0] + 1))
            four += all(cells.get((i0[k, 1] + dy, i0[k, 2] + dz), set()) & xs for dy in (0, 1) for dz in (0, 1))
    assert per_axis.min() >= 200, per_axis
    assert first >= 5 and last >= 5 and outside >= 5 and four >= 1, (first, last, outside, four)


STRETCHED_X = [n for n in nc.CASE_NAMES if n.startswith("stretched") and not n.endswith("axis2")]


@pytest.mark.parametrize("name", STRETCHED_X)
def test_stretched_face_has_neighbours_across_it(name):
    """The far point sets the cell (extent / 64), the face between cells 62 and 63 lies within (r (1 - 1e-4), r] of a
    column (row) of a face-on pose, and the rendered points of that column have their nearest neighbour across it,
    within r -- every one of them.  Only the samples of one column (row) of one depth share the coordinate, so the count
    asked for is not the 200 of the ordinary grid: at 0.6 m the box's face is 12 sample rows high (the in-plane shifts
    add more of the same column) and the can's cap 5 wide, hence at least 3 per segment and 12 per case."""
    case = nn_case(name)
    axis = int(name[-1])
    total = 0
    for L in (0, 1):
        s = case.meta["search"][L]
        u, seg, d2, idx = _unique_nn(case, L)
        g = nc.build_grid_np(seg, case.r)
        assert g.cell > 0.1 and g.n[axis] in (64, 65)
        assert case.r * (1 - 1e-4) < s["face"] - s["coord"] <= case.r
        col = u.Q[:, axis] == F32(s["coord"])
        across = col & (d2 <= nc.r2_of(case.r)) & (g.cxyz[idx, axis] == 63) & \
            (np.floor(nc.cell_coord(g, u.Q[:, axis], axis)) == 62)
        total += int(across.sum())
        assert across.sum() >= 3 and across.sum() == col.sum(), (L, int(col.sum()), int(across.sum()))
    assert total >= 12, total


# ---------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in nc.CASE_NAMES if n.startswith("radius")])
def test_mutant_radius_inclusive(name):
    for ct in (2, 0):
        assert len(_changed(name, ct, bad="ge")) > 0, ct


@pytest.mark.parametrize("name", [n for n in nc.CASE_NAMES if n.startswith("ties")])
@pytest.mark.parametrize("tie", ["high", "csr"])
def test_mutant_tie_rule(name, tie):
    """Visible in the depth costs (types 0 and 2) through the witnesses, and in the colour cost through the gate."""
    for ct in (2, 0, 1):
        assert len(_changed(name, ct, tie=tie)) > 0, ct


@pytest.mark.parametrize("name", [n for n in nc.CASE_NAMES if n.startswith("faces")])
@pytest.mark.parametrize("cand", ["own_cell", "first_x_cell"])
def test_mutant_candidate_cells(name, cand):
    for ct in (2, 0):
        assert len(_changed(name, ct, cand=cand)) > 0, ct


PARENT_BOX_KILLERS = ("stretched-r0.0075-far-30-axis0", "stretched-r0.0075-far-60-axis0",
                      "stretched-r0.0075-far-30-axis1", "stretched-r0.0075-far-60-axis1",
                      "stretched-r0.003-far-30-axis0")


@pytest.mark.parametrize("name", PARENT_BOX_KILLERS)
def test_mutant_parent_box_padding(name):
    """The box as it was before its rounding bound: r 1.0001 + 1e-7 alone.  With the grid's origin 30 m or more from
    the object the rounding of fl(fl(q - o) / cell) exceeds that pad, and the restated box leaves out the cell beyond
    the face for the rendered points of the chosen column: their neighbour within r is lost and the pose's costs
    change.  (At r = 0.01 and at 10 m the search of nn_cases.stretched_case finds no such placement.)"""
    case = nn_case(name)
    assert any(s["missed"] for s in case.meta["search"].values())
    assert len(_changed(name, 2, cand="parent_box")) > 0


# ---------------------------------------------------------------------------------------------
# per-triangle colours (cost type 1): what the colour cases can tell apart, from the oracle alone
# ---------------------------------------------------------------------------------------------

def _colour_want(geom, variant):
    key = ("colour", geom, variant)
    if key not in _ORACLE:
        _ORACLE[key] = nc.colour_case(geom, variant).oracle_costs(1)
    return _ORACLE[key]


def _differ(a, b):
    """Poses whose costs differ between two results."""
    return np.nonzero(~np.all([x.view(np.uint32) == y.view(np.uint32) for x, y in zip(a, b)], axis=0))[0]


_PAIRS = {}


def colour_pairs(geom, variant):
    """nn_cases.gated_pairs with the neighbours of this module's brute force (`nearest`), computed once."""
    if (geom, variant) not in _PAIRS:
        case = nc.colour_case(geom, variant)
        d2, idx = np.full(len(case.Q), np.inf, F32), np.full(len(case.Q), -1, np.int64)
        for p in range(case.n):
            sel = case.q_pose == p
            d2[sel], idx[sel] = nearest(case, None, case.Q[sel])
        _PAIRS[geom, variant] = nc.gated_pairs(case, (d2, idx))
    return _PAIRS[geom, variant]


@pytest.mark.parametrize("variant", nc.COLOUR_VARIANTS)
@pytest.mark.parametrize("geom", nc.COLOUR_GEOMETRIES)
def test_colour_pairs_restate_the_oracle_and_straddle_the_gate(geom, variant):
    """The gated (observed point, triangle) pairs -- the triangle from the oracle's colour planes with the triangle
    index in the colour bytes, the neighbour from the brute force above, the distance from the oracle -- give the
    oracle's costs bit for bit, at the default threshold and at two others; between 15 % and 85 % of them are within
    the gate; every pose has some."""
    case = nc.colour_case(geom, variant)
    pairs = colour_pairs(geom, variant)
    assert 32 <= case.n <= 64 and len(case.obs_xyz) <= 21000 and not case.src_depth.any()
    assert _same(nc.colour_costs_np(case, pairs, nc.COLOUR_THR), _colour_want(geom, variant))
    for thr in (6.5, 31.0):
        assert _same(nc.colour_costs_np(case, pairs, thr), case.oracle_costs(1, colour_thr=thr)), thr
    share = float((pairs.d <= nc.COLOUR_THR).mean())
    assert 0.15 <= share <= 0.85, share
    assert len(np.unique(pairs.pose)) == int((pairs.num > 0).sum()) == case.n
    assert not _same(_colour_want(geom, variant), case.oracle_costs(0))  # the gate matters


@pytest.mark.parametrize("geom", nc.COLOUR_GEOMETRIES)
def test_colour_table_rolled_by_one_triangle(geom):
    """A sample coloured by the triangle before its own (a stream slot with its neighbour's entry of stri_orig): the
    costs of at least 90 % of the poses that render anything change."""
    case = nc.colour_case(geom, "plain")
    want = _colour_want(geom, "plain")
    cnt = case.bank.tris_model_count
    rolled = nc._with_mesh(case, "rolled", [m.tris for m in case.bank.models],
                           np.split(np.roll(case.bank.colors, 1, axis=0), np.cumsum(cnt)[:-1]), case.obs_rgb)
    renders = int((want[0] != F32(-1.0)).sum())
    changed = len(_differ(rolled.oracle_costs(1), want))
    assert renders >= 32 and changed >= 0.9 * renders, (changed, renders)


@pytest.mark.parametrize("geom", nc.COLOUR_GEOMETRIES)
def test_colour_dup_copies_in_front_change_costs(geom):
    """dup: at least 32 triangles per model appended once more with a colour on the other side of the gate.  Behind
    their originals the copies change nothing (the lowest index wins a depth tie); in front of them they win, and
    some pose's costs change: the highest index winning, or an id left by a later fragment, shows in this case."""
    dup = nc.colour_case(geom, "dup")
    for m, ids in enumerate(dup.meta["copied"]):
        assert len(ids) >= 32 and len(np.unique(ids)) == len(ids), m
    assert _same(_colour_want(geom, "dup"), _colour_want(geom, "plain"))
    assert len(_differ(nc.colour_case(geom, "dup-front").oracle_costs(1), _colour_want(geom, "dup"))) > 0


def depth_ties(geom):
    """Rendered points whose minimum depth is reached by two or more triangles: the winner of the reversed mesh,
    mapped back to the plain order, is the highest tied index, the plain winner the lowest.  Returns (ties, ties
    between differently coloured triangles, those among the gated pairs)."""
    plain, rev = nc.colour_case(geom, "plain"), nc.colour_case(geom, "rev")
    hi = np.cumsum(plain.bank.tris_model_count)
    lo = hi - plain.bank.tris_model_count
    m = plain.pose_model[plain.q_pose]
    low, high = nc.sample_triangles(plain), lo[m] + (hi[m] - 1 - nc.sample_triangles(rev))
    assert (low <= high).all()
    col = plain.bank.colors
    tie = low != high
    coloured = tie & (col[low] != col[high]).any(1)
    return int(tie.sum()), int(coloured.sum()), int(coloured[colour_pairs(geom, "plain").q].sum())


@pytest.mark.parametrize("geom", nc.COLOUR_GEOMETRIES)
def test_colour_rev_differs_through_depth_ties(geom):
    """rev renders the same depths; only the winners of depth ties change.  Its costs differ from the plain case's in
    at least one pose: depth ties between differently coloured triangles occur among the gated samples and decide
    costs."""
    plain, rev = nc.colour_case(geom, "plain"), nc.colour_case(geom, "rev")
    assert np.array_equal(_colour_want(geom, "plain")[0] == F32(-1.0), _colour_want(geom, "rev")[0] == F32(-1.0))
    assert _same(plain.oracle_costs(0), rev.oracle_costs(0))  # the depth cost does not see the order
    ties, coloured, gated = depth_ties(geom)
    assert gated >= 8, (ties, coloured, gated)
    assert len(_differ(_colour_want(geom, "rev"), _colour_want(geom, "plain"))) > 0


def test_colour_id_ring_wraps():
    """A wave's record ring holds kRecCap = 128 records, and ring_id with it.  Every model has a pose that queues more
    than 128 triangles in every colour case; and in ties-TINY-s1 every model has a pose that queues more than 1.5
    times 4 x 128 records (the box does in segments-s4 too), so that whichever way the triangles fall to the
    workgroup's 4 waves, one wave's ring wraps.  (The window restated in float64 may differ from the kernel's by a
    sample on a few triangles: hence the factor.  On the SMALL camera the can's largest pose queues about 540
    records.)"""
    for geom in nc.COLOUR_GEOMETRIES:
        case = nc.colour_case(geom, "plain")
        q = np.array([nc.queued_records(case, p) for p in range(case.n)])
        for m in range(len(case.bank.models)):
            tris, recs = q[case.pose_model == m].max(0)
            assert tris > 128, (geom, m, tris)
            if geom == "ties-TINY-s1" or (geom, m) == ("segments-s4", 0):
                assert recs > 1.5 * 4 * 128, (geom, m, recs)


# ---------------------------------------------------------------------------------------------
# the threshold sweep: gated pairs whose distance, used as the threshold, pins the device's distance to the bit
# ---------------------------------------------------------------------------------------------

SWEEP_GEOM, SWEEP_MIN = "segments-s4", 64
_SWEEP = {}


def sweep_picks():
    """Gated pairs of the plain SWEEP_GEOM case for the sweep of tests/test_gpu_colour.py, computed once: a list of
    (pair, d as float32, the oracle's costs at threshold d, the oracle's costs at the float32 below d) and the number
    of candidates that had to be replaced.  The distance is a float32 widened to double (its last operation is a
    float square root), so the threshold d sits on it: at d the pair is within the gate, one float below it is
    beyond.  Candidates: the pairs at SWEEP_MIN evenly spaced ranks of the sorted distances, the smallest and the
    largest among them, then the median pair of every pose that has none yet.  A candidate for whose pose the
    oracle's own costs do not differ between the two thresholds is replaced by the pair of the next rank."""
    if "picks" in _SWEEP:
        return _SWEEP["picks"]
    case, pairs = nc.colour_case(SWEEP_GEOM, "plain"), colour_pairs(SWEEP_GEOM, "plain")
    order = np.argsort(pairs.d, kind="stable")
    cand = list(order[np.unique(np.linspace(0, len(order) - 1, SWEEP_MIN).round().astype(int))])
    have = set(pairs.pose[cand])
    for p in np.unique(pairs.pose):
        if p not in have:
            mine = order[pairs.pose[order] == p]
            cand.append(mine[len(mine) // 2])
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    picks, used, replaced = [], set(), 0
    for k in cand:
        first = True
        while True:
            d = F32(pairs.d[k])
            assert np.float64(d) == pairs.d[k] and np.isfinite(d)  # a float32, widened
            if k not in used:
                below = nc.step(d, -1)
                hi, lo = case.oracle_costs(1, colour_thr=float(d)), case.oracle_costs(1, colour_thr=float(below))
                if pairs.pose[k] in _differ(hi, lo):
                    break
            if first:
                replaced, first = replaced + 1, False
            k = order[(rank[k] + 1) % len(order)]
        used.add(k)
        picks.append((int(k), d, hi, lo))
    _SWEEP["picks"] = (picks, replaced)
    return _SWEEP["picks"]


def test_colour_sweep_picks():
    """At least 64 picked pairs; every pose with gated pairs has one; the smallest and the largest distance are
    among them and the picks span the distances' quantiles; for every pick the oracle's costs of its pose differ
    between the threshold on the distance and the float32 below it (sweep_picks replaces a candidate that fails)."""
    pairs = colour_pairs(SWEEP_GEOM, "plain")
    picks, replaced = sweep_picks()
    ks = np.array([k for k, *_ in picks])
    assert len(ks) >= SWEEP_MIN and len(np.unique(ks)) == len(ks)
    assert set(pairs.pose[ks]) == set(pairs.pose)
    ds = np.array([d for _, d, *_ in picks], np.float64)
    assert ds.min() == pairs.d.min() and ds.max() == pairs.d.max()
    q = np.searchsorted(np.sort(pairs.d), ds) / len(pairs.d)  # each decile of the distances has a pick
    assert (np.bincount(np.minimum((q * 10).astype(int), 9), minlength=10) >= 3).all()
    for k, d, hi, lo in picks:
        assert pairs.pose[k] in _differ(hi, lo)
    print(f"sweep: {len(picks)} pairs, {replaced} replaced, d in [{ds.min()}, {ds.max()}]")
