"""CPU certificates of tests/csr_rows_cases.py: the GPU test of tests/test_gpu_csr_rows.py could fail.  On the numpy
restatement of build_grid and of the query's radius box (tests/nn_cases.py): every chosen query's box has four rows
whose CSR lengths are the configuration's, {0, 1, 5, 0}, {3, 0, 0, 2} or {7, 7, 7, 7}; exactly one candidate of the
flattened sequence lies within r, at the planned position, and every position of every configuration is planned once;
the tie queries hold two candidates at exactly equal float distance within r in rows 1 and 2; and turning any planned
near point into a miss changes a cost (its query's sample has no other neighbour)."""
import numpy as np

from tests import csr_rows_cases as cr
from tests import nn_cases as nc


def _rows_of(case, g, m):
    """Per row of the query's box: the positions (in the segment's local order) of its points, in CSR order."""
    _, i0, i1 = nc.box_of(g, m["q"][None], cr.R)
    out = []
    for cell in cr._row_cells(i0[0], i1[0]):
        assert cell is not None
        iy, iz = cell
        inrow = np.nonzero((g.cxyz[:, 1] == iy) & (g.cxyz[:, 2] == iz) & (g.cxyz[:, 0] >= i0[0][0]) &
                           (g.cxyz[:, 0] <= i1[0][0]))[0]
        out.append(inrow[np.argsort(g.rank[inrow])])
    return out


def test_rows_positions_and_ties():
    case = cr.case()
    seg, _ = case.segment(0)
    g = nc.build_grid_np(seg, cr.R)
    assert np.array_equal(g.o, case.meta["grid_lo"]) and g.cell == np.float32(2.0) * np.float32(cr.R) * np.float32(1.01)
    r2 = nc.r2_of(cr.R)
    seen, ties = set(), 0
    for m in case.meta["queries"]:
        rows = _rows_of(case, g, m)
        assert tuple(len(r) for r in rows) == cr.ROWS[m["cfg"]], (m["cfg"], [len(r) for r in rows])
        flat = np.concatenate(rows)
        assert len(flat) == m["n"] and np.array_equal(np.sort(flat), np.arange(m["first"], m["first"] + m["n"]))
        d = nc.d2f(m["q"][None], seg[flat])
        near = np.nonzero(d <= r2)[0]
        if m["tie"]:
            l0, l1 = cr.ROWS[2][0], cr.ROWS[2][0] + cr.ROWS[2][1]
            assert len(near) == 2 and l0 <= near[0] < l1 <= near[1] < l1 + cr.ROWS[2][2]   # rows 1 and 2
            assert d[near[0]] == d[near[1]] and d[near[0]] > 0
            ties += 1
        else:
            assert list(near) == [m["pos"]], (m["cfg"], m["pos"], near)
            assert (d[np.arange(len(d)) != m["pos"]] > r2 * np.float32(1.3)).all()
            seen.add((m["cfg"], m["pos"]))
    assert seen == {(c, p) for c in range(3) for p in range(sum(cr.ROWS[c]))} and ties == cr.N_TIES
    assert sum(cr.ROWS[0]) % 4 and sum(cr.ROWS[1]) % 4


def test_a_lost_near_point_changes_a_cost():
    """Without the planned near points the 6-DoF rendered cost of their poses differs: each such query has no other
    neighbour, so a search that reads the wrong candidate there is seen."""
    case = cr.case()
    want = case.oracle_costs(2)
    import copy
    other = copy.copy(case)
    keep = np.ones(len(case.obs_xyz), bool)
    for m in case.meta["queries"]:
        if not m["tie"]:
            keep[m["first"] + _flat_index(case, m)] = False
    other.obs_xyz, other.obs_label, other.obs_rgb = case.obs_xyz[keep], case.obs_label[keep], case.obs_rgb[keep]
    other.finish()
    got = other.oracle_costs(2)
    removed = int((~keep).sum())
    assert removed == sum(sum(r) for r in cr.ROWS)
    # every removed point is one more bad sample in each pose that renders its query (a query is a distinct rendered
    # point: other face-on poses may render the same one)
    num = np.bincount(case.q_pose, minlength=case.n).astype(np.float64)
    more = (got[0].astype(np.float64) - want[0].astype(np.float64)) / 100.0 * num
    for m in case.meta["queries"]:
        if not m["tie"]:
            assert more[m["pose"]] > 0.5, m["pose"]
    assert more.sum() > removed - 0.01


def _flat_index(case, m):
    seg, _ = case.segment(0)
    g = nc.build_grid_np(seg, cr.R)
    flat = np.concatenate(_rows_of(case, g, m))
    return int(flat[m["pos"]]) - m["first"]
