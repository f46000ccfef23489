"""A segment whose radius boxes hold prescribed CSR rows, for the candidate loop of the fused kernel's 1-NN search
(process_points, pcore_fused.hip): the <= 4 (y, z) rows of a query's box are read as one flattened sequence, four
candidates at a time, and candidate k is mapped back to its row.

The camera, meshes and poses of tests/nn_cases.py (SMALL, stride 4, r = 0.01, the box face-on at 1.1 m).  Segment 0 is
built around chosen rendered points q of the twelve face-on poses, at least three cells apart, two frame points fixing the grid's
origin so that q's cell coordinate along z is c + 0.9: the box of q spans two cells along y and z, four rows.  Every row
gets the number of points its configuration names,
    ROWS = {0, 1, 5, 0}, {3, 0, 0, 2}, {7, 7, 7, 7}        (ltot = 6, 5, 28: 6 mod 4 and 5 mod 4 are not 0)
all of them `far` (in the row's cells, more than r from q: 0.1 or 0.9 of a cell along each axis) except ONE `near`
point within r, and there is one query per position of the near point in the flattened sequence (6 + 5 + 28 queries):
a loop that maps some k to the wrong point, skips an empty row wrongly or mishandles the clamped tail turns that
query's sample from explained to bad.  For {7, 7, 7, 7} four more queries carry two near points at exactly equal
float distance in rows 1 and 2 (across a row boundary; the lowest index wins, and either way one observed point is
explained).  tests/test_csr_rows_cases.py certifies rows, distances and ties on the numpy restatement of the grid."""
from __future__ import annotations

import functools

import numpy as np

from tests import nn_cases as nc
from tests.helpers import SMALL

F32 = np.float32
R = 0.01
ROWS = ((0, 1, 5, 0), (3, 0, 0, 2), (7, 7, 7, 7))
Z_FACE = 1.1
N_TIES = 4


def _row_cells(i0, i1):
    """The kernel's four rows (iy, iz), row q = (iy0 + (q & 1), iz0 + (q >> 1)); None where the box has no such row."""
    return [((i0[1] + (q & 1), i0[2] + (q >> 1)) if i0[1] + (q & 1) <= i1[1] and i0[2] + (q >> 1) <= i1[2] else None)
            for q in range(4)]


def _axis_coords(g, q, axis, c, t):
    """(near, far) coordinate along `axis` of a point in cell c for the query q: near is q's own coordinate in q's cell
    and q -+ t in the neighbour, far is 0.1 / 0.9 of the cell from its low face, whichever is further from q."""
    f = float(nc.cell_coord(g, q[axis], axis))
    cq = int(np.floor(f))
    cell, o = float(g.cell), float(g.o[axis])
    if c == cq:
        near = float(q[axis])
        far = o + (c + (0.1 if f - cq > 0.5 else 0.9)) * cell
    elif c == cq + 1:
        near, far = float(q[axis]) + t, o + (c + 0.9) * cell
    else:
        near, far = float(q[axis]) - t, o + (c + 0.1) * cell
    return F32(near), F32(far)


@functools.lru_cache(maxsize=None)
def case():
    P, M = nc.pose_set(Z_FACE)
    c = nc.NNCase("csr-rows", SMALL, 4, R, P, M)
    u = c.unique_queries(0)
    face = u.pose < 12                                    # the twelve face-on poses at Z_FACE
    zq = np.bincount(u.Z[face]).argmax()                  # the face's depth (cm)
    sel = np.nonzero(face & (u.Z == zq))[0]
    Q = u.Q[sel]
    cell = F32(2.0) * F32(R) * F32(1.01)
    lo = np.array([Q[:, 0].min() - 3 * cell, Q[:, 1].min() - 3 * cell, Q[0, 2] - F32(2.9) * cell], F32)
    hi = np.array([Q[:, 0].max() + 3 * cell, Q[:, 1].max() + 3 * cell, lo[2] + 6 * cell], F32)
    g = nc.grid_params(lo, hi, R)
    assert g.cell == cell
    t = float(F32(49 * 2.0 ** -13))  # 0.296 of a cell: across the nearer face from frac >= 0.73 / <= 0.27
    # queries whose box spans two cells along y and z, away from the x faces, three cells apart (a cluster stays
    # within one cell of its query's)
    fx, fy = nc.cell_coord(g, Q[:, 0], 0), nc.cell_coord(g, Q[:, 1], 1)
    frx, fry = fx - np.floor(fx), fy - np.floor(fy)
    ok = (frx > 0.1) & (frx < 0.8) & (((fry > 0.73) & (fry < 0.98)) | ((fry > 0.02) & (fry < 0.27)))
    chosen = []
    for i in np.nonzero(ok)[0]:
        if all(max(abs(fx[i] - fx[j]), abs(fy[i] - fy[j])) >= 3.0 for j in chosen):
            chosen.append(int(i))
    plan = [(cfg, p, False) for cfg in range(3) for p in range(sum(ROWS[cfg]))] + [(2, -1, True)] * N_TIES
    assert len(chosen) >= len(plan), (len(chosen), len(plan))
    # a tie needs the y neighbour above q's cell (rows 1 and 2 are then both one cell from q's own): those queries first
    upper = [i for i in chosen if fry[i] > 0.5]
    assert len(upper) >= N_TIES
    order = [i for i in chosen if i not in upper[:N_TIES]][:len(plan) - N_TIES] + upper[:N_TIES]
    pts, meta = [lo, hi], []
    for (cfg, p, tie), i in zip(plan, order):
        q = Q[i]
        _, i0, i1 = nc.box_of(g, q[None], R)
        rows = _row_cells(i0[0], i1[0])
        assert all(r is not None for r in rows)
        k = 0
        first = len(pts)
        for r, (cy, cz) in enumerate(rows):
            ny_, fy_ = _axis_coords(g, q, 1, cy, t)
            nz_, fz_ = _axis_coords(g, q, 2, cz, t)
            for j in range(ROWS[cfg][r]):
                near = (k == p) if not tie else (j == 3 and r in (1, 2))
                x = F32(q[0] + F32(0.01 * j) * cell)
                if near and tie and r == 1:
                    # the same float distance as row 2's near point, whose dz is exact: q.y -+ |dz|
                    dz = abs(F32(q[2]) - _axis_coords(g, q, 2, rows[2][1], t)[0])
                    ny_t = F32(q[1] + dz) if ny_ > q[1] else F32(q[1] - dz)
                    pts.append(np.array([q[0], ny_t, nz_], F32))
                elif near:
                    pts.append(np.array([q[0] if tie else x, ny_, nz_], F32))
                else:
                    pts.append(np.array([x, fy_, fz_], F32))
                k += 1
        meta.append(dict(q=q, cfg=cfg, pos=p, tie=tie, first=first, n=k, pose=int(u.pose[sel][i])))
    seg0 = np.stack(pts).astype(F32)
    # segment 1 (the can's poses): a few of its own rendered points, so that the label exists
    seg1 = c.unique_queries(1).Q[:40]
    c.obs_xyz = np.ascontiguousarray(np.concatenate([seg0, seg1]).astype(F32))
    c.obs_label = np.concatenate([np.zeros(len(seg0), np.int32), np.ones(len(seg1), np.int32)])
    c.obs_rgb = np.ascontiguousarray(nc._rgb_for(c.obs_label, np.ones(len(c.obs_label), bool)).astype(np.uint8))
    c.finish()
    c.meta.update(queries=meta, grid_lo=lo, grid_hi=hi)
    return c
