// pcore_nn_grid.h -- the exact neighbour search over a segment's grid (segments above kGridNNMin points;
// pcore_internal.h LabelGrid): grid_shells, the GICP correspondence by it (grid_nn) and the k-best list of the
// covariances' k-NN over the same shells (knn_insert_lex, covariance_grid_kernel).  Results are the brute-force
// scan's, bit for bit (tests/test_gpu_nn_adversarial.py).
#pragma once

#include "pcore_internal.h"

namespace pcore {
namespace {

__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;
}

// Cells are visited in shells of growing Chebyshev radius r around the query's cell.  A point binned in
// cell i has its float cell coordinate fp in [i, i + 1) (the grid spans the points' own bounds, so no
// clamping), so along each axis |fp - fq| is at least the gap between fq and that interval, and the true
// distance at least (gap - eps) * cell; a cell whose bound exceeds the caller's limit (the best distance,
// or the k-th best once k are held) is skipped without loading it, and the search stops once the limit is
// below the bound of the nearest face of the visited box that still has cells beyond it.  Every skipped
// point is strictly farther than the limit, so the result equals the brute-force scan's lexicographic
// minimum of (float distance, index).
// Returns false when the cell budget runs out first (or the query is far outside the grid): the caller
// then scans the whole segment.  Non-finite queries are the caller's business.
// Cell budget of one search: a visited cell costs about as much as two points of the in-order scan (its lower-bound
// test, the CSR range loads, the loop), so the shells may visit up to half the segment's point count before the scan
// would have been cheaper, and at least 343 cells (r <= 3 around an in-grid query).  C1 (a 19.2 k-point whole-scene
// target, `tools/c1_gicp_stats.py`): a fixed 343-cell budget sent the queries of poses that GICP walks away from the
// scene into the 19.2 k-point scan, 64.7 ms per GICP call; budgets of 2,197 / 9,261 / 35,937 cells gave 18.6 / 18.4 /
// 18.2 ms, and this rule 19.7 ms (profiles/r03x/).  Measured and dropped: the 343-cell shells followed by an exact
// search over the grid's list of non-empty cells (an upper bound from the least farthest-corner distance, then the
// cells whose lower bound is within it) instead of the in-order scan, 37.1 ms.
__device__ __forceinline__ int shell_budget(int n) { return max(343, n >> 1); }

template <typename Visit, typename Limit>
__device__ __forceinline__ bool grid_shells(const LabelGrid& g, const int32_t* cell_start, float qx, float qy,
                                            float qz, int budget, Visit&& visit, Limit&& limit) {
    const float fx = (qx - g.ox) * g.inv_c, fy = (qy - g.oy) * g.inv_c, fz = (qz - g.oz) * g.inv_c;
    const float fm = fmaxf(fabsf(fx), fmaxf(fabsf(fy), fabsf(fz)));
    if (!(fm < 65536.0f)) return false;
    const int cx = (int)floorf(fx), cy = (int)floorf(fy), cz = (int)floorf(fz);
    const float e = 0.01f + 1e-6f * fm;  // cell-unit slack for the rounding of fp, fq and inv_c
    const float c2 = g.cell * g.cell * 0.99999f;
    // lower bound of the float squared distance from q to any point binned in cell (ix, iy, iz): a point's
    // cell coordinate fp lies in [i, i + 1), so |fp - fq| >= gap along each axis
    auto cell_lb = [&](int ix, int iy, int iz) {
        const float gx = fmaxf(fmaxf((float)ix - fx, fx - (float)(ix + 1)) - e, 0.0f);
        const float gy = fmaxf(fmaxf((float)iy - fy, fy - (float)(iy + 1)) - e, 0.0f);
        const float gz = fmaxf(fmaxf((float)iz - fz, fz - (float)(iz + 1)) - e, 0.0f);
        return (gx * gx + gy * gy + gz * gz) * c2;
    };
    auto try_cell = [&](int row, int ix, int iy, int iz) {
        if (cell_lb(ix, iy, iz) > limit()) return;  // every point of the cell is strictly farther
        visit(cell_start[row + ix], cell_start[row + ix + 1]);
    };
    int visited = 0;
    for (int r = 0;; r++) {
        const int z0 = max(0, cz - r), z1 = min(g.nz - 1, cz + r);
        const int y0 = max(0, cy - r), y1 = min(g.ny - 1, cy + r);
        const int x0 = max(0, cx - r), x1 = min(g.nx - 1, cx + r);
        for (int iz = z0; iz <= z1; iz++)
            for (int iy = y0; iy <= y1; iy++) {
                const int row = g.cell_base + (iz * g.ny + iy) * g.nx;
                const bool face = iz == cz - r || iz == cz + r || iy == cy - r || iy == cy + r;
                if (face) {
                    for (int ix = x0; ix <= x1; ix++) try_cell(row, ix, iy, iz);
                    visited += x1 >= x0 ? x1 - x0 + 1 : 0;
                } else {
                    if (cx - r >= 0 && cx - r < g.nx) {
                        try_cell(row, cx - r, iy, iz);
                        visited++;
                    }
                    if (r > 0 && cx + r >= 0 && cx + r < g.nx) {
                        try_cell(row, cx + r, iy, iz);
                        visited++;
                    }
                }
            }
        // unvisited cells lie beyond the faces of the box [c - r, c + r + 1) that are inside the grid; the
        // distance from fq to the nearest such face bounds every unvisited point
        float B = INFINITY;
        if (cx - r > 0) B = fminf(B, fx - (float)(cx - r));
        if (cx + r < g.nx - 1) B = fminf(B, (float)(cx + r + 1) - fx);
        if (cy - r > 0) B = fminf(B, fy - (float)(cy - r));
        if (cy + r < g.ny - 1) B = fminf(B, (float)(cy + r + 1) - fy);
        if (cz - r > 0) B = fminf(B, fz - (float)(cz - r));
        if (cz + r < g.nz - 1) B = fminf(B, (float)(cz + r + 1) - fz);
        if (B == INFINITY) return true;  // every cell visited
        B -= e;
        if (B > 0.0f && limit() < B * B * c2) return true;
        if (visited >= budget) return false;
    }
}

// k best (distance, index) pairs in lexicographic order, as the brute-force insertion keeps them
template <int KMAX>
__device__ __forceinline__ void knn_insert_lex(float (&nd)[KMAX], int (&nb)[KMAX], int& cnt, int k, float d, int j) {
    if (cnt == k && !(d < nd[k - 1] || (d == nd[k - 1] && j < nb[k - 1]))) return;
    const int pos = cnt < k ? cnt : k - 1;
    int c = 0;
#pragma unroll
    for (int q = 0; q < KMAX; q++) c += (q < pos && (nd[q] > d || (nd[q] == d && nb[q] > j))) ? 1 : 0;
    const int fin = pos - c;
#pragma unroll
    for (int q = KMAX - 1; q >= 1; q--)
        if (q > fin && q <= pos) { nd[q] = nd[q - 1]; nb[q] = nb[q - 1]; }
#pragma unroll
    for (int q = 0; q < KMAX; q++)
        if (q == fin) { nd[q] = d; nb[q] = j; }
    if (cnt < k) cnt++;
}

// Nearest target by the segment's grid (segments above kGridNNMin): the lexicographic minimum of (float
// squared distance, index) -- the brute-force scan's first strict minimum -- or j = -1 when no distance is
// below +inf (a non-finite query).  Falls back to an in-order scan of the segment.
__device__ __forceinline__ void grid_nn(const LabelGrid& G, const int32_t* cell_start, const float4* gpts,
                                        const float4* tgt, int nt, float qx, float qy, float qz, float& best, int& j) {
    best = INFINITY;
    j = -1;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) return;
    auto visit = [&](int b, int e) {
        for (int pi = b; pi < e; pi++) {
            const float4 o = gpts[pi];
            const float d = sqdist3(qx, qy, qz, o.x, o.y, o.z);
            const int oi = __float_as_int(o.w);
            if (d < best || (d == best && j >= 0 && oi < j)) { best = d; j = oi; }
        }
    };
    if (grid_shells(G, cell_start, qx, qy, qz, shell_budget(nt), visit, [&] { return best; })) return;
    best = INFINITY;
    j = -1;
    for (int i = 0; i < nt; i++) {
        const float4 o = tgt[i];
        const float d = sqdist3(qx, qy, qz, o.x, o.y, o.z);
        if (d < best) { best = d; j = i; }
    }
}

}  // namespace
}  // namespace pcore
