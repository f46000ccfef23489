// The host preparation of pcore_set_observation and pcore_upload_meshes (perception_amd/csrc/pcore_prep.h) behind a C
// interface, on the CPU, for tests/test_prep.py:
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/prep_check.cpp
// No GPU and no HIP library: the header uses HIP's vector types only.  With -DPREP_CHECK_MAIN the file is a program
// that runs the degenerate inputs through every function, to be built with -fsanitize=address,undefined.
#include <cstdio>

#include "../perception_amd/csrc/pcore_prep.h"

using namespace pcore;

static std::vector<float4> local_points(const float* xyz, int n) {
    std::vector<float> v(xyz, xyz + 3 * (size_t)n);
    std::vector<float4> pts;
    for (int i = 0; i < n; i++) pts.push_back(prep::point_at(v, i, i));
    return pts;
}

extern "C" {

// build_grid over n points in local-index order.  grid: ox, oy, oz, cell, inv_c; dims: nx, ny, nz, pt_count, cell_base,
// the entries of cell_start, the points stored; cell_of[i]: the cell point i is stored in (-1: not stored); rank[i]: its
// position in the cell-sorted array.  Returns 0, or a negative number when the CSR arrays are inconsistent.
int prep_build_grid(const float* xyz, int n, float radius, float* grid, int* dims, int* cell_of, int* rank) {
    LabelGrid g;
    std::vector<int32_t> cell_start;
    std::vector<float4> gpts;
    prep::build_grid(local_points(xyz, n), radius, g, cell_start, gpts);
    grid[0] = g.ox; grid[1] = g.oy; grid[2] = g.oz; grid[3] = g.cell; grid[4] = g.inv_c;
    dims[0] = g.nx; dims[1] = g.ny; dims[2] = g.nz; dims[3] = g.pt_count; dims[4] = g.cell_base;
    dims[5] = (int)cell_start.size();
    dims[6] = (int)gpts.size();
    const int ncell = g.nx * g.ny * g.nz;
    if ((int)cell_start.size() != ncell + 1 || cell_start[0] != 0 || cell_start[ncell] != (int)gpts.size()) return -1;
    for (int i = 0; i < n; i++) cell_of[i] = rank[i] = -1;
    for (int c = 0; c < ncell; c++) {
        if (cell_start[c] > cell_start[c + 1]) return -2;
        for (int j = cell_start[c]; j < cell_start[c + 1]; j++) {
            int i;
            std::memcpy(&i, &gpts[j].w, 4);
            if (i < 0 || i >= n || cell_of[i] != -1) return -3;
            if (std::memcmp(&gpts[j].x, xyz + 3 * (size_t)i, 12) != 0) return -4;
            cell_of[i] = c;
            rank[i] = j;
        }
    }
    return 0;
}

void prep_lab_of(const uint8_t* rgb, int n, float* out) {
    for (int i = 0; i < n; i++) {
        const float4 v = prep::lab_of(rgb + 3 * (size_t)i);
        out[3 * (size_t)i] = v.x; out[3 * (size_t)i + 1] = v.y; out[3 * (size_t)i + 2] = v.z;
    }
}

// The label sort, the segment table and the quad table of n observed points.  order: n entries; seg: lo, hi, cnt of
// segment s at seg[3 s ...]; qoff: a quad offset per segment; quads: up to quads_cap floats.  Returns the number of
// segments (labels + 1); meta: max_seg, the floats of the quad table (which may exceed quads_cap: nothing is copied then).
int prep_targets(const float* xyz, const int32_t* lab, int n, int* order, int* seg, int* qoff, float* quads, int quads_cap,
                 int* meta) {
    const std::vector<float> v(xyz, xyz + 3 * (size_t)n);
    const std::vector<int32_t> l(lab, lab + n);
    const prep::Sorted s = prep::sort_by_label(v, l);
    const prep::Quads q = prep::target_quads(s);
    for (int i = 0; i < n; i++) order[i] = s.order[i];
    for (int k = 0; k <= s.num_labels; k++) {
        seg[3 * k] = s.lo[k]; seg[3 * k + 1] = s.hi[k]; seg[3 * k + 2] = s.cnt[k];
        qoff[k] = q.qoff[k];
    }
    meta[0] = s.max_seg;
    meta[1] = (int)q.quads.size();
    if ((int)q.quads.size() <= quads_cap) std::copy(q.quads.begin(), q.quads.end(), quads);
    return s.num_labels + 1;
}

}  // extern "C"

#ifdef PREP_CHECK_MAIN
// The degenerate inputs of tests/test_prep.py through every function of the header, for a sanitizer build.
int main() {
    const float inf = INFINITY, nan = NAN;
    const std::vector<std::vector<float>> clouds = {
        {},                                                     // no point
        {0.5f, -0.25f, 1.0f},                                   // one point
        {nan, nan, nan, inf, 0.0f, 0.0f, 0.0f, -inf, nan},      // all points non-finite
        {1.0f, 2.0f, 3.0f, 1.0f, 2.0f, 3.0f, 1.0f, 2.0f, 3.0f}, // zero extent
        {0.0f, 0.0f, 0.0f, 64.0f, 0.0f, 0.0f, nan, 1.0f, 1.0f, 1.0e30f, -1.0e30f, 0.0f, 1e-30f, 5.0f, -7.0f},
    };
    long checks = 0;
    for (const auto& xyz : clouds)
        for (float r : {0.0f, 0.0075f, 1.0e30f}) {
            const int n = (int)xyz.size() / 3;
            float grid[5];
            int dims[7];
            std::vector<int> cell_of(n + 1), rank(n + 1);
            if (prep_build_grid(xyz.data(), n, r, grid, dims, cell_of.data(), rank.data()) != 0) {
                std::printf("build_grid: inconsistent CSR arrays (n = %d, r = %g)\n", n, r);
                return 1;
            }
            // labels -1 .. 3 in turn: an absent label, segments of every small size, the quads' padding
            std::vector<int32_t> lab(n);
            for (int i = 0; i < n; i++) lab[i] = (i * 7) % 5 - 1;
            std::vector<int> order(n + 1), seg(3 * 8), qoff(8), meta(2);
            std::vector<float> quads(16 * 32);
            const int nseg = prep_targets(xyz.data(), lab.data(), n, order.data(), seg.data(), qoff.data(), quads.data(),
                                          (int)quads.size(), meta.data());
            if (nseg < 1 || seg[3 * (nseg - 1) + 2] != n) {
                std::printf("segment table: the whole-cloud segment has %d of %d points\n", seg[3 * (nseg - 1) + 2], n);
                return 1;
            }
            const prep::Sorted s = prep::sort_by_label(xyz, lab);
            const prep::Grids grids = prep::observation_grids(xyz, lab, s, r);
            checks += (long)grids.grids.size() + nseg;
        }
    const std::vector<float> tris = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, nan, inf, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int T : {0, 1, 3}) {
        const prep::ModelVerts m = prep::dedupe_model(tris.data(), T);
        if (m.tv.size() != 3 * (size_t)T || (T == 3 && m.vxyz.size() != 3 * 4)) {
            std::printf("dedupe_model: %zu vertices for %d triangles\n", m.vxyz.size() / 3, T);
            return 1;
        }
    }
    const uint8_t rgb[9] = {0, 0, 0, 255, 255, 255, 10, 11, 40};
    float lab3[9];
    prep_lab_of(rgb, 3, lab3);
    const prep::TriColours grey = prep::tri_colours(nullptr, 2), col = prep::tri_colours(rgb, 3);
    if (grey.packed[1] != 0x808080u || col.packed[1] != 0xffffffu || col.lab[1].x != lab3[3]) {
        std::printf("tri_colours: packed %x %x\n", grey.packed[1], col.packed[1]);
        return 1;
    }
    std::printf("prep_check: ok (%ld grids and segments)\n", checks);
    return 0;
}
#endif
