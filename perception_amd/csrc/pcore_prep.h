// pcore_prep.h -- host arithmetic of pcore_set_observation and pcore_upload_meshes (pcore_api.hip): the label sort, the
// neighbour grids, the GICP segment table and target quads, the vertex dedupe, the triangle colours.  Plain functions
// over std::vector, no HIP runtime call: tools/prep_check.cpp compiles them with g++ (tests/test_prep.py).  The float
// formulas are the ones the device queries repeat: neither they nor their order may change.
#pragma once
#include "pcore_internal.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

namespace pcore {
namespace prep {

// rgb2lab (compute_costs.cuh:57-88) in double with glibc pow / cbrt, stored as float.  The cost reads
// its "red" from colour plane 2 and "blue" from plane 0 (compute_costs.cuh:214-220): rgb2lab(c2, c1, c0).
inline float4 lab_of(const uint8_t c[3]) {
    const auto linear = [](double v) { return ((v > 0.04045) ? std::pow((v + 0.055) / 1.055, 2.4) : (v / 12.92)) * 100.0; };
    const auto f = [](double v) { return (v > 0.008856) ? std::cbrt(v) : (7.787 * v + 16.0 / 116.0); };
    const double r = linear(c[2] / 255.0), g = linear(c[1] / 255.0), b = linear(c[0] / 255.0);
    const double x = f((r * 0.4124564 + g * 0.3575761 + b * 0.1804375) / 95.047);
    const double y = f((r * 0.2126729 + g * 0.7151522 + b * 0.0721750) / 100.00);
    const double z = f((r * 0.0193339 + g * 0.1191920 + b * 0.9503041) / 108.883);
    const float l = (float)((116.0 * y) - 16), a = (float)(500 * (x - y)), bb = (float)(200 * (y - z));
    return make_float4(l, a, bb, 0.0f);
}

// Neighbour grid over one point set, appended to cell_start / grid_pts.  `pts` are (x,y,z, local index) in
// label-sorted order.
inline void build_grid(const std::vector<float4>& pts, float radius, LabelGrid& g, std::vector<int32_t>& cell_start,
                       std::vector<float4>& grid_pts) {
    g = LabelGrid{};
    g.pt_count = (int)pts.size();
    g.cell_base = (int)cell_start.size();
    if (pts.empty()) {
        g.ox = g.oy = g.oz = 0.0f;
        g.inv_c = 1.0f;
        g.cell = 1.0f;
        g.nx = g.ny = g.nz = 1;
        cell_start.push_back((int32_t)grid_pts.size());
        cell_start.push_back((int32_t)grid_pts.size());
        return;
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const float4& p : pts) {
        const float c[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(c[k])) continue;
            lo[k] = std::min(lo[k], c[k]);
            hi[k] = std::max(hi[k], c[k]);
        }
    }
    for (int k = 0; k < 3; k++)
        if (!(lo[k] <= hi[k])) { lo[k] = 0.0f; hi[k] = 0.0f; }
    // cell >= 2.02 r so a query's radius box touches <= 2 cells per axis (process_points writes the bound down); at
    // most 65 cells per axis: floor(ext / cell) + 1 is 65 when the extent sets the cell and the quotient reaches 64
    const float ext = std::max({hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]});
    float cell = std::max(2.0f * radius * 1.01f, ext / 64.0f);
    if (!(cell > 0.0f)) cell = 1.0f;
    g.ox = lo[0];
    g.oy = lo[1];
    g.oz = lo[2];
    g.inv_c = 1.0f / cell;
    g.cell = cell;
    g.nx = std::max(1, (int)std::floor((hi[0] - lo[0]) * g.inv_c) + 1);
    g.ny = std::max(1, (int)std::floor((hi[1] - lo[1]) * g.inv_c) + 1);
    g.nz = std::max(1, (int)std::floor((hi[2] - lo[2]) * g.inv_c) + 1);
    const int ncell = g.nx * g.ny * g.nz;
    std::vector<int> cell_of(pts.size());
    std::vector<int> cnt(ncell + 1, 0);
    for (size_t i = 0; i < pts.size(); i++) {
        // same float formula as the device query (pcore_fused.hip, process_points)
        const float fx = (pts[i].x - g.ox) * g.inv_c, fy = (pts[i].y - g.oy) * g.inv_c, fz = (pts[i].z - g.oz) * g.inv_c;
        int ix = (int)std::floor(std::max(fx, 0.0f)), iy = (int)std::floor(std::max(fy, 0.0f)),
            iz = (int)std::floor(std::max(fz, 0.0f));
        if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(fz)) {
            cell_of[i] = -1;  // non-finite points can never be within the radius of a finite query
            continue;
        }
        ix = std::min(ix, g.nx - 1);
        iy = std::min(iy, g.ny - 1);
        iz = std::min(iz, g.nz - 1);
        cell_of[i] = (iz * g.ny + iy) * g.nx + ix;
        cnt[cell_of[i] + 1]++;
    }
    for (int c = 0; c < ncell; c++) cnt[c + 1] += cnt[c];
    const int base = (int)grid_pts.size();
    grid_pts.resize(base + cnt[ncell]);
    std::vector<int> fillp(cnt.begin(), cnt.end() - 1);
    for (size_t i = 0; i < pts.size(); i++)
        if (cell_of[i] >= 0) grid_pts[base + fillp[cell_of[i]]++] = pts[i];
    for (int c = 0; c <= ncell; c++) cell_start.push_back(base + cnt[c]);
}

inline float4 point_at(const std::vector<float>& xyz, int i, int index) {
    float4 p = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.0f);
    std::memcpy(&p.w, &index, 4);
    return p;
}

// The observed cloud in label order -- a stable sort (renderer.cu:1674-1686), so a label's points keep the caller's
// order -- and the GICP target segments [lo, hi) of it: one per label, then the whole cloud
struct Sorted {
    int num_labels = 0;                // max label + 1
    std::vector<int> order;            // label-sorted position -> caller's index
    std::vector<float4> tgt;           // the points in that order (w = 0; one zero entry when there are none)
    std::vector<int32_t> lo, hi, cnt;  // num_labels + 1 segments
    int max_seg = 0;
};
inline Sorted sort_by_label(const std::vector<float>& xyz, const std::vector<int32_t>& lab) {
    const int n = (int)lab.size();
    Sorted s;
    for (int i = 0; i < n; i++) s.num_labels = std::max(s.num_labels, lab[i] + 1);
    for (int i = 0; i < n; i++) s.order.push_back(i);
    std::stable_sort(s.order.begin(), s.order.end(), [&](int a, int b) { return lab[a] < lab[b]; });
    s.tgt.resize(std::max(n, 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int k = 0; k < n; k++) s.tgt[k] = point_at(xyz, s.order[k], 0);
    s.lo.assign(s.num_labels + 1, 0);
    s.hi.assign(s.num_labels + 1, n);
    s.cnt.assign(s.num_labels + 1, n);
    s.max_seg = n;
    int pos = 0;
    for (int L = 0; L < s.num_labels; L++) {
        while (pos < n && lab[s.order[pos]] < L) pos++;
        s.lo[L] = pos;
        int e = pos;
        while (e < n && lab[s.order[e]] == L) e++;
        s.hi[L] = e;
        s.cnt[L] = e - pos;
        s.max_seg = std::max(s.max_seg, e - pos);
    }
    return s;
}

// The neighbour grids of an observation: one per label over its points (w: label-local index; 6-DoF; points with
// negative labels are never matched, no rendered label is < 0), then one over the whole label-sorted cloud (w: sorted
// position; 3-DoF)
struct Grids {
    std::vector<LabelGrid> grids;  // num_labels + 1
    std::vector<int32_t> cell_start;
    std::vector<float4> pts;
    int max_count = 0;             // points of the largest grid
};
inline Grids observation_grids(const std::vector<float>& xyz, const std::vector<int32_t>& lab, const Sorted& s,
                               float radius) {
    Grids out;
    out.grids.resize(s.num_labels + 1);
    for (int L = 0; L <= s.num_labels; L++) {
        std::vector<float4> pts;
        for (size_t k = 0; k < s.order.size(); k++)
            if (L == s.num_labels) pts.push_back(point_at(xyz, s.order[k], (int)k));
            else if (lab[s.order[k]] == L) pts.push_back(point_at(xyz, s.order[k], (int)pts.size()));
        out.max_count = std::max(out.max_count, (int)pts.size());
        build_grid(pts, radius, out.grids[L], out.cell_start, out.pts);
    }
    return out;
}

// Quad-SoA copy of every segment for the scalar-cache scan: a header quad (the segment's key origin c in [0..2]), then
// quads of four targets as correspondence keys (-2 t'x [4], -2 t'y [4], -2 t'z [4], |t'|^2 [4]; padding: 0, 0, 0,
// +inf), pcore_gicp_math.h
struct Quads {
    std::vector<float> quads;   // 16 floats each
    std::vector<int32_t> qoff;  // first quad of each segment
};
inline Quads target_quads(const Sorted& seg) {
    const std::vector<float4>& tgt = seg.tgt;
    Quads out;
    out.qoff.resize(seg.cnt.size());
    std::vector<float>& quads = out.quads;
    for (size_t L = 0; L < seg.cnt.size(); L++) {
        out.qoff[L] = (int32_t)(quads.size() / 16);
        const int n = seg.cnt[L], nq = (n + 3) / 4;
        float org[3];
        gicpm::nn_origin(n, [&](int i, float* p) {
            const float4 v = tgt[seg.lo[L] + i];
            p[0] = v.x; p[1] = v.y; p[2] = v.z;
        }, org);
        const size_t q0 = quads.size();
        quads.resize(q0 + (size_t)16 * (nq + 1), 0.0f);
        quads[q0] = org[0]; quads[q0 + 1] = org[1]; quads[q0 + 2] = org[2];
        for (int i = n; i < 4 * nq; i++) quads[q0 + 16 + (size_t)16 * (i / 4) + 12 + i % 4] = INFINITY;
        for (int i = 0; i < n; i++) {
            const float4 p = tgt[seg.lo[L] + i];
            const gicpm::NNTarget t = gicpm::nn_target(p.x, p.y, p.z, org[0], org[1], org[2]);
            float* Q = &quads[q0 + 16 + (size_t)16 * (i / 4)];
            Q[i % 4] = t.m2x;
            Q[4 + i % 4] = t.m2y;
            Q[8 + i % 4] = t.m2z;
            Q[12 + i % 4] = t.tt;
        }
    }
    return out;
}

// One model's triangles (T of them at tri_xyz, 9 floats each) over its exact-bit distinct vertices, and their box
struct ModelVerts {
    std::vector<int> tv;       // 3 vertex ids per triangle
    std::vector<float> vxyz;   // 3 floats per distinct vertex, in order of first use
    // FusedArgs::model_box (pose windows); bmin.w = 1 when every coordinate is finite
    float4 bmin = make_float4(INFINITY, INFINITY, INFINITY, 1.0f), bmax = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
};
inline ModelVerts dedupe_model(const float* tri_xyz, int T) {
    ModelVerts m;
    std::map<std::array<uint32_t, 3>, int> idx;  // a vertex's bits -> its id
    m.tv.resize((size_t)T * 3);
    std::vector<float>& vxyz = m.vxyz;
    for (size_t i = 0; i < (size_t)3 * T; i++) {
        const float* p = tri_xyz + 3 * i;
        std::array<uint32_t, 3> key;
        std::memcpy(key.data(), p, 12);
        const auto it = idx.emplace(key, (int)(vxyz.size() / 3));
        if (it.second) vxyz.insert(vxyz.end(), p, p + 3);
        m.tv[i] = it.first->second;
    }
    float4 &bmin = m.bmin, &bmax = m.bmax;
    for (size_t i = 0; i < vxyz.size(); i += 3) {
        if (!std::isfinite(vxyz[i]) || !std::isfinite(vxyz[i + 1]) || !std::isfinite(vxyz[i + 2])) bmin.w = 0.0f;
        bmin.x = std::min(bmin.x, vxyz[i]); bmax.x = std::max(bmax.x, vxyz[i]);
        bmin.y = std::min(bmin.y, vxyz[i + 1]); bmax.y = std::max(bmax.y, vxyz[i + 1]);
        bmin.z = std::min(bmin.z, vxyz[i + 2]); bmax.z = std::max(bmax.z, vxyz[i + 2]);
    }
    if (vxyz.empty()) bmin = bmax = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return m;
}

// Per triangle: its colour packed r | g << 8 | b << 16 (stage RENDER) and as Lab (the colour gate).  tri_rgb nullable:
// grey without vertex colours (model.cpp:97-101)
struct TriColours {
    std::vector<uint32_t> packed;
    std::vector<float4> lab;
};
inline TriColours tri_colours(const uint8_t* tri_rgb, int num_tris) {
    TriColours out{std::vector<uint32_t>((size_t)num_tris), std::vector<float4>((size_t)num_tris)};
    for (size_t t = 0; t < (size_t)num_tris; t++) {
        uint8_t col[3] = {128, 128, 128};
        if (tri_rgb) std::memcpy(col, tri_rgb + 3 * t, 3);
        out.packed[t] = (uint32_t)col[0] | (uint32_t)col[1] << 8 | (uint32_t)col[2] << 16;
        out.lab[t] = lab_of(col);
    }
    return out;
}

}  // namespace prep
}  // namespace pcore
