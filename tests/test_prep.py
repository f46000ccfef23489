"""The host preparation of pcore_set_observation and pcore_upload_meshes (perception_amd/csrc/pcore_prep.h), the shipped
C++ itself, on the CPU: tools/prep_check.cpp compiled with g++ against HIP's headers alone (no GPU, no HIP library).

build_grid against its float32 numpy restatement build_grid_np (tests/nn_cases.py, the independent side) on every
segment of every adversarial case and on the degenerate inputs, exactly: the origin, cell, 1 / cell, the cell counts,
each point's cell and the CSR order.  lab_of against the oracle's rgb2lab, bit for bit.  The label sort, the segment
table and the GICP quad table on segments of 0, 1, 4 and 5 points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
from perception_amd import build
from tests import nn_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("prep") / "libprepcheck.so"
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                    "-I" + rocm_include, os.path.join(ROOT, "tools", "prep_check.cpp"), "-o", str(out)], check=True)
    L = ctypes.CDLL(str(out))
    L.prep_build_grid.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 4
    L.prep_build_grid.restype = ctypes.c_int
    L.prep_lab_of.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.prep_lab_of.restype = None
    L.prep_targets.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.prep_targets.restype = ctypes.c_int
    return L


def _same_grid(lib, pts, r, what):
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
    n = len(pts)
    grid, dims = np.zeros(5, F32), np.zeros(7, np.int32)
    cell_of, rank = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    rc = lib.prep_build_grid(pts.ctypes.data, n, F32(r), grid.ctypes.data, dims.ctypes.data, cell_of.ctypes.data,
                             rank.ctypes.data)
    assert rc == 0, (what, rc)
    g = nc.build_grid_np(pts, r)
    want = np.array([g.o[0], g.o[1], g.o[2], g.cell, g.inv_c], F32)
    assert np.array_equal(grid.view(np.uint32), want.view(np.uint32)), (what, grid, want)
    assert np.array_equal(dims[:3], g.n), (what, dims, g.n)
    stored = g.cell_of >= 0
    assert dims[3] == n and dims[4] == 0 and dims[5] == int(np.prod(g.n)) + 1 and dims[6] == stored.sum(), (what, dims)
    assert np.array_equal(cell_of[:n], g.cell_of), (what, np.nonzero(cell_of[:n] != g.cell_of)[0][:8])
    # build_grid_np ranks the points that are not stored (cell -1) first
    assert np.array_equal(rank[:n], np.where(stored, g.rank - (~stored).sum(), -1)), what
    return g


@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_build_grid_equals_its_restatement_on_the_adversarial_cases(lib, name):
    """Every 6-DoF segment and the whole cloud (the 3-DoF grid) of the case, at the case's radius."""
    case = nc.nn_case(name)
    for label in list(range(case.num_labels)) + [None]:
        _same_grid(lib, case.segment(label)[0], case.r, f"{name} label {label}")


def test_the_segments_case_holds_the_degenerate_segments():
    """What the parametrised test relies on for its edge cases: an empty segment, one of one point, one of zero extent,
    segments with NaN and infinite points."""
    case = nc.nn_case("segments")
    sizes = [len(case.segment(L)[0]) for L in range(case.num_labels)]
    assert sizes[1] == 0 and sizes[3] == 1 and sizes[4] == 5 and (np.ptp(case.segment(4)[0], axis=0) == 0).all()
    assert np.isnan(case.segment(0)[0]).any() and np.isinf(case.segment(2)[0]).any()


DEGENERATE = {
    "empty": np.zeros((0, 3), F32),
    "one point": np.array([[0.5, -0.25, 1.0]], F32),
    "all non-finite": np.array([[np.nan] * 3, [np.inf, 0, 0], [0, -np.inf, np.nan]], F32),
    "one finite axis value": np.array([[np.nan, 2.0, np.nan], [np.inf, 3.0, 1.0]], F32),
    "zero extent": np.tile(np.array([[1.0, 2.0, 3.0]], F32), (7, 1)),
    "extent sets the cell": np.array([[0, 0, 0], [64, 1, 0.5], [63.99999, 0, 0], [32, 0.5, 0.25]], F32),
    "mixed": np.array([[0, 0, 0], [np.nan, 1, 1], [0.01, 0.02, 0.03], [1, np.inf, 0], [0.011, 0.02, 0.03]], F32),
}


@pytest.mark.parametrize("r", [0.0, 0.0075, 0.05])
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_build_grid_on_degenerate_inputs(lib, name, r):
    g = _same_grid(lib, DEGENERATE[name], r, f"{name} r {r}")
    if name in ("empty", "all non-finite") or (name == "zero extent" and r == 0.0):
        assert (g.n == 1).all()
    if r == 0.0 and name in ("one point", "all non-finite", "zero extent"):
        assert g.cell == 1.0  # the cell of a cloud without extent at r = 0


def test_lab_of_equals_the_oracle_bitwise(lib):
    """The 8 corners of the colour cube; 9 ... 12 either side of the sRGB switch at 0.04045 (between 10 and 11) in every
    channel, with the extremes in the others; every colour with all channels <= 40, within which X, Y and Z each cross
    the cube root / linear switch at 0.008856 -- against oracle.rgb2lab_n, the expectation tests/test_colour_spec.py
    holds pcore_debug_rgb2lab to."""
    low = np.array([0, 9, 10, 11, 12, 128, 255])
    rgb = np.concatenate([np.stack(np.meshgrid(*[[0, 255]] * 3, indexing="ij"), -1).reshape(-1, 3),
                          np.stack(np.meshgrid(low, low, low, indexing="ij"), -1).reshape(-1, 3),
                          np.stack(np.meshgrid(*[np.arange(41)] * 3, indexing="ij"), -1).reshape(-1, 3)]).astype(np.uint8)
    v = rgb[:, ::-1] / 255.0
    lin = np.where(v > 0.04045, ((v + 0.055) / 1.055) ** 2.4, v / 12.92) * 100.0
    M = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750],
                  [0.0193339, 0.1191920, 0.9503041]])
    xyz = lin @ M.T / np.array([95.047, 100.0, 108.883])
    assert ((xyz > 0.008856).sum(0) > 10).all() and ((xyz <= 0.008856).sum(0) > 10).all()
    assert all(((rgb[:, k] == 10).sum() > 10) and ((rgb[:, k] == 11).sum() > 10) for k in range(3))
    got = np.zeros((len(rgb), 3), F32)
    lib.prep_lab_of(rgb.ctypes.data, len(rgb), got.ctypes.data)
    want = oracle.rgb2lab_n(rgb)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (len(bad), rgb[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_label_sort_segments_and_quads(lib):
    """Labels 1, 2 and 3 with 1, 4 and 5 points (label 0 has none), given shuffled, one point of label 3 non-finite.  The
    order is the stable sort by label; the segment table has a segment per label and the whole cloud; a segment of n
    targets has a header quad (its key origin, the midpoint of its finite targets' box, then zeros) and ceil(n / 4) quads
    of keys -2 t', |t'|^2 with the padding (0, 0, 0, +inf).  Coordinates are multiples of 1 / 64: every product and sum
    of the keys is exact in float32, so the table is compared exactly."""
    rng = np.random.default_rng(3)
    lab = np.array([1] + [2] * 4 + [3] * 5, np.int32)
    xyz = (rng.integers(-64, 65, (10, 3)) / 64.0).astype(F32)
    xyz[7] = [np.nan, 0.5, 0.25]
    perm = rng.permutation(10)
    lab, xyz = np.ascontiguousarray(lab[perm]), np.ascontiguousarray(xyz[perm])
    order, seg, qoff = np.zeros(10, np.int32), np.zeros((8, 3), np.int32), np.zeros(8, np.int32)
    quads, meta = np.full(16 * 32, -7.0, F32), np.zeros(2, np.int32)
    nseg = lib.prep_targets(xyz.ctypes.data, lab.ctypes.data, 10, order.ctypes.data, seg.ctypes.data, qoff.ctypes.data,
                            quads.ctypes.data, len(quads), meta.ctypes.data)
    assert nseg == 5
    want_order = np.argsort(lab, kind="stable")
    assert np.array_equal(order, want_order)
    assert seg[:5].tolist() == [[0, 0, 0], [0, 1, 1], [1, 5, 4], [5, 10, 5], [0, 10, 10]] and meta[0] == 10
    tgt = xyz[want_order]
    want, want_off = [], []
    for lo, hi, n in seg[:5]:
        want_off.append(len(want) // 16)
        t = tgt[lo:hi]
        fin = np.isfinite(t).all(1)
        org = (t[fin].min(0) + t[fin].max(0)) * F32(0.5) if fin.any() else np.zeros(3, F32)
        want.extend(list(org) + [0.0] * 13)
        for q in range((n + 3) // 4):
            block = np.zeros((4, 4), F32)  # rows: -2 t'x, -2 t'y, -2 t'z, |t'|^2 of four targets
            block[3] = np.inf
            for j in range(4 * q, min(4 * q + 4, n)):
                if fin[j]:
                    d = t[j] - org
                    block[:3, j % 4] = F32(-2.0) * d
                    block[3, j % 4] = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])
            want.extend(block.ravel())
    want = np.array(want, F32)
    assert want_off == [0, 1, 3, 5, 8] and len(want) == 16 * 12
    assert np.array_equal(qoff[:5], want_off) and meta[1] == len(want)
    assert np.array_equal(quads[:len(want)].view(np.uint32), want.view(np.uint32))
    assert (quads[len(want):] == -7.0).all()
