"""CPU certificates of tests/interior_cases.py: the GPU tests of tests/test_gpu_interior_pose.py could fail.  On a
float32 restatement of pose_window's box and of the vertex pass (no GPU) this module asserts that the poses take the
raster's three copies -- interior (2), fastdiv (1), general (0) -- in that order as the sheet moves outward across each
of the four borders, that poses exist whose margin alone straddles a border, that vertices land exactly on the border
pixels 0, W-1 and H-1 and one float step beyond them, and that the mesh holds the triangles the fragment test's area
reciprocal has to get right: sub-pixel ones, vertices on sample centres, zero areas with X = 0 and with X != 0."""
import numpy as np

from tests import interior_cases as ic

W, H = ic.CAM["width"], ic.CAM["height"]


def _classes():
    poses, kinds = ic.poses()
    return np.array([ic.pose_class(m, ic.mesh()) for m in poses]), kinds


def test_the_cases_are_the_ones_described():
    case = ic.case()
    assert (case.width, case.height) == (72, 48) and set(ic.STRIDES) == {8, 3}
    assert all(case.width % s == 0 for s in ic.STRIDES)  # evaluate requires it
    assert len(ic.mesh()) <= 300 and np.isfinite(ic.mesh()).all()
    assert case.n == 6 * 4 + 2 and not case.src_depth.any()
    v = ic.mesh().reshape(-1, 3)
    assert np.array_equal(v.min(0), np.array([0, 0, -ic.Z_AMP], np.float32))
    assert np.array_equal(v.max(0), np.array(ic.SHEET + (ic.Z_AMP,), np.float32))


def test_every_class_occurs_and_every_border_flips_it():
    cls, kinds = _classes()
    for c, (border, kind) in zip(cls, kinds):
        assert c == ic.EXPECTED_CLASS[kind], (border, kind, c)
    assert all((cls == c).sum() >= 2 for c in (0, 1, 2))
    for border in ic.BORDERS:
        seq = [int(c) for c, (b, _) in zip(cls, kinds) if b == border]
        # moving outward: interior, then fastdiv only, then general
        assert seq == sorted(seq, reverse=True) and set(seq) == {0, 1, 2}, (border, seq)


def test_margin_poses_straddle_with_the_margin_alone():
    """The vertices (and the box's corners) lie inside the image, more than half a pixel from the border; the box
    widened by pose_window's margin does not: only the margin keeps the pose out of the interior class."""
    poses, kinds = ic.poses()
    v = ic.mesh().reshape(-1, 3)
    for m, (border, kind) in zip(poses, kinds):
        if kind != "margin":
            continue
        sx, sy, _ = ic.vertex_pass(m, v)
        xlo, xhi, ylo, yhi, sx0, sx1, sy0, sy1, fastdiv = ic.pose_box(m, ic.mesh())
        assert fastdiv
        assert 0.5 < min(sx.min(), sx0) and max(sx.max(), sx1) < W - 1.5
        assert 0.5 < min(sy.min(), sy0) and max(sy.max(), sy1) < H - 1.5
        out = dict(left=xlo < 0, right=xhi > W - 1, bottom=ylo < 0, top=yhi > H - 1)
        assert out[border] and sum(out.values()) == 1, (border, out)


def test_interior_poses_keep_every_vertex_inside_the_image():
    """What the interior class relies on: the computed screen coordinates of every vertex lie in [0, W-1] x [0, H-1]
    (here with the margin's two pixels to spare)."""
    poses, kinds = ic.poses()
    v = ic.mesh().reshape(-1, 3)
    for m, (_, kind) in zip(poses, kinds):
        if ic.EXPECTED_CLASS[kind] == 2:
            sx, sy, lz = ic.vertex_pass(m, v)
            assert 2 <= sx.min() and sx.max() <= W - 3 and 2 <= sy.min() and sy.max() <= H - 3 and lz.min() >= 1


def test_vertices_land_on_the_border_pixels_and_a_step_beyond():
    poses, kinds = ic.poses()
    v = ic.mesh().reshape(-1, 3)
    seen = set()
    for m, (border, kind) in zip(poses, kinds):
        if kind not in ("exact", "beyond"):
            continue
        sx, sy, _ = ic.vertex_pass(m, v)
        c = dict(left=sx.min(), right=sx.max(), bottom=sy.min(), top=sy.max())[border]
        tgt = np.float32(dict(left=0, right=W - 1, bottom=0, top=H - 1)[border])
        if kind == "exact":
            assert c == tgt, (border, c)
        else:
            out = c < tgt if border in ("left", "bottom") else c > tgt
            assert out and abs(float(c) - float(tgt)) < 1e-4, (border, c)
        seen.add((border, kind))
    assert len(seen) == 8


def test_the_mesh_holds_the_hard_triangles():
    """At an interior pose, from the vertex pass's float32 screen coordinates: triangles less than a pixel across,
    triangles with a vertex within 1e-3 pixels of a whole pixel, zero areas Y = 0 whose vertices all coincide (X = 0 at
    every sample) and zero areas with two distinct vertices (X != 0 at a sample of their bounding box)."""
    poses, kinds = ic.poses()
    m = poses[kinds.index(("left", "inside"))]
    t = ic.mesh().reshape(-1, 3)
    sx, sy, _ = ic.vertex_pass(m, t)
    A0, B0, C0 = sx.reshape(-1, 3).T
    A1, B1, C1 = sy.reshape(-1, 3).T
    Y = (C0 - A0) * (B1 - A1) - (B0 - A0) * (C1 - A1)
    ext = np.maximum(np.ptp(sx.reshape(-1, 3), axis=1), np.ptp(sy.reshape(-1, 3), axis=1))
    point = (A0 == B0) & (A0 == C0) & (A1 == B1) & (A1 == C1)
    assert ((ext < 1.0) & (Y != 0)).sum() >= 50
    on_pixel = (np.abs(sx - np.round(sx)) < 1e-3) & (np.abs(sy - np.round(sy)) < 1e-3)
    assert on_pixel.reshape(-1, 3).any(1).sum() >= 20
    assert (Y == 0).sum() >= 30 and point.sum() >= 10
    line = (Y == 0) & ~point
    assert line.sum() >= 20
    # X of beta at the sample (P0, P1) = (ceil of the box's corner): non-zero for the line triangles
    P0, P1 = np.ceil(np.minimum(np.minimum(A0, B0), C0)), np.ceil(np.minimum(np.minimum(A1, B1), C1))
    Xb = (C0 - A0) * (P1 - A1) - (P0 - A0) * (C1 - A1)
    Xg = (P0 - A0) * (B1 - A1) - (B0 - A0) * (P1 - A1)
    assert (((Xb != 0) | (Xg != 0)) & line).sum() >= 20
    assert ((Xb == 0) & (Xg == 0) & point).sum() == point.sum()


def test_every_pose_renders():
    """The oracle's render of every pose holds fragments, at both strides' sample grids for the poses that are not
    mostly off screen."""
    case = ic.case()
    z = case.z_full
    assert (z.reshape(case.n, -1) > 0).any(1).all()
    for s in ic.STRIDES:
        zs = case.zs(s)
        inside = [i for i, (_, k) in enumerate(case.kinds) if ic.EXPECTED_CLASS[k] == 2]
        assert all((zs[i] > 0).sum() >= 3 for i in inside), s
