"""The fragment test of a fastdiv pose computes its barycentrics without the reference's three multiplications by 0.5
(pcore_fdiv.h, frag_barycentrics<true>); every other path keeps the reference form.  Both must give the reference's bits.

1. tools/bary_check.hip (built by __graft_entry__.build()) compares the two forms on the GPU over 5e8 random
   (triangle, sample) pairs inside the bound pcore_fdiv.h documents -- coordinates that are multiples of 2^-25 below
   2^56 -- zero areas, collinear vertices, slivers a few 2^-25 across and samples on vertices and edges among them.
2. A hand-made mesh of 50 triangles on a 64 x 64 camera whose fastdiv pose puts every vertex on an exactly
   representable screen position: edges through sample centres, zero-area and collinear triangles, triangles 2^-11
   pixel across that hold a sample centre inside, on an edge and on a vertex, small triangles (the record flush) and
   large ones (the cooperative path) at three depths.  It is rendered at that pose and a rotated one (fastdiv), and at
   two poses with the camera plane inside the model's box (not fastdiv: the reference form, vertices at z = 0 and
   behind the camera); the z-samples at strides 8 and 1 equal the CPU oracle's."""
import json
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import synthetic as syn
from perception_amd.core import PoseCore
from perception_amd.model import init_from_eigen_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_barycentrics_without_halves_match_the_reference_form():
    exe = os.path.join(ROOT, "tools", "bin", "bary_check")
    if not os.path.exists(exe):
        pytest.fail("tools/bin/bary_check missing: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and res["mismatches"] == 0, r.stdout + r.stderr
    assert res["pairs"] >= 5e8
    # the draw holds zero areas (infinite / NaN barycentrics, which count as inside) and ordinary inside samples
    assert res["zero_area"] > 10**6 and res["nan"] > 10**5 and res["inside"] > res["nan"]


# ---------------------------------------------------------------------------------------------
# the hand-made mesh
# ---------------------------------------------------------------------------------------------

W = H = 64
CAM = dict(width=W, height=H, fx=32.0, fy=32.0, cx=32.0, cy=32.0)  # proj rows (1, 0, 0, 0), (0, -1, 0, 0)
TZ = 0.5  # the exact pose: identity rotation, 0.5 m in front of the camera
E = 2.0 ** -11  # 4.9e-4 pixel


def _vertex(sx, sy, lz):
    """The model point that the exact pose puts at screen (sx, sy) with camera z lz cm (25, 50 or 100): with
    z_cam = 100 (z + TZ) and screen x = 100 x / z_cam * 32 + 32 every step is exact in f32 (lz / 3200 is a power of
    two), likewise y."""
    assert lz in (25.0, 50.0, 100.0)
    return ((sx - 32.0) * lz / 3200.0, (32.0 - sy) * lz / 3200.0, lz / 100.0 - TZ)


def _mesh():
    # screen-space triangles ((sx, sy) x 3, lz); stride-8 sample centres are (8 i, 63 - 8 j)
    t = [
        (((8, 47), (40, 47), (8, 15)), 50.0),      # large: edges on a sample row, a sample column and a diagonal of centres
        (((16, 55), (16, 23), (48, 55)), 100.0),   # the same shape behind it, other winding
        (((30, 60), (62, 60), (62, 20)), 25.0),    # large, in front, overlapping both
        (((20, 20), (20, 20), (30, 30)), 50.0),    # zero area: two vertices coincide
        (((24, 31), (24, 31), (24, 31)), 25.0),    # a point on a sample centre
        (((8, 31), (24, 31), (40, 31)), 25.0),     # collinear along a sample row
        (((8, 63), (16, 55), (24, 47)), 25.0),     # collinear along a diagonal of centres
        (((32 - E, 39 - E), (32 + E, 39 - E), (32, 39 + E)), 25.0),  # 2^-11 pixel across, the centre inside
        (((40 - E, 39), (40 + E, 39), (40, 39 + E)), 25.0),          # the centre on an edge
        (((48, 39), (48 + E, 39), (48, 39 + E)), 25.0),              # the centre on a vertex
        (((56 + E, 39 + E), (56 + 2 * E, 39 + E), (56 + E, 39 + 2 * E)), 25.0),  # the centre just outside
        (((0, 10), (63, 10 + E), (63, 10 - E)), 50.0),               # a sliver across the image between sample rows
        (((0, 15), (63, 15 + E), (63, 15 - E)), 50.0),               # a sliver along a sample row
        (((14, 45), (18, 45), (16, 49)), 25.0),    # small: one sample (the record flush)
        (((14, 13), (26, 13), (14, 25)), 100.0),   # small: up to four samples, one on its hypotenuse
        (((40, 7), (48, 7), (40, 15)), 100.0),     # small: three centres on its vertices
    ]
    rng = np.random.default_rng(5)
    for _ in range(34):  # small and medium triangles on a quarter-pixel grid, at the three depths
        c = rng.integers(0, 64 * 4, 2) / 4.0
        d = rng.integers(-40, 41, (3, 2)) / 4.0
        t.append((tuple((float(c[0] + d[k, 0]), float(c[1] + d[k, 1])) for k in range(3)),
                  float(rng.choice([25.0, 50.0, 100.0]))))
    assert len(t) <= 64
    tris = np.array([[_vertex(sx, sy, lz) for (sx, sy) in v] for v, lz in t], np.float32).reshape(-1, 9)
    return tris


def _poses():
    rot = syn._rot_align_z(np.array([0.2, -0.1, 1.0])) @ syn._rot_z(0.3)
    out = []
    for R, tz in ((np.eye(3), TZ), (rot, 0.6), (np.eye(3), 0.0), (rot, 0.1)):
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = (0.0, 0.0, tz)
        out.append(T)
    return np.stack(out)


@pytest.fixture(scope="module")
def scene():
    tris = _mesh()
    cnt = np.array([len(tris)], np.int32)
    poses44 = _poses()
    poses = init_from_eigen_batch(poses44)
    pm = np.zeros(len(poses), np.int32)
    proj = oracle.compute_proj(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], W, H)
    src = np.zeros((H, W), np.int32)
    ref = oracle.render_depth(tris, cnt, poses, pm, None, W, H, proj, src, None, 1.0)
    dev = torch.device("cuda", 0)
    core = PoseCore(0)
    core.upload_meshes(tris, cnt)
    core.set_camera(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], proj)
    obs = torch.tensor([[0.0, 0.0, 0.5], [0.01, 0.0, 0.5], [0.0, 0.02, 0.6]], dtype=torch.float32, device=dev)
    core.set_observation(torch.from_numpy(src).to(dev), None, obs, None, 0.01)
    t = {"poses": torch.from_numpy(poses).to(dev), "pm": torch.from_numpy(pm).to(dev),
         "tot": torch.full((len(poses),), 3.0, dtype=torch.float32, device=dev)}
    yield tris, poses44, ref, core, t
    core.close()


def test_mesh_and_poses_are_what_the_docstring_says(scene):
    tris, poses44, ref, _, _ = scene
    v = tris.reshape(-1, 3).astype(np.float64)
    lz = [100.0 * (v @ T[:3, :3].T + T[:3, 3])[:, 2] for T in poses44]
    # pose_window's fastdiv bound: every vertex at least 1 cm (plus a margin of 1e-5 of the box's extent) in front
    assert lz[0].min() == 25.0 and lz[1].min() > 20.0
    assert lz[2].min() < 0.0 < lz[2].max() and (lz[2] == 0.0).any() and lz[3].min() < 0.0 < lz[3].max()
    # the exact pose: the first large triangle's vertices land on their pixels, so its hypotenuse holds sample centres
    # and the fragments there (barycentric exactly 0) are inside
    assert ref[0, H - 1 - 39, 16] == 50 and ref[0, H - 1 - 47, 8] == 50 and ref[0, H - 1 - 47, 40] == 50
    assert ref[0, H - 1 - 39, 32] == 25 and ref[0, H - 1 - 39, 40] == 25 and ref[0, H - 1 - 39, 48] == 25  # the tiny ones
    for k in range(4):
        assert (ref[k] != 0).sum() > 50, k  # behind the camera the reference renders negative depths


@pytest.mark.parametrize("stride", [8, 1])
def test_z_samples_equal_the_oracle(scene, stride):
    tris, poses44, ref, core, t = scene
    s = stride
    dbg = torch.full((len(poses44), H // s, W // s), -7, dtype=torch.int32, device=t["poses"].device)
    core.evaluate(t["poses"], t["pm"], None, t["tot"], cost_type=0, stride=s, dbg_zs=dbg)
    torch.cuda.synchronize()
    zs = dbg.cpu().numpy()
    want = ref[:, ::s, ::s]
    mism = np.argwhere(zs != want)
    assert len(mism) == 0, f"{len(mism)} mismatching (pose, ky, kx), first {mism[:6].tolist()}"
    assert (want[0] != 0).any() and (want[2] != 0).any()


def test_full_render_equals_the_oracle(scene):
    tris, poses44, ref, core, t = scene
    full = core.render(t["poses"], t["pm"], None).cpu().numpy()
    assert np.array_equal(full, ref)
