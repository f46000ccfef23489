"""GPU: the recognizer's per-state work on the device (pcore_state_poses, pcore_count_within) against the host
restatements it replaces -- bit for bit.

  pcore_state_poses   vs ObjectRecognizer._pose_in_cam's arithmetic (model.quat_xyzw_to_matrix_batch,
                      pose_matrix_batch, chain_matmul_batch, init_from_eigen_batch): GetStateImagesUnifiedGPU's
                      pose building (search_env.cpp:1535-1576);
  pcore_count_within  vs a numpy float32 loop of PCL's radiusSearch count (IsValidPose, search_env.cpp:359-396),
                      the restatement tests/test_valid_pose.py pins on the CPU.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from perception_amd import synthetic as syn
from perception_amd.core import PoseCore
from perception_amd.model import chain_matmul_batch, compute_proj, init_from_eigen_batch, pose_matrix_batch
from tests import nn_cases as nc
from tests.test_valid_pose import _pcl_counts

gpu = pytest.mark.gpu  # per test: the certificate of the count_within edge cases at the end runs without a device
DEV = torch.device("cuda", 0)
F32 = np.float32


def _core():
    cam = syn.CAM_640
    core = PoseCore(0)
    core.set_camera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                    compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"]))
    return core


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@gpu
def test_state_poses_bit_exact_vs_host_chain():
    rng = np.random.default_rng(11)
    n, K = 20000, 5
    states = np.empty((n, 7))
    states[:, :3] = rng.normal(scale=0.4, size=(n, 3)) + np.array([0.0, 0.0, 0.9])
    states[:, 3:] = rng.normal(size=(n, 4)) * rng.uniform(0.2, 3.0, size=(n, 1))  # not normalised
    states[:7, 3:] = [[0, 0, 0, 1], [1, 0, 0, 0], [0, 0, 0, -1], [0.5, 0.5, 0.5, 0.5], [0, 0, 1e-8, 1],
                      [0, 0, 0, 1e-30], [-0.0, 0.0, -0.0, 1.0]]
    model = rng.integers(0, K, n).astype(np.int32)
    pre = np.stack([np.eye(4) for _ in range(K)])
    for k in range(K):
        pre[k, :3, 3] = rng.normal(scale=0.05, size=3)
        pre[k, 2, 2] = -1.0 if k == 3 else 1.0
        pre[k] = pre[k].astype(np.float32).astype(np.float64)
    cam_pose = np.eye(4)
    cam_pose[:3, :3] = pose_matrix_batch(np.zeros((1, 3)), rng.normal(size=(1, 4)))[0, :3, :3]
    cam_pose[:3, 3] = rng.normal(size=3)
    cam_matrix = np.linalg.inv(cam_pose)
    want = init_from_eigen_batch(chain_matmul_batch(cam_matrix, pose_matrix_batch(states[:, :3], states[:, 3:7]),
                                                    pre[model]), 100)
    core = _core()
    got = core.state_poses(torch.from_numpy(states).to(DEV), torch.from_numpy(model).to(DEV), cam_matrix,
                           torch.from_numpy(pre.reshape(K, 16)).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    # empty batch
    out = core.state_poses(torch.zeros((0, 7), dtype=torch.float64, device=DEV),
                           torch.zeros(0, dtype=torch.int32, device=DEV), cam_matrix,
                           torch.from_numpy(pre.reshape(K, 16)).to(DEV))
    assert out.shape == (0, 16)


@gpu
def test_count_within_matches_pcl_restatement():
    rng = np.random.default_rng(12)
    cam = syn.CAM_640
    core = _core()
    # an observation with three labelled segments (plus unlabelled points), as set_observation takes it
    pts, labs = [], []
    for L, c in enumerate([(-0.1, 0.0, 0.8), (0.05, 0.02, 0.9), (0.15, -0.05, 0.7)]):
        m = 80 + 60 * L
        pts.append(np.asarray(c) + rng.normal(scale=0.03, size=(m, 3)))
        labs.append(np.full(m, L, np.int32))
    pts.append(rng.normal(scale=0.2, size=(50, 3)) + np.array([0, 0, 1.0]))
    labs.append(np.full(50, -1, np.int32))
    xyz = np.concatenate(pts).astype(np.float32)
    lab = np.concatenate(labs)
    perm = rng.permutation(len(xyz))
    xyz, lab = xyz[perm], lab[perm]
    H, W = cam["height"], cam["width"]
    mask = np.zeros((H, W), np.uint8)
    mask[0, :3] = [1, 2, 3]  # labels 0..2 present in the mask
    core.set_observation(torch.zeros((H, W), dtype=torch.int32, device=DEV), torch.from_numpy(mask).to(DEV),
                         torch.from_numpy(xyz).to(DEV), torch.from_numpy(lab).to(DEV), 0.01)
    n = 3000
    ql = rng.integers(-1, 5, n).astype(np.int32)  # labels outside the segments count 0
    centres = np.array([(-0.1, 0.0, 0.8), (0.05, 0.02, 0.9), (0.15, -0.05, 0.7), (0, 0, 1), (0, 0, 1), (0, 0, 1)])
    q = centres[np.clip(ql, 0, 5)] + rng.normal(scale=0.05, size=(n, 3))
    radius = rng.choice([0.02, 0.0566, 0.11], n)
    r2 = (radius * radius).astype(np.float32)
    got = core.count_within(torch.from_numpy(q.astype(np.float32)).to(DEV), torch.from_numpy(ql).to(DEV),
                            torch.from_numpy(r2).to(DEV)).cpu().numpy()
    want = np.zeros(n, np.int64)
    for L in range(3):
        seg = xyz[lab == L]
        for r in np.unique(radius):
            sel = (ql == L) & (radius == r)
            if sel.any():
                want[sel] = _pcl_counts(q[sel], seg, r)
    assert np.array_equal(got, want)
    assert got[(ql < 0) | (ql > 2)].sum() == 0


# ---------------------------------------------------------------------------------------------
# count_within's float semantics: ((0 + dx^2) + dy^2) + dz^2 < r^2, float32, no contraction
# ---------------------------------------------------------------------------------------------

EDGE_BATCHES = (0, 1, 255, 256, 257)
EDGE_RADII = (0.02, 0.0566, 0.11)
TINY_R2 = np.nextafter(F32(0.0), F32(1.0))  # the smallest positive float32


def _diffs(q, p):
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(np.asarray(q, F32)[..., a] - np.asarray(p, F32)[..., a] for a in range(3))


def _d2(q, p, mode="spec"):
    """The squared distance of float32 points under the documented arithmetic and under the ones it must not be:
    spec   float32, ((0 + dx dx) + dy dy) + dz dz, every operation rounded;
    fma    float32 with the multiply-adds contracted: fma(dz, dz, fma(dy, dy, dx dx));
    f64    the float32 differences squared and summed in float64."""
    dx, dy, dz = _diffs(q, p)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "spec":
            return (F32(0.0) + dx * dx + dy * dy) + dz * dz
        x, y, z = (v.astype(np.float64) for v in (dx, dy, dz))
        if mode == "f64":
            return (x * x + y * y) + z * z
        assert mode == "fma"  # a float32 product is exact in float64; one rounding per fused operation
        acc = (dx * dx).astype(np.float64)
        acc = (y * y + acc).astype(F32).astype(np.float64)
        return (z * z + acc).astype(F32)


def _radius_of(r2):
    """A radius whose float32 square, as _pcl_counts forms it, is exactly r2."""
    r = float(np.sqrt(np.float64(r2)))
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.isnan(r2) or F32(r * r) == F32(r2), r2
    return r


def count_within_edge_case():
    """-> (observed xyz, labels, queries, query labels, r2 per query, a note per query).  Segments: 0 the boundary
    points, 1 the rounding pairs, 2 empty, 3 one point, 4 finite and non-finite points."""
    rng = np.random.default_rng(31)
    pts, labs, Q, QL, R2, note = [], [], [], [], [], []

    def query(q, label, r2, what):
        Q.append(np.asarray(q, F32))
        QL.append(label)
        R2.append(F32(r2))
        note.append(what)

    # 0: for each query and radius, points whose float32 d^2 is r^2, the float above it and the float below it,
    # along one axis or two
    for i in range(24):
        r = EDGE_RADII[i % 3]
        r2 = F32(r * r)
        q = (np.array([-0.1, 0.0, 0.8]) + rng.normal(scale=0.4, size=3)).astype(F32)
        found = {}
        for cls, target in (("eq", r2), ("above", np.nextafter(r2, F32(np.inf))), ("below", np.nextafter(r2, F32(0)))):
            for two in (False, True):
                o = nc.edge_point(q, r, target, i % 3, (i + 1 + i // 3 % 2) % 3, 1 if i % 2 else -1, two_axes=two)
                if o is not None:
                    found[cls] = o
                    break
        if len(found) == 3:
            for cls, o in found.items():
                pts.append(o)
                labs.append(0)
            query(q, 0, r2, "boundary")
    # 1: pairs whose float32 sum and whose fused / float64 sum differ; r^2 is put between them
    n = 20000
    q = (np.array([0.05, 0.02, 0.9]) + rng.normal(scale=0.3, size=(n, 3))).astype(F32)
    off = rng.normal(size=(n, 3))
    off *= (rng.choice(EDGE_RADII, n) / np.linalg.norm(off, axis=1))[:, None]
    p = (q + off.astype(F32)).astype(F32)
    s, f, d = _d2(q, p), _d2(q, p, "fma"), _d2(q, p, "f64")
    up = np.nextafter(s, F32(np.inf))
    kinds = (("fma above", f > s, np.maximum(f, s)), ("fma below", f < s, s),
             ("f64 below", d < s.astype(np.float64), s), ("f64 above", d >= up.astype(np.float64), up))
    for what, sel, r2 in kinds:
        idx = np.nonzero(sel)[0][:12]
        assert len(idx) == 12, what
        for j in idx:
            pts.append(p[j])
            labs.append(1)
            query(q[j], 1, r2[j], what)
    # 3: one point; the query on it with r^2 = 0 (nothing is strictly within) and the smallest positive r^2
    one = np.array([0.3, -0.2, 1.1], F32)
    pts.append(one)
    labs.append(3)
    for r2 in (F32(0.0), TINY_R2, F32(1e-4)):
        query(one, 3, r2, "on the point")
    query(one + F32(0.01), 3, F32(1e-4), "beside the point")
    query(one, 2, F32(1.0), "empty segment")  # 2: no point has this label
    query(pts[0], 0, F32(0.0), "on a point, r2 = 0")
    query(pts[0], 0, TINY_R2, "on a point, the smallest r2")
    # 4: finite and non-finite points; finite and non-finite queries
    base = np.array([-0.4, 0.3, 0.7], F32)
    fin = (base + rng.normal(scale=0.02, size=(12, 3))).astype(F32)
    bad = np.repeat(base[None], 9, axis=0)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            bad[3 * k + a, a] = v
    mix = np.concatenate([fin, bad])[rng.permutation(21)]
    pts.extend(mix)
    labs.extend([4] * len(mix))
    query(base, 4, F32(0.01), "finite query, non-finite points")
    query(base, 4, F32(np.inf), "r2 = inf")
    for v in (np.nan, np.inf, -np.inf):
        for a in range(3):
            bq = base.copy()
            bq[a] = v
            query(bq, 4, F32(0.01), "non-finite query")
            query(bq, 4, F32(np.inf), "non-finite query, r2 = inf")
    query(np.full(3, np.nan, F32), 0, F32(1.0), "NaN query")
    # the rest: ordinary queries on every label, in range and out of it, up to the largest batch
    while len(Q) < max(EDGE_BATCHES):
        L = int(rng.integers(-1, 7))
        c = (np.array([-0.1, 0.0, 0.8]), np.array([0.05, 0.02, 0.9]), one, one, base)[L % 5]
        r = rng.choice(EDGE_RADII)
        query(c + rng.normal(scale=0.05, size=3), L, F32(r * r), "ordinary")
    order = rng.permutation(len(Q))  # the edge cases spread over the batches and the 256-thread blocks
    order = np.concatenate([order[np.array(note)[order] == "boundary"][:1], order])  # the batch of 1: a boundary query
    _, first = np.unique(order, return_index=True)
    order = order[np.sort(first)]
    pts, labs = np.stack(pts).astype(F32), np.array(labs, np.int32)
    perm = rng.permutation(len(pts))
    return (pts[perm], labs[perm], np.stack(Q)[order], np.array(QL, np.int32)[order], np.array(R2, F32)[order],
            np.array(note)[order])


def _edge_counts(case, mode="pcl"):
    """Expected counts: _pcl_counts per query (mode "pcl"), or this file's restatement with the strict float32 test
    ("spec"), an inclusive one ("le"), or a fused / float64 distance ("fma", "f64")."""
    xyz, lab, q, ql, r2, _ = case
    out = np.zeros(len(q), np.int64)
    for i in range(len(q)):
        if not 0 <= ql[i] <= lab.max():
            continue
        seg = xyz[lab == ql[i]]
        if len(seg) == 0:
            continue
        if mode == "pcl":
            out[i] = _pcl_counts(q[i][None], seg, _radius_of(r2[i]))[0]
            continue
        d = _d2(q[i][None], seg, "spec" if mode == "le" else mode)
        lim = np.float64(r2[i]) if mode == "f64" else r2[i]
        with np.errstate(invalid="ignore"):
            out[i] = int((d <= lim).sum() if mode == "le" else (d < lim).sum())
    return out


def test_count_within_edge_cases_can_tell_the_arithmetic():
    """No device: the hand-made case holds what it is meant to, and the expected counts (from _pcl_counts) change under
    an inclusive test, under a float64 distance and under an FMA-contracted one."""
    case = count_within_edge_case()
    xyz, lab, q, ql, r2, note = case
    want = _edge_counts(case)
    assert np.array_equal(want, _edge_counts(case, "spec"))
    assert len(q) == max(EDGE_BATCHES) and note[0] == "boundary"
    assert set(np.unique(lab)) == {0, 1, 3, 4} and (lab == 3).sum() == 1
    b = np.nonzero(note == "boundary")[0]
    assert len(b) >= 12
    for i in b:  # one point on r^2 (not counted), one on the float above, one on the float below (counted)
        d = _d2(q[i][None], xyz[lab == 0])
        assert (d == r2[i]).sum() >= 1 and (d == np.nextafter(r2[i], F32(np.inf))).sum() >= 1
        assert (d == np.nextafter(r2[i], F32(0))).sum() >= 1 and want[i] >= 1
    on = np.nonzero(note == "on the point")[0]
    assert sorted(zip(r2[on].tolist(), want[on].tolist())) == sorted([(0.0, 0), (float(TINY_R2), 1), (float(F32(1e-4)), 1)])
    assert want[note == "on a point, r2 = 0"][0] == 0 and want[note == "on a point, the smallest r2"][0] == 1
    assert want[note == "empty segment"][0] == 0 and want[note == "beside the point"][0] == 0
    assert (want[np.char.startswith(note, "non-finite query")] == 0).all() and want[note == "NaN query"][0] == 0
    assert want[note == "finite query, non-finite points"][0] > 0 and want[note == "r2 = inf"][0] == 12
    assert (want[(ql < 0) | (ql > 4)] == 0).all() and ((ql < 0) | (ql > 4)).sum() >= 10
    changed = {m: np.nonzero(_edge_counts(case, m) != want)[0] for m in ("le", "fma", "f64")}
    print({m: len(i) for m, i in changed.items()})
    assert len(changed["le"]) >= len(b)  # every boundary query has a point at d^2 == r^2
    for what in ("fma above", "fma below"):
        assert np.isin(np.nonzero(note == what)[0], changed["fma"]).all(), what
    for what in ("f64 above", "f64 below"):
        assert np.isin(np.nonzero(note == what)[0], changed["f64"]).all(), what
    # ... and in every batch size above 1 some query's count depends on each of the three
    for m, idx in changed.items():
        assert (idx < 255).any() and len(idx) >= 1, m


@gpu
def test_count_within_edge_cases():
    case = count_within_edge_case()
    xyz, lab, q, ql, r2, note = case
    want = _edge_counts(case)
    cam = syn.CAM_640
    core = _core()
    H, W = cam["height"], cam["width"]
    core.set_observation(torch.zeros((H, W), dtype=torch.int32, device=DEV), torch.zeros((H, W), dtype=torch.uint8, device=DEV),
                         torch.from_numpy(xyz).to(DEV), torch.from_numpy(lab).to(DEV), 0.01)
    tq, tl, tr = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (q, ql, r2))
    for n in EDGE_BATCHES:
        got = core.count_within(tq[:n].contiguous(), tl[:n].contiguous(), tr[:n].contiguous()).cpu().numpy()
        bad = np.nonzero(got != want[:n])[0]
        assert got.shape == (n,) and len(bad) == 0, (n, [(int(i), note[i], int(got[i]), int(want[i])) for i in bad[:8]])
    core.close()
