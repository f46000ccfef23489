"""CPU certificates of tests/one_sample_cases.py: the GPU tests of tests/test_gpu_one_sample_path.py could fail.  With
the stream builder and the reference's bounding-box rule alone (no GPU) this module asserts that the steps the fused
raster walks hold every class of sample window the triangle stage tells apart -- empty, one sample, 2 to 4 samples in
a row, in a column and as 2 x 2, more than 4 (the cooperative path), padding slots, NaN-vertex triangles -- that
steps mix one-sample lanes with other non-empty lanes, that such steps follow each other within a stream, and that
under the 64-sample tile one-sample windows exist that only the clip to a chunk makes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import one_sample_cases as oc
from tests.one_sample_cases import CLASSES, classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VRING, REF_PASSES, WAVES, CHUNKS = 4, 2, 4, 1  # pcore_internal.h: kVRing, kRefPasses, kFusedWaves, kStreamChunks
ONE, EMPTY, BIG = CLASSES.index("1"), CLASSES.index("empty"), CLASSES.index("big")
WHOLE, NAN, TIGHT = (oc.MODELS.index(m) for m in ("whole", "nan", "tight"))


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    """Per model: (steps, 64) int, the local triangle index of every slot of every step in stream order, -1 for a
    padding slot; and the model's number of streams."""
    out = tmp_path_factory.mktemp("one_sample_streams") / "libstreamsteps.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "stream_stats.cpp"),
                    "-o", str(out)], check=True)
    L = ctypes.CDLL(str(out))
    L.stream_steps.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int]
    L.stream_steps.restype = ctypes.c_int
    L.stream_check.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    L.stream_check.restype = ctypes.c_int
    res = []
    for tris in oc.bank().models:
        t = np.ascontiguousarray(tris, np.float32)
        buf = np.full((256, 64), -2, np.int32)
        n = L.stream_steps(t.ctypes.data, len(t), WAVES, VRING, REF_PASSES, CHUNKS, buf.ctypes.data, 256)
        assert 0 < n <= 256
        info = np.zeros(4, np.int64)
        assert L.stream_check(t.ctypes.data, len(t), WAVES, VRING, REF_PASSES, CHUNKS, info.ctypes.data) == 0
        assert info[1] == n
        res.append((buf[:n].astype(np.int64), int(info[3])))
    return res


def lane_classes(case, pose, stride, step_tris, clip=None):
    """(steps, 64) class index of every slot for this pose: -1 padding, -2 a NaN-vertex triangle, -3 a window that
    float32 rounding could change (counted as nothing)."""
    _, _, nx, ny, sure, nan = case.windows(pose, stride, clip)
    cl = np.where(nan, -2, np.where(sure, classify(nx, ny), -3))
    return np.where(step_tris < 0, -1, cl[np.maximum(step_tris, 0)])


def test_the_cases_are_the_ones_described():
    case = oc.case()
    b = case.bank
    assert case.width % 8 == 0 and case.width % 3 == 0 and set(oc.STRIDES) == {8, 3}
    assert case.width * case.height <= 168 * 120 and case.n <= 64 and b.tris_model_count.max() <= 400
    assert np.isfinite(b.models[WHOLE]).all() and np.isfinite(b.models[TIGHT]).all()
    assert np.isnan(b.models[NAN]).any(axis=1).sum() == oc.N_NAN
    assert not case.src_depth.any()
    # every pose of the finite models passes the fastdiv bound with room (camera depths in cm, 1 <= z): the fused
    # depth pass takes its fastdiv copy for them and the other copy for the NaN model
    for p in range(case.n):
        _, z = case.screen(p)
        if case.pose_model[p] != NAN:
            assert 20.0 < z.min() and z.max() < 100.0


def test_whole_models_pose_windows_are_the_sampled_image():
    """The corners of the model's box project at least 4 pixels beyond the image on every side (the pose window's
    margin only widens it), so the window is clamped to the whole sampled image and oc.chunks() are its chunks."""
    case = oc.case()
    box = case.bank.models[WHOLE].reshape(-1, 3).astype(np.float64)
    lo, hi = box.min(0), box.max(0)
    cor = np.array([[(hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2]] for k in range(8)])
    p = case.proj.astype(np.float64)
    W, H = case.width, case.height
    for pose in np.nonzero(case.pose_model == WHOLE)[0]:
        M = case.poses[pose].astype(np.float64).reshape(4, 4)
        cam = cor @ M[:3, :3].T + M[:3, 3]
        sx = (p[0] * cam[:, 0] + p[2] * cam[:, 2]) / cam[:, 2] * (W / 2) + W / 2
        sy = (p[5] * cam[:, 1] + p[6] * cam[:, 2]) / cam[:, 2] * (H / 2) + H / 2
        assert sx.min() < -4 and sx.max() > W + 4 and sy.min() < -4 and sy.max() > H + 4, case.describe(pose)


@pytest.mark.parametrize("stride", oc.STRIDES)
def test_every_class_shares_a_step_with_single_lanes(steps, stride):
    """For every model: each class of window occurs in a step that also holds one-sample lanes, padding slots occur in
    such a step, at least a third of the steps mix one-sample lanes with other non-empty lanes, and steps of only
    one-sample and empty lanes exist (the general path is skipped there)."""
    case = oc.case()
    for m in range(case.bank.K):
        step_tris, _ = steps[m]
        seen, mixed, only_single, total = set(), 0, 0, 0
        for pose in np.nonzero(case.pose_model == m)[0]:
            cl = lane_classes(case, pose, stride, step_tris)
            for row in cl:
                has_one = (row == ONE).any()
                other = ((row > ONE) | (row == -2)).any()
                total += 1
                mixed += has_one and other
                only_single += has_one and not other and not (row == -3).any()
                if has_one:
                    seen |= set(row.tolist())
        print(f"stride {stride}, model {oc.MODELS[m]}: {total} steps, {mixed} mix single and other lanes, "
              f"{only_single} hold single and empty lanes only")
        want = set(range(len(CLASSES))) | {-1} | ({-2} if m == NAN else set())
        assert want <= seen, (oc.MODELS[m], sorted(want - seen))
        assert 3 * mixed >= total and only_single > 0, (oc.MODELS[m], total, mixed, only_single)


@pytest.mark.parametrize("stride", oc.STRIDES)
def test_mixed_steps_follow_each_other_within_a_stream(steps, stride):
    """More consecutive pairs of mixed steps than the model has streams: two streams' steps meet at fewer places than
    that, so some pair lies within one stream, whose record ring carries over from one to the other."""
    case = oc.case()
    for m in range(case.bank.K):
        step_tris, nstreams = steps[m]
        assert nstreams == WAVES and len(step_tris) >= 2 * nstreams
        pose = int(np.nonzero(case.pose_model == m)[0][0])
        cl = lane_classes(case, pose, stride, step_tris)
        mix = np.array([(r == ONE).any() and ((r > ONE) | (r == -2)).any() for r in cl])
        assert (mix[1:] & mix[:-1]).sum() >= nstreams, (oc.MODELS[m], mix)


def test_nan_triangles_sit_next_to_single_lanes(steps):
    """At either stride, every pose of the NaN model has a step that holds a NaN-vertex triangle and one-sample lanes,
    and every NaN-vertex triangle is in such a step at some pose."""
    case = oc.case()
    step_tris, _ = steps[NAN]
    nan_rows = [r for r in range(len(step_tris)) if np.isin(step_tris[r], case.bank.exempt[NAN]).any()]
    assert len(nan_rows) == oc.N_NAN  # one to a step
    for stride in oc.STRIDES:
        beside = set()
        for pose in np.nonzero(case.pose_model == NAN)[0]:
            cl = lane_classes(case, pose, stride, step_tris)
            assert all((cl[r] == -2).sum() == 1 for r in nan_rows)
            hit = [r for r in nan_rows if (cl[r] == ONE).any()]
            assert hit, (stride, case.describe(pose))
            beside |= set(hit)
        assert beside == set(nan_rows), stride


@pytest.mark.parametrize("stride", oc.STRIDES)
def test_chunks_make_single_windows(steps, stride):
    """Under the 64-sample tile the whole-window models are scored in the chunks of oc.chunks(): in some chunk, a
    triangle whose unclipped window holds 2 to 4 samples and one whose window holds more than 4 are clipped to exactly
    one sample, in a step that also holds other non-empty lanes."""
    case = oc.case()
    chunks = case.chunks(stride)
    assert len(chunks) > 1 and all((c[2] - c[0] + 1) * (c[3] - c[1] + 1) <= oc.TCAP for c in chunks)
    for m in (WHOLE, NAN):
        step_tris, _ = steps[m]
        pose = int(np.nonzero(case.pose_model == m)[0][0])
        full = lane_classes(case, pose, stride, step_tris)
        small = big = 0
        for c in chunks:
            cl = lane_classes(case, pose, stride, step_tris, clip=c)
            for r_full, r in zip(full, cl):
                made = (r == ONE) & (r_full != ONE)
                if made.any() and (r > ONE).any():
                    small += int((made & (r_full > ONE) & (r_full < BIG)).sum())
                    big += int((made & (r_full == BIG)).sum())
        print(f"stride {stride}, model {oc.MODELS[m]}: single windows made by a chunk: {small} of small windows, "
              f"{big} of big ones")
        assert small > 0 and big > 0


@pytest.mark.parametrize("stride", oc.STRIDES)
def test_colour_costs_move_with_the_colouring(stride):
    """The colourings give every pair of triangles of a model different colours in some colouring (their indices
    differ in a bit), and the oracle's type-1 costs of every pose differ between colourings: a colour id taken from
    the wrong triangle shows in a cost."""
    case = oc.case()
    nb = case.bank.num_colourings()
    assert 2 ** nb >= case.bank.tris_model_count.max()
    rc = np.stack([case.oracle_colour_costs(stride, b)[0] for b in range(nb)])
    for p in range(case.n):
        assert len(np.unique(rc[:, p])) >= nb // 2, case.describe(p)


@pytest.mark.parametrize("stride", oc.STRIDES)
def test_a_triangles_colour_id_shows_in_a_cost(stride):
    """The GPU test sees colour ids through the type-1 costs.  A sample's colour moves a cost only where the sample has
    an observed neighbour within r.  The observation keeps two of every three blocks of samples, so at least two
    thirds of the triangles that own a sample must own one that counts: with such a triangle alone in colour A, some
    pose's cost differs from the all-B cost.  An id taken from another triangle then differs from the right one in
    the colouring of a bit in which their indices differ (test_colour_costs_move_with_the_colouring).  Checked on
    every pose of the model without corner triangles."""
    case = oc.case()
    b = case.bank
    sel = np.nonzero(case.pose_model == TIGHT)[0]
    base = np.tile(oc.mc.COLOUR_B, (len(b.tris), 1)).astype(np.uint8)
    rc0 = case.costs_of(stride, 1, case.poses[sel], case.pose_model[sel], None, colours=base)[0]
    owners = np.unique(case.owners[sel][:, ::stride, ::stride])
    owners = owners[owners >= 0]
    assert len(owners) >= 100
    moved = 0
    for t in owners:
        col = base.copy()
        col[t] = oc.mc.COLOUR_A
        rc = case.costs_of(stride, 1, case.poses[sel], case.pose_model[sel], None, colours=col)[0]
        moved += bool((rc != rc0).any())
    print(f"stride {stride}: {moved} of {len(owners)} owning triangles move a colour cost alone")
    assert 3 * moved >= 2 * len(owners)
