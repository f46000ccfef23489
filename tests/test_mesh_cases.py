"""CPU certificates of tests/mesh_cases.py: the GPU tests of tests/test_gpu_mesh_shapes.py could fail.  A parity
test on a mesh of which the image shows little proves little, so this module asserts, with the oracle and the stream
builder alone (no GPU), that nearly every triangle owns a sample, that deleting a triangle changes a depth, that a
wrong triangle index changes a colour cost, that the meshes do produce the stream shapes they are for, and that
samples exist whose colour is decided by the triangle order."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import mesh_cases as mc
from tests.mesh_cases import mesh_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VRING, REF_PASSES, WAVES = 4, 2, 4  # pcore_internal.h: kVRing, kRefPasses, kFusedWaves
MIN_SHARE = 0.90
COLOUR_RUNS = (("large", 1), ("large", 5), ("with_empty", 1))  # as tests/test_gpu_mesh_shapes.py runs them


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("mesh_streams") / "libstreamcheck.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "stream_stats.cpp"),
                    "-o", str(out)], check=True)
    L = ctypes.CDLL(str(out))
    L.stream_check.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    L.stream_check.restype = ctypes.c_int
    L.stream_vertex_passes.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 5 +
                                       [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int])
    L.stream_vertex_passes.restype = ctypes.c_int
    return L


def check(lib, tris, streams=WAVES, chunks=1):
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    info = np.zeros(4, np.int64)
    rc = lib.stream_check(t.ctypes.data, t.shape[0], streams, VRING, REF_PASSES, chunks, info.ctypes.data)
    assert rc == 0, f"stream invariant {-rc} broken"
    return dict(zip(["passes", "steps", "verts", "streams"], info.tolist()))


# ---------------------------------------------------------------------------------------------
# camera, poses, banks
# ---------------------------------------------------------------------------------------------

def test_camera_poses_and_banks_are_the_ones_described():
    W, H = mc.CAM["width"], mc.CAM["height"]
    assert W != H and all(W % s == 0 for s in (1, 2, 5, 8)) and set(mc.STRIDES) == {1, 2, 5, 8}
    assert 6 <= len(mc.POSES44) <= 8 and len(mc.POSE_KINDS) == len(mc.POSES44)
    assert np.array_equal(mc.POSES44[0][:3, :3], np.eye(3)) and mc.POSES44[0][2, 3] == 0.40
    for T in mc.POSES44:  # the tilt: the angle between the model's z axis and the camera's
        assert np.arccos(np.clip(T[2, 2], -1, 1)) <= 0.36
    sheet = mc.delaunay_sheet(2600).reshape(-1, 3).astype(np.float64)
    zc = sheet @ mc.POSES44[mc.NEAR_POSE][2, :3] + mc.POSES44[mc.NEAR_POSE][2, 3]
    assert zc.min() < 0 < zc.max()  # the camera plane cuts the model
    T = mc.POSES44[mc.OFF_SCREEN_POSE]
    cam = sheet @ T[:3, :3].T + T[:3, 3]
    u = cam[:, 0] / cam[:, 2] * mc.CAM["fx"] + mc.CAM["cx"]
    assert (u > W).any() and (u < W - 1).any()
    assert [len(mc.sized(T)) for T in mc.SIZES] == list(mc.SIZES)
    assert 370 <= len(mc.delaunay_sheet(200)) <= 400 and 1500 <= len(mc.delaunay_sheet(800)) <= 1600
    assert 5100 <= len(mc.delaunay_sheet(2600)) <= 5200
    assert len(mc.heightfield(24)) == 1152 and len(mc.fan(300)) == 300
    assert (mc.fan(300)[:, :3] == mc.FAN_HUB).all()
    b = mc.bank("small_sizes")
    assert sorted(b.tris_model_count) == sorted(mc.SIZES) and b.tris_model_count[-1] == 1
    assert list(b.tris_model_count) != sorted(mc.SIZES)
    b = mc.bank("with_empty")
    assert [lab.split("(")[0] for lab in b.labels] == ["sized", "EMPTY", "sized", "noisy", "EMPTY", "sized", "EMPTY"]
    assert list(b.tris_model_count[[0, 1, 2, 4, 5, 6]]) == [1, 0, 65, 0, 3, 0]
    assert mc.bank("empty_first").tris_model_count[0] == 0
    assert [lab for lab in mc.bank("large").labels] == ["delaunay(2600)", "fan(300)", "heightfield(24)",
                                                         "noisy(delaunay 800)"]
    for name in mc.ALL_BANKS:
        c = mesh_case(name)
        assert set(c.pose_model) == set(range(c.bank.K))  # the poses name every model, the empty ones included
        assert not c.src_depth.any()


def test_noisy_additions():
    """The additions of `noisy` are what they are listed as, at most 10 % of their model, and listed by index."""
    for arg in (200, 800):
        tris, extra = mc.noisy("delaunay", arg)
        base = mc.delaunay_sheet(arg)
        assert np.array_equal(tris[:len(base)].view(np.uint32), base.view(np.uint32))
        assert np.array_equal(extra, np.arange(len(base), len(tris))) and 10 * len(extra) <= len(tris)
        e = tris[extra].reshape(-1, 3, 3)
        rep = [(t[0] == t[1]).all() for t in e]
        assert sum(rep) >= 6
        base_keys = {t.tobytes() for t in base}
        assert sum(t.tobytes() in base_keys for t in tris[extra]) >= 6  # exact duplicates
        rev = {np.ascontiguousarray(t.reshape(3, 3)[[0, 2, 1]]).tobytes() for t in base}
        assert sum(t.tobytes() in rev for t in tris[extra]) >= 6  # duplicates with the winding reversed
        assert np.isnan(e).any(axis=(1, 2)).sum() == 2 and (e == np.inf).any(axis=(1, 2)).sum() == 2
        assert (e == -np.inf).any(axis=(1, 2)).sum() == 2
        v = e.reshape(-1, 3)
        zero = v[(v[:, 1] == 0)]
        assert len(zero) == 2 and np.array_equal(zero[0], zero[1])
        assert not np.array_equal(zero[0].view(np.uint32), zero[1].view(np.uint32))  # +0.0 and -0.0


# ---------------------------------------------------------------------------------------------
# witness share and delete-one
# ---------------------------------------------------------------------------------------------

def witnessed(case, m, stride=1, near=True):
    """The local indices of model m's triangles that own a sample of some pose of the case at this stride (near =
    False: of some pose other than the near one)."""
    sel = (case.pose_model == m) & (near | (case.pose_kind != mc.NEAR_POSE))
    own = case.owners[sel][:, ::stride, ::stride]
    w = np.unique(own)
    return w[w >= 0] - case.bank.lo[m]


@pytest.mark.parametrize("name", mc.ALL_BANKS)
def test_witness_share(name):
    """At stride 1, at least 90 % of the triangles of every surface mesh (the additions of `noisy` apart) own a
    sample in some pose.  A condition on the inputs: if a mesh falls short, the mesh or the poses change, not the
    bound.  Measured: delaunay of 5,179 triangles 0.915, noisy delaunay of 1,573 0.973, of 375 1.0, heightfield of
    1,152 1.0, fan of 300 1.0, every `sized` model 1.0."""
    case = mesh_case(name)
    b = case.bank
    for m in range(b.K):
        T = int(b.tris_model_count[m])
        if T == 0:
            continue
        assert b.surface[m]
        need = np.setdiff1d(np.arange(T), b.exempt[m])
        assert 10 * len(b.exempt[m]) <= T
        share = np.isin(need, witnessed(case, m)).mean()
        print(f"witness share: bank {name}, model {m} {b.labels[m]} ({T} triangles): {share:.3f}")
        assert share >= MIN_SHARE, (name, m, b.labels[m], share)


@pytest.mark.parametrize("name", mc.BANKS)
def test_delete_one(name):
    """For every model of at most 300 triangles and every tested stride: without any single triangle that owns a
    sample at that stride, some pose's z-samples at that stride differ.  Ownership in the near pose alone does not
    count here: triangles that cross the camera plane project over large parts of the image and cover each other at
    equal integer depths, so a sample there seldom depends on one triangle.  At stride 1 every triangle of these
    models owns a sample in another pose."""
    case = mesh_case(name)
    b = case.bank
    checked = 0
    for m in range(b.K):
        T = int(b.tris_model_count[m])
        if not 0 < T <= 300:
            continue
        sel = case.pose_model == m
        tris = b.models[m]
        z0 = case.z_full[sel]
        wit = {s: set(witnessed(case, m, s, near=False).tolist()) for s in mc.STRIDES}
        assert len(wit[1]) == T
        for t in sorted(set().union(*wit.values())):
            rest = np.ascontiguousarray(np.delete(tris, t, axis=0))
            if len(rest) == 0:
                z = np.zeros_like(z0)
            else:
                z = case.render(tris=rest, count=np.array([len(rest), 0], np.int32), poses=case.poses[sel],
                                pose_model=np.zeros(int(sel.sum()), np.int32))
            for s in mc.STRIDES:
                if t in wit[s]:
                    assert (z[:, ::s, ::s] != z0[:, ::s, ::s]).any(), (name, m, b.labels[m], t, s)
                    checked += 1
    assert checked > 0


# ---------------------------------------------------------------------------------------------
# colour identity
# ---------------------------------------------------------------------------------------------

def test_colours_are_beyond_the_gate():
    d = oracle.colour_distance(oracle.rgb2lab(mc.COLOUR_A), oracle.rgb2lab(mc.COLOUR_B))
    assert d > 2 * mc.COLOUR_THR


@pytest.mark.parametrize("name", mc.ALL_BANKS)
def test_colourings_separate_every_pair_of_triangles(name):
    """Colouring b paints a triangle A if bit b of its index within its model is set, else B; every observed point is
    B, and A and B are beyond the colour gate.  For every triangle t and every other index t' of its model some
    colouring gives them different colours (their indices differ in a bit below ceil(log2 T)).  What this pins: a
    stream slot that reports another triangle's index (a wrong stri_orig entry, a slot read from the wrong step)
    colours t's samples as t' in the colouring of a differing bit, which turns gated samples of t from good to bad
    or back and changes an expected cost -- provided t owns a gated sample, which the witness share and the check
    below (the costs do move with the colouring) are for."""
    b = mc.bank(name)
    nb = b.num_colourings()
    tables = np.stack([(b.colouring(k) == mc.COLOUR_A).all(1) for k in range(nb)], 1)  # (T, nb) bits
    for m in range(b.K):
        T = int(b.tris_model_count[m])
        if T < 2:
            continue
        assert T <= 2 ** nb
        codes = tables[b.lo[m]:b.hi[m]] @ (1 << np.arange(nb))
        assert np.array_equal(codes, np.arange(T))  # distinct codes: every pair differs in some colouring


@pytest.mark.parametrize("name,stride", COLOUR_RUNS)
def test_colour_costs_move_with_the_colouring(name, stride):
    """The oracle's type-1 costs differ between at least two colourings for every pose whose samples at the stride
    are owned by at least two different triangles (a pose that shows one triangle has one colour per colouring, and
    a one-triangle model, index 0, is colour B in all of them)."""
    case = mesh_case(name)
    nb = case.bank.num_colourings()
    rc = np.stack([case.oracle_colour_costs(stride, k)[0] for k in range(nb)])
    own = case.owners[:, ::stride, ::stride]
    moved = 0
    for p in range(case.n):
        ids = np.unique(own[p])
        ids = ids[ids >= 0]
        if len(ids) >= 2:
            assert len(np.unique(rc[:, p])) >= 2, case.describe(p)
            moved += 1
    assert moved >= 8


# ---------------------------------------------------------------------------------------------
# observation
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mc.BANKS)
def test_costs_are_sensitive(name):
    """No pose is trivially all-good or all-bad: every pose with at least 30 rendered points has a rendered cost
    strictly between 0 and 100 and leaves observed points unexplained.  Exempt: the near pose (its positive depths
    are a few centimetres, so its whole cloud is a few r across and any kept point explains all of it) and models of
    fewer than 63 triangles (a few isolated triangles can lie inside the kept blocks of samples)."""
    case = mesh_case(name)
    seen = 0
    for s in mc.STRIDES:
        o = case.observation(s)
        assert mc.N_DISPLACED < len(o.xyz) <= mc.MAX_OBS
        npts = (case.zs(s) > 0).reshape(case.n, -1).sum(1)
        for ct in (0, 2):
            rc, oc, df = case.oracle_costs(s, ct)
            for p in range(case.n):
                m = case.pose_model[p]
                if npts[p] == 0:
                    assert rc[p] == -1.0
                    continue
                if npts[p] < 30 or case.pose_kind[p] == mc.NEAR_POSE or case.bank.tris_model_count[m] < 63:
                    continue
                assert 0.0 < rc[p] < 100.0 and oc[p] > 0.0, (case.describe(p), s, ct, rc[p], oc[p])
                seen += 1
    assert seen >= 40


def test_out_of_range_models_are_empty_models():
    """The expectation for pose_model -1 and K: the costs and samples of an empty model's pose."""
    case = mesh_case("with_empty")
    pm = case.pose_model.copy()
    empty = np.nonzero(case.bank.tris_model_count[pm] == 0)[0]
    assert len(empty) >= 8 and not case.z_full[empty].any()
    pm2 = pm.copy()
    pm2[empty[::2]], pm2[empty[1::2]] = -1, case.bank.K
    for ct in (0, 2):
        a = case.costs_of(8, ct, case.poses, pm, case.pose_label)
        b = case.costs_of(8, ct, case.poses, pm2, case.pose_label)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
        assert (a[0][empty] == -1.0).all()


# ---------------------------------------------------------------------------------------------
# stream shapes
# ---------------------------------------------------------------------------------------------

def test_sized_models_yield_the_stream_counts_they_are_for(lib):
    got = [check(lib, mc.sized(T))["streams"] for T in mc.SIZES]
    assert got == list(mc.SIZED_STREAMS), got
    assert list(mc.SIZED_STREAMS) == [min(4, -(-T // 64)) for T in mc.SIZES]


def test_large_meshes_yield_four_streams_and_eight(lib):
    for tris in mc.bank("large").models:
        assert check(lib, tris)["streams"] == 4
    assert check(lib, mc.delaunay_sheet(2600), streams=8)["streams"] == 8
    assert check(lib, mc.delaunay_sheet(2600), streams=8, chunks=4)["streams"] == 8


def test_fan_hub_is_loaded_in_more_than_one_pass_per_stream(lib):
    """The hub occupies a slot in more than one vertex pass of every stream that holds triangles."""
    t = np.ascontiguousarray(mc.fan(300), np.float32)
    hub = np.ascontiguousarray(mc.FAN_HUB, np.float32)
    for streams in (1, 4):
        out = np.zeros(16, np.int32)
        S = lib.stream_vertex_passes(t.ctypes.data, len(t), streams, VRING, REF_PASSES, 1, hub.ctypes.data,
                                     out.ctypes.data, 16)
        # 300 triangles are one chunk of about 256 per stream that holds any: two of the four streams are empty
        assert S == min(streams, 4) and (out[:S] > 0).sum() == min(streams, 2)
        assert (out[:S][out[:S] > 0] > 1).all(), out[:S]


@pytest.mark.parametrize("name", mc.ALL_BANKS)
def test_stream_invariants_on_every_model(lib, name):
    for tris in mc.bank(name).models:
        for streams in (1, 3, 4, 8):
            for chunks in (1, 4):
                check(lib, tris, streams=streams, chunks=chunks)


# ---------------------------------------------------------------------------------------------
# depth ties
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["large", "with_empty"])
def test_depth_ties_between_different_triangles_exist(name):
    """Samples where two different triangles give the winning integer depth: with the model's triangles in reverse
    order the oracle colours them with the other triangle.  There the colour winner is decided by triangle order,
    which the streams permute.  Counted per delaunay / heightfield model and tested stride."""
    case = mesh_case(name)
    b = case.bank
    tie = case.owners != case.owners_reversed
    seen = 0
    for m in range(b.K):
        if not ("delaunay" in b.labels[m] or "heightfield" in b.labels[m]):
            continue
        for s in mc.STRIDES:
            n = int(tie[case.pose_model == m][:, ::s, ::s].sum())
            print(f"depth ties: bank {name}, model {m} {b.labels[m]}, stride {s}: {n}")
            assert n > 0, (name, m, b.labels[m], s)
            seen += 1
    assert seen >= 4
