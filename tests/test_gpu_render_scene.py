"""GPU: pcore_render_scene (the composed state: every pose into one frame) against the contract in numpy
(tests/scene_reference.py over the oracle's per-pose renders), bit for bit: depth, owner, colour planes and visible.
The cases and what makes them able to fail are in tests/scene_cases.py and tests/test_scene_cases.py."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from perception_amd import _native  # noqa: E402
from perception_amd.core import PcoreError, PoseCore  # noqa: E402
from tests import scene_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _core(observation):
    """A context on the cases' scene: meshes with colours and the camera; observation = None, "mask" or "nomask"."""
    case, rgb = sc.scene_case()
    s = case.scene
    core = PoseCore(0)
    core.upload_meshes(s.bank.tris, s.bank.tris_model_count, rgb)
    core.set_camera(s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.proj)
    if observation is not None:
        mask = torch.from_numpy(s.mask).to(DEV)
        xyz, lab = core.observed_cloud(torch.from_numpy(s.depth_raw).to(DEV), mask, case.stride, s.depth_factor)
        if observation == "mask":
            core.set_observation(torch.from_numpy(s.src_depth_cm).to(DEV), mask, xyz, lab, 0.01)
        else:
            core.set_observation(torch.from_numpy(s.src_depth_cm).to(DEV), None, xyz, None, 0.01)
    return core


@pytest.fixture(scope="module")
def core():
    return _core("mask")


@pytest.fixture(scope="module")
def bare_core():
    return _core(None)


def _run(core, name, mode, order=None, **kw):
    ps = sc.pose_set(name)
    idx = np.arange(ps.n) if order is None else np.asarray(order, np.int64)
    occlude, labels = sc.MODES[mode]
    poses = torch.from_numpy(ps.poses[idx]).to(DEV)
    pm = torch.from_numpy(ps.pose_model[idx]).to(DEV)
    pl = torch.from_numpy(ps.pose_label[idx]).to(DEV) if labels else None
    out = core.render_scene(poses, pm, pl, sc.THRESHOLD, occlude=occlude, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _assert_frame(got, want):
    depth, color, owner, visible = got
    wd, wc, wo, wv = want
    assert np.array_equal(depth, wd), f"depth differs on {(depth != wd).sum()} pixels"
    assert np.array_equal(owner, wo), f"owner differs on {(owner != wo).sum()} pixels"
    assert np.array_equal(color, wc), f"colour differs on {(color != wc).any(0).sum()} pixels"
    assert np.array_equal(visible, wv), (visible, wv)


@pytest.mark.parametrize("mode", list(sc.MODES))
@pytest.mark.parametrize("name", ["candidates", "state", "lens"])
def test_frame_equals_the_contract(core, name, mode):
    got = _run(core, name, mode)
    assert got[0].dtype == np.int32 and got[1].dtype == np.uint8 and got[1].shape == (3,) + got[0].shape
    _assert_frame(got, sc.expected(name, mode))


@pytest.mark.parametrize("name", ["candidates", "state"])
def test_occlude_off_needs_no_observation(bare_core, name):
    _assert_frame(_run(bare_core, name, "plain"), sc.expected(name, "plain"))


@pytest.mark.parametrize("mode", ["threshold", "labels"])
def test_one_pose_equals_pcore_render(core, mode):
    ps = sc.pose_set("state")
    for k in (0, 4):  # an object in the open and one behind another object's place
        depth, color, owner, visible = _run(core, "state", mode, order=[k])
        pl = torch.from_numpy(ps.pose_label[k:k + 1]).to(DEV) if mode == "labels" else None
        d1, c1 = core.render(torch.from_numpy(ps.poses[k:k + 1]).to(DEV), torch.from_numpy(ps.pose_model[k:k + 1]).to(DEV),
                             pl, sc.THRESHOLD, color=True)
        d1, c1 = d1.cpu().numpy()[0], c1.cpu().numpy()[:, 0]
        assert d1.any()
        assert np.array_equal(depth, d1) and np.array_equal(color, c1)
        assert np.array_equal(owner, np.where(d1 != 0, 0, -1)) and visible.tolist() == [int((d1 != 0).sum())]


def test_no_poses_give_the_empty_frame(core):
    _run(core, "state", "plain")  # keys of a full frame are in the scratch
    for mode in ("plain", "labels"):
        depth, color, owner, visible = _run(core, "state", mode, order=[])
        assert not depth.any() and not color.any() and (owner == -1).all() and visible.shape == (0,)


@pytest.mark.parametrize("name,mode", [("candidates", "plain"), ("candidates", "labels"), ("state", "labels")])
def test_pose_order_moves_only_the_owners_of_ties(core, name, mode):
    n = sc.pose_set(name).n
    D, _ = sc.per_pose(name, mode)
    base = _run(core, name, mode)
    key = np.where(D != 0, D.astype(np.int64), np.int64(1) << 40)
    attained = (key == key.min(0)[None]) & (D != 0)  # (N, H, W): the poses at each pixel's minimum
    tie = attained.sum(0) >= 2
    assert tie.sum() > 0
    for order in (np.arange(n)[::-1], np.random.default_rng(3).permutation(n)):
        got = _run(core, name, mode, order=order)
        _assert_frame(got, sc.expected(name, mode, order))
        assert np.array_equal(got[0], base[0])  # the same depth
        covered = base[0] != 0
        orig = np.where(got[2] >= 0, order[np.maximum(got[2], 0)], -1)  # owners as indices of the original order
        assert np.array_equal(orig[~tie], base[2][~tie])  # off the ties: the same pose, through the permutation
        # on them: the lowest NEW index among the poses at the minimum
        first = attained[order].argmax(0)
        assert np.array_equal(got[2][tie & covered], first[tie & covered])


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("owner", [False, True])
@pytest.mark.parametrize("visible", [False, True])
def test_nullable_outputs(core, color, owner, visible):
    want = sc.expected("state", "labels")
    depth, c, o, v = _run(core, "state", "labels", color=color, owner=owner, visible=visible)
    assert np.array_equal(depth, want[0])
    assert (c is not None) == color and (o is not None) == owner and (v is not None) == visible
    assert c is None or np.array_equal(c, want[1])
    assert o is None or np.array_equal(o, want[2])
    assert v is None or np.array_equal(v, want[3])


def test_second_call_with_fewer_poses_sees_no_stale_keys(core):
    _assert_frame(_run(core, "candidates", "labels"), sc.expected("candidates", "labels"))
    _assert_frame(_run(core, "state", "labels", order=[4, 1]), sc.expected("state", "labels", [4, 1]))
    _assert_frame(_run(core, "candidates", "plain"), sc.expected("candidates", "plain"))


@pytest.mark.parametrize("pad", [294, 65540])
def test_models_out_of_range_render_nothing_and_high_poses_count(core, pad):
    """`pad` poses of models outside the meshes, then the state set: the frame is the state set's with its owners moved
    up by `pad` -- past the poses whose pixels the finalize pass counts in LDS (256) and, for the larger one, past the
    65535 poses one pass of the raster grid covers."""
    ps = sc.pose_set("state")
    wd, wc, wo, wv = sc.expected("state", "labels")
    poses = torch.from_numpy(np.concatenate([np.tile(ps.poses[:1], (pad, 1)), ps.poses])).to(DEV)
    bad = np.where(np.arange(pad) % 2 == 0, 3, -1).astype(np.int32)  # one past the last model, and a negative id
    pm = torch.from_numpy(np.concatenate([bad, ps.pose_model])).to(DEV)
    pl = torch.from_numpy(np.concatenate([np.zeros(pad, np.int32), ps.pose_label])).to(DEV)
    depth, color, owner, visible = (t.cpu().numpy() for t in core.render_scene(poses, pm, pl, sc.THRESHOLD))
    want = (wd, wc, np.where(wo >= 0, wo + pad, -1), np.concatenate([np.zeros(pad, np.int32), wv]))
    _assert_frame((depth, color, owner, visible), want)


@pytest.mark.parametrize("drop", [(), ("behind", "straddle_z0"), ("behind", "straddle_z0", "very_close")],
                         ids=["all", "positive", "borders"])
@pytest.mark.parametrize("mode", list(sc.MODES))
def test_border_and_degenerate_poses(mode, drop):
    """A small camera (200 x 150) and the geometry cases' hand-made poses among the candidates: objects across every
    image border and out of view; one so close that it covers the whole image in front of all others; one behind the
    camera and one through the camera's own plane, which fill the image with negative depths that win everywhere.  So
    the last two, and then the close one, are taken out in turn."""
    from tests import scene_reference as ref
    from tests.helpers import geometry_case

    gc = geometry_case("SMALL", 8)
    s = gc.scene
    rgb = np.random.default_rng(8).integers(0, 256, (len(s.bank.tris), 3), dtype=np.uint8)
    occlude, labels = sc.MODES[mode]
    keep = np.ones(gc.n, bool)
    keep[[gc.edge_idx[k] for k in drop]] = False
    gposes, gmodel, glabel = gc.poses[keep], gc.pose_model[keep], gc.pose_label[keep]
    want = ref.render_scene(s, rgb, gposes, gmodel, glabel if labels else None, occlude, sc.THRESHOLD)
    assert (want[0] < 0).any() == (not drop) and (len(drop) < 3 or (want[3] > 0).sum() >= 10)
    core = PoseCore(0)
    core.upload_meshes(s.bank.tris, s.bank.tris_model_count, rgb)
    core.set_camera(s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.proj)
    mask = torch.from_numpy(s.mask).to(DEV)
    core.set_observation(torch.from_numpy(s.src_depth_cm).to(DEV), mask, torch.from_numpy(gc.obs_xyz_raw).to(DEV),
                         torch.from_numpy(gc.obs_label_raw).to(DEV), 0.01)
    out = core.render_scene(torch.from_numpy(gposes).to(DEV), torch.from_numpy(gmodel).to(DEV),
                            torch.from_numpy(glabel).to(DEV) if labels else None, sc.THRESHOLD, occlude=occlude)
    _assert_frame(tuple(t.cpu().numpy() for t in out), want)


# -- refusals: the status, and every output left as it was --------------------------------------------------------------

def _refused(core, n, labels, occlude, n_claimed=None):
    case, _ = sc.scene_case()
    h, w = case.scene.height, case.scene.width
    ps = sc.pose_set("state")
    poses = torch.from_numpy(ps.poses[:n]).to(DEV)
    pm = torch.from_numpy(ps.pose_model[:n]).to(DEV)
    pl = torch.from_numpy(ps.pose_label[:n]).to(DEV) if labels else None
    depth = torch.full((h, w), 77, dtype=torch.int32, device=DEV)
    color = torch.full((3, h, w), 7, dtype=torch.uint8, device=DEV)
    owner = torch.full((h, w), 55, dtype=torch.int32, device=DEV)
    visible = torch.full((n,), 33, dtype=torch.int32, device=DEV)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = core.lib.pcore_render_scene(core._h, vp(poses), vp(pm), vp(pl), n if n_claimed is None else n_claimed,
                                     int(occlude), 1.0, vp(depth), vp(color), vp(owner), vp(visible), None)
    torch.cuda.synchronize()
    assert (depth == 77).all() and (color == 7).all() and (owner == 55).all() and (visible == 33).all()
    return rc


def test_refusals_leave_the_outputs_untouched(core, bare_core):
    assert _refused(core, 6, labels=True, occlude=False) == _native.PCORE_E_INVALID_ARG
    assert _refused(bare_core, 6, labels=False, occlude=True) == _native.PCORE_E_STATE
    assert _refused(bare_core, 6, labels=True, occlude=True) == _native.PCORE_E_STATE
    assert _refused(_core("nomask"), 6, labels=True, occlude=True) == _native.PCORE_E_INVALID_ARG
    # the key's low word: num_poses * num_tris has to fit 32 bits; refused before anything is read or launched
    num_tris = len(sc.scene_case()[0].scene.bank.tris)
    over = (2 ** 32 - 1) // num_tris + 1
    assert over <= 2 ** 31 - 1
    assert _refused(core, 6, labels=False, occlude=False, n_claimed=over) == _native.PCORE_E_INVALID_ARG
    assert _refused(core, 6, labels=False, occlude=False, n_claimed=2 ** 31 - 1) == _native.PCORE_E_INVALID_ARG
    assert _refused(core, 6, labels=False, occlude=False, n_claimed=-1) == _native.PCORE_E_INVALID_ARG
    # and the Python face raises with the same code
    ps = sc.pose_set("state")
    with pytest.raises(PcoreError) as e:
        core.render_scene(torch.from_numpy(ps.poses).to(DEV), torch.from_numpy(ps.pose_model).to(DEV),
                          torch.from_numpy(ps.pose_label).to(DEV), occlude=False)
    assert e.value.code == _native.PCORE_E_INVALID_ARG
    _assert_frame(_run(core, "state", "labels"), sc.expected("state", "labels"))  # the context still works
