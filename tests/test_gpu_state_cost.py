"""GPU: pcore_evaluate_states (stage COST of composed states) against the contract in numpy
(tests/state_cost_reference.py over the oracle), every output bit for bit.  The cases and what makes them able to fail
are in tests/state_cost_cases.py and tests/test_state_cost_cases.py."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from perception_amd import _native  # noqa: E402
from perception_amd.core import PcoreError, PoseCore  # noqa: E402
from tests import nn_cases as nc  # noqa: E402
from tests import scene_cases  # noqa: E402
from tests import state_cost_cases as cases  # noqa: E402
from tests import state_cost_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _core(cam, obs_xyz, obs_label, r, core=None):
    """A context with the camera and the observation only: the state cost needs no meshes."""
    W, H = cam["width"], cam["height"]
    if core is None:
        core = PoseCore(0)
        core.set_camera(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                        oracle.compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H))
    core.set_observation(up(np.zeros((H, W), np.int32)), None, up(obs_xyz), None if obs_label is None else up(obs_label),
                         r)
    return core


def _case_core(c):
    return _core(c.cam, c.obs_xyz, c.obs_label, c.r)


def _run(core, c, states=None, tot=None, **kw):
    states = c.states if states is None else states
    tot = c.tot if tot is None else tot
    six = c.pose_label is not None
    out = core.evaluate_states(states, up(c.pose_label) if six else None, up(np.asarray(tot, F32)), zs=up(c.Z),
                               cost_type=2 if six else 0, stride=c.stride, sensor_resolution=c.r, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _assert_equal(got, want, what=""):
    for name, g, w in zip(("rc", "oc", "diff", "vis", "bad"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert len(bad) == 0, f"{what} {name}: {len(bad)} of {len(g)} differ, e.g. {bad[:6]}: gpu {g[bad[:6]]}, want {w[bad[:6]]}"


FUZZ = [("TINY", 8), ("TINY", 1), ("TINY", 4), ("SMALL", 1), ("SMALL", 4), ("SMALL", 5), ("SMALL", 8)]


@pytest.mark.parametrize("labelled", [True, False], ids=["labels", "nolabels"])
@pytest.mark.parametrize("cam,stride", FUZZ, ids=[f"{c}-s{s}" for c, s in FUZZ])
def test_random_states_equal_the_contract(cam, stride, labelled):
    c = cases.fuzz(cam, stride, labelled)
    if (cam, stride) == ("TINY", 8):
        assert c.Z[0].size == 108
    if (cam, stride) == ("SMALL", 1):
        assert c.Z[0].size == 30000
    if (cam, stride) == ("SMALL", 4):
        assert c.cam["height"] % stride != 0
    core = _case_core(c)
    _assert_equal(_run(core, c), c.expected(), c.name)
    _assert_equal(_run(core, c), c.expected(), c.name + " (second call)")
    # calc_obs_cost = 0: oc and diff are written as 0
    got = _run(core, c, calc_obs_cost=False)
    _assert_equal(got, c.expected(calc_obs=False), c.name + " calc_obs 0")
    assert not got[1].view(np.uint32).any() and not got[2].view(np.uint32).any()
    # nullable member outputs
    got = _run(core, c, member_counts=False)
    assert got[3] is None and got[4] is None
    _assert_equal(got[:3], c.expected()[:3], c.name + " without member outputs")
    # S = 1
    for k in (0, len(c.states) - 3):
        w = c.expected()
        off = np.concatenate([[0], np.cumsum([len(s) for s in c.states])])
        one = _run(core, c, states=[c.states[k]], tot=c.tot[k:k + 1])
        _assert_equal(one, tuple(x[k:k + 1] for x in w[:3]) + tuple(x[off[k]:off[k + 1]] for x in w[3:]), f"{c.name} S=1 [{k}]")
    core.close()


def test_hand_made_and_scene_states_equal_the_contract():
    for c in (cases.hand(), cases.scene().case):
        core = _case_core(c)
        _assert_equal(_run(core, c), c.expected(), c.name)
        core.close()


def test_csr_spans_empty_reversed_and_outside():
    c = cases.fuzz("TINY", 8, True)
    core = _case_core(c)
    member = np.array([0, 1, 2, 3, 1, 0], np.int32)
    off = np.array([0, 2, 2, 6, 4, 6, 9, 6], np.int32)  # spans: [0,2) [2,2) [2,6) [6,4) [4,6) [6,9) [9,6)
    tot = np.full(7, 50, F32)
    out = core.evaluate_states((up(off), up(member)), up(c.pose_label), up(tot), zs=up(c.Z), cost_type=2, stride=c.stride,
                               sensor_resolution=c.r)
    torch.cuda.synchronize()
    rc, oc, df, vis, bad = (t.cpu().numpy() for t in out)
    lists = [[0, 1], [], [2, 3, 1, 0], [], [1, 0], [], []]
    w = ref.evaluate_states(c.Z, lists, c.pose_label, tot, c.cam, c.stride, c.obs_sorted, c.label_start, c.label_end, c.r)
    _assert_equal((rc, oc, df), w[:3], "csr spans")
    assert rc[1] == -1.0 and rc[3] == -1.0 and rc[5] == -1.0 and rc[6] == -1.0
    # member entries are written by the state that spans them; [2, 6) is written by state 2 and [4, 6) again by state 4
    # (entries [4, 6) are shared by states 2 and 4: overlapping spans leave them undefined, include/pcore.h)
    assert vis[:2].tolist() == w[3][:2].tolist() and bad[:2].tolist() == w[4][:2].tolist()
    assert vis[2:4].tolist() == w[3][2:4].tolist() and bad[2:4].tolist() == w[4][2:4].tolist()
    core.close()


def test_seventy_thousand_one_member_states():
    c = cases.fuzz("TINY", 8, True)
    assert c.Z[0].size == 108
    n = len(c.Z)
    S = 70000
    mem = (np.arange(S) % (n + 1)).astype(np.int32)  # every (n + 1)-th member is out of range
    tot = np.full(n + 1, 37, F32)
    w = ref.evaluate_states(c.Z, [[i] for i in range(n + 1)], c.pose_label, tot, c.cam, c.stride, c.obs_sorted,
                            c.label_start, c.label_end, c.r)
    core = _case_core(c)
    out = core.evaluate_states((up(np.arange(S + 1, dtype=np.int32)), up(mem)), up(c.pose_label), up(tot[mem]),
                               zs=up(c.Z), cost_type=2, stride=c.stride, sensor_resolution=c.r)
    torch.cuda.synchronize()
    _assert_equal(tuple(t.cpu().numpy() for t in out), tuple(x[mem] for x in w), "S = 70000")
    core.close()


def _raw(core, p, zs, n, pl, off, mem, S, tot, rc, oc, df, vis, bad, nnz):
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return core.lib.pcore_evaluate_states(core._h, ptr(zs), n, ptr(pl), ptr(off), ptr(mem), S, ptr(tot), ctypes.byref(p),
                                          ptr(rc), ptr(oc), ptr(df), ptr(vis), ptr(bad), nnz,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_refusals_write_nothing_and_the_state_contract():
    c = cases.fuzz("TINY", 8, True)
    core = _case_core(c)
    off = up(np.array([0, 2, 3], np.int32))
    mem = up(np.array([0, 1, 2], np.int32))
    tot = up(np.array([10, 10], F32))
    zs, pl = up(c.Z), up(c.pose_label)
    n = len(c.Z)

    def poisoned():
        return [torch.full((2,), 7.5, dtype=torch.float32, device=DEV) for _ in range(3)] + \
               [torch.full((3,), -77, dtype=torch.int32, device=DEV) for _ in range(2)]

    def untouched(o):
        torch.cuda.synchronize()
        return all((t.cpu().numpy() == 7.5).all() for t in o[:3]) and all((t.cpu().numpy() == -77).all() for t in o[3:])

    P = _native.EvalParams
    o = poisoned()
    assert _raw(core, P(1, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, 2, tot, *o, 3) == _native.PCORE_E_INVALID_ARG
    assert untouched(o)  # cost_type 1
    assert _raw(core, P(2, 1, 5, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, 2, tot, *o, 3) == _native.PCORE_E_INVALID_ARG
    assert untouched(o)  # 96 % 5 != 0
    assert _raw(core, P(2, 1, 0, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, 2, tot, *o, 3) == _native.PCORE_E_INVALID_ARG
    assert _raw(core, P(2, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, None, off, mem, 2, tot, *o, 3) == _native.PCORE_E_INVALID_ARG
    assert _raw(core, P(2, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, 2, None, *o, 3) == _native.PCORE_E_INVALID_ARG
    assert _raw(core, P(2, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, -1, tot, *o, 3) == _native.PCORE_E_INVALID_ARG
    assert untouched(o)
    # num_states == 0 is a no-op
    assert _raw(core, P(2, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, pl, None, None, 0, None, None, None, None, None, None, 0) == 0
    assert untouched(o)
    # the good call, with the member outputs null
    assert _raw(core, P(2, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, 2, tot, o[0], o[1], o[2], None, None, 3) == 0
    torch.cuda.synchronize()
    w = ref.evaluate_states(c.Z, [[0, 1], [2]], c.pose_label, np.array([10, 10], F32), c.cam, c.stride, c.obs_sorted,
                            c.label_start, c.label_end, c.r)
    _assert_equal(tuple(t.cpu().numpy() for t in o[:3]), w[:3], "after the refusals")
    assert (o[3].cpu().numpy() == -77).all()
    # a new camera drops the observation: PCORE_E_STATE until the next set_observation, and nothing is written
    cam = c.cam
    core.set_camera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                    oracle.compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"]))
    o = poisoned()
    assert _raw(core, P(2, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, 2, tot, *o, 3) == _native.PCORE_E_STATE
    assert untouched(o)
    with pytest.raises(PcoreError) as e:
        _run(core, c)
    assert e.value.code == _native.PCORE_E_STATE
    _core(c.cam, c.obs_xyz, c.obs_label, c.r, core=core)
    _assert_equal(_run(core, c), c.expected(), "after set_observation")
    core.close()
    bare = PoseCore(0)  # no camera at all
    assert _raw(bare, P(2, 1, 8, 100.0, c.r, 1.0, 15.0), zs, n, pl, off, mem, 2, tot, *o, 3) == _native.PCORE_E_STATE
    bare.close()


# ---------------------------------------------------------------------------------------------
# one-member states equal pcore_evaluate
# ---------------------------------------------------------------------------------------------

def _one_member_equals_evaluate(core, poses, pm, pl, tot, tot0, stride, r):
    n, w, h = int(poses.shape[0]), core.width, core.height
    nsamp = (w // stride) * ((h + stride - 1) // stride)
    for ct in (2, 0):
        six = ct == 2
        zs = torch.zeros((n, nsamp), dtype=torch.int32, device=DEV)
        t = tot if six else tot0
        e = core.evaluate(poses, pm, pl if six else None, t, cost_type=ct, stride=stride, sensor_resolution=r, dbg_zs=zs)
        s = core.evaluate_states([[i] for i in range(n)], pl if six else None, t, zs=zs, cost_type=ct, stride=stride,
                                 sensor_resolution=r)
        torch.cuda.synchronize()
        for name, a, b in zip(("rc", "oc", "diff"), e, s[:3]):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
            assert len(bad) == 0, f"cost_type {ct} {name}: {len(bad)} of {n} differ, e.g. {bad[:6]}: evaluate {a[bad[:6]]}, states {b[bad[:6]]}"
        assert (s[3].cpu().numpy() > 0).any()


@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_one_member_states_equal_evaluate_on_the_nn_cases(name):
    case = nc.nn_case(name)
    c = case.cam
    core = PoseCore(0)
    core.upload_meshes(case.bank.tris, case.bank.tris_model_count)
    core.set_camera(case.width, case.height, c["fx"], c["fy"], c["cx"], c["cy"], case.proj)
    core.set_observation(up(case.src_depth), up(case.mask), up(case.obs_xyz), up(case.obs_label), case.r)
    _one_member_equals_evaluate(core, up(case.poses), up(case.pose_model), up(case.pose_label), up(case.pose_obs_total),
                                up(case.pose_obs_total0), case.stride, case.r)
    core.close()


@pytest.fixture(scope="module")
def scene_core():
    sc = cases.scene()
    s = sc.base.scene
    core = PoseCore(0)
    core.upload_meshes(s.bank.tris, s.bank.tris_model_count)
    core.set_camera(s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.proj)
    core.set_observation(up(s.src_depth_cm), up(s.mask), up(sc.base.obs_xyz_raw), up(sc.base.obs_label_raw), 0.01)
    yield core
    core.close()


def test_one_member_states_equal_evaluate_on_the_scene(scene_core):
    sc = cases.scene()
    tot0 = np.full(len(sc.poses), len(sc.base.obs_xyz_raw), F32)
    _one_member_equals_evaluate(scene_core, up(sc.poses), up(sc.pose_model), up(sc.pose_model), up(sc.pose_obs_total),
                                up(tot0), sc.case.stride, 0.01)


def test_poses_path_equals_zs_path(scene_core):
    sc = cases.scene()
    c = sc.case
    n = len(sc.poses)
    poses, pm = up(sc.poses), up(sc.pose_model)
    zs = torch.zeros((n,) + c.Z.shape[1:], dtype=torch.int32, device=DEV)
    scene_core.evaluate(poses, pm, pm, None, calc_obs_cost=False, stride=c.stride, dbg_zs=zs)
    torch.cuda.synchronize()
    assert np.array_equal(zs.cpu().numpy(), c.Z)  # the sampled z-buffers are the oracle's
    a = scene_core.evaluate_states(c.states, pm, up(c.tot), zs=zs, stride=c.stride)
    b = scene_core.evaluate_states(c.states, pm, up(c.tot), poses=poses, pose_model=pm, stride=c.stride)
    torch.cuda.synchronize()
    _assert_equal(tuple(t.cpu().numpy() for t in b), tuple(t.cpu().numpy() for t in a), "poses= against zs=")
    _assert_equal(tuple(t.cpu().numpy() for t in a), c.expected(), "scene through evaluate's z-buffers")


def test_vis_equals_render_scene_visible_at_stride_1(scene_core):
    ps = scene_cases.pose_set("state")
    poses, pm = up(ps.poses), up(ps.pose_model)
    D = scene_core.render(poses, pm, pm, scene_cases.THRESHOLD)  # the stride-1 z-buffers after source occlusion
    _, _, _, visible = scene_core.render_scene(poses, pm, pm, scene_cases.THRESHOLD, color=False, owner=False)
    out = scene_core.evaluate_states([list(range(ps.n))], pm, up(np.array([1000], F32)), zs=D, stride=1)
    torch.cuda.synchronize()
    assert not (D.cpu().numpy() < 0).any()
    assert visible.cpu().numpy().sum() > 0
    assert np.array_equal(out[3].cpu().numpy(), visible.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# a cloud whose explained bitmap does not fit the LDS
# ---------------------------------------------------------------------------------------------

def test_cloud_above_the_lds_limit_then_a_small_one():
    c = cases.fuzz("TINY", 8, True)
    n_big = _native.PCORE_STATE_LDS_OBS + 1500
    rng = np.random.default_rng(4)
    # a jittered lattice of 0.4 cm pitch, a 20 cm cube around the optical axis from 0.38 m: it holds the poses' points at
    # 40, 41 and 55 cm near the image centre (each then has a neighbour within the radius), the others stay as they were
    side = int(np.ceil(n_big ** (1 / 3))) + 1
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n_big]
    lattice = (g * 0.004 + rng.uniform(-0.0015, 0.0015, g.shape) + np.array([-0.1, -0.1, 0.38])).astype(F32)
    keep = np.concatenate([c.obs_xyz, lattice]).astype(F32)
    lab = np.concatenate([c.obs_label, rng.integers(0, 4, len(lattice)).astype(np.int32)])
    big = cases.StateCase("fuzz-big", c.cam, c.stride, c.Z, c.pose_label, c.states, keep, lab, c.r, tot=c.tot)
    assert len(big.obs_xyz) > _native.PCORE_STATE_LDS_OBS and big.Z[0].size == 108
    want = big.expected()
    assert (want[4] < want[3]).any() and want[4].any()  # some points explained, some not
    assert any(not np.array_equal(x, y) for x, y in zip(want, c.expected()))  # the lattice changes the result
    core = _case_core(c)
    _assert_equal(_run(core, c), c.expected(), "small cloud first")
    gen = core.generation()
    _core(big.cam, big.obs_xyz, big.obs_label, big.r, core=core)
    gen_obs = core.generation()
    _assert_equal(_run(core, big), want, "cloud above the LDS limit")
    assert core.generation() > gen_obs > gen  # the bitmap scratch grew
    g2 = core.generation()
    _assert_equal(_run(core, big), want, "cloud above the LDS limit, second call")
    assert core.generation() == g2
    # more states than the launch has workgroups (two per CU): every workgroup scores several states in turn on its one
    # bitmap slot, histogram and counters.  41 distinct states, state k of the call being number k mod 41, so that the
    # states one workgroup meets in a row differ in members, size and total (41 divides no workgroup count in use)
    rng2 = np.random.default_rng(8)
    extra = [rng2.integers(0, len(big.Z), int(m)).tolist() for m in rng2.integers(0, 6, 41 - len(big.states))]
    pool_states = big.states + extra
    pool_tot = np.concatenate([big.tot, rng2.integers(1, 900, len(extra)).astype(F32)])
    assert len(pool_states) == 41
    pw = ref.evaluate_states(big.Z, pool_states, big.pose_label, pool_tot, big.cam, big.stride, big.obs_sorted,
                             big.label_start, big.label_end, big.r)
    S = 3001
    pick = np.arange(S) % 41
    poff = np.concatenate([[0], np.cumsum([len(st) for st in pool_states])])
    want_many = tuple(x[pick] for x in pw[:3]) + tuple(
        np.concatenate([x[poff[k]:poff[k + 1]] for k in pick]) for x in pw[3:])
    got_many = _run(core, big, states=[pool_states[k] for k in pick], tot=pool_tot[pick])
    _assert_equal(got_many, want_many, "3001 states over the scratch bitmap")
    assert len({tuple(st) for st in pool_states}) > 30 and (want_many[3] > 0).any()
    # 3-DoF over the same cloud
    big0 = cases.StateCase("hand-big-3dof", c.cam, c.stride, c.Z, None, c.states, keep, None, c.r, tot=c.tot)
    _core(big0.cam, big0.obs_xyz, None, big0.r, core=core)
    _assert_equal(_run(core, big0), big0.expected(), "cloud above the LDS limit, 3-DoF")
    # the same context on a small cloud afterwards
    _core(c.cam, c.obs_xyz, c.obs_label, c.r, core=core)
    _assert_equal(_run(core, c), c.expected(), "small cloud after the large one")
    core.close()


def test_binding_refuses_sizes_that_do_not_fit():
    """The kernel trusts the sizes it is given; the binding checks them before the call."""
    c = cases.fuzz("TINY", 8, True)
    core = _case_core(c)
    pl, tot, zs = up(c.pose_label), up(c.tot), up(c.Z)
    kw = dict(cost_type=2, sensor_resolution=c.r)
    with pytest.raises(ValueError, match="samples of stride 4"):
        core.evaluate_states(c.states, pl, tot, zs=zs, stride=4, **kw)  # z-buffers of stride 8
    with pytest.raises(ValueError, match="pose_label"):
        core.evaluate_states(c.states, pl[:-1].contiguous(), tot, zs=zs, stride=8, **kw)
    with pytest.raises(ValueError, match="state_obs_total"):
        core.evaluate_states(c.states, pl, tot[:-1].contiguous(), zs=zs, stride=8, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        core.evaluate_states(c.states, pl, tot, stride=8, **kw)
    _assert_equal(_run(core, c), c.expected(), "after the refusals")
    core.close()
