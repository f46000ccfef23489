"""GPU: one context reused across scenes, cameras and mesh banks scores each scene as a fresh context would.

ObjectRecognizer keeps one PoseCore for its life and gives it a new mesh bank (set_static_input) and a new observation
(set_input) per request.  The context's device buffers only grow, and a dozen derived states sit behind keys (the
sampled source per stride, the target covariances per k, the planar ICP's world-frame grid, the point-to-plane scene,
the observed colours, the tile tier).  Here one context walks the scene sequences of tests/context_cases.py -- fewer
labels, points, triangles and models; a smaller image; everything larger again -- and after every step every call is
compared with its CPU reference (the oracle, tests/icp2d_reference.py, tests/p2p_reference.py, tests/topk_reference.py,
_pcl_counts), directly and bit for bit, never with a fresh context.  tests/test_context_reuse_cases.py certifies on the
CPU that each kind of state wrongly kept from the previous scene would change these references' results.

Then the state contract (what a setup call invalidates, what is refused until the next one, pcore_generation and
captured graphs, the generation across the slots the staged ICPs share, a context's teardown), and an ObjectRecognizer
that localises one scene, another with another model set, and the first again."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import _native, synthetic as syn
from perception_amd._native import PCORE_E_INVALID_ARG, PCORE_E_STATE, PcoreError
from perception_amd.core import PoseCore, decode_keys
from perception_amd.model import matrix_to_quat_xyzw
from perception_amd.recognizer import CameraIntrinsics, ModelMetaData, ObjectRecognizer, PerchParams, RecognitionInput
from tests import context_cases as cc
from tests import p2p_reference as refp
from tests.helpers import SMALL, oracle_recognizer_pipeline, oracle_render_fn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INDEX_BASE = 1000


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_f32(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} differ, e.g. {bad[:6]}: gpu {got[bad[:4]]} want {want[bad[:4]]}"


def _same_costs(got, want, what):
    for g, w, n in zip(got, want, ("rc", "oc", "diff")):
        _same_f32(g, w, f"{what} {n}")


def _tensors(s):
    return {k: _dev(v) for k, v in (("poses", s.poses), ("pm", s.pose_model), ("pl", s.pose_label),
                                    ("tot", s.pose_obs_total), ("tot0", s.pose_obs_total0),
                                    ("depth", s.scene.depth_raw), ("src", s.scene.src_depth_cm),
                                    ("mask", s.scene.mask), ("rgb", s.obs_rgb_raw))}


def _load(core, s, t, camera):
    """What a request does to the context: the scene's mesh bank, its camera where it differs from the last one, the
    observed cloud (unprojected on the GPU, equal to the oracle's) and the observation.  The colours come later."""
    sc = s.scene
    core.upload_meshes(sc.bank.tris, sc.bank.tris_model_count, colors=sc.bank.colors)
    if camera:
        core.set_camera(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy, sc.proj)
    xyz, lab = core.observed_cloud(t["depth"], t["mask"], s.stride, sc.depth_factor)
    _same_f32(xyz, s.case.obs_xyz_raw, f"{s.name} observed cloud")
    assert np.array_equal(lab.cpu().numpy(), s.case.obs_label_raw)
    core.set_observation(t["src"], t["mask"], xyz, lab, s.res)


def _evaluate(core, s, t, cost_type, **kw):
    six = cost_type == 2
    return core.evaluate(t["poses"], t["pm"], t["pl"] if six else None, t["tot"] if six else t["tot0"],
                         cost_type=cost_type, stride=s.stride, sensor_resolution=s.res,
                         color_distance_threshold=cc.COLOUR_THR, **kw)


def _check_costs(core, s, t, what):
    """Cost types 2 and 0, twice (the second call after the tile feedback); evaluate(select=) and select."""
    for call in range(2):
        for ct in (2, 0):
            _same_costs(_evaluate(core, s, t, ct), cc.want_costs(s.name, ct), f"{what} type {ct} call {call}")
    K = len(s.scene.bank.tris_model_count)
    orc, ooc, _ = cc.want_costs(s.name, 2)
    ocost, oidx = oracle.select(orc, ooc, s.pose_model, K, INDEX_BASE)
    keys = torch.full((K,), _native.PCORE_KEY_NONE, dtype=torch.int64, device=DEV)
    rc, oc, df = _evaluate(core, s, t, 2, select=(keys, INDEX_BASE, K))
    _same_costs((rc, oc, df), cc.want_costs(s.name, 2), f"{what} evaluate_select")
    for k in (keys, core.select(rc, oc, t["pm"], K, index_base=INDEX_BASE)):
        cost, idx = decode_keys(k)
        assert np.array_equal(cost, ocost) and np.array_equal(idx, oidx), (what, cost, idx, ocost, oidx)
    assert (oidx >= 0).all()
    # the poses of labels this scene does not have (segments the previous scene may have had): an empty segment's costs
    if len(s.empty_idx):
        got = rc.cpu().numpy()[s.empty_idx], oc.cpu().numpy()[s.empty_idx]
        assert (got[0] == 100.0).all() and (got[1] == 100.0).all(), (what, got)
    topk = core.select_topk(rc, oc, t["pm"], K, cc.TOPK, index_base=INDEX_BASE).cpu().numpy()
    assert np.array_equal(topk, cc.want_topk(s.name, INDEX_BASE)), what


def _check_colours(core, s, t, prev, what):
    """Cost type 1: refused after the new observation until its colours are set, and the previous scene's colours
    (another point count) are refused."""
    out = tuple(torch.full((s.n,), -7.0, device=DEV) for _ in range(3))
    with pytest.raises(PcoreError) as ei:
        _evaluate(core, s, t, 1, out=out)
    assert ei.value.code == PCORE_E_INVALID_ARG
    if prev is not None and len(prev.obs_rgb_raw) != len(s.obs_rgb_raw):
        with pytest.raises(PcoreError) as ei:
            core.set_observation_colors(_dev(prev.obs_rgb_raw))
        assert ei.value.code == PCORE_E_INVALID_ARG
        with pytest.raises(PcoreError):
            _evaluate(core, s, t, 1, out=out)
    assert all((o == -7.0).all().item() for o in out)
    core.set_observation_colors(t["rgb"])
    for call in range(2):
        _same_costs(_evaluate(core, s, t, 1), cc.want_costs(s.name, 1), f"{what} colour call {call}")


def _check_icp(core, s, t, ks, what):
    i = _dev(s.icp_idx)
    poses, pm, pl = t["poses"][i].contiguous(), t["pm"][i].contiguous(), t["pl"][i].contiguous()
    for k in ks:
        for six in (True, False):
            want = cc.want_icp(s.name, six, k)
            got = core.evaluate_icp(poses, pm, pl if six else None, (t["tot"] if six else t["tot0"])[i].contiguous(),
                                    cost_type=2 if six else 0, stride=s.stride, sensor_resolution=s.res, k=k)
            w = f"{what} evaluate_icp k {k} six {six}"
            assert np.array_equal(got[1].cpu().numpy(), want[1]), w
            _same_f32(got[0], want[0], w + " poses")
            _same_costs(got[2:], want[2:], w)


def _check_planar(core, s, t, what):
    """(M0, r0) first -- the matrix and radius of the previous scene's last call -- then the radius alone changes, then
    the matrix alone, then both back."""
    i = _dev(s.planar_idx)
    poses, pm = t["poses"][i].contiguous(), t["pm"][i].contiguous()
    for m, r in ((0, 0), (0, 1), (1, 1), (0, 0)):
        want = cc.want_planar(s.name, m, r)
        xf, it, st, mse = (x.cpu().numpy() for x in core.icp_planar(
            poses, pm, cc.PLANAR_M[m], stride=s.stride, depth_factor=100.0, occlusion_threshold=1.0,
            max_correspondence=cc.PLANAR_R[r]))
        w = f"{what} icp_planar matrix {m} radius {r}"
        assert np.array_equal(st, want[2]) and np.array_equal(it, want[1]), w
        assert np.array_equal(xf.view(np.uint64), np.ascontiguousarray(want[0]).view(np.uint64)), w
        assert np.array_equal(mse.view(np.uint64), np.ascontiguousarray(want[3]).view(np.uint64)), w


def _check_p2p(core, s, t, what):
    sc = s.scene
    pcd, nrm = (x.cpu().numpy() for x in core.scene_projective(t["src"], sc.fx, sc.fy, sc.cx, sc.cy))
    wp, wn = cc.want_scene(s.name)
    assert refp.same_bits(pcd, wp) and refp.same_bits(nrm, wn), what
    i = _dev(s.p2p_idx)
    got = core.evaluate_p2p(t["poses"][i].contiguous(), t["pm"][i].contiguous(), t["pl"][i].contiguous(),
                            t["tot"][i].contiguous(), stride=s.stride, sensor_resolution=s.res)
    want = cc.want_p2p(s.name)
    assert np.array_equal(got[1].cpu().numpy(), want[1]), f"{what} p2p iterations"
    for j, n in ((0, "poses"), (2, "rc"), (3, "oc"), (4, "diff"), (5, "fitness"), (6, "rmse")):
        assert refp.same_bits(got[j].cpu().numpy(), want[j]), f"{what} p2p {n}"


def _check_render(core, s, t, what):
    sc = s.scene
    i = _dev(s.render_idx)
    pl = t["pl"][i].contiguous()
    zb, col = core.render(t["poses"][i].contiguous(), t["pm"][i].contiguous(), pl, color=True)
    wz, wc = cc.want_render(s.name)
    assert np.array_equal(zb.cpu().numpy(), wz) and np.array_equal(col.cpu().numpy(), wc), what
    assert (wz > 0).any()
    xyz, pose, lab, dc = core.depth_to_cloud(zb, s.stride, 100.0, pose_label=pl, dc_index=True)
    oxyz, opose, olab = oracle.depth_to_cloud(wz, s.stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0,
                                              pose_label=s.pose_label[s.render_idx])
    _same_f32(xyz, oxyz, f"{what} depth_to_cloud")
    assert np.array_equal(pose.cpu().numpy(), opose) and np.array_equal(lab.cpu().numpy(), olab), what
    m = np.zeros(wz.shape, bool)
    m[:, ::s.stride, ::s.stride] = wz[:, ::s.stride, ::s.stride] > 0
    flat = m.ravel().astype(np.int64)
    assert np.array_equal(dc.cpu().numpy(), (np.cumsum(flat) - flat).reshape(wz.shape)), what


def _check_counts(core, s, what):
    q, lab, radius, want = cc.count_queries(s.name)
    got = core.count_within(_dev(q), _dev(lab), _dev((radius * radius).astype(np.float32))).cpu().numpy()
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:8])
    assert got[(lab < 0) | (lab >= s.num_labels)].sum() == 0 and got.sum() > 0


def _walk(names):
    core = PoseCore(0)
    prev = None
    for step, name in enumerate(names):
        s = cc.scene(name)
        t = _tensors(s)
        what = f"step {step} ({' -> '.join(names[:step + 1])})"
        _load(core, s, t, camera=prev is None or prev.cam != s.cam)
        _check_costs(core, s, t, what)
        _check_colours(core, s, t, prev, what)
        # k = 10 at every step (the same k across every scene change); 10, 5, 10 within the second scene
        _check_icp(core, s, t, (10, 5, 10) if step == 1 else (10,), what)
        _check_planar(core, s, t, what)
        _check_p2p(core, s, t, what)
        _check_render(core, s, t, what)
        _check_counts(core, s, what)
        _check_costs(core, s, t, what + ", after the refinements")
        prev = s
    core.close()


@pytest.mark.parametrize("names", cc.SEQUENCES, ids="-".join)
def test_scene_sequence_on_one_context(names):
    _walk(names)


def test_camera_that_differs_in_fx_alone():
    """B, then the same image size with another fx (set_camera, set_observation): the point-to-plane scene, which is
    keyed by the observation and four intrinsics, and everything else follow."""
    assert cc.scene("B").scene.src_depth_cm.shape == cc.scene("F").scene.src_depth_cm.shape
    _walk(("B", "F"))


# ---------------------------------------------------------------------------------------------
# the state contract
# ---------------------------------------------------------------------------------------------

N_CAP = 16


def _capture(core, s, t):
    replay, out = core.capture_evaluate(t["poses"][:N_CAP].clone(), t["pm"][:N_CAP].contiguous(),
                                        t["pl"][:N_CAP].contiguous(), t["tot"][:N_CAP].contiguous(), cost_type=2,
                                        stride=s.stride, sensor_resolution=s.res)
    replay()
    torch.cuda.synchronize()
    return replay, out


def _bumps(core, fn):
    """pcore_generation strictly increases across the setup call."""
    g = core.generation()
    fn()
    assert core.generation() > g


def _stale(replay):
    with pytest.raises(PcoreError) as ei:
        replay()
    assert ei.value.code == PCORE_E_STATE


def _refused(code, fn, outs):
    with pytest.raises(PcoreError) as ei:
        fn()
    assert ei.value.code == code
    torch.cuda.synchronize()
    assert all((o == -7).all().item() for o in outs)


def test_setup_calls_invalidate_and_refuse():
    """A context that holds scene A (with colours) is taken to scene B one setup call at a time.  Across each of
    upload_meshes, set_camera, set_observation and set_observation_colors pcore_generation strictly increases and a
    graph captured just before the call refuses to replay (PCORE_E_STATE); between set_camera and set_observation every
    call that needs an observation returns PCORE_E_STATE; after set_observation cost type 1 returns
    PCORE_E_INVALID_ARG until the colours are set again, and A's colours (another point count) are refused; no refused
    call touches its pre-filled outputs.  A fresh capture then replays to the oracle's costs of scene B."""
    A, B = cc.scene("A"), cc.scene("B")
    ta, tb = _tensors(A), _tensors(B)
    core = PoseCore(0)
    _load(core, A, ta, camera=True)
    core.set_observation_colors(ta["rgb"])
    sb = B.scene
    n = B.n

    def f32(*shape):
        return torch.full(shape, -7.0, dtype=torch.float32, device=DEV)

    def i32(*shape):
        return torch.full(shape, -7, dtype=torch.int32, device=DEV)

    # 1. upload_meshes
    replay, _ = _capture(core, A, ta)
    _bumps(core, lambda: core.upload_meshes(sb.bank.tris, sb.bank.tris_model_count, colors=sb.bank.colors))
    _stale(replay)
    # 2. set_camera (B's meshes under A's observation until then: a valid state, captured with B's poses)
    replay, _ = _capture(core, B, tb)
    _bumps(core, lambda: core.set_camera(sb.width, sb.height, sb.fx, sb.fy, sb.cx, sb.cy, sb.proj))
    _stale(replay)
    # ... after which every call that needs an observation is refused and writes nothing
    out3, out5 = tuple(f32(n) for _ in range(3)), (f32(n, 16), i32(n), f32(n), f32(n), f32(n))
    zb, cnt = i32(2, sb.height, sb.width), i32(8)
    q = torch.zeros((8, 3), device=DEV)
    for ct in (2, 0):
        _refused(PCORE_E_STATE, lambda: _evaluate(core, B, tb, ct, out=out3), out3)
    _refused(PCORE_E_STATE, lambda: core.evaluate_icp(tb["poses"], tb["pm"], tb["pl"], tb["tot"], stride=B.stride,
                                                      out=out5), out5)
    _refused(PCORE_E_STATE, lambda: core.render(tb["poses"][:2], tb["pm"][:2], tb["pl"][:2], out=zb), (zb,))
    _refused(PCORE_E_STATE, lambda: core.count_within(q, torch.zeros(8, dtype=torch.int32, device=DEV),
                                                      torch.ones(8, device=DEV), out=cnt), (cnt,))
    _refused(PCORE_E_STATE, lambda: core.set_observation_colors(tb["rgb"]), ())
    # 3. set_observation: cost type 1 is refused until the colours of this observation are set, and the previous
    # scene's colours (239 points, this one has 134) are refused
    xyz, lab = core.observed_cloud(tb["depth"], tb["mask"], B.stride, sb.depth_factor)
    _bumps(core, lambda: core.set_observation(tb["src"], tb["mask"], xyz, lab, B.res))
    assert len(A.obs_rgb_raw) != len(B.obs_rgb_raw)
    _refused(PCORE_E_INVALID_ARG, lambda: _evaluate(core, B, tb, 1, out=out3), out3)
    _refused(PCORE_E_INVALID_ARG, lambda: core.set_observation_colors(ta["rgb"]), ())
    _refused(PCORE_E_INVALID_ARG, lambda: _evaluate(core, B, tb, 1, out=out3), out3)
    # 4. set_observation_colors
    replay, _ = _capture(core, B, tb)
    _bumps(core, lambda: core.set_observation_colors(tb["rgb"]))
    _stale(replay)
    _same_costs(_evaluate(core, B, tb, 1), cc.want_costs("B", 1), "colours after the refusals")
    # 5. set_observation again: the graph is stale, and so are the colours
    replay, _ = _capture(core, B, tb)
    _bumps(core, lambda: core.set_observation(tb["src"], tb["mask"], xyz, lab, B.res))
    _stale(replay)
    _refused(PCORE_E_INVALID_ARG, lambda: _evaluate(core, B, tb, 1, out=out3), out3)
    # a fresh capture replays to the oracle's costs of the new scene, for other poses written into its tensor too
    poses = tb["poses"][:N_CAP].clone()
    replay, out = core.capture_evaluate(poses, tb["pm"][:N_CAP].contiguous(), tb["pl"][:N_CAP].contiguous(),
                                        tb["tot"][:N_CAP].contiguous(), cost_type=2, stride=B.stride,
                                        sensor_resolution=B.res)
    want = cc.want_costs("B", 2)
    for lo in (0, N_CAP, 0):
        poses.copy_(tb["poses"][lo:lo + N_CAP])
        for o in out:
            o.fill_(-7.0)
        replay()
        torch.cuda.synchronize()
        _same_costs(out, tuple(w[lo:lo + N_CAP] for w in want), f"fresh capture, poses from {lo}")
    assert (B.pose_model[:2 * N_CAP] == 0).all() and (B.pose_label[:2 * N_CAP] == 0).all()
    core.close()


def _staged_call(core, s, t, which, n):
    """One call of a staged ICP family on the first n poses of the scene (all of model 0 and label 0)."""
    poses, pm, pl, tot = (t[k][:n].contiguous() for k in ("poses", "pm", "pl", "tot"))
    if which == "gicp":
        return core.evaluate_icp(poses, pm, pl, tot, cost_type=2, stride=s.stride, sensor_resolution=s.res)
    if which == "planar":
        return core.icp_planar(poses, pm, cc.PLANAR_M[0], stride=s.stride, max_correspondence=cc.PLANAR_R[0])
    scene = {"point2plane": "projective", "point2plane_nn": "nn"}[which]
    return core.icp_point2plane(poses, pm, pl, stride=s.stride, scene=scene)


@pytest.mark.parametrize("first", ["planar", "point2plane"])
def test_evaluate_icp_growing_the_shared_slots_changes_the_generation(first):
    """pcore.h: the generation changes on every reallocation of per-batch scratch.  The staged ICPs share the slots
    their clouds are rendered into: after a planar (or point-to-plane) call on 2 poses has sized them, pcore_evaluate_icp
    on 8 poses at the same stride has to grow them -- memory a graph captured of the first call points into -- and the
    generation must increase; a second identical call reallocates nothing and leaves it as it is."""
    s = cc.scene("B")
    t = _tensors(s)
    core = PoseCore(0)
    _load(core, s, t, camera=True)
    _staged_call(core, s, t, first, 2)
    g0 = core.generation()
    _staged_call(core, s, t, "gicp", 8)
    g1 = core.generation()
    assert g1 > g0
    _staged_call(core, s, t, "gicp", 8)
    assert core.generation() == g1
    core.close()


def test_a_closed_context_leaves_nothing_the_next_one_sees():
    """A context runs an eager evaluate (the window probe), a captured one (the captured launches' own counters) and one
    call of each staged ICP family on 2 poses, then closes: every owner of device memory, pinned memory and events is
    destroyed once.  A second context in the same process repeats the sequence to the same bits."""
    s = cc.scene("B")
    t = _tensors(s)
    rounds = []
    for _ in range(2):
        core = PoseCore(0)
        _load(core, s, t, camera=True)
        got = list(_evaluate(core, s, t, 2))
        assert core.tile_info()["tcap"] > 0  # reads the mapped feedback buffer of the launch
        replay, out = _capture(core, s, t)
        got += list(out)
        for which in ("gicp", "planar", "point2plane", "point2plane_nn"):
            got += list(_staged_call(core, s, t, which, 2))
        torch.cuda.synchronize()
        rounds.append([g.cpu().numpy().tobytes() for g in got])
        del replay
        core.close()
    _same_costs([np.frombuffer(b, np.float32) for b in rounds[0][:3]], cc.want_costs("B", 2), "first round")
    assert len(rounds[0]) == 3 + 3 + 5 + 4 + 4 + 4 and rounds[0] == rounds[1]


# ---------------------------------------------------------------------------------------------
# the recognizer: one ObjectRecognizer, three requests
# ---------------------------------------------------------------------------------------------

def _request(names, centres, seed):
    rng = np.random.default_rng(seed)
    gts = np.stack([syn.default_gt_pose(rng, c) for c in centres])
    sc = syn.make_scene(list(names), gts, oracle_render_fn, cam=SMALL, rng=rng, k=8)
    lists = {}
    for k, name in enumerate(names):
        P = syn.candidate_poses(gts[k][:3, 3], 40, rng, include=gts[k], num_viewpoints=10, inplane=4)
        lists[name] = np.array([np.concatenate([T[:3, 3], matrix_to_quat_xyzw(T[:3, :3])]) for T in P])
    return sc, gts, lists


def _snapshot(res, out_dir):
    with open(os.path.join(out_dir, "output_poses.txt"), "rb") as f:
        poses_txt = f.read()
    with open(os.path.join(out_dir, "output_stats.txt")) as f:
        lines = f.read().splitlines()
    return dict(names=list(res.model_names), costs=list(res.costs), indices=list(res.indices),
                poses=np.asarray(res.detected_poses, np.float64).tobytes(),
                transforms=np.asarray(res.object_transforms, np.float64).tobytes(), poses_txt=poses_txt,
                # output_stats.txt: its header and the three counts; the fields after them are wall-clock times and
                # the allocator's peak, which no two runs share
                stats=(lines[0], lines[1], lines[2].split()[:3]))


@pytest.mark.parametrize("icp", [False, True], ids=["icp_type0", "icp_type3"])
def test_recognizer_three_requests_on_one_context(tmp_path, icp):
    """One ObjectRecognizer (one context for its life) localises a three-object scene, a scene with two other models
    and another depth image (set_static_input again), and the first scene again.  Every result equals the oracle
    pipeline's; the third equals the first byte for byte: names, costs, indices, poses, transforms, output_poses.txt
    and the counts of output_stats.txt (its other fields are wall-clock times and the allocator's peak)."""
    s1_names, s1_centres = cc.A_NAMES, cc.SCENES["A"][4]
    s2_names, s2_centres = ("036_wood_block", "061_foam_brick"), [(-0.08, -0.01, 0.52), (0.08, 0.02, 0.5)]
    req1, req2 = _request(s1_names, s1_centres, 5), _request(s2_names, s2_centres, 6)
    bank = {}
    for (sc, _, _), names in ((req1, s1_names), (req2, s2_names)):
        bank.update({n: ModelMetaData(n, model=sc.bank.models[i]) for i, n in enumerate(names)})
    cam = CameraIntrinsics(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"])
    rec = ObjectRecognizer(bank, cam, PerchParams(icp_type=3 if icp else 0, gpu_stride=4))
    snaps = []
    for step, ((sc, gts, lists), names) in enumerate(((req1, s1_names), (req2, s2_names), (req1, s1_names))):
        inp = RecognitionInput(list(names), sc.depth_raw, sc.mask, depth_factor=sc.depth_factor, pose_lists=lists,
                               use_icp=int(icp))
        res = rec.localize_objects_greedy_render(inp)
        assert res.model_names == list(names), step
        adj, bc, bi = oracle_recognizer_pipeline(rec, inp, sc, icp)
        assert res.indices == [int(i) for i in bi if i >= 0], (step, res.indices, bi)
        assert res.costs == [int(c) for c, i in zip(bc, bi) if i >= 0], (step, res.costs, bc)
        assert (bi >= 0).all(), (step, bi)  # every object of the request is found
        for k, i in enumerate(res.indices):
            T = np.asarray(adj[i], np.float32).reshape(4, 4)
            assert np.allclose(res.detected_poses[k][:3], T[:3, 3] / 100.0, atol=1e-6)
        out_dir = str(tmp_path / f"out{step}")
        rec.write_outputs(res, out_dir)
        snaps.append(_snapshot(res, out_dir))
    assert snaps[0]["names"] != snaps[1]["names"] and snaps[0]["poses_txt"] != snaps[1]["poses_txt"]
    for key, first in snaps[0].items():
        assert snaps[2][key] == first, key
    rec.core.close()
