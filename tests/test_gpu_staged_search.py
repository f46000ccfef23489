"""GPU: the staged search (score everything, refine the K best per model, select among the refined) against a numpy
construction from a full pre-ICP and a full post-ICP pass over the same candidates:
    shortlist S = top-K of the full pre-ICP keys; expected key per model = min over S of the full post-ICP keys.
Refining a subset must not change a pose's result, so every refined row equals the full pass's row bit for bit."""
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

from tests import topk_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["003_cracker_box", "005_tomato_soup_can", "061_foam_brick"]


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def expected_keys(pre_keys, post_keys, pm, M, K, index_base=0):
    """(shortlist (M, K), expected final key per model) of the numpy construction."""
    S = ref.topk_of_keys(pre_keys, pm, M, K)
    want = np.full(M, ref.KEY_NONE, np.int64)
    for m in range(M):
        idx = (S[m][S[m] != ref.KEY_NONE] & 0x7FFFFFFF) - index_base
        if len(idx):
            want[m] = post_keys[idx].min()
    return S, want


@pytest.fixture(scope="module")
def passes():
    """A 3-model x 400-pose batch, its full pre-ICP evaluate and its full evaluate_icp: computed once, never changed."""
    from perception_amd import workloads

    w = workloads.build(names=NAMES, poses_per_model=400)
    args = (w.poses, w.pose_model, w.pose_label, w.pose_obs_total)
    pre = tuple(t.clone() for t in w.core.evaluate(*args, stride=w.stride))
    full = tuple(t.clone() for t in w.core.evaluate_icp(*args, stride=w.stride))
    torch.cuda.synchronize()
    return w, pre, full


@pytest.mark.parametrize("K", [1, 8, 64])
def test_staged_rows_and_keys_equal_the_full_passes(passes, K):
    from perception_amd.staged import staged_step

    w, pre, full = passes
    M, pm = w.num_models, w.pose_model.cpu().numpy()
    pre_keys = ref.select_keys(pre[0].cpu().numpy(), pre[1].cpu().numpy(), pm, M)
    post_keys = ref.select_keys(full[2].cpu().numpy(), full[3].cpu().numpy(), pm, M)
    S, want = expected_keys(pre_keys, post_keys, pm, M, K)
    assert (S[:, 0] != ref.KEY_NONE).all()  # every model has candidates
    keys, topk, refined, pre2 = staged_step(w.core, w.poses, w.pose_model, w.pose_label, w.pose_obs_total, M, K,
                                            eval_kw=dict(stride=w.stride))
    for a, b in zip(pre2, pre):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(topk.cpu().numpy(), S)
    members = np.unique(S[S != ref.KEY_NONE] & 0x7FFFFFFF)
    assert len(members) == (S != ref.KEY_NONE).sum() <= M * K
    sub = refined[0].cpu().numpy()
    assert np.array_equal(sub, members)
    for name, got, whole in zip(("adjusted pose", "iterations", "rc", "oc", "diff"), refined[1:], full):
        assert np.array_equal(_bits(got), _bits(whole)[members]), (K, name)
    assert np.array_equal(keys.cpu().numpy(), want)


def _recognizer_case(root, icp_type, top_k, write=True):
    """The scene and pose lists of tests/test_gpu_recognizer.py's pipeline test -> (recognizer, input)."""
    from perception_amd import synthetic as syn
    from perception_amd.recognizer import (CameraIntrinsics, ModelMetaData, ObjectRecognizer, PerchParams,
                                           RecognitionInput)
    from tests.helpers import oracle_render_fn
    from tests.test_gpu_recognizer import _write_pose_lists

    rng = np.random.default_rng(5)
    gts = np.stack([syn.default_gt_pose(rng, c) for c in [(-0.12, 0.0, 0.8), (0.0, 0.05, 0.85), (0.13, -0.03, 0.75)]])
    sc = syn.make_scene(NAMES, gts, oracle_render_fn, rng=rng)
    if write:
        _write_pose_lists(root, NAMES, gts, rng)
    bank = {n: ModelMetaData(n, model=sc.bank.models[i]) for i, n in enumerate(NAMES)}
    cam = CameraIntrinsics(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy)
    rec = ObjectRecognizer(bank, cam, PerchParams(icp_type=icp_type, icp_top_k=top_k))
    inp = RecognitionInput(NAMES, sc.depth_raw, sc.mask, depth_factor=sc.depth_factor, rendered_root_dir=root, use_icp=1)
    return rec, inp


def _summary(rec, res):
    """Everything a search returns and keeps, as plain arrays (compared byte for byte between runs)."""
    return dict(indices=np.array(res.indices, np.int64), costs=np.array(res.costs, np.int64),
                poses=np.array(res.detected_poses, np.float64).reshape(-1, 7),
                transforms=np.array(res.object_transforms, np.float64).reshape(-1, 16),
                shortlist=rec.last_shortlist.cpu().numpy(), names=list(res.model_names))


@pytest.mark.parametrize("icp_type", [3, 4])
def test_recognizer_staged_equals_the_numpy_construction(tmp_path, icp_type):
    K = 8
    rec, inp = _recognizer_case(str(tmp_path), icp_type, K)
    res = rec.localize_objects_greedy_render(inp)
    rc, oc, df = rec._last_costs
    p, M = rec.params, 3
    states = rec.generate_successor_states(inp)
    n = len(states)
    poses = rec._poses_device(states)
    pm = torch.from_numpy(states.model.copy()).to(poses.device)
    args = (poses, pm, rec._pose_labels(states), torch.from_numpy(rec._obs_totals(states)).to(poses.device))
    kw = dict(cost_type=rec._cost_type(), stride=p.gpu_stride, depth_factor=p.gpu_depth_factor,
              sensor_resolution=p.sensor_resolution, occlusion_threshold=p.gpu_occlusion_threshold)
    pre = rec.core.evaluate(*args, **kw)
    full = (rec.core.evaluate_icp if icp_type == 3 else rec.core.evaluate_p2p)(*args, **kw)[:5]
    pmh = states.model
    pre_keys = ref.select_keys(pre[0].cpu().numpy(), pre[1].cpu().numpy(), pmh, M)
    post_keys = ref.select_keys(full[2].cpu().numpy(), full[3].cpu().numpy(), pmh, M)
    S, want = expected_keys(pre_keys, post_keys, pmh, M, K)
    assert np.array_equal(rec.last_shortlist.cpu().numpy(), S)
    from perception_amd.core import decode_keys

    cost, idx = decode_keys(want)
    found = idx >= 0
    assert found.all()
    assert res.indices == [int(i) for i in idx] and res.costs == [int(c) for c in cost]
    adj = full[0].cpu().numpy()
    conts = rec.adjusted_cont_poses(adj[idx], np.arange(M, dtype=np.int32), inp.use_external_pose_list)
    assert np.array_equal(np.array(res.detected_poses), conts)
    # the kept costs: post-ICP at the refined rows, pre-ICP everywhere else
    members = np.unique(S[S != ref.KEY_NONE] & 0x7FFFFFFF)
    rest = np.setdiff1d(np.arange(n), members)
    for got, after, before in zip((rc, oc, df), full[2:], pre):
        assert np.array_equal(_bits(got)[members], _bits(after)[members])
        assert np.array_equal(_bits(got)[rest], _bits(before)[rest])
    assert rec.last_stats.scenes_rendered == n
    assert (rec.last_stats.icp_time > 0) == (icp_type == 3)


def test_icp_top_k_is_refused_where_it_cannot_run(tmp_path):
    rec, inp = _recognizer_case(str(tmp_path), 0, 8)
    with pytest.raises(ValueError):
        rec.localize_objects_greedy_render(inp)
    for bad in (-1, 65):
        rec.params.icp_type, rec.params.icp_top_k = 3, bad
        with pytest.raises(ValueError):
            rec.localize_objects_greedy_render(inp)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, root, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch
    import torch.distributed as dist

    from perception_amd.distributed import init_from_env, shard_range

    torch.cuda.set_device(0)
    init_from_env("gloo")
    rec, inp = _recognizer_case(root, 3, 8, write=False)
    res = rec.localize_objects_greedy_render(inp)
    out = _summary(rec, res)
    out["shard"] = shard_range(rec.last_stats.scenes_rendered, rank, world)
    q.put((rank, out))
    dist.destroy_process_group()


def test_gloo_world2_staged_search_equals_one_process(tmp_path):
    """Two gloo ranks on cuda:0 (spawned children), each with half of the states: the shortlists meet in
    allgather_topk_keys, each rank refines the members of its shard, and the result equals the one-process staged
    search byte for byte.  The boundary lies inside the second model's states, whose shortlist has members on both
    sides of it."""
    root = str(tmp_path)
    rec, inp = _recognizer_case(root, 3, 8)
    one = _summary(rec, rec.localize_objects_greedy_render(inp))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, root, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    boundary = res[0][1]["shard"][1]
    assert res[1][1]["shard"][0] == boundary
    idx = one["shortlist"][one["shortlist"] != ref.KEY_NONE] & 0x7FFFFFFF
    straddles = [m for m in range(3) if len({bool(i < boundary) for i in
                                             (one["shortlist"][m][one["shortlist"][m] != ref.KEY_NONE] & 0x7FFFFFFF)}) == 2]
    assert straddles, (boundary, sorted(idx))
    for _, got in res:
        assert got["names"] == one["names"]
        for k in ("indices", "costs", "poses", "transforms", "shortlist"):
            assert got[k].tobytes() == one[k].tobytes(), k
