#!/usr/bin/env python
"""Time the BASELINE.json configs other than the headline one on ONE GPU (per-GPU shares of the
multi-GPU configs).  Prints one JSON line per config.  Not the driver's bench (bench.py is).

  C1  1 mesh, 128 3-DoF table-top poses, render + GICP + re-render + score (cost type 0), 640x480 -- the GPU
      side of the workload bench.py's cpu_reference_path times on the reference's CPU/OMP path
  c1_planar  C1's scene and grid scaled to 20,000 states: the planar (x, y, yaw) ICP stage, the two-pass 3-DoF search
      and GICP on the same states (not in the default list: --configs c1_planar)
  c1_p2p  the same 20,000 states: the point-to-plane projective ICP stage beside the planar ICP stage and GICP
  c3_p2p  C3's batch through evaluate_p2p (point-to-plane ICP + re-score) beside evaluate_icp (GICP + re-score)
  c1_nn   c1_p2p's states through the nearest-neighbour scene's ICP stage beside the projective stage and GICP
  c3_nn   C3's batch through evaluate_p2p(scene="nn") beside the projective scene and GICP; the staged step at K = 16
  c3_topk  C3's batch through the staged search (evaluate + select_topk + evaluate_icp on the K best per model + select)
      for K = 1, 4, 16, 64 beside the full evaluate_icp + select
  C2  1 mesh, 10k poses, render + score, 640x480
  C3  5 objects, 50k poses, render + GICP + re-render + score, 640x480 (+ argmin vs GT)
  C4  21 objects, 200k poses over 8 GPUs -> 25k poses per GPU, render + score
  C5  1 mesh, 1M poses at 1280x720 over 8 GPUs -> 125k poses per GPU, render + score
  C2scan_blob / C2scan_shell  C2 on a scan-like irregular mesh; C3scan  C3's flow on two scan meshes + the box
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from perception_amd import metrics  # noqa: E402
from perception_amd import synthetic as syn  # noqa: E402
from perception_amd import workloads  # noqa: E402
from perception_amd.model import to_eigen  # noqa: E402
from perception_amd._native import PCORE_KEY_NONE  # noqa: E402
from perception_amd.core import decode_keys  # noqa: E402

C3_NAMES = ["003_cracker_box", "005_tomato_soup_can", "006_mustard_bottle", "010_potted_meat_can", "024_bowl"]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def run(name, names, per_model, cam, icp, steps, warmup):
    w = workloads.build(names=names, poses_per_model=per_model, cam=cam)
    n = int(w.poses.shape[0])
    dev = w.poses.device
    keys = torch.full((w.num_models,), PCORE_KEY_NONE, dtype=torch.int64, device=dev)
    if icp:
        out = (torch.empty((n, 16), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               *(torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)))

        def step():
            keys.fill_(PCORE_KEY_NONE)
            adj, it, rc, oc, df = w.core.evaluate_icp(w.poses, w.pose_model, w.pose_label, w.pose_obs_total,
                                                      stride=w.stride, out=out)
            w.core.select(rc, oc, w.pose_model, w.num_models, keys=keys)
    else:
        out = tuple(torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))

        def step():
            keys.fill_(PCORE_KEY_NONE)
            workloads.step(w, out, keys)
    dt = timed(step, steps, warmup)
    cost, idx = decode_keys(keys)
    res = {"config": name, "poses": n, "models": w.num_models, "width": w.scene.width, "height": w.scene.height,
           "triangles": [int(c) for c in w.scene.bank.tris_model_count], "icp": icp, "s_per_step": dt, "poses_per_s": n / dt,
           "argmin_index": [int(i) for i in idx], "gt_index": [int(i) for i in w.gt_index],
           "argmin_cost": [int(c) for c in cost]}
    if icp:
        it = out[1].float()
        res["gicp_iters_mean"] = float(it.mean().item())
        res["gicp_iters_max"] = int(it.max().item())
        itn = out[1].cpu().numpy()
        edges = [1, 2, 5, 10, 20, 50, 100, 149, 150]
        res["gicp_iters_hist"] = {f"<={e}": int((itn <= e).sum()) for e in edges}
        res["gicp_iters_at_max"] = int((itn >= 150).sum())
        res["gicp_iters_p50_p90"] = [float(np.percentile(itn, 50)), float(np.percentile(itn, 90))]
    # pose accuracy of the selected poses against the synthetic ground truth (f3 metrics, on the GPU)
    final = (out[0] if icp else w.poses).cpu().numpy()
    errs_add, errs_adds = [], []
    for m in range(w.num_models):
        if idx[m] < 0:
            errs_add.append(np.inf)
            errs_adds.append(np.inf)
            continue
        est = to_eigen(final[idx[m]]).astype(np.float64)
        pts = np.unique(w.scene.bank.models[m].tris.reshape(-1, 3), axis=0)
        a, s_ = metrics.pose_distances(w.core, pts, w.scene.gt_poses[m][None], est[None])
        errs_add.append(float(a[0]))
        errs_adds.append(float(s_[0]))
    res["add_m"] = errs_add
    res["adds_m"] = errs_adds
    # the ground-truth candidates' own final costs (search_env.cpp:2022-2048 int conversion and filter), to explain a
    # winner other than the ground truth: a symmetric proxy (cylinder) renders the same at other yaws (ADD-S ~ 0)
    rcs, ocs = out[-3].cpu().numpy() if icp else out[0].cpu().numpy(), out[-2].cpu().numpy() if icp else out[1].cpu().numpy()
    gt_cost = []
    for g in w.gt_index:
        r, o = float(rcs[g]), float(ocs[g])
        gt_cost.append({"cost": int(np.float32(r) + np.float32(o)) if r >= 0 else -1, "rc": r, "oc": o,
                        "passes_filter": bool(r >= 0 and abs(int(r) - int(o)) < 30)})
    res["gt_candidate"] = gt_cost
    res["shapes"] = [syn.YCB_PROXIES[nm][0] if nm in syn.YCB_PROXIES else "?" for nm in names]
    res["adds_auc"] = metrics.compute_pose_metrics(np.array(errs_adds))["auc"]
    print(json.dumps(res), flush=True)
    del w
    torch.cuda.empty_cache()


def run_c1(steps, warmup, stride=4):
    """C1 on the GPU: the 128 3-DoF poses of workloads.c1_tabletop, scored against the whole observed cloud
    (3-DoF, no labels), with and without GICP."""
    from perception_amd.core import PoseCore
    from perception_amd.model import compute_proj
    dev = torch.device("cuda", 0)
    bank = syn.model_bank(["003_cracker_box"])
    core = PoseCore(0)
    core.upload_meshes(bank.tris, bank.tris_model_count)
    cam = syn.CAM_640
    core.set_camera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                    compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"]))
    W, H = cam["width"], cam["height"]
    core.set_observation(torch.zeros((H, W), dtype=torch.int32, device=dev), None,
                         torch.zeros((0, 3), dtype=torch.float32, device=dev), None, 0.01)
    c1 = workloads.c1_tabletop(workloads.gpu_render_fn(core, dev))
    sc = c1.scene
    xyz, _ = core.observed_cloud_bounded(torch.from_numpy(sc.depth_raw).to(dev), stride, sc.depth_factor)
    core.set_observation(torch.from_numpy(c1.src_depth_cm).to(dev), None, xyz, None, 0.0075)
    n = len(c1.poses)
    poses = torch.from_numpy(c1.poses).to(dev)
    pm = torch.zeros(n, dtype=torch.int32, device=dev)
    tot = torch.full((n,), float(xyz.shape[0]), dtype=torch.float32, device=dev)
    for icp in (False, True):
        if icp:
            fn = lambda: core.evaluate_icp(poses, pm, None, tot, cost_type=0, stride=stride,  # noqa: E731
                                           sensor_resolution=0.0075)
        else:
            fn = lambda: core.evaluate(poses, pm, None, tot, cost_type=0, stride=stride,  # noqa: E731
                                       sensor_resolution=0.0075)
        dt = timed(fn, steps, warmup)
        print(json.dumps({"config": "C1", "poses": n, "models": 1, "width": W, "height": H, "stride": stride,
                          "icp": icp, "s_per_step": dt, "poses_per_s": n / dt, "observed_points": int(xyz.shape[0])}),
              flush=True)
    # the launch-bound render + score as a captured HIP graph (PoseCore.capture_evaluate)
    replay, _ = core.capture_evaluate(poses, pm, None, tot, cost_type=0, stride=stride, sensor_resolution=0.0075)
    dt = timed(replay, steps, warmup)
    print(json.dumps({"config": "C1", "poses": n, "models": 1, "width": W, "height": H, "stride": stride,
                      "icp": False, "graph": True, "s_per_step": dt, "poses_per_s": n / dt,
                      "observed_points": int(xyz.shape[0])}), flush=True)


def c1_grid(nxy, stride):
    """C1's table-top scene with its observation set, and C1's 4 x 4 cells of 4 cm around the ground truth cut into
    nxy x nxy positions with its 8 yaws: the states of c1_planar and c1_p2p."""
    from perception_amd.core import PoseCore
    from perception_amd.model import compute_proj
    from perception_amd.recognizer import preprocessing_transform
    from perception_amd.tabletop import planar_adjusted_states, pose_in_cam_3dof
    dev = torch.device("cuda", 0)
    bank = syn.model_bank(["003_cracker_box"])
    pre = [preprocessing_transform(bank.models[0], six_dof=False)]
    core = PoseCore(0)
    core.upload_meshes(bank.tris, bank.tris_model_count)
    cam = syn.CAM_640
    W, H = cam["width"], cam["height"]
    core.set_camera(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                    compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H))
    core.set_observation(torch.zeros((H, W), dtype=torch.int32, device=dev), None,
                         torch.zeros((0, 3), dtype=torch.float32, device=dev), None, 0.01)
    c1 = workloads.c1_tabletop(workloads.gpu_render_fn(core, dev))
    sc = c1.scene
    xyz, _ = core.observed_cloud_bounded(torch.from_numpy(sc.depth_raw).to(dev), stride, sc.depth_factor)
    core.set_observation(torch.from_numpy(c1.src_depth_cm).to(dev), None, xyz, None, 0.0075)
    # C1's 4 x 4 cells of 4 cm around the ground truth, cut into nxy x nxy positions; its 8 yaws
    gx, gy = 0.60, -0.04
    xs = gx - 0.08 + 0.16 * (np.arange(nxy) + 0.5) / nxy
    ys = gy - 0.08 + 0.16 * (np.arange(nxy) + 0.5) / nxy
    X, Y, K = np.meshgrid(xs, ys, np.arange(8), indexing="ij")
    states = np.stack([X.ravel(), Y.ravel(), np.full(X.size, sc.table_height), K.ravel() * np.pi / 4], 1)
    n = len(states)
    model0 = np.zeros(n, np.int32)
    M = (sc.camera_pose @ syn.CAM_TO_BODY).astype(np.float32)
    poses = torch.from_numpy(pose_in_cam_3dof(sc.camera_pose, pre, model0, states)).to(dev)
    pm = torch.zeros(n, dtype=torch.int32, device=dev)
    tot = torch.full((n,), float(xyz.shape[0]), dtype=torch.float32, device=dev)
    return dict(core=core, sc=sc, pre=pre, xyz=xyz, states=states, model0=model0, M=M, poses=poses, pm=pm, tot=tot,
                n=n, W=W, H=H, dev=dev)


def run_c1_planar(nxy=50, stride=4, runs=5, host_poses=16):
    """c1_planar: C1's table-top scene and grid scaled to nxy x nxy x 8 states (20,000), refined by the planar
    (x, y, yaw) ICP.  Reports the planar stage alone (PoseCore.icp_planar), the two-pass search (planar ICP, the host
    pose update and pose rebuild, stage COST with the selection) and, as the yardstick, the only refinement the library
    had for these states before: evaluate_icp (GICP) at 3-DoF on the same context -- `runs` alternating runs each,
    medians.  For context also the numpy restatement of the spec (tests/icp2d_reference.py) on host_poses poses, one
    thread each, in the place of the reference's OpenMP loop."""
    from perception_amd.tabletop import planar_adjusted_states, pose_in_cam_3dof
    g = c1_grid(nxy, stride)
    core, sc, pre, xyz, states, model0, M = (g[k] for k in ("core", "sc", "pre", "xyz", "states", "model0", "M"))
    poses, pm, tot, n, W, H, dev = (g[k] for k in ("poses", "pm", "tot", "n", "W", "H", "dev"))
    keys = torch.full((1,), PCORE_KEY_NONE, dtype=torch.int64, device=dev)
    out_p = None

    def planar():
        nonlocal out_p
        out_p = core.icp_planar(poses, pm, M, stride=stride, out=out_p)

    def two_pass():
        planar()
        adj = planar_adjusted_states(states, out_p[0].cpu().numpy(), out_p[2].cpu().numpy())
        p2 = torch.from_numpy(pose_in_cam_3dof(sc.camera_pose, pre, model0, adj)).to(dev)
        keys.fill_(PCORE_KEY_NONE)
        core.evaluate(p2, pm, None, tot, cost_type=0, stride=stride, sensor_resolution=0.0075, select=(keys, 0, 1))

    def gicp():
        core.evaluate_icp(poses, pm, None, tot, cost_type=0, stride=stride, sensor_resolution=0.0075)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for fn in (planar, two_pass, gicp):  # warm-up: scratch, grids, target covariances
        once(fn)
    t = {"planar": [], "two_pass": [], "gicp": []}
    gicp_stage = []
    for _ in range(runs):  # alternating
        t["planar"].append(once(planar))
        t["gicp"].append(once(gicp))
        gicp_stage.append(float(core.stats()["icp_runtime"]))
        t["two_pass"].append(once(two_pass))
    med = {k: float(np.median(v)) for k, v in t.items()}
    status = out_p[2].cpu().numpy()
    iters = out_p[1].cpu().numpy()
    res = {"config": "c1_planar", "poses": n, "width": W, "height": H, "stride": stride,
           "observed_points": int(xyz.shape[0]), "runs": runs,
           "planar_s": med["planar"], "planar_poses_per_s": n / med["planar"],
           "two_pass_s": med["two_pass"], "two_pass_poses_per_s": n / med["two_pass"],
           "gicp_call_s": med["gicp"], "gicp_call_poses_per_s": n / med["gicp"],
           "gicp_stage_s": float(np.median(gicp_stage)),
           "planar_s_all": t["planar"], "gicp_call_s_all": t["gicp"], "two_pass_s_all": t["two_pass"],
           "status_counts": [int(v) for v in np.bincount(status, minlength=6)],
           "iters_mean": float(iters.mean()), "iters_at_cap": int((iters >= 20).sum())}
    if host_poses > 0:
        from tests import icp2d_reference as ref
        zb = core.render(poses[:host_poses].contiguous(), pm[:host_poses].contiguous(), None).cpu().numpy()
        import oracle
        pts, pidx, _ = oracle.depth_to_cloud(zb, stride, sc.cx, sc.cy, sc.fx, sc.fy, 100.0)
        clouds = [pts[pidx == i] for i in range(host_poses)]
        obs = xyz.cpu().numpy()
        t0 = time.perf_counter()
        h = ref.run_poses(clouds, obs, M, threads=16)
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(h[0].view(np.uint64), out_p[0][:host_poses].cpu().numpy().view(np.uint64)))
        res.update({"host_numpy_poses": host_poses, "host_numpy_threads": 16, "host_numpy_s": dt,
                    "host_numpy_poses_per_s": host_poses / dt, "host_numpy_bit_equal": same})
    print(json.dumps(res), flush=True)


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_c1_p2p(nxy=50, stride=4, runs=5):
    """c1_p2p: the point-to-plane projective ICP stage (PoseCore.icp_point2plane) on c1_planar's 20,000 states, beside
    the planar ICP stage and GICP (the evaluate_icp call and its GICP stage alone) on the same context -- `runs`
    alternating runs each after one warm-up, medians."""
    g = c1_grid(nxy, stride)
    core, poses, pm, tot, M, n = (g[k] for k in ("core", "poses", "pm", "tot", "M", "n"))
    out = {"p2p": None, "planar": None}

    def p2p():
        out["p2p"] = core.icp_point2plane(poses, pm, None, cost_type=0, stride=stride, out=out["p2p"])

    def planar():
        out["planar"] = core.icp_planar(poses, pm, M, stride=stride, out=out["planar"])

    def gicp():
        core.evaluate_icp(poses, pm, None, tot, cost_type=0, stride=stride, sensor_resolution=0.0075)

    for fn in (p2p, planar, gicp):  # warm-up: scratch, the scene, grids, target covariances
        _once(fn)
    t = {"p2p": [], "planar": [], "gicp": []}
    gicp_stage = []
    for _ in range(runs):  # alternating
        t["p2p"].append(_once(p2p))
        t["planar"].append(_once(planar))
        t["gicp"].append(_once(gicp))
        gicp_stage.append(float(core.stats()["icp_runtime"]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    _, fit, rmse, iters = (x.cpu().numpy() for x in out["p2p"])
    print(json.dumps({"config": "c1_p2p", "poses": n, "width": g["W"], "height": g["H"], "stride": stride, "runs": runs,
                      "p2p_s": med["p2p"], "p2p_poses_per_s": n / med["p2p"],
                      "planar_s": med["planar"], "planar_poses_per_s": n / med["planar"],
                      "gicp_call_s": med["gicp"], "gicp_call_poses_per_s": n / med["gicp"],
                      "gicp_stage_s": float(np.median(gicp_stage)),
                      "p2p_s_all": t["p2p"], "planar_s_all": t["planar"], "gicp_call_s_all": t["gicp"],
                      "iters_mean": float(iters.mean()), "iters_at_cap": int((iters >= 30).sum()),
                      "fitness_mean": float(fit.mean()), "rmse_mean": float(rmse.mean())}), flush=True)


def run_c3_p2p(per_model=10000, runs=5):
    """c3_p2p: C3's batch (5 objects, 50k 6-DoF poses) through evaluate_p2p (point-to-plane ICP + re-score) and through
    evaluate_icp (GICP + re-score) on the same context -- `runs` alternating runs each after one warm-up, medians; the
    point-to-plane stage alone too."""
    w = workloads.build(names=C3_NAMES, poses_per_model=per_model, cam=syn.CAM_640)
    n = int(w.poses.shape[0])
    res = {}

    def p2p():
        res["p2p"] = w.core.evaluate_p2p(w.poses, w.pose_model, w.pose_label, w.pose_obs_total, stride=w.stride)

    def p2p_stage():
        w.core.icp_point2plane(w.poses, w.pose_model, w.pose_label, stride=w.stride)

    def gicp():
        res["gicp"] = w.core.evaluate_icp(w.poses, w.pose_model, w.pose_label, w.pose_obs_total, stride=w.stride)

    for fn in (p2p, p2p_stage, gicp):
        _once(fn)
    t = {"p2p": [], "p2p_stage": [], "gicp": []}
    gicp_stage = []
    for _ in range(runs):  # alternating
        t["p2p"].append(_once(p2p))
        t["p2p_stage"].append(_once(p2p_stage))
        t["gicp"].append(_once(gicp))
        gicp_stage.append(float(w.core.stats()["icp_runtime"]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    iters = res["p2p"][1].cpu().numpy()
    print(json.dumps({"config": "c3_p2p", "poses": n, "models": w.num_models, "stride": w.stride, "runs": runs,
                      "evaluate_p2p_s": med["p2p"], "evaluate_p2p_poses_per_s": n / med["p2p"],
                      "p2p_stage_s": med["p2p_stage"], "evaluate_icp_s": med["gicp"],
                      "evaluate_icp_poses_per_s": n / med["gicp"], "gicp_stage_s": float(np.median(gicp_stage)),
                      "evaluate_p2p_s_all": t["p2p"], "p2p_stage_s_all": t["p2p_stage"], "evaluate_icp_s_all": t["gicp"],
                      "p2p_iters_mean": float(iters.mean()), "p2p_iters_at_cap": int((iters >= 30).sum()),
                      "gicp_iters_mean": float(res["gicp"][1].float().mean().item())}), flush=True)


def run_c1_nn(nxy=50, stride=4, runs=5):
    """c1_nn: the point-to-plane ICP against the nearest-neighbour scene (icp_point2plane(scene="nn"), the defaults:
    radius 0.01 m, window 32) on c1_planar's 20,000 states, beside the projective stage and GICP on the same context
    -- `runs` alternating runs each after one warm-up, medians and every run."""
    g = c1_grid(nxy, stride)
    core, poses, pm, tot, M, n = (g[k] for k in ("core", "poses", "pm", "tot", "M", "n"))
    out = {"nn": None, "p2p": None}

    def nn():
        out["nn"] = core.icp_point2plane(poses, pm, None, cost_type=0, stride=stride, out=out["nn"], scene="nn")

    def p2p():
        out["p2p"] = core.icp_point2plane(poses, pm, None, cost_type=0, stride=stride, out=out["p2p"])

    def gicp():
        core.evaluate_icp(poses, pm, None, tot, cost_type=0, stride=stride, sensor_resolution=0.0075)

    fns = {"nn": nn, "p2p": p2p, "gicp": gicp}
    for fn in fns.values():  # warm-up: scratch, the scene, grids, target covariances
        _once(fn)
    t = {k: [] for k in fns}
    gicp_stage = []
    for _ in range(runs):  # alternating
        for k, fn in fns.items():
            t[k].append(_once(fn))
        gicp_stage.append(float(core.stats()["icp_runtime"]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    _, fit, rmse, iters = (x.cpu().numpy() for x in out["nn"])
    _, pfit, _, piters = (x.cpu().numpy() for x in out["p2p"])
    print(json.dumps({"config": "c1_nn", "poses": n, "width": g["W"], "height": g["H"], "stride": stride, "runs": runs,
                      "max_dist_diff": 0.01, "window": 32,
                      "nn_s": med["nn"], "nn_poses_per_s": n / med["nn"], "p2p_s": med["p2p"],
                      "gicp_call_s": med["gicp"], "gicp_stage_s": float(np.median(gicp_stage)),
                      "nn_s_all": t["nn"], "p2p_s_all": t["p2p"], "gicp_call_s_all": t["gicp"],
                      "nn_iters_mean": float(iters.mean()), "nn_iters_at_cap": int((iters >= 30).sum()),
                      "nn_fitness_mean": float(fit.mean()), "nn_rmse_mean": float(rmse.mean()),
                      "p2p_iters_mean": float(piters.mean()), "p2p_fitness_mean": float(pfit.mean())}), flush=True)


def run_c3_nn(per_model=10000, runs=5, k=16):
    """c3_nn: C3's batch (5 objects, 50k 6-DoF poses) through evaluate_p2p(scene="nn") (the defaults: radius 0.01 m,
    window 32), beside evaluate_p2p (the projective scene) and evaluate_icp (GICP) on the same context, the two
    point-to-plane stages alone, and the staged search at K = `k` with icp_type 5 -- `runs` alternating runs each
    after one warm-up, medians and every run."""
    from perception_amd.staged import ICP_P2P_NN, staged_step
    w = workloads.build(names=C3_NAMES, poses_per_model=per_model, cam=syn.CAM_640)
    n = int(w.poses.shape[0])
    args = (w.poses, w.pose_model, w.pose_label, w.pose_obs_total)
    res = {}

    def nn():
        res["nn"] = w.core.evaluate_p2p(*args, stride=w.stride, scene="nn")

    def nn_stage():
        res["nn_stage"] = w.core.icp_point2plane(*args[:3], stride=w.stride, scene="nn")

    def p2p():
        res["p2p"] = w.core.evaluate_p2p(*args, stride=w.stride)

    def p2p_stage():
        res["p2p_stage"] = w.core.icp_point2plane(*args[:3], stride=w.stride)

    def gicp():
        res["gicp"] = w.core.evaluate_icp(*args, stride=w.stride)

    def staged():
        res["staged"] = staged_step(w.core, *args, w.num_models, k, icp_type=ICP_P2P_NN, eval_kw=dict(stride=w.stride))

    fns = {"nn": nn, "nn_stage": nn_stage, "p2p": p2p, "p2p_stage": p2p_stage, "gicp": gicp, "staged": staged}
    for fn in fns.values():
        _once(fn)
    t = {name: [] for name in fns}
    gicp_stage = []
    for _ in range(runs):  # alternating
        for name, fn in fns.items():
            t[name].append(_once(fn))
            if name == "gicp":
                gicp_stage.append(float(w.core.stats()["icp_runtime"]))
    med = {name: float(np.median(v)) for name, v in t.items()}
    _, fit, rmse, iters = (x.cpu().numpy() for x in res["nn_stage"])
    _, pfit, _, piters = (x.cpu().numpy() for x in res["p2p_stage"])
    refined = res["staged"][2]
    print(json.dumps({"config": "c3_nn", "poses": n, "models": w.num_models, "stride": w.stride, "runs": runs,
                      "max_dist_diff": 0.01, "window": 32,
                      "evaluate_nn_s": med["nn"], "evaluate_nn_poses_per_s": n / med["nn"], "nn_stage_s": med["nn_stage"],
                      "evaluate_p2p_s": med["p2p"], "p2p_stage_s": med["p2p_stage"], "evaluate_icp_s": med["gicp"],
                      "gicp_stage_s": float(np.median(gicp_stage)),
                      "staged_k": k, "staged_nn_s": med["staged"],
                      "staged_poses_refined": 0 if refined is None else int(len(refined[0])),
                      "evaluate_nn_s_all": t["nn"], "nn_stage_s_all": t["nn_stage"], "evaluate_p2p_s_all": t["p2p"],
                      "p2p_stage_s_all": t["p2p_stage"], "evaluate_icp_s_all": t["gicp"], "staged_nn_s_all": t["staged"],
                      "nn_iters_mean": float(iters.mean()), "nn_iters_at_cap": int((iters >= 30).sum()),
                      "nn_fitness_mean": float(fit.mean()), "nn_rmse_mean": float(rmse.mean()),
                      "p2p_iters_mean": float(piters.mean()), "p2p_fitness_mean": float(pfit.mean()),
                      "gicp_iters_mean": float(res["gicp"][1].float().mean().item())}), flush=True)


def run_c3_topk(per_model=10000, runs=5, ks=(1, 4, 16, 64)):
    """c3_topk: C3's batch (5 objects, 50k 6-DoF poses) through the staged search (evaluate + select_topk + evaluate_icp
    on the shortlist + select; perception_amd/staged.py) for each K, beside the full evaluate_icp + select on the same
    context in the same job -- `runs` alternating runs each after one warm-up, medians; select_topk alone too."""
    from perception_amd.staged import staged_step
    w = workloads.build(names=C3_NAMES, poses_per_model=per_model, cam=syn.CAM_640)
    n = int(w.poses.shape[0])
    args = (w.poses, w.pose_model, w.pose_label, w.pose_obs_total)
    res = {}

    def full():
        keys = torch.full((w.num_models,), PCORE_KEY_NONE, dtype=torch.int64, device=w.poses.device)
        out = w.core.evaluate_icp(*args, stride=w.stride)
        w.core.select(out[2], out[3], w.pose_model, w.num_models, keys=keys)
        res["full"] = (keys, out)

    def staged(k):
        def fn():
            res[k] = staged_step(w.core, *args, w.num_models, k, eval_kw=dict(stride=w.stride))
        return fn

    pre = w.core.evaluate(*args, stride=w.stride)
    lists = {k: torch.full((w.num_models, k), PCORE_KEY_NONE, dtype=torch.int64, device=w.poses.device) for k in ks}

    def topk_only(k):
        def fn():
            lists[k].fill_(PCORE_KEY_NONE)
            w.core.select_topk(pre[0], pre[1], w.pose_model, w.num_models, k, topk=lists[k])
        return fn

    fns = {"full": full, **{f"staged_{k}": staged(k) for k in ks}, **{f"topk_{k}": topk_only(k) for k in ks}}
    for fn in fns.values():  # warm-up: scratch, grids, target covariances
        _once(fn)
    t = {name: [] for name in fns}
    for _ in range(runs):  # alternating
        for name, fn in fns.items():
            t[name].append(_once(fn))
    med = {name: float(np.median(v)) for name, v in t.items()}
    full_cost, full_idx = decode_keys(res["full"][0])
    out = {"config": "c3_topk", "poses": n, "models": w.num_models, "stride": w.stride, "runs": runs,
           "full_s": med["full"], "full_poses_per_s": n / med["full"], "full_s_all": t["full"],
           "full_argmin_index": [int(i) for i in full_idx], "full_argmin_cost": [int(c) for c in full_cost],
           "gt_index": [int(i) for i in w.gt_index], "staged": []}
    for k in ks:
        keys, _, refined, _ = res[k]
        cost, idx = decode_keys(keys)
        out["staged"].append({"k": k, "s_per_step": med[f"staged_{k}"], "poses_per_s": n / med[f"staged_{k}"],
                              "select_topk_s": med[f"topk_{k}"], "poses_refined": 0 if refined is None else int(len(refined[0])),
                              "full_over_staged": med["full"] / med[f"staged_{k}"], "s_all": t[f"staged_{k}"],
                              "argmin_index": [int(i) for i in idx], "argmin_cost": [int(c) for c in cost],
                              "same_winner_as_full": [bool(a == b) for a, b in zip(idx, full_idx)]})
    print(json.dumps(out), flush=True)


def run_c3_joint(per_model=10000, runs=5, k=16):
    """c3_joint: one sweep of the joint search (perception_amd/joint.py) on C3's batch (5 objects, 50k 6-DoF poses) at
    K = `k`: the evaluate(dbg_zs) call over the shortlisted candidates that feeds the sweep, the evaluate_states call
    over the sweep's S states of M members, and for scale a plain evaluate over the same S x M member poses -- `runs`
    alternating runs each after one warm-up, medians and every run."""
    from perception_amd.joint import state_obs_total, sweep_states
    w = workloads.build(names=C3_NAMES, poses_per_model=per_model, cam=syn.CAM_640)
    n = int(w.poses.shape[0])
    dev = w.poses.device
    rc, oc, _ = w.core.evaluate(w.poses, w.pose_model, w.pose_label, w.pose_obs_total, stride=w.stride)
    _, idx = decode_keys(w.core.select_topk(rc, oc, w.pose_model, w.num_models, k))
    shortlists = np.where(idx >= 0, idx, -1)
    used = np.unique(shortlists[shortlists >= 0])
    compact = {int(c): i for i, c in enumerate(used)}
    sub = torch.from_numpy(used).to(dev)
    poses, pm, pl = w.poses[sub].contiguous(), w.pose_model[sub].contiguous(), w.pose_label[sub].contiguous()
    nsamp = (w.core.width // w.stride) * ((w.core.height + w.stride - 1) // w.stride)
    zs = torch.zeros((len(used), nsamp), dtype=torch.int32, device=dev)
    slot = [0 if shortlists[m][0] >= 0 else -1 for m in range(w.num_models)]
    states, _ = sweep_states(shortlists, slot)
    label_h = w.pose_label.cpu().numpy()
    obs_lab = w.obs_label.cpu().numpy()
    counts = np.bincount(obs_lab[obs_lab >= 0], minlength=w.num_models)
    tot = torch.from_numpy(np.array([state_obs_total(st, label_h, counts) for st in states], np.float32)).to(dev)
    members = [[compact[c] for c in st] for st in states]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)).to(dev)
    mem = torch.from_numpy(np.concatenate(members).astype(np.int32)).to(dev)
    flat = sub[mem.long()]
    fp, fm, fl, ft = (t[flat].contiguous() for t in (w.poses, w.pose_model, w.pose_label, w.pose_obs_total))
    res = {}

    def feed():
        res["feed"] = w.core.evaluate(poses, pm, pl, None, calc_obs_cost=False, stride=w.stride, dbg_zs=zs)

    def states_call():
        res["states"] = w.core.evaluate_states((off, mem), pl, tot, zs=zs, stride=w.stride)

    def plain():
        res["plain"] = w.core.evaluate(fp, fm, fl, ft, stride=w.stride)

    fns = {"feed": feed, "states": states_call, "plain": plain}
    for fn in fns.values():
        _once(fn)
    t = {name: [] for name in fns}
    for _ in range(runs):  # alternating
        for name, fn in fns.items():
            t[name].append(_once(fn))
    med = {name: float(np.median(v)) for name, v in t.items()}
    print(json.dumps({"config": "c3_joint", "poses": n, "models": w.num_models, "stride": w.stride, "runs": runs, "k": k,
                      "shortlisted": int(len(used)), "states": len(states), "members_per_state": len(states[0]),
                      "member_poses": int(mem.shape[0]), "evaluate_dbg_zs_s": med["feed"],
                      "evaluate_states_s": med["states"], "evaluate_member_poses_s": med["plain"],
                      "evaluate_dbg_zs_s_all": t["feed"], "evaluate_states_s_all": t["states"],
                      "evaluate_member_poses_s_all": t["plain"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,C3,C4,C5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the per-GPU pose count")
    a = ap.parse_args()
    sel = a.configs.split(",")
    sc = a.scale
    if "C1" in sel:
        run_c1(max(a.steps, 10), max(a.warmup, 2))
    if "c1_planar" in sel:
        run_c1_planar(nxy=max(2, int(round(50 * sc ** 0.5))))
    if "c1_p2p" in sel:
        run_c1_p2p(nxy=max(2, int(round(50 * sc ** 0.5))))
    if "c3_p2p" in sel:
        run_c3_p2p(per_model=max(1, int(10000 * sc)))
    if "c1_nn" in sel:
        run_c1_nn(nxy=max(2, int(round(50 * sc ** 0.5))))
    if "c3_nn" in sel:
        run_c3_nn(per_model=max(1, int(10000 * sc)))
    if "c3_topk" in sel:
        run_c3_topk(per_model=max(1, int(10000 * sc)))
    if "c3_joint" in sel:
        run_c3_joint(per_model=max(1, int(10000 * sc)))
    if "C2" in sel:
        run("C2", ["003_cracker_box"], int(10000 * sc), syn.CAM_640, False, a.steps, a.warmup)
    if "C3" in sel:
        run("C3", C3_NAMES, int(10000 * sc), syn.CAM_640, True, a.steps, a.warmup)
    if "C4" in sel:
        run("C4/8", list(syn.YCB_PROXIES), int(25000 / 21 * sc), syn.CAM_640, False, a.steps, a.warmup)
    if "C5" in sel:
        run("C5/8", ["003_cracker_box"], int(125000 * sc), syn.CAM_1280, False, a.steps, a.warmup)
    # the scan-like irregular meshes (synthetic.scan_mesh) in C2's and C3's shape
    for nm in ("scan_blob", "scan_shell"):
        if "C2" + nm in sel:
            run("C2:" + nm, [nm], int(10000 * sc), syn.CAM_640, False, a.steps, a.warmup)
    if "C3scan" in sel:
        run("C3:scan", ["scan_blob", "scan_shell", "003_cracker_box"], int(10000 * sc), syn.CAM_640, True, a.steps,
            a.warmup)


if __name__ == "__main__":
    main()
