#!/usr/bin/env python
"""How short may the staged search's shortlist be?  On C3's workload (5 objects x 10k poses) and on the two scan-like
meshes of synthetic.SCAN_MESHES (with the box, C3scan's bank), one full pre-ICP evaluate and one full evaluate_icp give,
per model and for K = 1 .. 64:
  - whether the full flow's winning index is in the pre-ICP top-K (its pre-ICP rank, 1-based; null: filtered out
    before ICP or beyond 64), and
  - the staged winner's post-ICP cost (the minimum over the pre-ICP top-K of the post-ICP keys) against the full
    winner's.
The scenes are synthetic proxies (primitive YCB stand-ins and noise meshes, rendered observations): the figures say how
the ranking behaves on them, not on real scans.  One JSON line per workload.

  tools/topk_recall.py [--scale 1.0] [--out profiles/topk_recall.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from perception_amd import workloads  # noqa: E402
from perception_amd._native import PCORE_KEY_NONE, PCORE_TOPK_MAX  # noqa: E402
from perception_amd.core import decode_keys  # noqa: E402

C3_NAMES = ["003_cracker_box", "005_tomato_soup_can", "006_mustard_bottle", "010_potted_meat_can", "024_bowl"]
SCAN_NAMES = ["scan_blob", "scan_shell", "003_cracker_box"]


def recall(name, names, per_model):
    w = workloads.build(names=names, poses_per_model=per_model)
    M, K = w.num_models, PCORE_TOPK_MAX
    args = (w.poses, w.pose_model, w.pose_label, w.pose_obs_total)
    pre = w.core.evaluate(*args, stride=w.stride)
    short = w.core.select_topk(pre[0], pre[1], w.pose_model, M, K).cpu().numpy()
    full = w.core.evaluate_icp(*args, stride=w.stride)
    full_keys = w.core.select(full[2], full[3], w.pose_model, M)
    full_cost, full_idx = decode_keys(full_keys)
    # every pose's post-ICP key, by the selection itself: one model per pose, so that no minimum is taken
    n = int(w.poses.shape[0])
    own = torch.arange(n, dtype=torch.int32, device=w.poses.device)
    post = w.core.select(full[2], full[3], own, n).cpu().numpy()
    models = []
    for m in range(M):
        row = short[m][short[m] != PCORE_KEY_NONE]
        idx = row & 0x7FFFFFFF
        pre_cost, _ = decode_keys(row)
        hit = np.nonzero(idx == full_idx[m])[0]
        best = np.minimum.accumulate(post[idx]) if len(idx) else np.zeros(0, np.int64)
        staged_cost, staged_idx = decode_keys(best)
        models.append({
            "model": names[m], "gt_index": int(w.gt_index[m]), "full_winner_index": int(full_idx[m]),
            "full_winner_cost": int(full_cost[m]), "shortlist_len": int(len(idx)),
            "full_winner_pre_icp_rank": int(hit[0]) + 1 if len(hit) else None,
            "pre_icp_cost_of_rank": [int(c) for c in pre_cost],
            # entry K - 1: the staged search's winner with a shortlist of K (INT_MAX / -1: none survives the filter)
            "staged_winner_cost": [int(c) for c in staged_cost], "staged_winner_index": [int(i) for i in staged_idx],
            "smallest_k_same_winner": next((k + 1 for k, i in enumerate(staged_idx) if i == full_idx[m]), None),
            "smallest_k_same_cost": next((k + 1 for k, c in enumerate(staged_cost) if c <= full_cost[m]), None)})
    res = {"workload": name, "poses": n, "models": M, "k_max": K, "synthetic_proxy_scene": True, "per_model": models}
    del w
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 10k poses per model")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    per_model = max(64, int(10000 * a.scale))
    for name, names in (("C3", C3_NAMES), ("C3:scan", SCAN_NAMES)):
        line = json.dumps(recall(name, names, per_model))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
