"""The staged search (a build extension; INTEGRATION.md "Staged search"): score every candidate without ICP, refine only
the k best per model, select among the refined.  The reference refines every candidate (renderer.cu:1688-1817) and
tracks the pre-ICP ranking beside the post-ICP one (lowest_preicp_cost_per_object, search_env.cpp:2567-2572); the
shortlist acts on that ranking.  A candidate the pre-ICP selection filters out is never refined.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._native import PCORE_KEY_NONE
from .core import PoseCore, decode_keys
from .distributed import allgather_topk_keys

ICP_GICP, ICP_P2P, ICP_P2P_NN = 3, 4, 5  # perch_params icp_type


def shortlist_members(topk, lo: int, hi: int) -> np.ndarray:
    """The shortlist's global indices (an (M, k) key tensor) that lie in [lo, hi), ascending, as shard-local indices."""
    _, idx = decode_keys(topk)
    return (np.unique(idx[(idx >= lo) & (idx < hi)]) - lo).astype(np.int64)


def refine_shortlist(core: PoseCore, members: np.ndarray, poses: torch.Tensor, pose_model: torch.Tensor,
                     pose_label: Optional[torch.Tensor], pose_obs_total: torch.Tensor, icp_type: int, eval_kw: dict,
                     icp_kw: dict):
    """ICP (icp_type 3: evaluate_icp, 4: evaluate_p2p, 5: evaluate_p2p with scene="nn") and re-scoring of the rows `members` of a shard ->
    (sub, adjusted poses, iterations, rc, oc, diff) of those rows, or None when there is none (no call is made).  A
    pose's result does not depend on the batch it is refined in."""
    if len(members) == 0:
        return None
    sub = torch.from_numpy(np.asarray(members, np.int64)).to(poses.device)
    args = (poses[sub].contiguous(), pose_model[sub].contiguous(),
            None if pose_label is None else pose_label[sub].contiguous(), pose_obs_total[sub].contiguous())
    if icp_type == ICP_GICP:
        a, it, r, o, d = core.evaluate_icp(*args, **eval_kw, **icp_kw)
    elif icp_type == ICP_P2P:
        a, it, r, o, d, _, _ = core.evaluate_p2p(*args, **eval_kw, **icp_kw)
    elif icp_type == ICP_P2P_NN:
        a, it, r, o, d, _, _ = core.evaluate_p2p(*args, **eval_kw, **{**icp_kw, "scene": "nn"})
    else:
        raise ValueError(f"the staged search refines with icp_type 3, 4 or 5, got {icp_type}")
    return sub, a, it, r, o, d


def select_refined(core: PoseCore, refined, pose_model: torch.Tensor, num_models: int, index_base: int,
                   keys: torch.Tensor) -> torch.Tensor:
    """The existing selection over the refined rows only: their post-ICP costs scattered into arrays that hold -1 (the
    reference's invalid cost, which the key excludes) elsewhere, folded into `keys`."""
    if refined is None:
        return keys
    sub, _, _, r, o, _ = refined
    n = int(pose_model.shape[0])
    sel_rc = torch.full((n,), -1.0, dtype=torch.float32, device=pose_model.device)
    sel_oc = torch.full_like(sel_rc, -1.0)
    sel_rc[sub], sel_oc[sub] = r, o
    return core.select(sel_rc, sel_oc, pose_model, num_models, index_base=index_base, keys=keys)


def staged_step(core: PoseCore, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor],
                pose_obs_total: torch.Tensor, num_models: int, k: int, index_base: int = 0, icp_type: int = ICP_GICP,
                eval_kw: Optional[dict] = None, icp_kw: Optional[dict] = None):
    """One staged search over a batch: evaluate, select_topk (exchanged between ranks when an exchange is active),
    ICP of the shortlist members of this batch, select among them.  Returns (keys, shortlist, refined, pre): the
    per-model keys of this batch (not yet reduced across ranks), the (M, k) pre-ICP shortlist, refine_shortlist's
    result and the pre-ICP (rc, oc, diff)."""
    eval_kw, icp_kw = eval_kw or {}, icp_kw or {}
    n = int(poses.shape[0])
    pre = core.evaluate(poses, pose_model, pose_label, pose_obs_total, **eval_kw)
    topk = core.select_topk(pre[0], pre[1], pose_model, num_models, k, index_base=index_base)
    topk = allgather_topk_keys(topk)
    members = shortlist_members(topk, index_base, index_base + n)
    refined = refine_shortlist(core, members, poses, pose_model, pose_label, pose_obs_total, icp_type, eval_kw, icp_kw)
    keys = torch.full((num_models,), PCORE_KEY_NONE, dtype=torch.int64, device=poses.device)
    select_refined(core, refined, pose_model, num_models, index_base, keys)
    return keys, topk, refined, pre
