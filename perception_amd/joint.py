"""Joint search over the per-model shortlists: a deterministic coordinate descent on the cost of the composed state
(PoseCore.evaluate_states; DESIGN.md section 2, "State cost").

The greedy search picks every model's winner alone.  Here the incumbent state takes slot 0 of every model's shortlist
(the greedy winners); one sweep scores every state "incumbent with model m's slot replaced by j", ordered by (m, j), in
one evaluate_states call, takes the lowest selection key among them (PoseCore.select with all states in one group: ties
go to the lowest state index) and adopts that state only if its integer cost is strictly below the incumbent's.  The
integer cost strictly decreases, so the search terminates; it stops at the first sweep that adopts nothing."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _native
from .core import PoseCore, decode_keys

INT_MAX = 2 ** 31 - 1


def state_obs_total(members, cand_label, obs_counts) -> np.float32:
    """The observed points a state has to explain: those whose label is among the members' distinct labels (6-DoF:
    cand_label per candidate, obs_counts per label), or the whole cloud's count (3-DoF: cand_label None, obs_counts a
    number)."""
    if cand_label is None:
        return np.float32(obs_counts)
    cnt = np.asarray(obs_counts)
    labs = sorted({int(cand_label[m]) for m in members})
    return np.float32(sum(int(cnt[L]) for L in labs if 0 <= L < len(cnt)))


def sweep_states(shortlists, slot):
    """The states of one sweep ordered by (m, j) -> (member lists over the candidates, [(m, j)]).  j = slot[m] is the
    incumbent itself."""
    models = [m for m in range(len(shortlists)) if shortlists[m][0] >= 0]
    states, moves = [], []
    for m in models:
        for j in range(len(shortlists[m])):
            if shortlists[m][j] < 0:
                continue
            states.append([int(shortlists[mm][j if mm == m else slot[mm]]) for mm in models])
            moves.append((m, j))
    return states, moves


def joint_search(core: PoseCore, cand_poses: torch.Tensor, cand_model: torch.Tensor, cand_label: Optional[torch.Tensor],
                 shortlists, obs_counts, *, max_sweeps: Optional[int] = None, cost_type: int = _native.COST_DEPTH_6DOF,
                 stride: int = 8, depth_factor: float = 100.0, sensor_resolution: float = 0.01,
                 occlusion_threshold: float = 1.0):
    """cand_poses (N, 16), cand_model (N,), cand_label (N,) or None (3-DoF) on the GPU; shortlists (models, K) candidate
    indices, best first, -1 where a model has fewer (decode_keys of select_topk); obs_counts the observed points per
    label (6-DoF) or the cloud's count (3-DoF).  The shortlisted candidates are rendered once (evaluate's dbg_zs); every
    sweep is one evaluate_states call and two select calls.  -> SimpleNamespace(slot: the chosen slot per model, -1
    for a model without a winner; cost: the final state's integer cost, INT_MAX when the selection's filter excludes
    it; trace: per sweep incumbent_cost, best_cost, best_move (m, j), adopted, and the members' vis / bad of the best
    state)."""
    shortlists = np.asarray(shortlists.cpu() if isinstance(shortlists, torch.Tensor) else shortlists, np.int64)
    K = len(shortlists)
    dev = cand_poses.device
    six = cost_type == _native.COST_DEPTH_6DOF
    label_h = cand_label.cpu().numpy() if (six and cand_label is not None) else None
    kw = dict(cost_type=cost_type, stride=stride, depth_factor=depth_factor, sensor_resolution=sensor_resolution,
              occlusion_threshold=occlusion_threshold)
    slot = [0 if shortlists[m][0] >= 0 else -1 for m in range(K)]
    models = [m for m in range(K) if slot[m] == 0]
    trace = []
    cost = INT_MAX
    if not models:
        return SimpleNamespace(slot=slot, cost=cost, trace=trace)
    # the shortlisted candidates' sampled z-buffers, once: members index this compact batch
    used = np.unique(shortlists[shortlists >= 0])
    compact = {int(c): i for i, c in enumerate(used)}
    sub = torch.from_numpy(used).to(dev)
    nsamp = (core.width // stride) * ((core.height + stride - 1) // stride)
    zs = torch.zeros((len(used), nsamp), dtype=torch.int32, device=dev)
    sub_label = cand_label[sub].contiguous() if (six and cand_label is not None) else None
    core.evaluate(cand_poses[sub].contiguous(), cand_model[sub].contiguous(), sub_label, None, calc_obs_cost=False,
                  dbg_zs=zs, **kw)
    for _ in range(2 * K if max_sweeps is None else max_sweeps):
        states, moves = sweep_states(shortlists, slot)
        tot = np.array([state_obs_total(st, label_h, obs_counts) for st in states], np.float32)
        rc, oc, _, vis, bad = core.evaluate_states([[compact[c] for c in st] for st in states], sub_label,
                                                   torch.from_numpy(tot).to(dev), zs=zs, **kw)
        group = torch.zeros(len(states), dtype=torch.int32, device=dev)
        inc = moves.index((models[0], slot[models[0]]))
        keys = torch.cat([core.select(rc, oc, group, 1), core.select(rc[inc:inc + 1], oc[inc:inc + 1], group[:1], 1)])
        (best_cost, inc_cost), (best, inc_ok) = decode_keys(keys)
        best, nm = int(best), len(models)
        adopted = best >= 0 and int(best_cost) < int(inc_cost)
        shown = best if best >= 0 else inc
        v, b = vis.cpu().numpy(), bad.cpu().numpy()
        trace.append(dict(incumbent_cost=int(inc_cost), best_cost=int(best_cost),
                          best_move=moves[best] if best >= 0 else None, adopted=bool(adopted),
                          vis=v[shown * nm:(shown + 1) * nm].tolist(), bad=b[shown * nm:(shown + 1) * nm].tolist()))
        cost = int(best_cost) if adopted else int(inc_cost)
        if not adopted:
            break
        slot[moves[best][0]] = moves[best][1]
    return SimpleNamespace(slot=slot, cost=cost, trace=trace)
