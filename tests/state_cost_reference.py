"""The state-cost contract ("State cost") in numpy over the oracle, and the joint search over it.

Inputs are the poses' sampled z-buffers after source occlusion, Z (N, hs, ws) int32 -- oracle.render_depth(...)[:, ::s,
::s] or hand-made -- and states as member lists.  `rule` swaps one rule of the contract for a wrong one, for the
certification of the case sets (tests/test_state_cost_cases.py):

  alone      (a) the members scored alone and summed
  last_wins  (b) the highest list position wins depth ties
  expl_sum   (c) expl summed per member instead of the union
  label0     (d) the first member's label used for all members
  clamp      (e) an out-of-range member clamped instead of skipped
  negative   (f) a negative depth treated as transparent
  ge         (g) d^2 = r^2 counted as bad
"""
from types import SimpleNamespace

import numpy as np

import oracle

F32 = np.float32
RULES = ("alone", "last_wins", "expl_sum", "label0", "clamp", "negative", "ge")
INT_MAX = 2 ** 31 - 1


def compose(Z, members, rule=None):
    """(depth, owner) of one state: the minimum non-zero depth per sample and the lowest list position attaining it."""
    N = len(Z)
    depth = np.zeros(Z.shape[1:], np.int32)
    owner = np.full(Z.shape[1:], -1, np.int32)
    for j, m in enumerate(members):
        if rule == "clamp" and N > 0:
            m = min(max(int(m), 0), N - 1)
        if not 0 <= m < N:
            continue
        z = Z[m]
        there = (z > 0) if rule == "negative" else (z != 0)
        take = there & ((owner < 0) | ((z <= depth) if rule == "last_wins" else (z < depth)))
        depth = np.where(take, z, depth)
        owner = np.where(take, j, owner)
    return depth, owner


def _points(depth, cam, s, depth_factor):
    """oracle.depth_to_cloud of the composed samples: the points of the samples with depth > 0, row-major."""
    hs, ws = depth.shape
    img = np.zeros(((hs - 1) * s + 1, ws * s), np.int32)
    img[::s, ::s] = depth
    xyz, _, _ = oracle.depth_to_cloud(img, s, cam["cx"], cam["cy"], cam["fx"], cam["fy"], depth_factor)
    return xyz


def _costs(num, bad, expl, tot, calc_obs):
    num, bad, expl = F32(num), F32(bad), F32(expl)
    rc = F32(-1.0) if num == 0 else F32(F32(bad / num) * F32(100.0))
    if not calc_obs:
        return rc, F32(0.0), F32(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        oc = F32(F32(F32(F32(tot) - expl) / F32(tot)) * F32(100.0))
    return rc, oc, F32(F32(num - bad) - expl)


def _score(Z, members, pose_label, cam, s, obs_sorted, label_start, label_end, r, depth_factor, rule):
    """-> (vis (M,), bad (M,), list of the explained observed positions per member)"""
    M = len(members)
    depth, owner = compose(Z, members, rule)
    valid = depth > 0
    xyz = _points(depth, cam, s, depth_factor)
    own = owner[valid]
    assert len(own) == len(xyz)
    vis = np.bincount(own, minlength=M).astype(np.int32)
    six = pose_label is not None
    lab = None
    if six:
        mem = np.asarray(members, np.int64)
        if rule == "clamp":
            mem = np.clip(mem, 0, len(Z) - 1)
        lab = np.asarray(pose_label, np.int32)[mem[own]] if len(own) else np.zeros(0, np.int32)
        if rule == "label0" and len(own):
            lab = np.full(len(own), pose_label[mem[0]] if 0 <= mem[0] < len(Z) else -1, np.int32)
    d2, idx = oracle.knn1(xyz, lab, obs_sorted, label_start if six else None, label_end if six else None)
    r2 = F32(r) * F32(r)
    is_bad = (d2 >= r2) if rule == "ge" else (d2 > r2)
    bad = np.bincount(own[is_bad], minlength=M).astype(np.int32)
    ok = ~is_bad & (idx >= 0)
    expl = [np.unique(idx[ok & (own == j)]) for j in range(M)]
    return vis, bad, expl


def evaluate_states(Z, states, pose_label, state_obs_total, cam, stride, obs_sorted, label_start=None, label_end=None,
                    r=0.01, depth_factor=100.0, calc_obs=True, rule=None):
    """The contract: (rc (S,), oc, diff float32; vis, bad int32 over the concatenated member lists).  obs_sorted is the
    label-sorted observed cloud; pose_label None is 3-DoF (the whole cloud)."""
    Z = np.asarray(Z, np.int32)
    rc, oc, df, vis, bad = [], [], [], [], []
    for k, members in enumerate(states):
        members = [int(m) for m in members]
        args = (pose_label, cam, stride, obs_sorted, label_start, label_end, r, depth_factor)
        if rule == "alone":
            parts = [_score(Z, [m], *args, None) for m in members]
            v = np.array([p[0][0] for p in parts], np.int32).reshape(-1)
            b = np.array([p[1][0] for p in parts], np.int32).reshape(-1)
            n_expl = sum(len(p[2][0]) for p in parts)
        else:
            v, b, ex = _score(Z, members, *args, rule)
            n_expl = sum(len(e) for e in ex) if rule == "expl_sum" else \
                len(np.unique(np.concatenate(ex))) if ex else 0
        c = _costs(int(v.sum()), int(b.sum()), n_expl, None if state_obs_total is None else state_obs_total[k], calc_obs)
        rc.append(c[0]); oc.append(c[1]); df.append(c[2]); vis.append(v); bad.append(b)
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)  # noqa: E731
    return np.array(rc, F32), np.array(oc, F32), np.array(df, F32), cat(vis), cat(bad)


def state_obs_total(members, cand_label, obs_counts):
    """The observed points a state has to explain: those whose label is among the members' distinct labels (6-DoF,
    obs_counts per label), the whole cloud's count (3-DoF, cand_label None and obs_counts a number)."""
    if cand_label is None:
        return F32(obs_counts)
    cnt = np.asarray(obs_counts)
    labs = sorted({int(cand_label[m]) for m in members})
    return F32(sum(int(cnt[L]) for L in labs if 0 <= L < len(cnt)))


def sweep_states(shortlists, slot):
    """The states of one sweep, ordered by (m, j): the incumbent with model m's slot replaced by j (j = slot[m] is the
    incumbent itself).  -> (list of member lists, list of (m, j))"""
    models = [m for m in range(len(shortlists)) if shortlists[m][0] >= 0]
    states, moves = [], []
    for m in models:
        for j in range(len(shortlists[m])):
            if shortlists[m][j] < 0:
                continue
            states.append([int(shortlists[mm][j if mm == m else slot[mm]]) for mm in models])
            moves.append((m, j))
    return states, moves


def joint_search(score, cand_label, shortlists, obs_counts, max_sweeps=None):
    """The deterministic coordinate descent over the per-model shortlists.  score(states, tot) -> (rc, oc, diff, vis,
    bad) is the state cost (this module's evaluate_states with the scene bound).  -> SimpleNamespace(slot, cost, trace)"""
    shortlists = np.asarray(shortlists, np.int64)
    K = len(shortlists)
    slot = [0 if shortlists[m][0] >= 0 else -1 for m in range(K)]
    models = [m for m in range(K) if slot[m] == 0]
    trace = []
    cost = INT_MAX
    for _ in range(2 * K if max_sweeps is None else max_sweeps):
        states, moves = sweep_states(shortlists, slot)
        if not states:
            break
        tot = np.array([state_obs_total(st, cand_label, obs_counts) for st in states], F32)
        rc, oc, df, vis, bad = score(states, tot)
        bc, bi = oracle.select(rc, oc, np.zeros(len(states), np.int32), 1)
        inc = moves.index((models[0], slot[models[0]]))
        ic, _ = oracle.select(rc[inc:inc + 1], oc[inc:inc + 1], np.zeros(1, np.int32), 1)
        best, nm = int(bi[0]), len(models)
        adopted = best >= 0 and int(bc[0]) < int(ic[0])
        shown = best if best >= 0 else inc
        trace.append(dict(incumbent_cost=int(ic[0]), best_cost=int(bc[0]), best_move=moves[best] if best >= 0 else None,
                          adopted=bool(adopted), vis=vis[shown * nm:(shown + 1) * nm].tolist(),
                          bad=bad[shown * nm:(shown + 1) * nm].tolist()))
        cost = int(bc[0]) if adopted else int(ic[0])
        if not adopted:
            break
        slot[moves[best][0]] = moves[best][1]
    return SimpleNamespace(slot=slot, cost=cost, trace=trace)
