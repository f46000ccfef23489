"""The case sets of the state-cost tests (tests/test_state_cost_cases.py certifies them on the oracle,
tests/test_gpu_state_cost.py and tests/test_gpu_joint_search.py run them on the GPU).

  scene   the three-object scene of tests/scene_cases.py at stride 8 with labels: every candidate pose, and each
          model's best candidate moved 2 cm sideways and 1 cm nearer; states "winners + shifted copies", "two best per
          model", the winners alone and in reverse.  Separates the wrong rules (a) - (d) of state_cost_reference.
  hand    hand-made z-buffers and observed points on a 96 x 72 camera whose samples unproject exactly: an out-of-range
          member (e), a negative depth in front of another pose (f), an observed point at d^2 = r^2 (g).
  fuzz    random z-buffers (zeros, negatives, ties) and observed clouds near their points, for any camera and stride:
          every state shape of the contract.
  boxes   the joint-search scene: one box mesh uploaded as two models, two boxes observed side by side, no labels."""
import functools
from types import SimpleNamespace

import numpy as np

import oracle
from perception_amd import synthetic as syn
from perception_amd.model import init_from_eigen_batch
from tests import scene_cases
from tests import state_cost_reference as ref

F32 = np.float32


def _sorted_obs(xyz, lab):
    """The observation in the label-sorted order the oracle takes, with its segment table."""
    order = np.argsort(lab, kind="stable")
    xs, ls = np.ascontiguousarray(xyz[order], F32), lab[order]
    nl = max(0, int(lab.max()) + 1) if len(lab) else 0
    start = np.array([np.searchsorted(ls, L, "left") for L in range(nl)], np.int32)
    end = np.array([np.searchsorted(ls, L, "right") for L in range(nl)], np.int32)
    return xs, start, end


class StateCase:
    """Z (N, hs, ws) int32, pose_label (N,) or None, states, per-state totals, the camera and stride, the observation
    as given to set_observation (obs_xyz, obs_label or None) and label-sorted (obs_sorted, label_start, label_end)."""

    def __init__(self, name, cam, stride, Z, pose_label, states, obs_xyz, obs_label, r, tot=None):
        self.name, self.cam, self.stride, self.r = name, cam, stride, float(r)
        self.Z = np.ascontiguousarray(Z, np.int32)
        self.pose_label = None if pose_label is None else np.ascontiguousarray(pose_label, np.int32)
        self.states = [list(map(int, st)) for st in states]
        self.obs_xyz = np.ascontiguousarray(obs_xyz, F32).reshape(-1, 3)
        self.obs_label = None if obs_label is None else np.ascontiguousarray(obs_label, np.int32)
        if self.pose_label is None:
            self.obs_sorted = _sorted_obs(self.obs_xyz, np.zeros(len(self.obs_xyz), np.int32) if obs_label is None
                                          else self.obs_label)[0]
            self.label_start = self.label_end = None
            counts = len(self.obs_xyz)
        else:
            self.obs_sorted, self.label_start, self.label_end = _sorted_obs(self.obs_xyz, self.obs_label)
            counts = self.label_end - self.label_start
        N = len(self.Z)
        self.tot = np.asarray(tot, F32) if tot is not None else np.array(
            [max(ref.state_obs_total([m for m in st if 0 <= m < N], self.pose_label, counts), F32(1)) for st in self.states],
            F32)

    def expected(self, rule=None, calc_obs=True):
        return ref.evaluate_states(self.Z, self.states, self.pose_label, self.tot, self.cam, self.stride, self.obs_sorted,
                                   self.label_start, self.label_end, self.r, 100.0, calc_obs, rule)


# ---------------------------------------------------------------------------------------------
# the three-object scene
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene():
    """The scene case: the 24 candidate poses, then every model's best candidate (by the oracle's selection) moved 2 cm
    sideways and 1 cm nearer.  -> SimpleNamespace(case: StateCase, poses, pose_model, rc, oc, diff of every pose alone,
    best, second: each model's two best candidates)"""
    base, _ = scene_cases.scene_case()
    sc, s = base.scene, base.stride
    rc, oc, _ = base.oracle_costs()
    best, second = [], []
    for m in range(base.K):
        idx = np.nonzero(base.pose_model == m)[0]
        cost = np.array([int(oracle.select(rc[i:i + 1], oc[i:i + 1], np.zeros(1, np.int32), 1)[0][0]) for i in idx])
        o = np.argsort(cost, kind="stable")
        best.append(int(idx[o[0]]))
        second.append(int(idx[o[1]]))
    moved = []
    for m in range(base.K):
        T = base.poses44[best[m]].copy()
        T[:3, 3] += np.array([0.02, 0.0, -0.01])
        moved.append(T)
    poses44 = np.concatenate([base.poses44, np.stack(moved)])
    poses = init_from_eigen_batch(poses44)
    pm = np.concatenate([base.pose_model, np.arange(base.K, dtype=np.int32)])
    D = oracle.render_depth(sc.bank.tris, sc.bank.tris_model_count, poses, pm, pm, sc.width, sc.height, sc.proj,
                            sc.src_depth_cm, sc.mask, 1.0)
    n0 = len(base.poses)
    shifted = [n0 + m for m in range(base.K)]
    states = [best + shifted, best + second, list(best), list(best)[::-1], shifted + best, second + best,
              [best[0]], [shifted[1]], [], best + best]
    cam = dict(cx=sc.cx, cy=sc.cy, fx=sc.fx, fy=sc.fy, width=sc.width, height=sc.height)
    case = StateCase("scene", cam, s, D[:, ::s, ::s], pm, states, base.obs_xyz_raw, base.obs_label_raw, 0.01)
    tot1 = np.concatenate([base.pose_obs_total, base.pose_obs_total[best]])
    return SimpleNamespace(case=case, base=base, poses=poses, pose_model=pm, pose_obs_total=tot1, best=best,
                           second=second, shifted=shifted)


# ---------------------------------------------------------------------------------------------
# hand-made z-buffers
# ---------------------------------------------------------------------------------------------

# samples at multiples of 8 pixels unproject exactly: (kx 8 - 48) / 64 and (ky 8 - 32) / 64 are multiples of 1 / 8
HAND_CAM = dict(width=96, height=72, fx=64.0, fy=64.0, cx=48.0, cy=32.0)
HAND_R = 2.0 ** -7


def _unproject(cam, s, kx, ky, Z):
    z = F32(Z) / F32(100.0)
    return np.array([(F32(kx * s) - F32(cam["cx"])) / F32(cam["fx"]) * z, (F32(ky * s) - F32(cam["cy"])) / F32(cam["fy"]) * z,
                     z], F32)


@functools.lru_cache(maxsize=None)
def hand():
    """Four poses on the 12 x 9 sample grid (stride 8), depths 50 and 100 (0.5 m and 1 m: exact floats):
      0  a 3 x 3 block at depth 50, every point observed exactly
      1  the same block one column to the right at depth 100, its points observed exactly; the shared columns lie
         behind pose 0
      2  negative depths (-7) over pose 1's last column: they win the minimum there and yield no point (f)
      3  a lone sample at depth 50 on the optical axis's row whose only observed point is at distance exactly r (g)
    States: [0, 9] with pose 3 the last one, so that a clamped member adds pose 3's sample (e); [2, 1] and [1, 2] (f);
    [3] (g); and their union."""
    cam, s = HAND_CAM, 8
    Z = np.zeros((4, 9, 12), np.int32)
    Z[0, 2:5, 2:5] = 50
    Z[1, 2:5, 3:6] = 100
    Z[2, 2:5, 5] = -7
    Z[3, 7, 9] = 50
    obs, lab = [], []
    for m in (0, 1):
        ky, kx = np.nonzero(Z[m])
        for y, x in zip(ky, kx):
            obs.append(_unproject(cam, s, x, y, Z[m, y, x]))
            lab.append(m)
    q = _unproject(cam, s, 9, 7, 50)
    obs.append(q + np.array([0.0, 0.0, HAND_R], F32))  # 0.5 + 2^-7 is exact: d^2 = 2^-14 = r^2
    lab.append(3)
    assert F32(obs[-1][2] - q[2]) * F32(obs[-1][2] - q[2]) == F32(HAND_R) * F32(HAND_R)
    states = [[0, 9], [2, 1], [1, 2], [3], [0, 1, 2, 3], [-1, 0], [4, 1]]
    return StateCase("hand", cam, s, Z, np.array([0, 1, 1, 3], np.int32), states, np.stack(obs), np.array(lab, np.int32),
                     HAND_R)


# ---------------------------------------------------------------------------------------------
# random z-buffers
# ---------------------------------------------------------------------------------------------

def fuzz_states(rng, n, big=(21, 300)):
    """Every state shape of the contract over n poses: 0, 1, 2, 21 and 300 members, duplicates, out-of-range members."""
    states = [[], [0], [n - 1], [1, 0], [0, 1], [2, 2], [3, 1, 3, 1], [n, 0], [-1, 1, n + 5], [-3], [2 ** 31 - 1, 2]]
    for m in big:
        states.append(rng.integers(0, n, m).tolist())
        states.append(rng.integers(-2, n + 2, m).tolist())
    states.append(list(range(n)))
    states.append(list(range(n))[::-1])
    # owners beyond list position 256, where the kernel counts in place instead of in its LDS histogram: out-of-range
    # fillers (a duplicate of a real pose would own nothing) and the real poses after them, or straddling the boundary
    states.append([n, -1] * (DEEP_FILL // 2) + list(range(n)))
    states.append([n + 7] * (DEEP - n // 2) + list(range(n))[::-1])
    states.append([-2] * DEEP_FILL + rng.integers(0, n, 40).tolist())
    return states


DEEP = 256       # list positions the kernel counts in LDS
DEEP_FILL = 260  # fillers of the states whose owners all lie beyond them


def deep_positions(states):
    """Positions in the concatenated member outputs that lie at list position >= DEEP of their state."""
    off = np.concatenate([[0], np.cumsum([len(st) for st in states])])
    return np.concatenate([np.arange(off[k] + DEEP, off[k + 1]) for k in range(len(states)) if len(states[k]) > DEEP]
                          + [np.zeros(0, np.int64)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def fuzz(cam_name, stride, labelled, seed=0, n_poses=6, n_obs_per=1.0):
    """Random z-buffers on a camera of tests/helpers.py: each pose a rectangle of depths 40 .. 90 cm drawn from few
    values (ties across poses everywhere), holes of 0, a few negative samples; the observed cloud is a random subset of
    the poses' own points, some moved by about the radius, some by more, in a random order, with labels 0 .. 3 (label
    3 has one point, label 2 none; poses carry labels -1 .. 5)."""
    from tests import helpers

    cam = helpers.GEOMETRY_CAMERAS[cam_name]
    s = stride
    ws, hs = cam["width"] // s, (cam["height"] + s - 1) // s
    rng = np.random.default_rng([seed, ws, hs, int(labelled)])
    r = 0.01
    Z = np.zeros((n_poses, hs, ws), np.int32)
    pts, plab = [], []
    pose_label = np.array([0, 1, 0, 3, 5, -1, 1, 2][:n_poses] + [0] * max(0, n_poses - 8), np.int32)
    for m in range(n_poses):
        w, h = int(rng.integers(ws // 4, ws // 2 + 2)), int(rng.integers(hs // 4, hs // 2 + 2))
        x0, y0 = int(rng.integers(0, ws - w + 1)), int(rng.integers(0, hs - h + 1))
        z = rng.choice(np.array([40, 41, 55, 90]), (h, w))
        z = np.where(rng.random((h, w)) < 0.15, 0, z)
        z = np.where(rng.random((h, w)) < 0.03, -int(rng.integers(1, 50)), z)
        Z[m, y0:y0 + h, x0:x0 + w] = z
    # a negative depth of pose 1 in front of a point of pose 0, whatever the rectangles do
    ky, kx = np.nonzero(Z[0] > 0)
    Z[1, ky[0], kx[0]] = -5
    for m in range(n_poses):
        ky, kx = np.nonzero(Z[m] > 0)
        keep = rng.random(len(ky)) < min(1.0, n_obs_per * 400.0 / max(len(ky), 1))
        for y, x in zip(ky[keep], kx[keep]):
            pts.append(_unproject(cam, s, x, y, Z[m, y, x]))
            plab.append(int(np.clip(pose_label[m], 0, 1)))
    pts = np.array(pts, F32).reshape(-1, 3)
    scale = rng.choice(np.array([0.0, 0.5, 0.99, 1.01, 3.0]), len(pts))
    d = rng.normal(size=pts.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True) + 1e-12
    obs = (pts + (d * (scale * r)[:, None])).astype(F32)
    lab = np.array(plab, np.int32)
    obs = np.concatenate([obs, obs[:1] + F32(0.002)])  # label 3: one point; label 2: none
    lab = np.concatenate([lab, [3]]).astype(np.int32)
    perm = rng.permutation(len(obs))
    obs, lab = obs[perm], lab[perm]
    states = fuzz_states(rng, n_poses)
    return StateCase(f"fuzz-{cam_name}-s{s}-{'lab' if labelled else 'nolab'}", cam, s, Z,
                     pose_label if labelled else None, states, obs, lab if labelled else None, r)


# ---------------------------------------------------------------------------------------------
# the joint-search scene
# ---------------------------------------------------------------------------------------------

BOX_CAM = dict(width=200, height=152, fx=180.0, fy=180.0, cx=100.0, cy=76.0)
BOX_STRIDE = 4
BOX_K = 4


@functools.lru_cache(maxsize=None)
def boxes():
    """One box mesh uploaded as two models; two boxes observed side by side, 16 cm apart, at 0.8 m.  Of every observed
    box only the left 70 % of the face is observed, so a pose at a box has about 30 % of bad points: a pose alone
    explains half of the cloud (rc near 30, oc near 50: inside the selection's |rc - oc| < 30 window), and both models'
    candidates -- the same four poses: at the left box, at the right box, and each moved 1 cm -- rank alike, so greedy
    puts both models on the same box.  No labels: cost_type 0, every state has to explain the whole cloud."""
    cam, s = BOX_CAM, BOX_STRIDE
    W, H = cam["width"], cam["height"]
    tris = syn.box_mesh((0.10, 0.10, 0.06), k=4)
    tris2 = np.concatenate([tris, tris]).astype(F32)
    cnt = np.array([len(tris), len(tris)], np.int32)
    proj = oracle.compute_proj(cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H)

    def at(x, y=0.0):
        T = np.eye(4)
        T[:3, 3] = (x, y, 0.8)
        return T

    cand44 = np.stack([at(-0.08), at(0.08), at(-0.07, 0.004), at(0.09, 0.004)])
    poses44 = np.concatenate([cand44, cand44])
    poses = init_from_eigen_batch(poses44)
    pm = np.repeat(np.arange(2, dtype=np.int32), len(cand44))
    src = np.zeros((H, W), np.int32)
    D = oracle.render_depth(tris2, cnt, poses, pm, None, W, H, proj, src, None, 1.0)
    obs = []
    for k, xc in ((0, -0.08), (1, 0.08)):
        xyz, _, _ = oracle.depth_to_cloud(D[k], s, cam["cx"], cam["cy"], cam["fx"], cam["fy"], 100.0)
        obs.append(xyz[xyz[:, 0] < xc - 0.05 + 0.07])
    obs = np.concatenate(obs).astype(F32)
    return SimpleNamespace(cam=cam, stride=s, tris=tris2, cnt=cnt, proj=proj, poses=poses, pose_model=pm, src=src,
                           Z=np.ascontiguousarray(D[:, ::s, ::s]), obs=obs, r=0.01, K=BOX_K)


def boxes_reference():
    """The numpy side of the joint-search scene: every candidate's costs alone, greedy's shortlists (the K best per
    model by the oracle's selection key order) and the joint search over them."""
    b = boxes()
    n = len(b.poses)
    score = lambda states, tot: ref.evaluate_states(b.Z, states, None, tot, b.cam, b.stride, b.obs, None, None, b.r)  # noqa: E731
    tot1 = np.full(n, len(b.obs), F32)
    rc, oc, df, _, _ = score([[i] for i in range(n)], tot1)
    shortlists = np.full((2, b.K), -1, np.int64)
    for m in range(2):
        idx = np.nonzero(b.pose_model == m)[0]
        keyed = []
        for i in idx:
            c, bi = oracle.select(rc[i:i + 1], oc[i:i + 1], np.zeros(1, np.int32), 1)
            if bi[0] >= 0:
                keyed.append((int(c[0]), int(i)))
        for j, (_, i) in enumerate(sorted(keyed)[:b.K]):
            shortlists[m, j] = i
    res = ref.joint_search(score, None, shortlists, len(b.obs))
    return SimpleNamespace(rc=rc, oc=oc, diff=df, shortlists=shortlists, result=res, score=score)
