"""Cost type 1 on the GPU where no uniform colour hides a mistake: the fused kernel's colour id pass (raster_phase<STRIDE,
true>, ring_id, stri_orig, cid) on meshes whose every triangle has a colour of its own, and colour::colour_distance as
the device computes it.  Everything is compared with the oracle for equality; there are no tolerances.

  A  the per-triangle colour cases of tests/nn_cases.py (certified on the CPU by tests/test_nn_cases.py: a colour table
     rolled by one triangle, copies that win a depth tie against their originals, or the other winner of a depth tie
     each change some pose's costs);
  B  a threshold sweep: for 64 or more gated pairs the colour threshold is set on the pair's distance and on the float32
     below it, which pins the device's distance of that pair to the bit through the public ABI;
  C  pcore_debug_colour_distance on 150,000 random and several thousand directed Lab pairs, bit for bit.
(The host's rgb2lab is checked without a device in tests/test_colour_spec.py.)"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import _native
from perception_amd.core import PoseCore
from tests import nn_cases as nc
from tests.test_gpu_nn_adversarial import _assert_costs, _evaluate, _setup
from tests.test_nn_cases import SWEEP_GEOM, _colour_want, colour_pairs, sweep_picks

pytestmark = pytest.mark.gpu
F32 = np.float32


# ---------------------------------------------------------------------------------------------
# A: per-triangle colours
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", ["auto", "tcap64"])
@pytest.mark.parametrize("variant", nc.COLOUR_VARIANTS)
@pytest.mark.parametrize("geom", nc.COLOUR_GEOMETRIES)
def test_per_triangle_colours(geom, variant, tile, monkeypatch):
    """Strides 4 and 5 on SMALL and 1 on TINY; the automatic LDS tile and a 64-sample one (every pose in chunks, each
    with its own id pass); twice on the same context: the second call runs after the tile-tier feedback."""
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    case = nc.colour_case(geom, variant)
    core, t = _setup(case, colours=True)
    for call in range(2):
        _assert_costs(_evaluate(core, t, case, 1), _colour_want(geom, variant), f"{case.name} {tile} call {call}")
    if tile == "tcap64":
        assert core.tile_info()["tcap"] == 64
    core.close()


@pytest.mark.parametrize("geom", ["segments-s4", "ties-TINY-s1"])
def test_mesh_uploaded_after_another(geom):
    """The reversed mesh uploaded into a context that holds the plain one (and back): stri_orig and tri_lab are
    rebuilt together."""
    plain, rev = nc.colour_case(geom, "plain"), nc.colour_case(geom, "rev")
    core, t = _setup(plain, colours=True)
    _assert_costs(_evaluate(core, t, plain, 1), _colour_want(geom, "plain"), "plain")
    for case, variant in ((rev, "rev"), (plain, "plain")):
        core.upload_meshes(case.bank.tris, case.bank.tris_model_count, colors=case.bank.colors)
        _assert_costs(_evaluate(core, t, case, 1), _colour_want(geom, variant), f"{variant} after the other mesh")
    core.close()


# ---------------------------------------------------------------------------------------------
# B: the threshold sweep
# ---------------------------------------------------------------------------------------------

def _same_float32_both_sides(thr):
    """The threshold reaches the library (EvalParams) and the oracle (a ctypes float argument) as this float32."""
    bits = F32(thr).view(np.uint32)
    p = _native.EvalParams(1, 1, 4, 100.0, 0.01, 1.0, float(thr))
    assert F32(p.color_distance_threshold).view(np.uint32) == bits
    assert F32(ctypes.c_float(float(thr)).value).view(np.uint32) == bits


def test_threshold_sweep_pins_device_distances():
    case = nc.colour_case(SWEEP_GEOM, "plain")
    pairs = colour_pairs(SWEEP_GEOM, "plain")
    picks, replaced = sweep_picks()
    assert len(picks) >= 64
    for _, d, _, _ in picks:
        _same_float32_both_sides(d)
        _same_float32_both_sides(nc.step(d, -1))
    core, t = _setup(case, colours=True)
    for k, d, want_at, want_below in picks:
        what = f"pair {k} (pose {pairs.pose[k]}, observed {pairs.obs[k]}, triangle {pairs.tri[k]}), d = {d!r}"
        _assert_costs(_evaluate(core, t, case, 1, colour_thr=float(d)), want_at, what + ", threshold d")
        _assert_costs(_evaluate(core, t, case, 1, colour_thr=float(nc.step(d, -1))), want_below,
                      what + ", threshold one float below d")
    for thr in (F32(0.0), np.finfo(F32).max, F32(-1.0)):
        _same_float32_both_sides(thr)
        _assert_costs(_evaluate(core, t, case, 1, colour_thr=float(thr)), case.oracle_costs(1, colour_thr=float(thr)),
                      f"threshold {thr!r}")
    core.close()
    print(f"sweep: {len(picks)} pairs of {len(pairs.d)} gated, {replaced} replaced")


# ---------------------------------------------------------------------------------------------
# C: the device's colour distance, value for value
# ---------------------------------------------------------------------------------------------

TWO_PI_F = F32(2 * np.pi)


def _polar(L, C, deg):
    th = np.deg2rad(np.asarray(deg, np.float64))
    return np.stack([np.asarray(L, np.float64), C * np.cos(th), C * np.sin(th)], -1).astype(F32)


def _pair(a, b):
    return np.concatenate([a, b], -1).astype(F32)


def distance_classes():
    """name -> (n, 6) float32 Lab pairs."""
    rng = np.random.default_rng(77)
    cls = {}

    def lab(n):
        return np.stack([rng.uniform(0, 100, n), rng.uniform(-128, 128, n), rng.uniform(-128, 128, n)], 1).astype(F32)

    rgb = rng.integers(0, 256, (200000, 3)).astype(np.uint8)
    labs = oracle.rgb2lab_n(rgb)
    cls["random rgb"] = _pair(labs[:100000], labs[100000:])
    cls["random lab"] = _pair(lab(50000), lab(50000))
    # a = b = +-0 on one side (either side) and on both: atan2_f's y == 0 cases with x = +-0
    zeros = np.array([(a, b) for a in (0.0, -0.0) for b in (0.0, -0.0)], F32)
    one = lab(320)
    one[:, 1:] = zeros[np.arange(320) % 4]
    both = lab(320)
    both[:, 1:] = zeros[(np.arange(320) // 4) % 4]
    cls["zero chroma"] = np.concatenate([_pair(one, lab(320)), _pair(lab(320), one), _pair(one, both)])
    # b = +-0 with a < 0: the hue is +-pi before the 2 pi is added
    neg = lab(400)
    neg[:, 1] = -np.abs(neg[:, 1]) - F32(0.5)
    neg[:, 2] = np.where(np.arange(400) % 2, F32(0.0), F32(-0.0))
    cls["hue pi"] = np.concatenate([_pair(neg, lab(400)), _pair(lab(400), neg), _pair(neg[:200], neg[200:])])
    # b a float or a little more below zero with a > 0: the hue just under 2 pi, fmod_f subtracts once or not at all
    pos = lab(640)
    pos[:, 1] = np.abs(pos[:, 1]) + F32(1.0)
    scale = np.array([0, 1e-40, 1e-30, 1e-12, 3e-8, 6e-8, 1.2e-7, 2.4e-7, 4.8e-7, 1e-6, 1e-5, 1e-3])[np.arange(640) % 12]
    pos[:, 2] = np.where(scale == 0, nc.step(F32(0.0), -1), (-scale * pos[:, 1]).astype(F32))
    cls["hue under 2 pi"] = np.concatenate([_pair(pos, lab(640)), _pair(lab(640), pos), _pair(pos[:320], pos[320:])])
    # opposite hues (a, b) against (-a, -b) and its neighbours at +-1 and +-2 floats: |h2 - h1| about pi
    a = lab(120)
    a[:, 1:] = np.where(np.abs(a[:, 1:]) < 1, F32(7.0), a[:, 1:])
    opp = []
    for da in range(-2, 3):
        for db in range(-2, 3):
            o = lab(120)
            o[:, 1], o[:, 2] = nc.step(-a[:, 1], da), nc.step(-a[:, 2], db)
            opp += [_pair(a, o), _pair(o, a)]
    cls["opposite hues"] = np.concatenate(opp)
    # mean hue within a degree of 275 (the exp_f term), of 0 and of 360
    for name, centre in (("mean hue 275", 275.0), ("mean hue 0 / 360", 0.0)):
        n = 600
        delta, half = rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 80.0, n)
        C = rng.uniform(40, 110, (2, n))
        cls[name] = _pair(_polar(rng.uniform(0, 100, n), C[0], centre + delta + half),
                          _polar(rng.uniform(0, 100, n), C[1], centre + delta - half))
    same = np.concatenate([lab(300), labs[:300]])
    cls["identical"] = _pair(same, same)
    # the sRGB gamut's corners and edges (two channels at 0 or 255, the third swept): its chroma extremes
    sweep = np.arange(0, 256, 5)
    edge = [np.roll(np.array([[v, p, q] for v in sweep]), k, 1) for p in (0, 255) for q in (0, 255) for k in range(3)]
    gam = oracle.rgb2lab_n(np.concatenate(edge).astype(np.uint8))
    cls["gamut edges"] = _pair(gam[rng.integers(0, len(gam), 1500)], gam[rng.integers(0, len(gam), 1500)])
    return cls


def _hues(p):
    """h1, h2 (float32 values, as float64), the hue before fmod_f, and meanH, restated in numpy for the branch census."""
    p = p.astype(np.float64)
    a1, b1, a2, b2 = p[:, 1], p[:, 2], p[:, 4], p[:, 5]
    mc = (np.sqrt((a1 * a1 + b1 * b1).astype(F32)).astype(np.float64) +
          np.sqrt((a2 * a2 + b2 * b2).astype(F32)).astype(np.float64)) / 2
    mc7 = mc ** 7
    g = 0.5 * (1 - np.sqrt((mc7 / (mc7 + 6103515625.0)).astype(F32)).astype(np.float64))
    pre, h = [], []
    for a, b in ((a1, b1), (a2, b2)):
        ap = (a * (1 + g)).astype(F32)
        t = (np.arctan2(b.astype(F32), ap).astype(F32).astype(np.float64) + 2 * np.pi).astype(F32)
        pre.append(t)
        h.append(np.where(t >= TWO_PI_F, t - TWO_PI_F, t).astype(np.float64))
    h1, h2 = h
    mean = np.where(np.abs(h1 - h2) <= np.pi + 1e-5, (h1 + h2) / 2,
                    np.where(h1 + h2 < 2 * np.pi, (h1 + h2 + 2 * np.pi) / 2, (h1 + h2 - 2 * np.pi) / 2))
    return h1, h2, np.stack(pre), mean


def test_device_colour_distance_equals_the_oracle_bitwise():
    cls = distance_classes()
    for name, p in cls.items():
        assert p.dtype == F32 and p.shape[1] == 6 and len(p) >= 300 and np.isfinite(p).all(), name
    assert len(cls["random rgb"]) == 100000 and len(cls["random lab"]) == 50000
    # the branch census, from the CPU's side: the directed inputs take the branches they were made for
    directed = np.concatenate([p for n, p in cls.items() if not n.startswith("random")])
    h1, h2, pre, mean = _hues(directed)
    dh, far, wide = h2 - h1, np.abs(h2 - h1) > np.pi, np.abs(h1 - h2) > np.pi + 1e-5
    sides = {
        "fmod_f subtracts": pre >= TWO_PI_F, "fmod_f leaves": pre < TWO_PI_F,
        "|dh| <= pi": ~far, "dh > pi": far & (dh > 0), "dh < -pi": far & (dh < 0),
        "pi < |dh| <= pi + 1e-5": far & ~wide,
        "mean: wide, h1 + h2 < 2 pi": wide & (h1 + h2 < 2 * np.pi), "mean: wide, h1 + h2 >= 2 pi": wide & (h1 + h2 >= 2 * np.pi),
        "mean hue in 275 +- 1": np.abs(np.rad2deg(mean) - 275) <= 1, "mean hue in [0, 1]": np.rad2deg(mean) <= 1,
        "mean hue in [359, 360]": np.rad2deg(mean) >= 359,
    }
    z = cls["zero chroma"]
    sides.update({"y = +0, x = +0": (z[:, 2] == 0) & ~np.signbit(z[:, 2]) & (z[:, 1] == 0) & ~np.signbit(z[:, 1]),
                  "y = -0, x = -0": (z[:, 2] == 0) & np.signbit(z[:, 2]) & (z[:, 1] == 0) & np.signbit(z[:, 1]),
                  "y = +0, x = -0": (z[:, 2] == 0) & ~np.signbit(z[:, 2]) & (z[:, 1] == 0) & np.signbit(z[:, 1]),
                  "y = -0, x = +0": (z[:, 2] == 0) & np.signbit(z[:, 2]) & (z[:, 1] == 0) & ~np.signbit(z[:, 1]),
                  "both sides zero": (z[:, 1:3] == 0).all(1) & (z[:, 4:6] == 0).all(1)})
    hp = cls["hue pi"]
    sides.update({"y = +0, x < 0": (hp[:, 2] == 0) & ~np.signbit(hp[:, 2]) & (hp[:, 1] < 0),
                  "y = -0, x < 0": (hp[:, 2] == 0) & np.signbit(hp[:, 2]) & (hp[:, 1] < 0)})
    under = _hues(cls["hue under 2 pi"][:640])[2][0]  # b < 0 < a on side 1: atan2_f + 2 pi rounds to 2 pi or stays below
    sides.update({"hue under 2 pi rounds to 2 pi": under == TWO_PI_F, "hue under 2 pi stays below": under < TWO_PI_F})
    census = {k: int(np.sum(v)) for k, v in sides.items()}
    print("classes:", {n: len(p) for n, p in cls.items()})
    print("census:", census)
    assert min(census.values()) >= 10, census

    pairs = np.ascontiguousarray(np.concatenate(list(cls.values())))
    want = oracle.colour_distance_n(pairs)
    assert want[:3].tolist() == [oracle.colour_distance(p[:3], p[3:]) for p in pairs[:3]]  # the batched entry is the scalar one
    lo = np.cumsum([0] + [len(p) for p in cls.values()])
    ident = list(cls).index("identical")
    assert not want[lo[ident]:lo[ident + 1]].view(np.uint64).any()  # identical pairs: exactly +0.0
    core = PoseCore(0)
    got = core.colour_distance(torch.from_numpy(pairs).to(torch.device("cuda", 0))).cpu().numpy()
    core.close()
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    where = {n: int(((bad >= a) & (bad < b)).sum()) for n, a, b in zip(cls, lo[:-1], lo[1:])}
    assert len(bad) == 0, (f"{len(bad)} of {len(pairs)} distances differ, by class {where}; e.g. "
                           f"{[(pairs[i].tolist(), got[i], want[i]) for i in bad[:4]]}")
