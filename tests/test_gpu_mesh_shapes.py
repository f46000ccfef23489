"""The fused raster on mesh and bank shapes it never saw: the cases of tests/mesh_cases.py (certified on the CPU by
tests/test_mesh_cases.py: nearly every triangle owns a sample, deleting one changes a depth, a wrong triangle index
changes a colour cost) through the C ABI, bit for bit against the oracle.  Everything is compared for equality: there
are no tolerances.

What the banks put in front of the kernel's stream walk (raster_phase, pcore_fused.hip): models with fewer streams
than waves next to larger ones, streams without a step, empty models (st_lo == st_hi) first, inside and last, a
one-triangle model as the bank's last (the prefetch runs into the padding step), unstructured meshes of a few thousand
shuffled triangles, a hub vertex shared by 300 triangles, NaN / inf vertices in an ordinary model (whole-image window,
the non-fastdiv copy), and -- with PCORE_MODEL_STREAMS = 8 -- waves that walk two streams each, the only place where
the stream-switch flush runs."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle
from perception_amd import _native
from perception_amd.core import PoseCore, decode_keys
from tests import mesh_cases as mc
from tests.mesh_cases import mesh_case

pytestmark = pytest.mark.gpu

CAM = mc.CAM


def _up(a):
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))  # a copy: the cases are read-only


class Ctx:
    """A context with a case's bank (and a colour per triangle, when given), the camera, and the case's pose batch on
    the GPU; observe(stride) gives it the observation of that stride."""

    def __init__(self, case, colours=None, core=None):
        self.case, self.coloured = case, colours is not None
        self.core = core or PoseCore(0)
        self.core.upload_meshes(case.bank.tris, case.bank.tris_model_count, colors=colours)
        if core is None:
            self.core.set_camera(case.width, case.height, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], case.proj)
        self.src, self.mask = _up(case.src_depth), _up(case.mask)
        self.poses, self.pm, self.pl = _up(case.poses), _up(case.pose_model), _up(case.pose_label)
        self.stride = None

    def observe(self, stride):
        o = self.case.observation(stride)
        self.core.set_observation(self.src, self.mask, _up(o.xyz), _up(o.label), mc.R)
        if self.coloured:
            self.core.set_observation_colors(_up(o.rgb))
        self.stride, self.obs = stride, o

    def evaluate(self, cost_type, zs=False, poses=None, pm=None, pl=None, **kw):
        """(costs, z-samples or None) of the case's batch (or the one given) at the observed stride."""
        s, case = self.stride, self.case
        poses = self.poses if poses is None else poses
        pm = self.pm if pm is None else pm
        pl = self.pl if pl is None else pl
        n = int(poses.shape[0])
        six = cost_type == 2
        tot = _up(self.obs.totals(pl.cpu().numpy()) if six else self.obs.totals0(n))
        dbg = None
        if zs:
            dbg = torch.full((n, -(-case.height // s), case.width // s), -7, dtype=torch.int32, device=poses.device)
        got = self.core.evaluate(poses, pm, pl if six else None, tot, cost_type=cost_type, stride=s,
                                 sensor_resolution=mc.R, color_distance_threshold=mc.COLOUR_THR, dbg_zs=dbg, **kw)
        torch.cuda.synchronize()
        return got, (None if dbg is None else dbg.cpu().numpy())

    def close(self):
        self.core.close()


def _assert_zs(case, got, want, what):
    bad = np.argwhere(got != want)
    if len(bad):
        p, ky, kx = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} z-samples differ in {len(np.unique(bad[:, 0]))} poses; first: "
                             f"{case.describe(p)}, (ky, kx) = ({ky}, {kx}): gpu {got[p, ky, kx]}, oracle "
                             f"{want[p, ky, kx]}")


def _assert_costs(case, got, want, what, describe=None):
    rc, oc, df = (x.cpu().numpy() for x in got)
    orc, ooc, odf = want
    bad = np.nonzero(~((rc.view(np.uint32) == orc.view(np.uint32)) & (oc.view(np.uint32) == ooc.view(np.uint32)) &
                       (df.view(np.uint32) == odf.view(np.uint32))))[0]
    if len(bad):
        p = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(rc)} poses differ ({bad[:8]}); first: "
                             f"{(describe or case.describe)(p)}: gpu rc {rc[p]} oc {oc[p]} diff {df[p]}, oracle rc "
                             f"{orc[p]} oc {ooc[p]} diff {odf[p]}")


def _check_depth_costs(ctx, what, cost_types=(2, 0), calls=1):
    """z-samples and costs of the context's case at its observed stride."""
    case, s = ctx.case, ctx.stride
    for call in range(calls):
        for ct in cost_types:
            got, zs = ctx.evaluate(ct, zs=True)
            _assert_zs(case, zs, case.zs(s), f"{what}, stride {s}, type {ct}, call {call}")
            _assert_costs(case, got, case.oracle_costs(s, ct), f"{what}, stride {s}, type {ct}, call {call}")


# ---------------------------------------------------------------------------------------------
# sampled raster and depth costs
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", ["auto", "tcap64"])
@pytest.mark.parametrize("name", mc.ALL_BANKS)
def test_sampled_raster_and_costs(name, tile, monkeypatch):
    """evaluate(..., dbg_zs) equals the oracle's render at the sample grid, and rc / oc / diff of cost types 2 and 0
    equal the oracle's, at strides 1 and 8 (templated) and 2 and 5 (generic), twice per stride (the second call runs
    after the first one's tile feedback), with the automatic tile and with a 64-sample tile (every pose in chunks,
    each chunk a full stream walk)."""
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    case = mesh_case(name)
    ctx = Ctx(case)
    for s in mc.STRIDES:
        ctx.observe(s)
        _check_depth_costs(ctx, f"bank {name}, tile {tile}", calls=2)
    if tile == "tcap64":
        assert ctx.core.tile_info()["tcap"] == 64
    ctx.close()


@pytest.mark.parametrize("name", ["with_empty", "empty_first"])
def test_select_keys_with_empty_models(name):
    """pcore_evaluate_select on a bank with empty models: the keys equal oracle.select of the oracle's costs, and the
    empty models' keys stay PCORE_KEY_NONE."""
    case = mesh_case(name)
    K = case.bank.K
    ctx = Ctx(case)
    for s in (8, 1):
        ctx.observe(s)
        for ct in (2, 0):
            keys = torch.full((K,), _native.PCORE_KEY_NONE, dtype=torch.int64, device=ctx.poses.device)
            got, _ = ctx.evaluate(ct, select=(keys, 1000, K))
            want = case.oracle_costs(s, ct)
            _assert_costs(case, got, want, f"bank {name}, stride {s}, type {ct}, evaluate_select")
            cost, idx = decode_keys(keys)
            ocost, oidx = oracle.select(want[0], want[1], case.pose_model, K, 1000)
            assert np.array_equal(cost, ocost) and np.array_equal(idx, oidx), (name, s, ct, cost, idx, ocost, oidx)
            empty = case.bank.tris_model_count == 0
            assert (keys.cpu().numpy()[empty] == _native.PCORE_KEY_NONE).all() and (idx[empty] == -1).all()
            assert (idx[~empty] >= 1000).any()  # the selection is not vacuous
    ctx.close()


# ---------------------------------------------------------------------------------------------
# colour-id pass
# ---------------------------------------------------------------------------------------------

def _colour_params():
    out = []
    for name, stride in (("large", 1), ("large", 5), ("with_empty", 1)):
        for b in range(mc.bank(name).num_colourings()):
            out.append(pytest.param(name, stride, b, "auto", id=f"{name}-s{stride}-bit{b}"))
    out.append(pytest.param("large", 5, 3, "tcap64", id="large-s5-bit3-tcap64"))
    return out


@pytest.mark.parametrize("name,stride,b,tile", _colour_params())
def test_colour_id_pass(name, stride, b, tile, monkeypatch):
    """Cost type 1 with colouring b (colour A on the triangles whose index within their model has bit b set, every
    observed point colour B, beyond the gate): rc / oc / diff equal oracle.evaluate_colour.  A stream slot that reports
    another triangle's index -- a wrong stri_orig entry of a mesh reordered by look-ahead batches -- changes a cost in
    the colouring of a bit in which the two indices differ (tests/test_mesh_cases.py)."""
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    case = mesh_case(name)
    ctx = Ctx(case, colours=case.bank.colouring(b))
    ctx.observe(stride)
    for call in range(2):
        got, _ = ctx.evaluate(1)
        _assert_costs(case, got, case.oracle_colour_costs(stride, b),
                      f"bank {name}, stride {stride}, colouring {b}, tile {tile}, call {call}")
    if tile == "tcap64":
        assert ctx.core.tile_info()["tcap"] == 64
    ctx.close()


# ---------------------------------------------------------------------------------------------
# rendered clouds and the full render
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mc.ALL_BANKS)
def test_rendered_clouds(name):
    """render_clouds (render_cloud_kernel, the path every ICP starts from) equals the oracle's compaction of the
    oracle's z-buffers, points and counts, at strides 8 and 5."""
    case = mesh_case(name)
    ctx = Ctx(case)
    for s in (8, 5):
        ctx.observe(s)
        xyzw, cnt = ctx.core.render_clouds(ctx.poses, ctx.pm, None, stride=s)
        torch.cuda.synchronize()
        xyzw, cnt = xyzw.cpu().numpy(), cnt.cpu().numpy()
        oxyz, opose = case.cloud(s)
        ocnt = np.bincount(opose, minlength=case.n)
        bad = np.nonzero(cnt != ocnt)[0]
        assert len(bad) == 0, f"stride {s}: counts differ; first: {case.describe(int(bad[0]))}: gpu {cnt[bad[0]]}, " \
                              f"oracle {ocnt[bad[0]]}"
        assert cnt.sum() > 0
        start = np.cumsum(ocnt) - ocnt
        for p in range(case.n):
            g, w = xyzw[p, :cnt[p], :3], oxyz[start[p]:start[p] + ocnt[p]]
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"stride {s}: points differ, " \
                                                                          f"{case.describe(p)}"
        assert (xyzw[..., 3] == 0.0).all()
    ctx.close()


@pytest.mark.parametrize("name", ["with_empty", "empty_first", "large"])
def test_full_render_with_colour(name):
    """render(color=True) equals oracle.render_depth_color, planes included, with every triangle's index as its colour.
    This path reads the triangle soup and the per-model ranges, not the streams; empty models and the model with NaN /
    inf vertices are new to it."""
    case = mesh_case(name)
    code = case.bank.index_colours()
    ctx = Ctx(case, colours=code)
    ctx.observe(8)  # the source depth (all zero) comes with the observation
    z, col = ctx.core.render(ctx.poses, ctx.pm, None, color=True)
    torch.cuda.synchronize()
    z, col = z.cpu().numpy(), col.cpu().numpy()
    oz, ocol = case.render_colour(code)
    assert np.array_equal(oz, case.z_full)
    bad = np.argwhere(z != oz)
    assert len(bad) == 0, f"depth: {len(bad)} pixels differ; first: {case.describe(int(bad[0][0]))}, (y, x) = " \
                          f"{tuple(bad[0][1:])}: gpu {z[tuple(bad[0])]}, oracle {oz[tuple(bad[0])]}"
    bad = np.argwhere((col != ocol).any(0))
    assert len(bad) == 0, f"colour: {len(bad)} pixels differ; first: {case.describe(int(bad[0][0]))}, (y, x) = " \
                          f"{tuple(bad[0][1:])}: gpu {col[(slice(None),) + tuple(bad[0])]}, oracle " \
                          f"{ocol[(slice(None),) + tuple(bad[0])]}"
    ctx.close()


# ---------------------------------------------------------------------------------------------
# stream knobs
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("streams,chunks", [(1, None), (3, None), (8, None), (8, 4)])
@pytest.mark.parametrize("name", ["large", "small_sizes"])
def test_stream_knobs(name, streams, chunks, monkeypatch):
    """PCORE_MODEL_STREAMS = 1, 3 and 8, and PCORE_STREAM_CHUNKS = 4 with 8 streams, set before upload_meshes:
    z-samples and type-0 costs at strides 1 and 5, and one colouring of type 1.  With 8 streams every wave of the
    workgroup walks two streams: the second one numbers its ring slots from buffer 0 again, so the records still
    pending from the first have to be flushed at the switch."""
    monkeypatch.setenv("PCORE_MODEL_STREAMS", str(streams))
    if chunks is not None:
        monkeypatch.setenv("PCORE_STREAM_CHUNKS", str(chunks))
    case = mesh_case(name)
    b = 2
    ctx = Ctx(case, colours=case.bank.colouring(b))
    for s in (1, 5):
        ctx.observe(s)
        _check_depth_costs(ctx, f"bank {name}, {streams} streams, chunks {chunks}", cost_types=(0,))
    got, _ = ctx.evaluate(1)
    _assert_costs(case, got, case.oracle_colour_costs(5, b),
                  f"bank {name}, {streams} streams, chunks {chunks}, stride 5, colouring {b}")
    ctx.close()


# ---------------------------------------------------------------------------------------------
# one context, bank after bank
# ---------------------------------------------------------------------------------------------

def test_bank_after_bank_on_one_context():
    """large, then with_empty, then small_sizes, then large again on one context: the device buffers only grow, so
    after a smaller bank the stream buffers keep the previous bank's tail behind the new padding step and pass."""
    first = Ctx(mesh_case("large"))
    ctx = first
    for i, name in enumerate(("large", "with_empty", "small_sizes", "large")):
        if i:
            ctx = Ctx(mesh_case(name), core=first.core)
        for s in (8, 2):
            ctx.observe(s)
            _check_depth_costs(ctx, f"upload {i} (bank {name})")
    first.close()


# ---------------------------------------------------------------------------------------------
# models out of range
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["with_empty", "large"])
def test_out_of_range_models_in_a_batch(name):
    """Poses with pose_model -1 and K mixed into a batch: their costs and z-samples are those of an empty model's
    pose (nothing rendered), and the other poses' are unchanged.  The same batch through render_clouds: no points."""
    case = mesh_case(name)
    K = case.bank.K
    n = case.n
    take = np.arange(0, n, 3)
    order = np.random.default_rng(5).permutation(n + len(take))
    poses = np.concatenate([case.poses, case.poses[take]])[order]
    pm = np.concatenate([case.pose_model, np.where(np.arange(len(take)) % 2 == 0, -1, K)]).astype(np.int32)[order]
    pl = np.concatenate([case.pose_label, case.pose_label[take]]).astype(np.int32)[order]
    src = np.concatenate([np.arange(n), take])[order]
    out = (pm < 0) | (pm >= K)
    assert out.sum() == len(take) and (pm == -1).any() and (pm == K).any()

    def describe(i):
        return f"batch index {i} (pose_model {pm[i]}), a copy of {case.describe(int(src[i]))}"

    ctx = Ctx(case)
    for s in (8, 1):
        ctx.observe(s)
        want_zs = np.where(out[:, None, None], 0, case.zs(s)[src])
        for ct in (2, 0):
            got, zs = ctx.evaluate(ct, zs=True, poses=_up(poses), pm=_up(pm), pl=_up(pl))
            bad = np.argwhere(zs != want_zs)
            assert len(bad) == 0, f"stride {s}, type {ct}: z-samples differ; first: {describe(int(bad[0][0]))}, " \
                                  f"(ky, kx) = {tuple(bad[0][1:])}"
            want = case.costs_of(s, ct, poses, pm, pl)
            _assert_costs(case, got, want, f"bank {name}, stride {s}, type {ct}, models out of range", describe)
            base = case.oracle_costs(s, ct)
            for g, w in zip(want, base):  # the oracle's expectation for the poses in range is their own
                assert np.array_equal(g[~out].view(np.uint32), w[src[~out]].view(np.uint32))
            assert (want[0][out] == -1.0).all()
    xyzw, cnt = ctx.core.render_clouds(_up(poses), _up(pm), None, stride=8)
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    ocnt = np.bincount(case.cloud(8)[1], minlength=n)
    assert np.array_equal(cnt, np.where(out, 0, ocnt[src]))
    ctx.close()
