"""GPU: pcore_select_topk against the numpy restatement (tests/topk_reference.py), bit for bit -- shapes around the
wave and the slice of the partial kernel, merge orders, special values, folding across batches and graph capture."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from perception_amd import _native  # noqa: E402
from perception_amd._native import PCORE_KEY_NONE, PCORE_TOPK_SLICE, PcoreError  # noqa: E402
from perception_amd.core import PoseCore  # noqa: E402
from tests import topk_reference as ref  # noqa: E402
from tests.test_topk_spec import hard_costs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S = PCORE_TOPK_SLICE
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 3 * S + 1)
KS = (1, 2, 7, 16, 63, 64)


@pytest.fixture(scope="module")
def core():
    return PoseCore(0)  # the selection needs no meshes, camera or observation


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(core, rc, oc, pm, M, k, base=0, topk=None):
    return core.select_topk(_dev(rc), _dev(oc), _dev(pm), M, k, index_base=base, topk=topk)


def _models(rng, n, M, grouped):
    pm = rng.integers(0, M, n).astype(np.int32)
    return np.sort(pm) if grouped else pm


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("M", [1, 5, 21, 33])
def test_shapes(core, M, grouped):
    rng = np.random.default_rng(100 + M + int(grouped))
    for n in SIZES:
        pm = _models(rng, n, M, grouped)
        rc = rng.integers(0, 25, n).astype(np.float32)  # few distinct costs: equal costs in every list
        oc = rng.integers(0, 25, n).astype(np.float32)
        d_rc, d_oc, d_pm = _dev(rc), _dev(oc), _dev(pm)
        keys = ref.select_keys(rc, oc, pm, M)
        for k in KS:
            got = core.select_topk(d_rc, d_oc, d_pm, M, k)
            assert got.shape == (M, k) and got.dtype == torch.int64
            assert np.array_equal(got.cpu().numpy(), ref.topk_of_keys(keys, pm, M, k)), (n, M, k, grouped)


@pytest.mark.parametrize("k", KS)
def test_orders(core, k):
    M, n = 3, 2 * S + 77
    pm = (np.arange(n) % M).astype(np.int32)
    # all costs equal: the index order decides
    rc, oc = np.full(n, 7.0, np.float32), np.full(n, 5.0, np.float32)
    want = ref.topk(rc, oc, pm, M, k)
    assert np.array_equal(want[0], (np.int64(12 ^ 0x80000000) << 31) | (np.arange(k, dtype=np.int64) * M))
    assert np.array_equal(_run(core, rc, oc, pm, M, k).cpu().numpy(), want)
    # costs strictly descending: every step of every wave merges
    rc = np.arange(n, 0, -1).astype(np.float32)
    oc = rc.copy()
    want = ref.topk(rc, oc, pm, M, k)
    assert (want[:, 0] & 0x7FFFFFFF).min() >= n - M
    assert np.array_equal(_run(core, rc, oc, pm, M, k).cpu().numpy(), want)
    # fewer than k valid poses (model 1: three, in different slices; model 2: one), model 0: none at all
    rc, oc = np.full(n, -1.0, np.float32), np.zeros(n, np.float32)
    m1 = np.nonzero(pm == 1)[0]
    for i in (m1[0], m1[m1 >= S][0], m1[m1 >= 2 * S][0], np.nonzero(pm == 2)[0][0]):
        rc[i] = oc[i] = float(n - i)
    want = ref.topk(rc, oc, pm, M, k)
    assert (want[0] == PCORE_KEY_NONE).all() and (want[1] != PCORE_KEY_NONE).sum() == min(k, 3)
    assert np.array_equal(_run(core, rc, oc, pm, M, k).cpu().numpy(), want)
    # no valid pose at all
    rc[:] = -1.0
    assert (_run(core, rc, oc, pm, M, k).cpu().numpy() == PCORE_KEY_NONE).all()


@pytest.mark.parametrize("k", [1, 7, 64])
def test_values(core, k):
    rng = np.random.default_rng(7)
    M = 5
    for n in (257, 3 * S + 1):
        rc, oc, pm = hard_costs(rng, n, M)
        want = ref.topk(rc, oc, pm, M, k)
        assert (want != PCORE_KEY_NONE).any()
        assert np.array_equal(_run(core, rc, oc, pm, M, k).cpu().numpy(), want), (n, k)
        base = 2 ** 31 - n  # the last global index is 2^31 - 1
        want = ref.topk(rc, oc, pm, M, k, index_base=base)
        got = _run(core, rc, oc, pm, M, k, base=base).cpu().numpy()
        assert np.array_equal(got, want), (n, k)
        assert (got[got != PCORE_KEY_NONE] & 0x7FFFFFFF).max() <= 2 ** 31 - 1
    # one past the index range is refused
    with pytest.raises(PcoreError) as ei:
        _run(core, rc, oc, pm, M, k, base=2 ** 31 - n + 1)
    assert ei.value.code == _native.PCORE_E_INVALID_ARG


@pytest.mark.parametrize("k", [1, 16, 64])
def test_folding(core, k):
    rng = np.random.default_rng(21)
    M, n, base = 5, 3 * S + 1, 1000
    rc, oc, pm = hard_costs(rng, n, M)
    want = ref.topk(rc, oc, pm, M, k, index_base=base)
    one = _run(core, rc, oc, pm, M, k, base=base).cpu().numpy()
    assert np.array_equal(one, want)
    cuts = [0, 70, S + 131, n]  # three unequal pieces
    pieces = [(cuts[j], cuts[j + 1]) for j in range(3)]
    for order in (pieces, pieces[::-1]):
        topk = torch.full((M, k), PCORE_KEY_NONE, dtype=torch.int64, device=DEV)
        for lo, hi in order:
            out = _run(core, rc[lo:hi], oc[lo:hi], pm[lo:hi], M, k, base=base + lo, topk=topk)
            assert out is topk
        assert np.array_equal(topk.cpu().numpy(), want), (k, order)
    # an empty batch leaves the lists as they are
    _run(core, rc[:0], oc[:0], pm[:0], M, k, base=base, topk=topk)
    assert np.array_equal(topk.cpu().numpy(), want)
    if k == 1:  # the row is what pcore_select leaves in d_keys[m]
        keys = core.select(_dev(rc), _dev(oc), _dev(pm), M, index_base=base)
        assert np.array_equal(keys.cpu().numpy(), one[:, 0])
    with pytest.raises(ValueError):
        _run(core, rc, oc, pm, M, k, topk=torch.full((M, k + 1), PCORE_KEY_NONE, dtype=torch.int64, device=DEV))


def test_graph_capture():
    rng = np.random.default_rng(33)
    M, k, n = 5, 16, 2 * S + 9
    core = PoseCore(0)
    rc, oc, pm = hard_costs(rng, n, M)
    d_rc, d_oc, d_pm = _dev(rc), _dev(oc), _dev(pm)
    topk = torch.full((M, k), PCORE_KEY_NONE, dtype=torch.int64, device=DEV)
    # a capture that would have to allocate the partial lists is refused
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(PcoreError) as ei:
            core.select_topk(d_rc, d_oc, d_pm, M, k, topk=topk)
    assert ei.value.code == _native.PCORE_E_STATE
    del graph
    # after one eager call the capture succeeds and replays to the same lists
    want = ref.topk(rc, oc, pm, M, k)
    assert np.array_equal(core.select_topk(d_rc, d_oc, d_pm, M, k, topk=topk).cpu().numpy(), want)
    gen = core.generation()
    topk.fill_(PCORE_KEY_NONE)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        core.select_topk(d_rc, d_oc, d_pm, M, k, topk=topk)
    assert core.generation() == gen
    topk.fill_(PCORE_KEY_NONE)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(topk.cpu().numpy(), want)
    # new costs in the captured tensors, the lists reset: the replay ranks the new batch
    rc2, oc2, _ = hard_costs(rng, n, M)
    d_rc.copy_(_dev(rc2))
    d_oc.copy_(_dev(oc2))
    topk.fill_(PCORE_KEY_NONE)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(topk.cpu().numpy(), ref.topk(rc2, oc2, pm, M, k))
    # a larger batch needs more partial lists: refused while capturing, and it would change the generation
    big = _dev(np.zeros(5 * S, np.float32))
    big_pm = _dev(np.zeros(5 * S, np.int32))
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        with pytest.raises(PcoreError) as ei:
            core.select_topk(big, big, big_pm, M, k)
    assert ei.value.code == _native.PCORE_E_STATE
    assert core.generation() == gen
