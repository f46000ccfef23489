"""pcore_select_topk without a GPU: the numpy restatement of its rule (tests/topk_reference.py) against the oracle's
selection at k = 1, the entry point's argument checks, and the shortlist exchange between two gloo ranks."""
import ctypes
import os
import socket

import numpy as np
import torch.multiprocessing as mp

from tests import topk_reference as ref


def hard_costs(rng, n, num_models):
    """Costs with everything the key has to handle: small integers (many equal costs), fractions, NaN, +-inf, negative
    values, rc = -1, |(int) rc - (int) oc| of 29 and 30, sums at the int32 range's edge, model ids -1 and num_models."""
    rc = rng.integers(0, 40, n).astype(np.float32)
    oc = rng.integers(0, 40, n).astype(np.float32)
    frac = rng.random(n) < 0.3
    rc[frac] += rng.random(int(frac.sum())).astype(np.float32)
    pm = rng.integers(0, num_models, n).astype(np.int32)
    special = [(np.nan, 3.0), (3.0, np.nan), (np.nan, np.nan), (np.inf, 1.0), (1.0, np.inf), (-np.inf, 1.0),
               (1.0, -np.inf), (np.inf, -np.inf), (-1.0, 5.0), (-1.0, -1.0), (5.0, -1.0), (-2.0, 1.0), (-0.5, 0.25),
               (0.0, -0.5), (0.0, np.nan), (40.0, 11.0), (40.0, 10.0), (11.0, 40.0), (10.0, 40.0), (3.0e9, 3.0e9),
               (1.0737418e9, 1.0737418e9), (2147483520.0, 2147483520.0), (0.0, 0.0), (-3.0e9, 1.0)]
    at = rng.choice(n, min(n, 3 * len(special)), replace=False)
    for j, i in enumerate(at):
        rc[i], oc[i] = special[j % len(special)]
    if n >= 8:
        out = rng.choice(n, max(2, n // 16), replace=False)
        pm[out[::2]] = -1
        pm[out[1::2]] = num_models
    return rc, oc, pm


def test_reference_at_k1_equals_oracle_select():
    import oracle
    from perception_amd.core import decode_keys

    rng = np.random.default_rng(11)
    for n, M, base in [(1, 1, 0), (97, 1, 0), (500, 3, 0), (2000, 5, 12345), (300, 7, 2 ** 31 - 300)]:
        rc, oc, pm = hard_costs(rng, n, M)
        # the oracle indexes its result by the model id unchecked: it gets the ids shifted by one and two more models,
        # so that ids -1 and M have rows of their own (dropped here; the restatement ignores those poses)
        ocost, oidx = (r[1:M + 1] for r in oracle.select(rc, oc, pm + 1, M + 2, index_base=base))
        cost, idx = decode_keys(ref.topk(rc, oc, pm, M, 1, index_base=base)[:, 0])
        found = oidx >= 0
        assert np.array_equal(idx >= 0, found), (n, M)
        assert np.array_equal(idx[found], oidx[found]) and np.array_equal(cost[found], ocost[found]), (n, M)
    # the list at any k is the sorted valid keys of the model, cut and padded: its first column is the k = 1 list
    rc, oc, pm = hard_costs(rng, 700, 4)
    full = ref.topk(rc, oc, pm, 4, 64)
    assert np.array_equal(full[:, :1], ref.topk(rc, oc, pm, 4, 1))
    assert (np.diff(full, axis=1) >= 0).all()
    valid = full[full != ref.KEY_NONE]
    assert len(np.unique(valid)) == len(valid)


def test_select_topk_checks_its_arguments_before_any_launch():
    from perception_amd import _native

    lib = _native.load()
    bad = _native.PCORE_E_INVALID_ARG
    assert lib.pcore_select_topk(None, None, None, None, 0, 0, 1, 1, None, None) == bad  # NULL context
    for k in (0, 65, -1):
        assert lib.pcore_select_topk(None, None, None, None, 0, 0, 1, k, None, None) == bad
    assert lib.pcore_select_topk(None, None, None, None, 0, 0, 0, 1, None, None) == bad  # num_models 0
    import torch

    if torch.cuda.is_available():  # with a context the checks themselves answer (none of the calls launches)
        h = ctypes.c_void_p()
        assert lib.pcore_create(0, ctypes.byref(h)) == _native.PCORE_OK
        try:
            for k in (0, 65, -1):
                assert lib.pcore_select_topk(h, None, None, None, 0, 0, 1, k, None, None) == bad
            assert lib.pcore_select_topk(h, None, None, None, 0, 0, 0, 1, None, None) == bad
            assert lib.pcore_select_topk(h, None, None, None, -1, 0, 1, 1, None, None) == bad
            assert lib.pcore_select_topk(h, None, None, None, 4, 0, 1, 1, None, None) == bad  # NULL arrays
            assert lib.pcore_select_topk(h, None, None, None, 0, 2 ** 31 + 1, 1, 1, None, None) == bad
            assert lib.pcore_select_topk(h, None, None, None, 0, 0, 1, 64, None, None) == _native.PCORE_OK
        finally:
            lib.pcore_destroy(h)


def test_icp_top_k_parameter_defaults_to_the_reference_flow():
    """PerchParams.icp_top_k is 0 unless /perch_params/icp_top_k sets it (perch_fat's parameter table)."""
    from perception_amd.perch_fat import ParamServer, perch_params
    from perception_amd.recognizer import PerchParams

    assert PerchParams().icp_top_k == 0
    assert perch_params(ParamServer()).icp_top_k == 0
    p = perch_params(ParamServer([{"perch_params": {"icp_top_k": 16, "icp_type": 3}}]))
    assert p.icp_top_k == 16 and isinstance(p.icp_top_k, int) and p.icp_type == 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, lists, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist

    from perception_amd.distributed import allgather_topk_keys, init_from_env

    mine = torch.from_numpy(lists[rank].copy())
    alone = allgather_topk_keys(mine)  # no process group yet: the argument itself
    init_from_env("gloo")
    got = allgather_topk_keys(mine)
    q.put((rank, alone is mine, got.numpy().copy(), mine.numpy().copy()))
    dist.destroy_process_group()


def test_gloo_world2_shortlists_equal_topk_of_the_union():
    """Two ranks' lists of their own shards: duplicated costs across the ranks (the index decides), one model with
    fewer than k poses on both ranks together, one with poses on one rank only, one with none at all."""
    from perception_amd.distributed import shard_range

    rng = np.random.default_rng(5)
    n, M, k = 900, 5, 16
    rc = rng.integers(0, 6, n).astype(np.float32)  # few distinct costs: every one occurs on both ranks
    oc = rng.integers(0, 6, n).astype(np.float32)
    pm = rng.integers(0, 2, n).astype(np.int32)
    pm[[10, 700, 820]] = 2          # fewer than k in all
    pm[[5, 17, 300]] = 3            # rank 0's shard only
    lists = []
    for r in range(2):
        lo, hi = shard_range(n, r, 2)
        lists.append(ref.topk(rc[lo:hi], oc[lo:hi], pm[lo:hi], M, k, index_base=lo))
    want = ref.topk(rc, oc, pm, M, k)
    assert np.array_equal(ref.union_topk(lists, k), want)
    assert (want[2] != ref.KEY_NONE).sum() == 3 and (want[4] == ref.KEY_NONE).all()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, lists, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, alone, got, mine in res:
        assert alone
        assert got.dtype == np.int64 and np.array_equal(got, want), rank
        assert np.array_equal(mine, lists[rank])  # the argument is left as it was
