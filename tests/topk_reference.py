"""numpy restatement of pcore_select's key (include/pcore.h, pcore_raster.h select_key; search_env.cpp:1987-2051,
2554-2566) and of pcore_select_topk's rule: per model, the k smallest keys in ascending order, padded with
PCORE_KEY_NONE.  Float-to-int conversions are x86 cvttss2si (recognizer.cvtt_i32), sums are float32."""
import numpy as np

from perception_amd.recognizer import cvtt_i32

KEY_NONE = np.int64(0x7FFFFFFFFFFFFFFF)
INT_MAX = 2 ** 31 - 1


def _wrap_i32(x):
    """An int64 array reduced to two's-complement int32 values."""
    return ((np.asarray(x, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def select_keys(rc, oc, pose_model, num_models, index_base=0):
    """Every pose's key: ((cost ^ 0x80000000) << 31) | (index_base + i), or KEY_NONE where the selection skips it."""
    rc, oc = np.asarray(rc, np.float32), np.asarray(oc, np.float32)
    pm = np.asarray(pose_model, np.int64)
    target, source = cvtt_i32(rc), cvtt_i32(oc)
    with np.errstate(invalid="ignore", over="ignore"):
        total = cvtt_i32(rc + oc)  # a float32 sum
    cost = np.where(target < 0, -1, total)
    d = _wrap_i32(target - source)            # the int32 difference, wrapped
    adiff = _wrap_i32(np.where(d < 0, -d, d))  # abs() of it: INT_MIN stays INT_MIN
    ok = (cost != -1) & (cost != -2) & (adiff < 30) & (cost != INT_MAX) & (pm >= 0) & (pm < num_models)
    hi = (cost & 0xFFFFFFFF) ^ 0x80000000
    idx = (np.int64(index_base) + np.arange(len(rc), dtype=np.int64)) & 0x7FFFFFFF
    return np.where(ok, (hi << 31) | idx, KEY_NONE).astype(np.int64)


def topk_of_keys(keys, pose_model, num_models, k, prev=None):
    """(num_models, k): per model the k smallest of its poses' keys and of prev's row, ascending, KEY_NONE padded."""
    keys, pm = np.asarray(keys, np.int64), np.asarray(pose_model, np.int64)
    out = np.full((num_models, k), KEY_NONE, np.int64)
    for m in range(num_models):
        mine = keys[(pm == m) & (keys != KEY_NONE)]
        if prev is not None:
            row = np.asarray(prev[m], np.int64)
            mine = np.concatenate([mine, row[row != KEY_NONE]])
        mine = np.sort(mine)[:k]
        out[m, :len(mine)] = mine
    return out


def topk(rc, oc, pose_model, num_models, k, index_base=0, prev=None):
    return topk_of_keys(select_keys(rc, oc, pose_model, num_models, index_base), pose_model, num_models, k, prev)


def union_topk(lists, k):
    """The k smallest per model of several (M, k') lists' union, ascending, KEY_NONE padded."""
    allk = np.sort(np.concatenate([np.asarray(l, np.int64) for l in lists], axis=1), axis=1)
    out = np.full((allk.shape[0], k), KEY_NONE, np.int64)
    out[:, :min(k, allk.shape[1])] = allk[:, :k]
    return out
