"""CPU certificates of tests/fallback_ring_cases.py: the GPU tests of tests/test_gpu_depth_fallback_ring.py could fail.
With the stream builder and a float32 restatement of the vertex pass, the reference's barycentrics and the IEEE depth
chain (no GPU): the `wrap` model is one stream of at least 6 vertex passes, the `switch` model 8 streams, the `one`
model one triangle; the poses are of the interior and of the fastdiv class; and for every fragment inside its triangle
the IEEE quotient Q lies within 2^-21 Q of the patch's k + 0.5, so the certified depth (bracket 2^-19 |f| around an
estimate f within 2^-20 of Q) cannot decide int(Q + 0.5) and takes the fallback."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import fallback_ring_cases as fc
from tests import interior_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VRING, REF_PASSES, WAVES, CHUNKS = 4, 2, 4, 1  # pcore_internal.h: kVRing, kRefPasses, kFusedWaves, kStreamChunks


@pytest.fixture(scope="module")
def builder(tmp_path_factory):
    out = tmp_path_factory.mktemp("fallback_streams") / "libstreamstats.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "stream_stats.cpp"),
                    "-o", str(out)], check=True)
    L = ctypes.CDLL(str(out))
    L.stream_check.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    L.stream_check.restype = ctypes.c_int

    def info(name):
        t = np.ascontiguousarray(fc.mesh(name)[0], np.float32)
        out = np.zeros(4, np.int64)  # passes, steps, vertices, streams
        assert L.stream_check(t.ctypes.data, len(t), fc.MODELS[name][1] or WAVES, VRING, REF_PASSES, CHUNKS,
                              out.ctypes.data) == 0
        return out

    return info


def test_the_streams_are_the_ones_described(builder):
    passes, _, _, streams = builder("wrap")
    assert streams == 1 and passes >= 6 > VRING  # the ring wraps within the stream
    passes, _, _, streams = builder("switch")
    assert streams == 8 == 2 * WAVES and passes >= 16  # every wave walks two streams
    assert builder("one")[3] == 1 and len(fc.mesh("one")[0]) == 1


def test_the_poses_are_interior_and_border():
    for name in fc.MODELS:
        c = fc.case(name)
        assert [ic.pose_class(m, c.bank.tris, fc.CAM) for m in c.poses] == [2, 1], name
        # the patches are fronto-parallel at k + 0.5 cm exactly
        for m in c.poses:
            lz = ic.vertex_pass(m, c.bank.tris.reshape(-1, 3), fc.CAM)[2].reshape(-1, 3)
            assert np.array_equal(lz, np.repeat(c.tris_k[:, None] + 0.5, 3, axis=1).astype(np.float32))


@pytest.mark.parametrize("stride", fc.STRIDES)
@pytest.mark.parametrize("name", list(fc.MODELS))
def test_covered_samples_take_the_fallback(name, stride):
    c = fc.case(name)
    for pose in range(c.n):
        fr = c.fragments(pose, stride)
        zs = c.zs(stride)[pose]
        # the restatement finds the oracle's covered samples
        cov = np.zeros(zs.shape, bool)
        cov[fr[:, 1].astype(int), fr[:, 0].astype(int)] = True
        assert np.array_equal(cov, zs > 0), c.describe(pose)
        rel = np.abs(fr[:, 3] - (fr[:, 2] + 0.5)) / fr[:, 3]
        good = rel <= 2.0 ** -21
        # a sample counts where every fragment on it does (whichever wins took the fallback)
        bad = np.zeros(zs.shape, bool)
        bad[fr[~good, 1].astype(int), fr[~good, 0].astype(int)] = True
        n_cov, n_good = int(cov.sum()), int((cov & ~bad).sum())
        print(f"{c.describe(pose)}, stride {stride}: {n_good} of {n_cov} covered samples certified, largest relative "
              f"distance {rel.max():.3g}")
        assert n_cov >= (8 if name != "one" or stride == 2 else 4) and 2 * n_good >= n_cov
        # and the oracle's depth there is k or k + 1 of some patch covering the sample
        ks = {}
        for kx, ky, k, _ in fr:
            ks.setdefault((int(ky), int(kx)), set()).update((int(k), int(k) + 1))
        assert all(int(zs[p]) in v for p, v in ks.items())
