"""The stream builder (perception_amd/csrc/pcore_streams.h) never needs more vertex passes or steps than its baseline
did: for every YCB proxy and both scan meshes the builder's invariants hold (tools/stream_stats.cpp, stream_check) and
its passes and steps are at most the counts recorded in tests/golden/stream_counts_parent.json -- the builder before the
look-ahead batches and the band orders, with the fused kernel's four streams, four-pass ring and one chunk per stream.
CPU only (g++, no HIP)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from perception_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS, VRING, REF_PASSES, CHUNKS = 4, 4, 2, 1  # pcore_internal.h: kFusedWaves, kVRing, kRefPasses, kStreamChunks

with open(os.path.join(ROOT, "tests", "golden", "stream_counts_parent.json")) as _f:
    PARENT = json.load(_f)
MESHES = list(syn.YCB_PROXIES) + list(syn.SCAN_MESHES)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("stream_counts") / "libstreamcheck.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "stream_stats.cpp"),
                    "-o", str(out)], check=True)
    L = ctypes.CDLL(str(out))
    L.stream_check.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.c_void_p]
    L.stream_check.restype = ctypes.c_int
    return L


def test_fixture_covers_every_mesh():
    assert sorted(PARENT) == sorted(MESHES)
    assert PARENT["003_cracker_box"] == {"passes": 110, "steps": 195, "verts": 6146, "tris": 12288}  # the C2 mesh


@pytest.mark.parametrize("name", MESHES)
def test_passes_and_steps_do_not_exceed_the_parent(lib, name):
    tris = np.ascontiguousarray(syn.ycb_proxy(name).tris, dtype=np.float32).reshape(-1, 9)
    info = np.zeros(4, np.int64)
    rc = lib.stream_check(tris.ctypes.data, tris.shape[0], STREAMS, VRING, REF_PASSES, CHUNKS, info.ctypes.data)
    assert rc == 0, f"stream invariant {-rc} broken"
    passes, steps, verts, streams = info.tolist()
    want = PARENT[name]
    assert (verts, tris.shape[0]) == (want["verts"], want["tris"])  # the mesh the counts were recorded for
    assert streams == STREAMS
    assert passes <= want["passes"] and steps <= want["steps"], (passes, steps, want)
    assert passes * 64 >= verts and steps * 64 >= tris.shape[0]  # every vertex loaded, every triangle in a slot
