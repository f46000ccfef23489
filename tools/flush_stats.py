#!/usr/bin/env python
"""Small-triangle flush statistics of the fused kernel (C2 workload) from a -DPCORE_FLUSH_STATS build
(PCORE_LIB=build_ab/fst.so), one launch, per pose: flush batches (64 lanes), queued records, fragment tests,
partial flushes forced by the vertex ring or a stream switch, big (cooperative) triangles, triangles touching
a sample, triangle lanes, triangle batches (steps), vertex passes and the steps that enter the general path
behind the one-sample fast path.  --mesh NAME and --cam 1280 give the other single-mesh workloads of
tools/bench_configs.py (C2:scan_blob, C5/8's camera)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from perception_amd import _native, synthetic, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="003_cracker_box")
ap.add_argument("--cam", default="640", choices=("640", "1280"))
ap.add_argument("--poses", type=int, default=10000)
a = ap.parse_args()
w = workloads.build(names=[a.mesh], poses_per_model=a.poses,
                    cam=synthetic.CAM_1280 if a.cam == "1280" else synthetic.CAM_640)
w.core.evaluate(w.poses, w.pose_model, w.pose_label, w.pose_obs_total, stride=w.stride)
torch.cuda.synchronize()
L = _native.load()
L.pcore_debug_flush_stats.argtypes = [ctypes.c_void_p]
base = np.zeros(10, dtype=np.uint64)
assert L.pcore_debug_flush_stats(base.ctypes.data) == 0
w.core.evaluate(w.poses, w.pose_model, w.pose_label, w.pose_obs_total, stride=w.stride)
torch.cuda.synchronize()
after = np.zeros(10, dtype=np.uint64)
assert L.pcore_debug_flush_stats(after.ctypes.data) == 0
d = (after - base).astype(np.int64) / float(a.poses)
names = ["batches", "records", "frag_tests", "forced_flushes", "big_tris", "tris_touching", "tri_lanes", "tri_steps",
         "vertex_passes", "slow_steps"]
res = {k: float(v) for k, v in zip(names, d)}
res["slow_step_share"] = res["slow_steps"] / max(res["tri_steps"], 1e-9)
res["lane_util_flush"] = res["records"] / max(res["batches"] * 64, 1)
print(json.dumps({"mesh": a.mesh, "cam": a.cam, "poses": a.poses, "per_pose": res}))
