"""bench.py's multi-GPU launch contract, CPU side: a WORLD_SIZE that disagrees with --gpus
exits non-zero, and `--gpus N` without a launcher refuses to start N RCCL ranks on fewer GPUs.  The N-rank run
itself is exercised on a GPU host (PCORE_DIST_BACKEND=gloo python bench.py --gpus 2).  Also bench.py's run contract:
--steps 0 is refused, and (GPU) a plain run prints the headline line without the --full legs and writes its
--dump-outputs arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, **env):
    e = dict(os.environ, **env)
    e.pop("PCORE_DIST_BACKEND", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=300)


def test_world_size_disagreeing_with_gpus_exits_nonzero():
    r = _bench(["--gpus", "1"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2 and "WORLD_SIZE=2 but --gpus 1" in r.stderr
    r = _bench(["--gpus", "4"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2


def test_gpus_n_without_enough_devices_refuses_rccl_ranks():
    import torch

    if torch.cuda.device_count() >= 2:  # a multi-GPU host would really launch the ranks
        return
    r = _bench(["--gpus", "2", "--steps", "1"])
    assert r.returncode == 2 and "needs 2 GPUs" in r.stderr


def test_zero_steps_is_refused():
    r = _bench(["--gpus", "1", "--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    """A plain run carries none of the --full legs, --steps is the number of timed steps, and --dump-outputs writes
    the last timed step's per-pose costs (float32) and decoded argmin (float64), which agree with the line's argmin."""
    import bench

    n = 300
    r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--poses", str(n), "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "poses/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - n * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert not {"roofline", "host_timing", "c3", "cpu_baseline", "cpu_reference_path"} & set(d)
    assert sorted(os.listdir(tmp_path)) == sorted(name + ".npy" for name in bench.DUMP_NAMES)
    out = {name: np.load(tmp_path / (name + ".npy")) for name in bench.DUMP_NAMES}
    for name in ("rendered_cost", "observed_cost", "points_diff"):
        assert out[name].dtype == np.float32 and out[name].shape == (n,)
    for name in ("best_cost", "best_index"):
        assert out[name].dtype == np.float64 and out[name].shape == (1,)
    assert int(out["best_cost"][0]) == d["argmin"]["best_cost"]
    assert int(out["best_index"][0]) == d["argmin"]["best_index"]
