"""GPU: the picture of the greedy state (PrintStateGPU, search_env.cpp:1718-1781, 1025-1091) from the recognizer and
from the perch_fat executable: with debug_dir set a search writes gpu-graph_state-0-color.png and
gpu-graph_state-0-depth.png, which decode to last_state's arrays; last_state is the composed-state contract
(tests/scene_reference.py) on the winners' poses rebuilt from their ContPoses; the executable, as one process and as two
gloo ranks, writes the same bytes as the API; without debug_dir nothing is rendered or written."""
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from perception_amd import io, synthetic as syn  # noqa: E402
from perception_amd.model import matrix_to_quat_xyzw  # noqa: E402
from perception_amd.recognizer import (CAM_TO_BODY, CameraIntrinsics, ModelMetaData, ObjectRecognizer,  # noqa: E402
                                       PerchParams, RecognitionInput, States)
from perception_amd.tabletop import TableParams, TabletopRecognizer, pr2_gpu_params  # noqa: E402
from tests import scene_reference as ref  # noqa: E402
from tests.helpers import oracle_render_fn  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["003_cracker_box", "005_tomato_soup_can", "061_foam_brick"]
FILES = ("gpu-graph_state-0-color.png", "gpu-graph_state-0-depth.png")


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    """A small 6-DoF scene on disk as perch_fat reads it: 20 listed poses per object, no ICP."""
    root = tmp_path_factory.mktemp("state_image")
    rng = np.random.default_rng(5)
    gts = np.stack([syn.default_gt_pose(rng, c) for c in [(-0.12, 0.0, 0.8), (0.0, 0.05, 0.85), (0.13, -0.03, 0.75)]])
    sc = syn.make_scene(NAMES, gts, oracle_render_fn, rng=rng)
    rows = []
    for k, name in enumerate(NAMES):
        os.makedirs(root / "models" / name, exist_ok=True)
        io.save_ply(str(root / "models" / name / "textured.ply"), sc.bank.models[k])
        P = syn.candidate_poses(gts[k][:3, 3], 20, rng, include=gts[k], num_viewpoints=10, inplane=2)
        lst = np.array([np.concatenate([T[:3, 3], matrix_to_quat_xyzw(T[:3, :3])]) for T in P])
        os.makedirs(root / "rendered" / name, exist_ok=True)
        io.write_poses_txt(str(root / "rendered" / name / "poses.txt"), lst, decimals=6)
        rows.append([name, str(root / "models" / name / "textured.ply"), False, False, 0, 0.06, 1])
    io.save_png(str(root / "depth.png"), sc.depth_raw.astype(np.uint16))
    io.save_png(str(root / "mask.png"), sc.mask)
    import yaml

    params = {
        "perch_params": {"sensor_resolution_radius": 0.01, "min_neighbor_points_for_valid_pose": 30,
                         "gpu_batch_size": 700, "gpu_stride": 8, "icp_type": 3, "use_color_cost": False,
                         "use_cylinder_observed": False},
        "model_bank": rows, "mesh_in_mm": False, "mesh_scaling_factor": 1.0,
        "required_object": NAMES, "use_external_pose_list": 1, "use_icp": 0, "compute_type": 1,
        "input_depth_image": str(root / "depth.png"), "predicted_mask_image": str(root / "mask.png"),
        "input_color_image": "", "depth_factor": float(sc.depth_factor), "rendered_root_dir": str(root / "rendered"),
        "camera_pose": np.linalg.inv(CAM_TO_BODY).reshape(-1).tolist(), "perch_debug_dir": str(root / "debug"),
        "camera_width": sc.width, "camera_height": sc.height, "camera_fx": float(sc.fx), "camera_fy": float(sc.fy),
        "camera_cx": float(sc.cx), "camera_cy": float(sc.cy),
    }
    with open(root / "params.yaml", "w") as f:
        yaml.safe_dump(params, f)
    return root, sc


def _recognizer(root, sc):
    from perception_amd import perch_fat as pf

    ps = pf.ParamServer([str(root / "params.yaml")])
    bank = {n: ModelMetaData(n, file=str(root / "models" / n / "textured.ply")) for n in NAMES}
    rec = ObjectRecognizer(bank, CameraIntrinsics(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy), pf.perch_params(ps), 0)
    inp = RecognitionInput(NAMES, str(root / "depth.png"), str(root / "mask.png"), depth_factor=sc.depth_factor,
                           rendered_root_dir=str(root / "rendered"), use_icp=0)
    return rec, inp


def _reference(rec, sc, res, src_cm, labels, occlude):
    """The contract on the recognizer's own meshes and the winners' poses rebuilt on the host from their ContPoses
    (ObjectRecognizer._pose_in_cam: camera * T(ContPose) * preprocess, the restatement pcore_state_poses is held to)."""
    model = np.array([rec.model_names.index(n) for n in res.model_names], np.int32)
    states = States(model, model, np.array(res.detected_poses).reshape(-1, 7))
    poses = ObjectRecognizer._pose_in_cam(rec, states)
    tris = np.concatenate([m.tris for m in rec.models])
    rgb = np.concatenate([m.colors for m in rec.models])
    scene = types.SimpleNamespace(bank=types.SimpleNamespace(tris=tris, tris_model_count=[m.num_tris for m in rec.models]),
                                  width=sc.width, height=sc.height, proj=rec.proj, src_depth_cm=src_cm,
                                  mask=getattr(sc, "mask", None))
    return poses, ref.render_scene(scene, rgb, poses, model, model if labels else None, occlude,
                                   rec.params.gpu_occlusion_threshold)


def _assert_state(got, want):
    for k, name in enumerate(("depth", "color", "owner", "visible")):
        assert np.array_equal(got[name], want[k]), name


@pytest.fixture(scope="module")
def api_run(scene_dir):
    root, sc = scene_dir
    rec, inp = _recognizer(root, sc)
    os.makedirs(root / "api", exist_ok=True)
    rec.debug_dir = str(root / "api")
    res = rec.localize_objects_greedy_render(inp)
    rec.write_outputs(res, str(root / "api"))
    return rec, res


def test_search_writes_the_state_image_and_keeps_it(scene_dir, api_run):
    root, sc = scene_dir
    rec, res = api_run
    assert res.model_names == NAMES
    st = rec.last_state
    from PIL import Image

    with Image.open(root / "api" / FILES[0]) as im:
        assert im.mode == "RGB"
        assert np.array_equal(np.asarray(im), st["color"].transpose(1, 2, 0))  # red, green, blue = planes 0, 1, 2
    with Image.open(root / "api" / FILES[1]) as im:
        assert im.mode.startswith("I;16")
        assert np.array_equal(np.asarray(im, dtype=np.uint16).astype(np.int32), st["depth"])
    assert st["depth"].shape == (sc.height, sc.width) and st["depth"].max() < 65536 and st["depth"].min() >= 0
    assert (st["visible"] > 0).all() and len(st["visible"]) == 3  # every winner shows


def test_state_image_equals_the_contract_on_the_rebuilt_poses(scene_dir, api_run):
    _, sc = scene_dir
    rec, res = api_run
    poses, want = _reference(rec, sc, res, sc.src_depth_cm, labels=False, occlude=False)
    assert np.array_equal(rec.last_state["poses"].view(np.uint32), poses.view(np.uint32))
    _assert_state(rec.last_state, want)
    # with the source: each winner's own label (6-DoF)
    _, want = _reference(rec, sc, res, sc.src_depth_cm, labels=True, occlude=True)
    out = rec.render_state(res, occlude=True)
    _assert_state(dict(zip(("poses", "depth", "color", "owner", "visible"), (t.cpu().numpy() for t in out))), want)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(cmd, env_extra=None):
    env = dict(os.environ, PYTHONPATH=ROOT, **(env_extra or {}))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r


def test_perch_fat_writes_the_same_bytes_as_the_api(scene_dir, api_run):
    root, _ = scene_dir
    _run([sys.executable, "-u", "-m", "perception_amd.perch_fat", "state_w1", "--params", str(root / "params.yaml")])
    for name in FILES + ("output_poses.txt",):
        one = (root / "debug" / "state_w1" / name).read_bytes()
        assert one and one == (root / "api" / name).read_bytes(), name


def test_perch_fat_two_ranks_write_the_same_bytes(scene_dir, api_run):
    root, _ = scene_dir
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
              "127.0.0.1", "--master-port", str(_free_port()), "-m", "perception_amd.perch_fat", "state_w2",
              "--params", str(root / "params.yaml")], {"PCORE_DIST_BACKEND": "gloo", "OMP_NUM_THREADS": "1"})
    for name in FILES + ("output_poses.txt",):
        two = (root / "debug" / "state_w2" / name).read_bytes()
        assert two and two == (root / "api" / name).read_bytes(), (name, r.stdout[-2000:])


def test_without_debug_dir_nothing_is_rendered_or_written(scene_dir, tmp_path, monkeypatch):
    root, sc = scene_dir
    rec, inp = _recognizer(root, sc)
    calls = []
    real = rec.core.render_scene
    monkeypatch.setattr(rec.core, "render_scene", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    monkeypatch.chdir(tmp_path)
    res = rec.localize_objects_greedy_render(inp)
    assert res.model_names == NAMES
    assert rec.debug_dir is None and rec.last_state is None and not calls
    assert os.listdir(tmp_path) == []
    rec.render_state(res)  # on request it still draws
    assert calls == [1]


def test_tabletop_state_image(tmp_path):
    """3-DoF: the winners' ContPoses go through the same state -> pose path, and no labels are passed."""
    names = ["003_cracker_box", "005_tomato_soup_can"]
    from perception_amd.recognizer import preprocessing_transform

    pre = [preprocessing_transform(m, six_dof=False) for m in syn.model_bank(names).models]
    sc = syn.make_tabletop_scene(names, [(0.60, -0.08, 0.4), (0.64, 0.10, 0.0)], pre, oracle_render_fn, table_height=0.7,
                                 rng=np.random.default_rng(4))
    table = TableParams(x_min=0.52, x_max=0.68, y_min=-0.16, y_max=0.16, table_height=0.7, res=0.04)
    bank = {n: ModelMetaData(n, model=sc.bank.models[i]) for i, n in enumerate(names)}
    rec = TabletopRecognizer(bank, CameraIntrinsics(sc.width, sc.height, sc.fx, sc.fy, sc.cx, sc.cy), table,
                             pr2_gpu_params(use_color_cost=False, use_cylinder_observed=False))
    rec.debug_dir = str(tmp_path)
    res = rec.localization_result(rec.localize(names, sc.depth_raw, sc.camera_pose, sc.depth_factor))
    assert len(res.model_names) >= 1 and all(os.path.exists(tmp_path / f) for f in FILES)
    src_cm = (sc.depth_raw.astype(np.float32) / (np.float32(sc.depth_factor) / np.float32(100))).astype(np.int32)
    poses, want = _reference(rec, sc, res, src_cm, labels=False, occlude=False)
    assert np.array_equal(rec.last_state["poses"].view(np.uint32), poses.view(np.uint32))
    assert rec.last_state["depth"].any()
    _assert_state(rec.last_state, want)
    _, want = _reference(rec, sc, res, src_cm, labels=False, occlude=True)  # the threshold rule, no labels
    out = rec.render_state(res, occlude=True)
    _assert_state(dict(zip(("poses", "depth", "color", "owner", "visible"), (t.cpu().numpy() for t in out))), want)
