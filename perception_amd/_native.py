"""ctypes binding of libpcore.so (include/pcore.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, importing the
binding raises.  `load()` never builds implicitly on a machine without hipcc.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import build as _build

PCORE_OK = 0
PCORE_E_INVALID_ARG = 1
PCORE_E_HIP = 2
PCORE_E_OOM = 3
PCORE_E_STATE = 4
PCORE_KEY_NONE = 0x7FFFFFFFFFFFFFFF
# pcore_select_topk (include/pcore.h): the largest k, and the poses per partial list of a batch of at most 2^20 poses
PCORE_TOPK_MAX = 64
PCORE_TOPK_SLICE = 1024
# pcore_evaluate_states (include/pcore.h): the most observed points whose explained bitmap lives in LDS
PCORE_STATE_LDS_OBS = 131072

COST_DEPTH_3DOF = 0
COST_RGBD_3DOF = 1
COST_DEPTH_6DOF = 2

# every symbol declared in include/pcore.h
EXPORTED_SYMBOLS = (
    "pcore_create", "pcore_destroy", "pcore_last_error", "pcore_abi_version", "pcore_upload_meshes",
    "pcore_set_camera", "pcore_observed_cloud", "pcore_set_observation", "pcore_evaluate", "pcore_evaluate_icp",
    "pcore_render", "pcore_render_scene",
    "pcore_depth_to_cloud", "pcore_select", "pcore_pose_distances",
    "pcore_observed_cloud_bounded", "pcore_set_observation_colors", "pcore_generation", "pcore_get_stats",
    "pcore_count_within", "pcore_state_poses", "pcore_evaluate_select", "pcore_get_tile_info", "pcore_debug_lm_solve",
    "pcore_debug_covariances", "pcore_debug_covariances_cloud", "pcore_depth_to_cloud_ex",
    "pcore_icp_planar", "pcore_debug_planar_step",
    "pcore_scene_projective", "pcore_debug_render_clouds", "pcore_debug_colour_distance",
    "pcore_select_topk", "pcore_evaluate_states",
)
# declared in include/pcore.h too; kept apart because tests/test_abi.py's symbol pattern stops at a digit
EXPORTED_SYMBOLS_WITH_DIGITS = ("pcore_icp_point2plane", "pcore_debug_p2p_clouds", "pcore_debug_rgb2lab",
                                "pcore_icp_point2plane_nn", "pcore_debug_p2p_nn_clouds")


class PcoreError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pcore error {code}: {msg}")
        self.code = code


class Camera(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fx", ctypes.c_float),
                ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("proj", ctypes.c_float * 16)]


class EvalParams(ctypes.Structure):
    _fields_ = [("cost_type", ctypes.c_int32), ("calc_obs_cost", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("depth_factor", ctypes.c_float), ("sensor_resolution", ctypes.c_float),
                ("occlusion_threshold", ctypes.c_float), ("color_distance_threshold", ctypes.c_float)]


class GpuStats(ctypes.Structure):
    """pcore_gpu_stats (include/pcore.h; the reference's gpu_stats, model.h:24-27)."""
    _fields_ = [("icp_runtime", ctypes.c_float), ("peak_memory_usage", ctypes.c_double), ("gicp_ms", ctypes.c_float),
                ("icp_chunks", ctypes.c_int32), ("gicp_iterations", ctypes.c_int64),
                ("gicp_iterations_run", ctypes.c_int64), ("gicp_cycle_exits", ctypes.c_int64)]


MAX_TILE_TIERS = 8


class TileInfo(ctypes.Structure):
    """pcore_tile_info (include/pcore.h): the fused window launch's LDS tile and its window histogram."""
    _fields_ = [("num_tiers", ctypes.c_int32), ("tier", ctypes.c_int32), ("tcap", ctypes.c_int32),
                ("seq", ctypes.c_int32), ("edge", ctypes.c_int32 * MAX_TILE_TIERS),
                ("wgs_per_cu", ctypes.c_int32 * MAX_TILE_TIERS), ("hist", ctypes.c_int32 * (MAX_TILE_TIERS + 1)),
                ("chunked", ctypes.c_int32)]


class IcpParams(ctypes.Structure):
    _fields_ = [("k_correspondences", ctypes.c_int32), ("max_iterations", ctypes.c_int32),
                ("rotation_epsilon", ctypes.c_double), ("transformation_epsilon", ctypes.c_double),
                ("cycle_exit_window", ctypes.c_int32)]


class PlanarIcpParams(ctypes.Structure):
    """pcore_planar_icp_params (include/pcore.h)."""
    _fields_ = [("max_iterations", ctypes.c_int32), ("max_correspondence", ctypes.c_float),
                ("transformation_epsilon", ctypes.c_double), ("fitness_epsilon", ctypes.c_double)]


class P2pIcpParams(ctypes.Structure):
    """pcore_p2p_icp_params (include/pcore.h)."""
    _fields_ = [("max_iterations", ctypes.c_int32), ("relative_fitness", ctypes.c_float),
                ("relative_rmse", ctypes.c_float), ("max_dist_diff", ctypes.c_float)]


class NnIcpParams(ctypes.Structure):
    """pcore_nn_icp_params (include/pcore.h)."""
    _fields_ = [("max_iterations", ctypes.c_int32), ("relative_fitness", ctypes.c_float),
                ("relative_rmse", ctypes.c_float), ("max_dist_diff", ctypes.c_float), ("window", ctypes.c_int32)]


# ICPConvergenceCriteria (cuda_icp icp.h:39-51) and Scene_projective's max_dist_diff (depth_scene.h:9)
P2P_MAX_ITER = 30
P2P_REL_FITNESS = 1e-5
P2P_REL_RMSE = 1e-5
P2P_MAX_DIST_DIFF = 0.1
# Scene_nn's radius (pcd_scene.h:49) and the search window's half-width in pixels
NN_MAX_DIST_DIFF = 0.01
NN_WINDOW = 32
NN_MAX_WINDOW = 128

# GetICPAdjustedPose's settings (search_env.cpp:6235-6396; env_config.yaml max_icp_iterations, icp_max_correspondence)
PLANAR_MAX_ITER = 20
PLANAR_MAX_CORRESPONDENCE = 0.05
PLANAR_TRANS_EPS = 1e-8
PLANAR_FIT_EPS = 1e-5
# pcore_icp_planar's status values
PLANAR_ITERATION_CAP, PLANAR_TRANSFORM, PLANAR_ABS_MSE, PLANAR_REL_MSE, PLANAR_NO_CORRESPONDENCES, PLANAR_EMPTY_RENDER = \
    range(6)

# renderer.cu:1696-1699
ICP_K = 10
ICP_MAX_ITER = 150
# renderer.cu:1698-1699 declares both as float and passes them to set_*_epsilon(double): the float values widened
ICP_ROT_EPS = float(np.float32(2e-3))
ICP_TRANS_EPS = float(np.float32(5e-4))
# the GICP cycle exit's window (include/pcore.h PCORE_GICP_CYCLE_WINDOW; 0 = off)
ICP_CYCLE_WINDOW = 8

_lib = None


def library_path() -> str:
    return _build.LIB


def load(auto_build: bool = True) -> ctypes.CDLL:
    """Load libpcore.so (building it in-tree first when hipcc is available and sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    override = os.environ.get("PCORE_LIB")  # A/B profiling of alternative builds of the same sources
    if override:
        auto_build = False
    if auto_build:
        try:
            if _build.needs_build():
                _build.build()
        except (RuntimeError, OSError) as e:  # no hipcc on this machine: fall through to the prebuilt .so
            if not os.path.exists(_build.LIB):
                raise RuntimeError(f"libpcore.so is missing and cannot be built: {e}") from e
    path = override or _build.LIB
    if not os.path.exists(path):
        raise RuntimeError(f"libpcore.so not found at {path}; run `python -m perception_amd.build`")
    L = ctypes.CDLL(path)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    L.pcore_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.pcore_destroy.argtypes = [vp]
    L.pcore_destroy.restype = None
    L.pcore_last_error.argtypes = [vp]
    L.pcore_last_error.restype = ctypes.c_char_p
    L.pcore_abi_version.argtypes = []
    L.pcore_upload_meshes.argtypes = [vp, vp, vp, i32, vp, i32]
    L.pcore_set_camera.argtypes = [vp, ctypes.POINTER(Camera)]
    L.pcore_observed_cloud.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, vp, i32, ctypes.POINTER(i32), vp]
    L.pcore_set_observation.argtypes = [vp, vp, vp, vp, vp, i32, f32, vp]
    L.pcore_evaluate.argtypes = [vp, vp, vp, vp, vp, i32, ctypes.POINTER(EvalParams), vp, vp, vp, vp, vp]
    L.pcore_evaluate_icp.argtypes = [vp, vp, vp, vp, vp, i32, ctypes.POINTER(EvalParams), ctypes.POINTER(IcpParams),
                                     vp, vp, vp, vp, vp, vp]
    L.pcore_render.argtypes = [vp, vp, vp, vp, i32, f32, vp, vp, vp]
    if hasattr(L, "pcore_render_scene"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_render_scene.argtypes = [vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp]
    L.pcore_get_stats.argtypes = [vp, ctypes.POINTER(GpuStats), i32]
    if hasattr(L, "pcore_get_tile_info"):  # diagnostics / test hooks: absent from older A/B builds (PCORE_LIB)
        L.pcore_get_tile_info.argtypes = [vp, ctypes.POINTER(TileInfo)]
    if hasattr(L, "pcore_debug_lm_solve"):
        L.pcore_debug_lm_solve.argtypes = [vp, vp, vp, i32, vp]
    if hasattr(L, "pcore_debug_covariances"):
        L.pcore_debug_covariances.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    if hasattr(L, "pcore_debug_covariances_cloud"):
        f32 = ctypes.c_float
        L.pcore_debug_covariances_cloud.argtypes = [vp, vp, i32, i32, f32, f32, f32, f32, i32, vp, vp]
    if hasattr(L, "pcore_depth_to_cloud_ex"):
        L.pcore_depth_to_cloud_ex.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                              ctypes.POINTER(i32), vp]
    L.pcore_depth_to_cloud.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, i32,
                                       ctypes.POINTER(i32), vp]
    if hasattr(L, "pcore_icp_planar"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_icp_planar.argtypes = [vp, vp, vp, i32, ctypes.POINTER(EvalParams), ctypes.POINTER(ctypes.c_float),
                                       ctypes.POINTER(PlanarIcpParams), vp, vp, vp, vp, vp]
    if hasattr(L, "pcore_debug_planar_step"):
        L.pcore_debug_planar_step.argtypes = [vp, vp, i32, vp]
    if hasattr(L, "pcore_icp_point2plane"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_scene_projective.argtypes = [vp, vp, i32, i32, f32, f32, f32, f32, vp, vp, vp]
        L.pcore_icp_point2plane.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(EvalParams),
                                            ctypes.POINTER(P2pIcpParams), vp, vp, vp, vp, vp, vp]
        L.pcore_debug_p2p_clouds.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, f32, f32, f32, f32,
                                             ctypes.POINTER(P2pIcpParams), vp, vp, vp, vp, vp]
    if hasattr(L, "pcore_icp_point2plane_nn"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_icp_point2plane_nn.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(EvalParams),
                                               ctypes.POINTER(NnIcpParams), vp, vp, vp, vp, vp, vp]
        L.pcore_debug_p2p_nn_clouds.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, f32, f32, f32, f32,
                                                ctypes.POINTER(NnIcpParams), vp, vp, vp, vp, vp]
    if hasattr(L, "pcore_debug_render_clouds"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_debug_render_clouds.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(EvalParams), vp, vp, vp]
    if hasattr(L, "pcore_debug_colour_distance"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_debug_colour_distance.argtypes = [vp, vp, i32, vp]
        L.pcore_debug_rgb2lab.argtypes = [vp, vp, i32]
    L.pcore_select.argtypes = [vp, vp, vp, vp, i32, i64, i32, vp, vp]
    if hasattr(L, "pcore_select_topk"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_select_topk.argtypes = [vp, vp, vp, vp, i32, i64, i32, i32, vp, vp]
    if hasattr(L, "pcore_evaluate_states"):  # absent from older A/B builds (PCORE_LIB)
        L.pcore_evaluate_states.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, ctypes.POINTER(EvalParams), vp, vp, vp,
                                            vp, vp, i32, vp]
    L.pcore_pose_distances.argtypes =[vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.pcore_set_observation_colors.argtypes = [vp, vp, i32, vp]
    L.pcore_observed_cloud_bounded.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, i32,
                                               ctypes.POINTER(i32), vp]
    L.pcore_generation.argtypes = [vp]
    L.pcore_evaluate_select.argtypes = [vp, vp, vp, vp, vp, i32, ctypes.POINTER(EvalParams), vp, vp, vp, i64, i32,
                                        vp, vp]
    L.pcore_count_within.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    L.pcore_state_poses.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_double), vp, i32, i32, vp, vp]
    for name in EXPORTED_SYMBOLS + EXPORTED_SYMBOLS_WITH_DIGITS:
        if name not in ("pcore_destroy", "pcore_last_error", "pcore_generation") and hasattr(L, name):
            getattr(L, name).restype = ctypes.c_int
    L.pcore_generation.restype = ctypes.c_uint64
    _lib = L
    return L
