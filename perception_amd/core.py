"""PoseCore: the device-side context of the pose-search core, driven with PyTorch-ROCm tensors.

This is the Python face of include/pcore.h.  Every array argument of the per-batch calls is a CUDA
(HIP) torch tensor; its data_ptr() goes straight into the C ABI, and the work runs on torch's
current stream.  There is no CPU fallback: a missing libpcore.so or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from ._native import Camera, EvalParams, IcpParams, P2pIcpParams, PcoreError, PlanarIcpParams


def _ptr(t: Optional[torch.Tensor], dtype: torch.dtype, name: str):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name}: expected a GPU torch tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _stream(stream: Optional[torch.cuda.Stream]):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


class PoseCore:
    """One context per (host thread, device), like the reference's single-threaded caller
    (search_env.cpp:2506-2525)."""

    def __init__(self, device: int = 0):
        self.lib = _native.load()
        self.device = int(device)
        h = ctypes.c_void_p()
        rc = self.lib.pcore_create(self.device, ctypes.byref(h))
        if rc != _native.PCORE_OK:
            raise PcoreError(rc, f"pcore_create(device={device}) failed")
        self._h = h
        self.width = self.height = 0
        self.num_models = 0

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.pcore_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != _native.PCORE_OK:
            msg = self.lib.pcore_last_error(self._h)
            raise PcoreError(rc, msg.decode() if msg else "")

    # -- static inputs ----------------------------------------------------------------------------
    def upload_meshes(self, tris: np.ndarray, tris_model_count, colors: Optional[np.ndarray] = None):
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        cnt = np.ascontiguousarray(tris_model_count, dtype=np.int32)
        col = None if colors is None else np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
        self._check(self.lib.pcore_upload_meshes(
            self._h, tris.ctypes.data_as(ctypes.c_void_p),
            None if col is None else col.ctypes.data_as(ctypes.c_void_p), tris.shape[0],
            cnt.ctypes.data_as(ctypes.c_void_p), cnt.shape[0]))
        self.num_models = int(cnt.shape[0])

    def set_camera(self, width: int, height: int, fx: float, fy: float, cx: float, cy: float, proj: np.ndarray):
        cam = Camera()
        cam.width, cam.height = int(width), int(height)
        cam.fx, cam.fy, cam.cx, cam.cy = float(fx), float(fy), float(cx), float(cy)
        pj = np.asarray(proj, dtype=np.float32).reshape(16)
        for i in range(16):
            cam.proj[i] = float(pj[i])
        self._check(self.lib.pcore_set_camera(self._h, ctypes.byref(cam)))
        self.width, self.height = int(width), int(height)

    # -- per-scene inputs -------------------------------------------------------------------------
    def observed_cloud(self, depth: torch.Tensor, label_mask: Optional[torch.Tensor], stride: int,
                       depth_factor: float, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """depth2cloud_global (renderer.cu:1936-2069): returns (xyz (P,3) f32, label (P,) i32) on the GPU."""
        h, w = depth.shape[-2:]
        cap = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
        xyz = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=depth.device)
        lab = torch.empty((max(cap, 1),), dtype=torch.int32, device=depth.device)
        cnt = ctypes.c_int32(0)
        self._check(self.lib.pcore_observed_cloud(
            self._h, _ptr(depth, torch.int32, "depth"), _ptr(label_mask, torch.uint8, "label_mask"), w, h, stride,
            float(depth_factor), _ptr(xyz, torch.float32, "xyz"), _ptr(lab, torch.int32, "label"), cap,
            ctypes.byref(cnt), _stream(stream)))
        n = cnt.value
        return xyz[:n], lab[:n]

    def observed_cloud_bounded(self, depth: torch.Tensor, stride: int, depth_factor: float,
                               cam_to_world: Optional[np.ndarray] = None, bounds: Optional[Sequence[float]] = None,
                               rgb: Optional[torch.Tensor] = None, stream=None
                               ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """3-DoF depth2cloud_global: camera-frame points of the pixels whose world point (cam_to_world, 4x4)
        lies inside bounds = (x_max, x_min, y_max, y_min, z_max, z_min); with `rgb` (H, W, 3) uint8 also the
        points' colours.  Returns (xyz (P,3) f32, rgb (P,3) u8 or None) on the GPU."""
        h, w = depth.shape[-2:]
        cap = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
        xyz = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=depth.device)
        out_rgb = torch.empty((max(cap, 1), 3), dtype=torch.uint8, device=depth.device) if rgb is not None else None
        M = None if cam_to_world is None else (ctypes.c_float * 16)(*np.asarray(cam_to_world, np.float32).reshape(16))
        B = None if bounds is None else (ctypes.c_double * 6)(*np.asarray(bounds, np.float64).reshape(6))
        cnt = ctypes.c_int32(0)
        self._check(self.lib.pcore_observed_cloud_bounded(
            self._h, _ptr(depth, torch.int32, "depth"), _ptr(None if rgb is None else rgb.contiguous(), torch.uint8, "rgb"),
            w, h, stride, float(depth_factor), M, B, _ptr(xyz, torch.float32, "xyz"),
            _ptr(out_rgb, torch.uint8, "out_rgb"), cap, ctypes.byref(cnt), _stream(stream)))
        n = cnt.value
        return xyz[:n], (out_rgb[:n] if out_rgb is not None else None)

    def set_observation(self, src_depth_cm: torch.Tensor, src_mask: Optional[torch.Tensor],
                        obs_xyz: torch.Tensor, obs_label: Optional[torch.Tensor], sensor_resolution: float,
                        stream=None):
        obs_xyz = obs_xyz.contiguous()
        n = int(obs_xyz.shape[0])
        self._check(self.lib.pcore_set_observation(
            self._h, _ptr(src_depth_cm.contiguous(), torch.int32, "src_depth"),
            _ptr(None if src_mask is None else src_mask.contiguous(), torch.uint8, "src_mask"),
            _ptr(obs_xyz, torch.float32, "obs_xyz") if n else None,
            _ptr(None if obs_label is None else obs_label.contiguous(), torch.int32, "obs_label") if n else None,
            n, float(sensor_resolution), _stream(stream)))

    def set_observation_colors(self, obs_rgb: torch.Tensor, stream=None):
        """Colours (n, 3) uint8 of the observed points given to set_observation, in the same order
        (cost_type 1)."""
        rgb = obs_rgb.contiguous()
        n = int(rgb.shape[0])
        self._check(self.lib.pcore_set_observation_colors(
            self._h, _ptr(rgb, torch.uint8, "obs_rgb") if n else None, n, _stream(stream)))

    # -- per-batch hot path -----------------------------------------------------------------------
    def evaluate(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor],
                 pose_obs_total: Optional[torch.Tensor], cost_type: int = _native.COST_DEPTH_6DOF,
                 calc_obs_cost: bool = True, stride: int = 8, depth_factor: float = 100.0,
                 sensor_resolution: float = 0.01, occlusion_threshold: float = 1.0,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                 dbg_zs: Optional[torch.Tensor] = None, color_distance_threshold: float = 15.0, stream=None,
                 select: Optional[Tuple[torch.Tensor, int, int]] = None):
        """Stage COST (do_icp = false).  Returns (rendered_cost, observed_cost, points_diff_cost).  With
        select = (keys, index_base, num_models) the launch also folds every pose's argmin key into `keys`
        (pcore_evaluate_select: the same keys as a following select() call)."""
        n = int(poses.shape[0])
        dev = poses.device
        if out is None:
            out = tuple(torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        rc, oc, df = out
        p = EvalParams(int(cost_type), int(bool(calc_obs_cost)), int(stride), float(depth_factor),
                       float(sensor_resolution), float(occlusion_threshold), float(color_distance_threshold))
        if select is not None:
            keys, index_base, num_models = select
            if dbg_zs is not None:
                raise ValueError("evaluate: dbg_zs and select are exclusive")
            self._check(self.lib.pcore_evaluate_select(
                self._h, _ptr(poses, torch.float32, "poses"), _ptr(pose_model, torch.int32, "pose_model"),
                _ptr(pose_label, torch.int32, "pose_label"), _ptr(pose_obs_total, torch.float32, "pose_obs_total"),
                n, ctypes.byref(p), _ptr(rc, torch.float32, "rc"), _ptr(oc, torch.float32, "oc"),
                _ptr(df, torch.float32, "diff"), int(index_base), int(num_models), _ptr(keys, torch.int64, "keys"),
                _stream(stream)))
            return rc, oc, df
        self._check(self.lib.pcore_evaluate(
            self._h, _ptr(poses, torch.float32, "poses"), _ptr(pose_model, torch.int32, "pose_model"),
            _ptr(pose_label, torch.int32, "pose_label"), _ptr(pose_obs_total, torch.float32, "pose_obs_total"),
            n, ctypes.byref(p), _ptr(rc, torch.float32, "rc"), _ptr(oc, torch.float32, "oc"),
            _ptr(df, torch.float32, "diff"), _ptr(dbg_zs, torch.int32, "dbg_zs"), _stream(stream)))
        return rc, oc, df

    def evaluate_states(self, states, pose_label: Optional[torch.Tensor], state_obs_total: Optional[torch.Tensor], *,
                        zs: Optional[torch.Tensor] = None, poses: Optional[torch.Tensor] = None,
                        pose_model: Optional[torch.Tensor] = None, cost_type: int = _native.COST_DEPTH_6DOF,
                        calc_obs_cost: bool = True, stride: int = 8, depth_factor: float = 100.0,
                        sensor_resolution: float = 0.01, occlusion_threshold: float = 1.0,
                        member_counts: bool = True, stream=None):
        """Stage COST of composed states (pcore_evaluate_states; DESIGN.md section 2, "State cost").  `states` is a list
        of member lists or an (off (S + 1,), member (nnz,)) pair of int32 GPU tensors; members index the poses behind
        `zs` (N, hs, ws) int32 -- evaluate's dbg_zs -- and `pose_label` (N,).  With `poses` (N, 16) and `pose_model`
        instead of `zs`, the poses that are a member of some state are rendered first by evaluate(..., dbg_zs=...).
        Returns (rc, oc, diff) per state and (vis, bad) per member entry (None with member_counts=False).  Selecting
        among states is select() with a group id per state in place of pose_model."""
        if (zs is None) == (poses is None):
            raise ValueError("evaluate_states: give exactly one of zs and poses")
        dev = zs.device if zs is not None else poses.device
        if isinstance(states, (tuple, list)) and len(states) == 2 and all(isinstance(t, torch.Tensor) for t in states):
            off, member = states
        else:
            lens = [len(m) for m in states]
            off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev)
            flat = np.concatenate([np.asarray(m, np.int64).reshape(-1) for m in states]) if lens else np.zeros(0)
            member = torch.from_numpy(flat.astype(np.int32)).to(dev)
        S, nnz = int(off.shape[0]) - 1, int(member.shape[0])
        kw = dict(cost_type=cost_type, stride=stride, depth_factor=depth_factor,
                  sensor_resolution=sensor_resolution, occlusion_threshold=occlusion_threshold)
        if poses is not None:
            if pose_model is None:
                raise ValueError("evaluate_states: poses need pose_model")
            n = int(poses.shape[0])
            ok = (member >= 0) & (member < n)
            uniq = torch.unique(member[ok].long())  # sorted: the rendered batch keeps the members' order
            remap = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
            remap[uniq] = torch.arange(int(uniq.shape[0]), dtype=torch.int32, device=dev)
            member = torch.where(ok, remap[member.long().clamp(0, max(n, 1) - 1)], torch.full_like(member, -1))
            nsamp = (self.width // stride) * ((self.height + stride - 1) // stride) if stride > 0 else 0
            zs = torch.zeros((int(uniq.shape[0]), max(nsamp, 1)), dtype=torch.int32, device=dev)
            sub_label = None if pose_label is None else pose_label[uniq].contiguous()
            if int(uniq.shape[0]):
                self.evaluate(poses[uniq].contiguous(), pose_model[uniq].contiguous(), sub_label, None,
                              calc_obs_cost=False, dbg_zs=zs, stream=stream, **kw)
            pose_label = sub_label
        n = int(zs.shape[0])
        # the kernel trusts the sizes: a wrong stride or shape would be an out-of-bounds read on the device
        if S < 0:
            raise ValueError("evaluate_states: state_off needs at least one entry")
        if stride > 0 and self.width % stride == 0:  # otherwise the call itself refuses
            nsamp = (self.width // stride) * ((self.height + stride - 1) // stride)
            if zs.numel() != n * nsamp:
                raise ValueError(f"evaluate_states: zs holds {zs.numel()} values, not {n} x {nsamp} samples of stride {stride}")
        if pose_label is not None and pose_label.numel() != n:
            raise ValueError(f"evaluate_states: pose_label has {pose_label.numel()} entries for {n} z-buffers")
        if state_obs_total is not None and state_obs_total.numel() != S:
            raise ValueError(f"evaluate_states: state_obs_total has {state_obs_total.numel()} entries for {S} states")
        rc, oc, df = (torch.empty(S, dtype=torch.float32, device=dev) for _ in range(3))
        vis = torch.empty(nnz, dtype=torch.int32, device=dev) if member_counts else None
        bad = torch.empty(nnz, dtype=torch.int32, device=dev) if member_counts else None
        p = EvalParams(int(cost_type), int(bool(calc_obs_cost)), int(stride), float(depth_factor),
                       float(sensor_resolution), float(occlusion_threshold), 0.0)
        self._check(self.lib.pcore_evaluate_states(
            self._h, _ptr(zs, torch.int32, "zs") if n else None, n, _ptr(pose_label, torch.int32, "pose_label"),
            _ptr(off, torch.int32, "state_off"), _ptr(member, torch.int32, "state_member") if nnz else None, S,
            _ptr(state_obs_total, torch.float32, "state_obs_total"), ctypes.byref(p), _ptr(rc, torch.float32, "rc"),
            _ptr(oc, torch.float32, "oc"), _ptr(df, torch.float32, "diff"),
            _ptr(vis, torch.int32, "vis") if nnz else None, _ptr(bad, torch.int32, "bad") if nnz else None, nnz,
            _stream(stream)))
        return rc, oc, df, vis, bad

    def capture_evaluate(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor],
                         pose_obs_total: Optional[torch.Tensor], **kw):
        """Stage COST of a fixed-size batch as a HIP graph (torch.cuda.CUDAGraph over the C-ABI launches).
        One warm-up call reserves the scratch, samples the source and picks the LDS tile tier; then the
        launches of one evaluate are captured.  Returns (replay, (rc, oc, diff)): replay() re-scores the batch
        from the tensors' current contents (write new poses into `poses` in place).  For batches small enough
        to be launch-bound (C1: 128 poses); the results equal evaluate()'s.

        The graph bakes in the context state of the capture (sampled source, neighbour grids, scratch
        pointers, tile size).  Any later setup call (upload_meshes, set_camera, set_observation,
        set_observation_colors), a new stride or a larger batch that reallocates scratch changes the
        context's generation (pcore_generation), and replay() then raises PcoreError(PCORE_E_STATE)
        instead of running stale launches: capture again.  The check runs when replay() enqueues the graph, so a
        setup call must be stream-ordered after any replay still in flight."""
        n = int(poses.shape[0])
        out = tuple(torch.empty(n, dtype=torch.float32, device=poses.device) for _ in range(3))
        self.evaluate(poses, pose_model, pose_label, pose_obs_total, out=out, **kw)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.evaluate(poses, pose_model, pose_label, pose_obs_total, out=out, **kw)
        gen = self.generation()

        def replay():
            if self.generation() != gen:
                raise PcoreError(_native.PCORE_E_STATE, "captured evaluate graph is stale: the context changed "
                                 "(setup call, new stride or scratch reallocation) since the capture")
            graph.replay()

        return replay, out

    def generation(self) -> int:
        """pcore_generation: changes whenever state a captured evaluate graph depends on may have changed."""
        return int(self.lib.pcore_generation(self._h))

    def evaluate_icp(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor],
                     pose_obs_total: Optional[torch.Tensor], cost_type: int = _native.COST_DEPTH_6DOF,
                     calc_obs_cost: bool = True, stride: int = 8, depth_factor: float = 100.0,
                     sensor_resolution: float = 0.01, occlusion_threshold: float = 1.0,
                     k: int = _native.ICP_K, max_iterations: int = _native.ICP_MAX_ITER,
                     rotation_epsilon: float = _native.ICP_ROT_EPS,
                     transformation_epsilon: float = _native.ICP_TRANS_EPS, out=None,
                     color_distance_threshold: float = 15.0, stream=None,
                     cycle_exit_window: int = _native.ICP_CYCLE_WINDOW):
        """Stage COST with do_icp = true.  Returns (adjusted poses (N,16), iterations (N,), rc, oc, diff)."""
        n = int(poses.shape[0])
        dev = poses.device
        if out is None:
            out = (torch.empty((n, 16), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                   *(torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)))
        adj, iters, rc, oc, df = out
        p = EvalParams(int(cost_type), int(bool(calc_obs_cost)), int(stride), float(depth_factor),
                       float(sensor_resolution), float(occlusion_threshold), float(color_distance_threshold))
        ip = IcpParams(int(k), int(max_iterations), float(rotation_epsilon), float(transformation_epsilon),
                       int(cycle_exit_window))
        self._check(self.lib.pcore_evaluate_icp(
            self._h, _ptr(poses, torch.float32, "poses"), _ptr(pose_model, torch.int32, "pose_model"),
            _ptr(pose_label, torch.int32, "pose_label"), _ptr(pose_obs_total, torch.float32, "pose_obs_total"),
            n, ctypes.byref(p), ctypes.byref(ip), _ptr(adj, torch.float32, "adjusted_poses"),
            _ptr(iters, torch.int32, "iterations"), _ptr(rc, torch.float32, "rc"), _ptr(oc, torch.float32, "oc"),
            _ptr(df, torch.float32, "diff"), _stream(stream)))
        return adj, iters, rc, oc, df

    def icp_planar(self, poses: torch.Tensor, pose_model: torch.Tensor, world_from_cam: np.ndarray,
                   cost_type: int = _native.COST_DEPTH_3DOF, stride: int = 4, depth_factor: float = 100.0,
                   occlusion_threshold: float = 1.0, max_iterations: int = _native.PLANAR_MAX_ITER,
                   max_correspondence: float = _native.PLANAR_MAX_CORRESPONDENCE,
                   transformation_epsilon: float = _native.PLANAR_TRANS_EPS,
                   fitness_epsilon: float = _native.PLANAR_FIT_EPS, out=None, stream=None):
        """Planar (x, y, yaw) ICP of every pose's rendered stride-sample cloud onto the observation, both moved to the
        world frame by world_from_cam (4 x 4; pcore_icp_planar).  Returns (xform (N, 4) float64: c s tx ty, iterations
        (N,) int32, status (N,) int32, mse (N,) float64) on the GPU."""
        n = int(poses.shape[0])
        dev = poses.device
        if out is None:
            out = (torch.empty((n, 4), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev))
        xform, iters, status, mse = out
        p = EvalParams(int(cost_type), 0, int(stride), float(depth_factor), 0.0, float(occlusion_threshold), 0.0)
        pp = PlanarIcpParams(int(max_iterations), float(max_correspondence), float(transformation_epsilon),
                             float(fitness_epsilon))
        M = (ctypes.c_float * 16)(*np.asarray(world_from_cam, np.float32).reshape(16))
        self._check(self.lib.pcore_icp_planar(
            self._h, _ptr(poses, torch.float32, "poses"), _ptr(pose_model, torch.int32, "pose_model"), n,
            ctypes.byref(p), M, ctypes.byref(pp), _ptr(xform, torch.float64, "xform"),
            _ptr(iters, torch.int32, "iterations"), _ptr(status, torch.int32, "status"),
            _ptr(mse, torch.float64, "mse"), _stream(stream)))
        return xform, iters, status, mse

    def planar_step(self, sums: torch.Tensor, stream=None) -> torch.Tensor:
        """pcore_debug_planar_step: the planar ICP's estimation step of (n, 10) float64 raw sum records -> (n, 4)
        float64 (c', s', tx', ty')."""
        sums = sums.contiguous()
        n = int(sums.shape[0])
        out = torch.empty((n, 4), dtype=torch.float64, device=sums.device)
        rc = self.lib.pcore_debug_planar_step(_ptr(sums, torch.float64, "sums"), _ptr(out, torch.float64, "out"), n,
                                              _stream(stream))
        if rc != _native.PCORE_OK:
            raise PcoreError(rc, "pcore_debug_planar_step failed")
        return out

    def colour_distance(self, lab_pairs: torch.Tensor, stream=None) -> torch.Tensor:
        """pcore_debug_colour_distance (test hook): the colour gate's CIEDE2000 distance of (n, 6) float32 Lab pairs
        (l1 a1 b1 l2 a2 b2) as the fused cost kernel evaluates it -> (n,) float64."""
        lab_pairs = lab_pairs.contiguous()
        n = int(lab_pairs.shape[0])
        out = torch.empty(n, dtype=torch.float64, device=lab_pairs.device)
        rc = self.lib.pcore_debug_colour_distance(_ptr(lab_pairs, torch.float32, "lab_pairs"),
                                                  _ptr(out, torch.float64, "out"), n, _stream(stream))
        if rc != _native.PCORE_OK:
            raise PcoreError(rc, "pcore_debug_colour_distance failed")
        return out

    @staticmethod
    def rgb2lab(rgb: np.ndarray) -> np.ndarray:
        """pcore_debug_rgb2lab (test hook, host only, no context): the Lab values upload_meshes and
        set_observation_colors store for (n, 3) uint8 colours -> (n, 3) float32."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
        out = np.empty((rgb.shape[0], 3), np.float32)
        rc = _native.load().pcore_debug_rgb2lab(rgb.ctypes.data_as(ctypes.c_void_p),
                                                out.ctypes.data_as(ctypes.c_void_p), rgb.shape[0])
        if rc != _native.PCORE_OK:
            raise PcoreError(rc, "pcore_debug_rgb2lab failed")
        return out

    def scene_projective(self, depth_cm: torch.Tensor, fx: float, fy: float, cx: float, cy: float, stream=None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
        """pcore_scene_projective: the reference's Scene_projective buffers of an (H, W) int32 cm depth image ->
        (points (H, W, 3) float32, linemod normals (H, W, 3) float32) on the GPU."""
        h, w = depth_cm.shape[-2:]
        pcd = torch.empty((h, w, 3), dtype=torch.float32, device=depth_cm.device)
        nrm = torch.empty((h, w, 3), dtype=torch.float32, device=depth_cm.device)
        self._check(self.lib.pcore_scene_projective(
            self._h, _ptr(depth_cm, torch.int32, "depth_cm"), int(w), int(h), float(fx), float(fy), float(cx),
            float(cy), _ptr(pcd, torch.float32, "pcd"), _ptr(nrm, torch.float32, "normal"), _stream(stream)))
        return pcd, nrm

    def icp_point2plane(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor] = None,
                        cost_type: int = _native.COST_DEPTH_6DOF, stride: int = 8, depth_factor: float = 100.0,
                        occlusion_threshold: float = 1.0, max_iterations: int = _native.P2P_MAX_ITER,
                        relative_fitness: float = _native.P2P_REL_FITNESS,
                        relative_rmse: float = _native.P2P_REL_RMSE, max_dist_diff: Optional[float] = None,
                        out=None, out_poses: Optional[torch.Tensor] = None, stream=None, scene: str = "projective",
                        window: int = _native.NN_WINDOW):
        """Point-to-plane ICP of every pose's rendered stride-sample cloud against the projective scene of the
        observation's source depth (pcore_icp_point2plane); pose_label selects the 6-DoF source occlusion, None the
        3-DoF one.  Returns (T (N, 16) float32, fitness (N,), rmse (N,), iterations (N,) int32) on the GPU; with
        out_poses (N, 16) also writes concatenate_transforms(T, pose) there.  scene="nn" pairs each point with its
        nearest scene point within max_dist_diff among the pixels within `window` of its own (pcore_icp_point2plane_nn);
        max_dist_diff defaults to 0.1 for the projective scene and to 0.01 for the nearest-neighbour one."""
        fn, ip = self._p2p_call(scene, "pcore_icp_point2plane", max_iterations, relative_fitness, relative_rmse,
                                max_dist_diff, window)
        n = int(poses.shape[0])
        dev = poses.device
        if out is None:
            out = (torch.empty((n, 16), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                   torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        T, fitness, rmse, iters = out
        p = EvalParams(int(cost_type), 0, int(stride), float(depth_factor), 0.0, float(occlusion_threshold), 0.0)
        self._check(fn(
            self._h, _ptr(poses, torch.float32, "poses"), _ptr(pose_model, torch.int32, "pose_model"),
            _ptr(pose_label, torch.int32, "pose_label"), n, ctypes.byref(p), ctypes.byref(ip),
            _ptr(T, torch.float32, "T"), _ptr(fitness, torch.float32, "fitness"), _ptr(rmse, torch.float32, "rmse"),
            _ptr(iters, torch.int32, "iterations"), _ptr(out_poses, torch.float32, "out_poses"), _stream(stream)))
        return T, fitness, rmse, iters

    def _p2p_call(self, scene, name, max_iterations, relative_fitness, relative_rmse, max_dist_diff, window):
        """The entry point and the parameter struct of a point-to-plane call against the named scene."""
        if scene == "projective":
            d = _native.P2P_MAX_DIST_DIFF if max_dist_diff is None else max_dist_diff
            return getattr(self.lib, name), P2pIcpParams(int(max_iterations), float(relative_fitness),
                                                         float(relative_rmse), float(d))
        if scene != "nn":
            raise ValueError(f"scene must be 'projective' or 'nn', not {scene!r}")
        d = _native.NN_MAX_DIST_DIFF if max_dist_diff is None else max_dist_diff
        name = {"pcore_icp_point2plane": "pcore_icp_point2plane_nn", "pcore_debug_p2p_clouds": "pcore_debug_p2p_nn_clouds"}[name]
        return getattr(self.lib, name), _native.NnIcpParams(int(max_iterations), float(relative_fitness),
                                                            float(relative_rmse), float(d), int(window))

    def debug_p2p_clouds(self, *args, **kw):
        """p2p_clouds under the C entry point's name."""
        return self.p2p_clouds(*args, **kw)

    def p2p_clouds(self, xyzw: torch.Tensor, seg_cnt: torch.Tensor, scene_pcd4: torch.Tensor,
                   scene_normal4: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                   max_iterations: int = _native.P2P_MAX_ITER, relative_fitness: float = _native.P2P_REL_FITNESS,
                   relative_rmse: float = _native.P2P_REL_RMSE, max_dist_diff: Optional[float] = None,
                   stream=None, scene: str = "projective", window: int = _native.NN_WINDOW):
        """pcore_debug_p2p_clouds: the point-to-plane ICP kernel over caller-made slots xyzw (S, cap, 4) float32 with
        seg_cnt (S,) int32 points each (moved in place) and a caller-made scene (H, W, 4) + (H, W, 4).  Returns (T
        (S, 16), fitness, rmse, iterations).  scene="nn": pcore_debug_p2p_nn_clouds, whose scene points must be dep2pcd
        of a centimetre depth image under the camera given."""
        fn, ip = self._p2p_call(scene, "pcore_debug_p2p_clouds", max_iterations, relative_fitness, relative_rmse,
                                max_dist_diff, window)
        s, cap = int(xyzw.shape[0]), int(xyzw.shape[1])
        h, w = int(scene_pcd4.shape[0]), int(scene_pcd4.shape[1])
        dev = xyzw.device
        T = torch.empty((s, 16), dtype=torch.float32, device=dev)
        fitness = torch.empty(s, dtype=torch.float32, device=dev)
        rmse = torch.empty(s, dtype=torch.float32, device=dev)
        iters = torch.empty(s, dtype=torch.int32, device=dev)
        rc = fn(
            _ptr(xyzw, torch.float32, "xyzw"), _ptr(seg_cnt, torch.int32, "seg_cnt"), cap, s,
            _ptr(scene_pcd4, torch.float32, "scene_pcd4"), _ptr(scene_normal4, torch.float32, "scene_normal4"), w, h,
            float(fx), float(fy), float(cx), float(cy), ctypes.byref(ip), _ptr(T, torch.float32, "T"),
            _ptr(fitness, torch.float32, "fitness"), _ptr(rmse, torch.float32, "rmse"),
            _ptr(iters, torch.int32, "iterations"), _stream(stream))
        if rc != _native.PCORE_OK:
            raise PcoreError(rc, f"{fn.__name__} failed")
        return T, fitness, rmse, iters

    def evaluate_p2p(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor],
                     pose_obs_total: Optional[torch.Tensor], cost_type: int = _native.COST_DEPTH_6DOF,
                     calc_obs_cost: bool = True, stride: int = 8, depth_factor: float = 100.0,
                     sensor_resolution: float = 0.01, occlusion_threshold: float = 1.0,
                     max_iterations: int = _native.P2P_MAX_ITER, relative_fitness: float = _native.P2P_REL_FITNESS,
                     relative_rmse: float = _native.P2P_REL_RMSE, max_dist_diff: Optional[float] = None,
                     color_distance_threshold: float = 15.0, stream=None, scene: str = "projective",
                     window: int = _native.NN_WINDOW):
        """Stage COST with the point-to-plane ICP in GICP's place: icp_point2plane with out_poses, then evaluate on the
        adjusted poses (scene and window as icp_point2plane).  Returns (adjusted poses (N, 16), iterations (N,), rc, oc, diff, fitness, rmse)."""
        n = int(poses.shape[0])
        adj = torch.empty((n, 16), dtype=torch.float32, device=poses.device)
        label = pose_label if cost_type == _native.COST_DEPTH_6DOF else None
        _, fitness, rmse, iters = self.icp_point2plane(
            poses, pose_model, label, cost_type=cost_type, stride=stride, depth_factor=depth_factor,
            occlusion_threshold=occlusion_threshold, max_iterations=max_iterations,
            relative_fitness=relative_fitness, relative_rmse=relative_rmse, max_dist_diff=max_dist_diff,
            out_poses=adj, stream=stream, scene=scene, window=window)
        rc, oc, df = self.evaluate(adj, pose_model, pose_label, pose_obs_total, cost_type=cost_type,
                                   calc_obs_cost=calc_obs_cost, stride=stride, depth_factor=depth_factor,
                                   sensor_resolution=sensor_resolution, occlusion_threshold=occlusion_threshold,
                                   color_distance_threshold=color_distance_threshold, stream=stream)
        return adj, iters, rc, oc, df, fitness, rmse

    def render_clouds(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor] = None,
                      stride: int = 8, depth_factor: float = 100.0, occlusion_threshold: float = 1.0, stream=None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
        """pcore_debug_render_clouds (test hook): stage CLOUD of every pose as the ICP entry points render their source
        clouds.  Returns (xyzw (N, ws * hs, 4) float32, count (N,) int32): pose i's points are xyzw[i, :count[i]]."""
        n = int(poses.shape[0])
        w, h = self.width, self.height
        nsamp = (w // stride) * ((h + stride - 1) // stride)
        xyzw = torch.zeros((n, nsamp, 4), dtype=torch.float32, device=poses.device)
        cnt = torch.zeros(n, dtype=torch.int32, device=poses.device)
        p = EvalParams(_native.COST_DEPTH_6DOF, 0, int(stride), float(depth_factor), 0.0, float(occlusion_threshold),
                       0.0)
        self._check(self.lib.pcore_debug_render_clouds(
            self._h, _ptr(poses, torch.float32, "poses"), _ptr(pose_model, torch.int32, "pose_model"),
            _ptr(pose_label, torch.int32, "pose_label"), n, ctypes.byref(p), _ptr(xyzw, torch.float32, "xyzw"),
            _ptr(cnt, torch.int32, "count"), _stream(stream)))
        return xyzw, cnt

    def render(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor],
               occlusion_threshold: float = 1.0, out: Optional[torch.Tensor] = None, color: bool = False,
               out_color: Optional[torch.Tensor] = None, stream=None):
        """Stage RENDER: (N, H, W) int32 z-buffers in cm; with color=True also the reference's result_color planes,
        returned as (depth, color (3, N, H, W) uint8 red / green / blue)."""
        n = int(poses.shape[0])
        if out is None:
            out = torch.empty((n, self.height, self.width), dtype=torch.int32, device=poses.device)
        if color and out_color is None:
            out_color = torch.empty((3, n, self.height, self.width), dtype=torch.uint8, device=poses.device)
        self._check(self.lib.pcore_render(
            self._h, _ptr(poses, torch.float32, "poses"), _ptr(pose_model, torch.int32, "pose_model"),
            _ptr(pose_label, torch.int32, "pose_label"), n, float(occlusion_threshold),
            _ptr(out, torch.int32, "out"), _ptr(out_color, torch.uint8, "out_color") if color else None,
            _stream(stream)))
        return (out, out_color) if color else out

    def render_scene(self, poses: torch.Tensor, pose_model: torch.Tensor, pose_label: Optional[torch.Tensor] = None,
                     occlusion_threshold: float = 1.0, occlude: bool = True, color: bool = True, owner: bool = True,
                     visible: bool = True, stream=None):
        """The composed state (pcore_render_scene): every pose into one frame.  Returns (depth (H, W) int32 cm, color
        (3, H, W) uint8 red / green / blue or None, owner (H, W) int32 -- the pose that owns each pixel, -1 for none --
        or None, visible (N,) int32 -- the pixels each pose owns -- or None).  occlude=False needs no observation and
        takes no pose_label."""
        n = int(poses.shape[0])
        dev = poses.device
        h, w = self.height, self.width
        depth = torch.empty((h, w), dtype=torch.int32, device=dev)
        out_color = torch.empty((3, h, w), dtype=torch.uint8, device=dev) if color else None
        out_owner = torch.empty((h, w), dtype=torch.int32, device=dev) if owner else None
        out_visible = torch.empty(n, dtype=torch.int32, device=dev) if visible else None
        self._check(self.lib.pcore_render_scene(
            self._h, _ptr(poses, torch.float32, "poses") if n else None,
            _ptr(pose_model, torch.int32, "pose_model") if n else None, _ptr(pose_label, torch.int32, "pose_label"), n,
            int(bool(occlude)), float(occlusion_threshold), _ptr(depth, torch.int32, "depth"),
            _ptr(out_color, torch.uint8, "color"), _ptr(out_owner, torch.int32, "owner"),
            _ptr(out_visible, torch.int32, "visible") if n else None, _stream(stream)))
        return depth, out_color, out_owner, out_visible

    def stats(self, reset: bool = False) -> dict:
        """pcore_get_stats: the reference's gpu_stats of the last evaluate_icp (waits for its GICP stage)."""
        st = _native.GpuStats()
        self._check(self.lib.pcore_get_stats(self._h, ctypes.byref(st), int(bool(reset))))
        return {"icp_runtime": st.icp_runtime, "peak_memory_usage": st.peak_memory_usage, "gicp_ms": st.gicp_ms,
                "icp_chunks": st.icp_chunks, "gicp_iterations": st.gicp_iterations,
                "gicp_iterations_run": st.gicp_iterations_run, "gicp_cycle_exits": st.gicp_cycle_exits}

    def tile_info(self) -> dict:
        """pcore_get_tile_info: the fused window launch's tile tier and the last published window histogram."""
        ti = _native.TileInfo()
        self._check(self.lib.pcore_get_tile_info(self._h, ctypes.byref(ti)))
        n = ti.num_tiers
        return {"tier": ti.tier, "tcap": ti.tcap, "seq": ti.seq, "edge": list(ti.edge[:n]),
                "wgs_per_cu": list(ti.wgs_per_cu[:n]), "hist": list(ti.hist[:n + 1]), "chunked": ti.chunked}

    def depth_to_cloud(self, depth: torch.Tensor, stride: int, depth_factor: float,
                       label_mask: Optional[torch.Tensor] = None, pose_label: Optional[torch.Tensor] = None,
                       stream=None, color_planes: Optional[torch.Tensor] = None, dc_index: bool = False):
        """Stage CLOUD (compute_point_clouds): returns (xyz (P,3), pose (P,), label (P,)); with `color_planes` (the
        rendered colour planes, uint8 (3, N, H, W): `render(..., color=True)`'s second output) also the points'
        colours (3, P) -- renderer.cu's result_cloud_color -- and with dc_index=True also result_dc_index (N, H, W)
        int32 (pcore_depth_to_cloud_ex), appended in that order."""
        if depth.dim() == 2:
            depth = depth.unsqueeze(0)
        n, h, w = depth.shape
        cap = n * ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
        dev = depth.device
        xyz = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=dev)
        pose = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
        lab = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
        cnt = ctypes.c_int32(0)
        extra = color_planes is not None or dc_index
        if not extra:
            self._check(self.lib.pcore_depth_to_cloud(
                self._h, _ptr(depth.contiguous(), torch.int32, "depth"), n, w, h, stride, float(depth_factor),
                _ptr(label_mask, torch.uint8, "label_mask"), _ptr(pose_label, torch.int32, "pose_label"),
                _ptr(xyz, torch.float32, "xyz"), _ptr(pose, torch.int32, "pose"), _ptr(lab, torch.int32, "label"),
                cap, ctypes.byref(cnt), _stream(stream)))
            k = cnt.value
            return xyz[:k], pose[:k], lab[:k]
        planes = None
        col = None
        if color_planes is not None:
            planes = color_planes.contiguous()
            if tuple(planes.shape) != (3, n, h, w):
                raise ValueError(f"color_planes must be (3, {n}, {h}, {w}), got {tuple(planes.shape)}")
            col = torch.empty((3, max(cap, 1)), dtype=torch.uint8, device=dev)
        dc = torch.empty((n, h, w), dtype=torch.int32, device=dev) if dc_index else None
        self._check(self.lib.pcore_depth_to_cloud_ex(
            self._h, _ptr(depth.contiguous(), torch.int32, "depth"), n, w, h, stride, float(depth_factor),
            _ptr(label_mask, torch.uint8, "label_mask"), _ptr(pose_label, torch.int32, "pose_label"),
            _ptr(planes, torch.uint8, "color_planes"), _ptr(xyz, torch.float32, "xyz"), _ptr(pose, torch.int32, "pose"),
            _ptr(lab, torch.int32, "label"), _ptr(col, torch.uint8, "color"), _ptr(dc, torch.int32, "dc_index"),
            max(cap, 1) if col is not None else cap, ctypes.byref(cnt), _stream(stream)))
        k = cnt.value
        out = [xyz[:k], pose[:k], lab[:k]]
        if col is not None:
            out.append(col[:, :k])
        if dc is not None:
            out.append(dc)
        return tuple(out)

    def select(self, rc: torch.Tensor, oc: torch.Tensor, pose_model: torch.Tensor, num_models: int,
               index_base: int = 0, keys: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """Per-model argmin keys (int64), folded into `keys` (initialised to PCORE_KEY_NONE)."""
        if keys is None:
            keys = torch.full((num_models,), _native.PCORE_KEY_NONE, dtype=torch.int64, device=rc.device)
        self._check(self.lib.pcore_select(
            self._h, _ptr(rc, torch.float32, "rc"), _ptr(oc, torch.float32, "oc"),
            _ptr(pose_model, torch.int32, "pose_model"), int(rc.shape[0]), int(index_base), int(num_models),
            _ptr(keys, torch.int64, "keys"), _stream(stream)))
        return keys

    def select_topk(self, rc: torch.Tensor, oc: torch.Tensor, pose_model: torch.Tensor, num_models: int, k: int,
                    index_base: int = 0, topk: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """The k smallest select keys per model (pcore_select_topk) as a (num_models, k) int64 tensor: every row
        ascending and padded with PCORE_KEY_NONE, folded into `topk` (initialised to PCORE_KEY_NONE) when given.
        decode_keys works on it elementwise."""
        if topk is None:
            topk = torch.full((int(num_models), int(k)), _native.PCORE_KEY_NONE, dtype=torch.int64, device=rc.device)
        elif tuple(topk.shape) != (int(num_models), int(k)):
            raise ValueError(f"topk: expected shape {(int(num_models), int(k))}, got {tuple(topk.shape)}")
        self._check(self.lib.pcore_select_topk(
            self._h, _ptr(rc, torch.float32, "rc"), _ptr(oc, torch.float32, "oc"),
            _ptr(pose_model, torch.int32, "pose_model"), int(rc.shape[0]), int(index_base), int(num_models), int(k),
            _ptr(topk, torch.int64, "topk"), _stream(stream)))
        return topk

    def count_within(self, queries: torch.Tensor, labels: torch.Tensor, radius_sq: torch.Tensor,
                     out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """IsValidPose neighbour counts (pcore_count_within): for every query (n x 3 float32), the points of its
        observed label segment strictly within sqrt(radius_sq) (float32 per query), PCL radiusSearch semantics."""
        n = int(queries.shape[0])
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=queries.device)
        self._check(self.lib.pcore_count_within(
            self._h, _ptr(queries.contiguous(), torch.float32, "queries"), _ptr(labels.contiguous(), torch.int32, "labels"),
            _ptr(radius_sq.contiguous(), torch.float32, "radius_sq"), n, _ptr(out, torch.int32, "counts"),
            _stream(stream)))
        return out

    def state_poses(self, states: torch.Tensor, model: torch.Tensor, cam_from_world, preprocess: torch.Tensor,
                    out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """The states' search poses (pcore_state_poses): init_from_eigen(cam_from_world * T(state) *
        preprocess[model], 100) for states (n x 7 float64: x y z qx qy qz qw), as N x 16 float32."""
        n = int(states.shape[0])
        if out is None:
            out = torch.empty((n, 16), dtype=torch.float32, device=states.device)
        cam = (ctypes.c_double * 16)(*[float(v) for v in np.asarray(cam_from_world, np.float64).reshape(16)])
        k = int(preprocess.shape[0])
        self._check(self.lib.pcore_state_poses(
            self._h, _ptr(states.contiguous(), torch.float64, "states"), _ptr(model.contiguous(), torch.int32, "model"),
            cam, _ptr(preprocess.contiguous(), torch.float64, "preprocess"), k, n, _ptr(out, torch.float32, "poses"),
            _stream(stream)))
        return out


class PoseLanes:
    """Batches in flight on one device: `lanes` independent contexts, each with its own HIP stream.

    A stage-COST launch ends with a drain (its last workgroups leave CUs idle) and starts with a fill in which
    every workgroup runs the same phase at once; on one stream the next batch waits for the drain.  Consecutive
    batches submitted to consecutive lanes overlap one batch's drain with the next one's fill (C2, 10k poses
    per batch: 0.40 -> 0.36 ms per batch with two lanes; tools/pipeline_probe.py).  Every lane holds the same
    meshes, camera and observation (setup calls go to all of them) and its own scratch, so lanes never share
    per-batch state, and each lane's results equal a single context's bit for bit.

    Work on lane i runs on streams[i]: run the whole step (evaluate, select, anything reading its outputs) under
    `with torch.cuda.stream(lanes.streams[i])`, or pass stream=.  Inputs written on another stream must be
    ordered before the lane's stream (lanes.streams[i].wait_stream(...)); lane i's output buffers are reused
    only by lane i, so stream order protects them."""

    def __init__(self, device: int = 0, lanes: int = 2):
        if lanes < 1:
            raise ValueError("lanes must be >= 1")
        self.cores = [PoseCore(device) for _ in range(lanes)]
        dev = torch.device("cuda", int(device))
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(lanes)]

    def __len__(self):
        return len(self.cores)

    def __getitem__(self, i: int) -> Tuple[PoseCore, torch.cuda.Stream]:
        return self.cores[i], self.streams[i]

    def upload_meshes(self, *a, **kw):
        for c in self.cores:
            c.upload_meshes(*a, **kw)

    def set_camera(self, *a, **kw):
        for c in self.cores:
            c.set_camera(*a, **kw)

    def set_observation(self, *a, **kw):
        for c in self.cores:
            c.set_observation(*a, **kw)

    def set_observation_colors(self, *a, **kw):
        for c in self.cores:
            c.set_observation_colors(*a, **kw)

    @classmethod
    def replicate(cls, core: "PoseCore", scene_setup, lanes: int = 2) -> "PoseLanes":
        """Lanes whose lane 0 is an existing, set-up context; scene_setup(c) repeats its setup on a new one."""
        if lanes < 1:
            raise ValueError("lanes must be >= 1")
        self = cls.__new__(cls)
        self.cores = [core] + [PoseCore(core.device) for _ in range(lanes - 1)]
        dev = torch.device("cuda", core.device)
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(lanes)]
        for c in self.cores[1:]:
            scene_setup(c)
        return self


def decode_keys(keys) -> Tuple[np.ndarray, np.ndarray]:
    """Per-model key -> (best cost, best global index); (INT_MAX, -1) where no pose qualified."""
    k = np.asarray(keys.cpu() if isinstance(keys, torch.Tensor) else keys, dtype=np.int64)
    none = k == _native.PCORE_KEY_NONE
    hi = (k >> 31).astype(np.uint64).astype(np.uint32)
    cost = (hi ^ np.uint32(0x80000000)).view(np.int32).astype(np.int32)
    idx = (k & 0x7FFFFFFF).astype(np.int64)
    cost = np.where(none, np.int32(2**31 - 1), cost)
    idx = np.where(none, -1, idx)
    return cost, idx


def encode_key(cost: int, index: int) -> int:
    """The int64 selection key of pcore_select (include/pcore.h): ((cost ^ 0x80000000) << 31) | index."""
    if cost == 2**31 - 1 and index < 0:
        return _native.PCORE_KEY_NONE
    hi = (int(cost) & 0xFFFFFFFF) ^ 0x80000000
    return (hi << 31) | (int(index) & 0x7FFFFFFF)
