/*
 * pcore.h -- C ABI of the MI355X render-and-compare pose-search core (libpcore.so).
 *
 * Drop-in boundary for the reference's GPU seam
 *   cuda_renderer::render_cuda_multi_unified(...)   (cuda_renderer/include/cuda_renderer/renderer.h:221-268,
 *                                                     cuda_renderer/src/cuda/renderer.cu:1431-1934)
 *   cuda_renderer::depth2cloud_global(...)          (renderer.h:131-153, renderer.cu:1936-2069)
 * and for the host selection it feeds
 *   EnvObjectRecognition::ComputeGreedyCostsInParallelGPU / ComputeGreedyRenderPoses
 *                                                    (sbpl_perception/src/search_env.cpp:1987-2051, 2542-2636).
 *
 * Conventions (differences from the reference are deliberate and listed in INTEGRATION.md):
 *   - Plain C types only.  Large per-batch arrays are DEVICE pointers (e.g. tensor.data_ptr() of a
 *     PyTorch-ROCm tensor); mesh and camera setup take HOST pointers (copied once).
 *   - Every call is asynchronous on the caller's stream (`stream` may be NULL = default stream); the
 *     caller synchronises.  One context per (host thread, device); calls on a context are not re-entrant,
 *     and its calls must all go to one stream (the context's device scratch -- GICP slots, the fused
 *     kernel's overflow list and window histogram -- is reused by the next call in stream order).
 *   - Caller-allocated outputs.  The context owns persistent device scratch and never frees caller memory.
 *   - Return value: PCORE_OK or an error code; pcore_last_error() describes the last failure.
 *     The reference's in-band "invalid pose" convention (rendered cost -1, compute_costs.cuh:28-31) is kept.
 *   - Poses are the reference's Model::mat4x4 (model.h:76-107): 16 floats a0..d3, row-major, rotation AND
 *     translation scaled by 100 (mat4x4::init_from_eigen(pose_in_cam, 100)), so vertices land in cm.
 */
#ifndef PCORE_H_
#define PCORE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCORE_ABI_VERSION 9

enum pcore_status {
    PCORE_OK = 0,
    PCORE_E_INVALID_ARG = 1, /* bad size / pointer / parameter */
    PCORE_E_HIP = 2,         /* a HIP runtime call failed */
    PCORE_E_OOM = 3,         /* device allocation failed */
    PCORE_E_STATE = 4        /* required setup call missing (meshes / camera / observation) */
};

/* Cost types of render_cuda_multi_unified (renderer.cu:1498): 0 = 3-DoF depth, 1 = 3-DoF RGB-D (a
 * matched point also needs CIEDE2000 <= color_distance_threshold, compute_costs.cuh:57-159, 222-240;
 * needs pcore_set_observation_colors), 2 = 6-DoF depth + labels. */
enum pcore_cost_type { PCORE_COST_DEPTH_3DOF = 0, PCORE_COST_RGBD_3DOF = 1, PCORE_COST_DEPTH_6DOF = 2 };

typedef struct pcore_ctx pcore_ctx;
typedef void* pcore_stream; /* hipStream_t */

/* Image geometry + intrinsics.  `proj` replaces the reference's proj_mat argument (renderer.h:225,
 * built by compute_proj, renderer.cu:1386-1410); fx/fy/cx/cy are kCameraFX.. (renderer.h:231-234). */
typedef struct pcore_camera {
    int32_t width, height;
    float fx, fy, cx, cy;
    float proj[16];
} pcore_camera;

/* Per-batch parameters of render_cuda_multi_unified that are not arrays (renderer.h:228-252). */
typedef struct pcore_eval_params {
    int32_t cost_type;           /* enum pcore_cost_type */
    int32_t calc_obs_cost;       /* calculate_observed_cost */
    int32_t stride;              /* gpu_stride; width % stride == 0 (compute_point_clouds.cuh:271) */
    float depth_factor;          /* rendered cm -> metres (the reference passes 100) */
    float sensor_resolution;     /* metres; squared internally like renderer.cu:1877 */
    float occlusion_threshold;   /* 3-DoF source-occlusion threshold in cm (gpu_occlusion_threshold) */
    float color_distance_threshold; /* cost_type 1: CIEDE2000 gate (renderer.h:247) */
} pcore_eval_params;

/* ---- lifetime ---------------------------------------------------------------------------------- */
int pcore_create(int device, pcore_ctx** out_ctx);
void pcore_destroy(pcore_ctx* ctx);
const char* pcore_last_error(const pcore_ctx* ctx);
int pcore_abi_version(void);

/* Generation of the context's device state.  A captured HIP graph of pcore_evaluate bakes in the kernel
 * arguments and the scratch pointers of the call it captured (sampled source, neighbour grids, overflow
 * list, colour scratch, tile size); the counter changes whenever any of them may have changed:
 * pcore_upload_meshes, pcore_set_camera, pcore_set_observation, pcore_set_observation_colors, a new
 * sampling stride, and every reallocation of per-batch scratch.  A replay is valid only while the
 * generation equals the one read right after the capture (no reference counterpart: the reference
 * re-uploads everything per call, renderer.cu:1532-1544).  0 for a NULL context.  A C caller that captures
 * pcore_evaluate into a graph compares pcore_generation before every replay, and orders its setup calls
 * after any replay still in flight on its stream (the check runs when the replay is enqueued). */
uint64_t pcore_generation(const pcore_ctx* ctx);

/* ---- static inputs ----------------------------------------------------------------------------- */
/* Triangles of all models concatenated + triangles per model: the `tris` and `tris_model_count`
 * arguments (renderer.h:223-226; filled by LoadObjFiles, search_env.cpp:253-307 / Model::LoadModel,
 * model.cpp:16-135).  tri_xyz: num_tris x 9 floats (v0,v1,v2) in metres, HOST.  tri_rgb: num_tris x 3
 * (vertex-0 colour, model.cpp:81-97), HOST, may be NULL (colour 128).  The context deduplicates
 * vertices and builds meshlets once here. */
int pcore_upload_meshes(pcore_ctx* ctx, const float* tri_xyz, const uint8_t* tri_rgb, int32_t num_tris,
                        const int32_t* tris_model_count, int32_t num_models);

int pcore_set_camera(pcore_ctx* ctx, const pcore_camera* cam);

/* ---- per-scene inputs -------------------------------------------------------------------------- */
/* depth2cloud_global (renderer.h:131-153; used by SetInput, search_env.cpp:5993-6017): unproject the
 * observed depth image (raw sensor units, e.g. YCB uint16 widened to int32) at `stride`, keeping pixels
 * with depth > 0 and (if label_mask != NULL) label > 0.  Writes xyz (cap x 3, metres) and label
 * (mask - 1) in the reference's compaction order; *out_count (HOST) receives the point count (the call
 * synchronises `stream` to return it).  Device pointers. */
int pcore_observed_cloud(pcore_ctx* ctx, const int32_t* d_depth, const uint8_t* d_label_mask, int32_t width,
                         int32_t height, int32_t stride, float depth_factor, float* d_out_xyz,
                         int32_t* d_out_label, int32_t cap, int32_t* out_count, pcore_stream stream);

/* depth2cloud_global for 3-DoF table-top scenes (renderer.cu:1936-2069 with camera_transform and
 * observed_cloud_bounds; compute_point_clouds.cuh:14-35, 79-91, 125-157): as pcore_observed_cloud
 * without a label mask, keeping only pixels whose point, moved to the world frame by `cam_to_world`
 * (HOST, 4 x 4 row-major float, R p + t evaluated left to right in float), lies inside `bounds` (HOST,
 * 6 doubles: x_max, x_min, y_max, y_min, z_max, z_min, compared as floats).  The output points stay in
 * the CAMERA frame, as in the reference.  cam_to_world and bounds are both given or both NULL.
 * d_rgb (nullable): H x W x 3 uint8 image; d_out_rgb (nullable, needs d_rgb) receives each kept
 * pixel's 3 bytes in the input's channel order. */
int pcore_observed_cloud_bounded(pcore_ctx* ctx, const int32_t* d_depth, const uint8_t* d_rgb, int32_t width,
                                 int32_t height, int32_t stride, float depth_factor, const float* cam_to_world,
                                 const double* bounds, float* d_out_xyz, uint8_t* d_out_rgb, int32_t cap,
                                 int32_t* out_count, pcore_stream stream);

/* Observation used by every evaluate call until replaced: the source depth in cm (H x W int32; the
 * reference's source_depth after search_env.cpp:2487-2498), the source mask label (H x W uint8, the
 * reference's source_mask_label; NULL for 3-DoF) and the observed cloud with its labels (the
 * observed_depth_eigen / result_observed_cloud_label pair, renderer.h:236-242).  The context sorts the
 * cloud by label (stable, renderer.cu:1674-1686) and builds its fixed-radius neighbour grids for
 * `sensor_resolution` metres.  Device pointers; the call synchronises `stream`. */
int pcore_set_observation(pcore_ctx* ctx, const int32_t* d_src_depth_cm, const uint8_t* d_src_mask,
                          const float* d_obs_xyz, const int32_t* d_obs_label, int32_t num_obs,
                          float sensor_resolution, pcore_stream stream);

/* Colours of the observed points for cost_type 1 (the observed_color argument, renderer.h:236-238):
 * n x 3 uint8 (DEVICE) in the order of the d_obs_xyz given to pcore_set_observation, channels as the
 * image (the reference's result_observed_cloud_color planes).  The context converts them to CIE Lab with
 * the reference's channel order (rgb2lab(c2, c1, c0), compute_costs.cuh:57-88, 214-220).  Valid until the
 * next pcore_set_observation.  Triangle colours come from pcore_upload_meshes (tri_rgb; 128 grey when
 * NULL, model.cpp:97-101). */
int pcore_set_observation_colors(pcore_ctx* ctx, const uint8_t* d_obs_rgb, int32_t num_obs, pcore_stream stream);

/* ---- per-batch hot path ------------------------------------------------------------------------ */
/* Stage "COST" of render_cuda_multi_unified with do_icp = false: render every pose, unproject at
 * stride, 1-NN against the same-label observed points, and the rendered / observed / points-diff
 * costs (compute_costs.cuh:293-457).  d_pose_label NULL selects 3-DoF (all observed points, occlusion
 * by threshold).  d_pose_obs_total: pose_observed_points_total (renderer.h:240).  Outputs N floats each
 * (d_out_oc / d_out_diff are written as 0 when calc_obs_cost == 0).  d_dbg_zs (nullable): the sampled
 * z-buffer after source occlusion, N x ceil(H/stride) x (W/stride) int32 (parity / debugging). */
int pcore_evaluate(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model,
                   const int32_t* d_pose_label, const float* d_pose_obs_total, int32_t num_poses,
                   const pcore_eval_params* params, float* d_out_rc, float* d_out_oc, float* d_out_diff,
                   int32_t* d_dbg_zs, pcore_stream stream);

/* GICP settings; the reference hard-codes the first four at renderer.cu:1696-1705.  cycle_exit_window (no
 * reference counterpart): a pose whose float transforms have recurred with the same period for
 * this many iterations, each step accepted at its first trial with an inert damping, stops and reports
 * max_iterations and the cycle member the remaining iterations end on; 0 runs every iteration out, as fast_gicp
 * does; the spec's value is 8 (PCORE_GICP_CYCLE_WINDOW). */
#define PCORE_GICP_CYCLE_WINDOW 8
typedef struct pcore_icp_params {
    int32_t k_correspondences;      /* covariance neighbours, 10 (<= 16) */
    int32_t max_iterations;         /* 150 */
    double rotation_epsilon;        /* 2e-3 */
    double transformation_epsilon;  /* 5e-4 */
    int32_t cycle_exit_window;      /* 8 (0 = off) */
} pcore_icp_params;

/* pcore_evaluate followed by pcore_select in one launch: every pose's argmin key (pcore_select's, global index
 * index_base + i) is folded into d_keys[model] (atomic MIN) by the workgroup that scores the pose, so the batch
 * needs no separate selection pass.  The costs are written as by pcore_evaluate (d_out_oc may not be null); the
 * keys equal pcore_evaluate + pcore_select's. */
int pcore_evaluate_select(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model,
                          const int32_t* d_pose_label, const float* d_pose_obs_total, int32_t num_poses,
                          const pcore_eval_params* params, float* d_out_rc, float* d_out_oc, float* d_out_diff,
                          int64_t index_base, int32_t num_models, int64_t* d_keys, pcore_stream stream);

/* Stage "COST" with do_icp = true (renderer.cu:1688-1817): render, unproject at stride, per-pose GICP of
 * the rendered cloud onto the pose's observed label segment (FastGICPCudaCore::optimize_multi), compose
 * T * pose (concatenate_transforms, renderer.cu:1412-1429), re-render and re-score.  d_out_poses: N x 16
 * adjusted mat4x4 (the reference's adjusted_poses); d_out_iters (nullable): GICP iterations per pose.
 * Costs as pcore_evaluate, for the adjusted poses.  Device pointers; needs per-context scratch that
 * grows on first use (64 B per pose and stride sample; a batch is split into equal chunks that fit a
 * budget of min(32 GiB, 40 % of the free device memory)). */
int pcore_evaluate_icp(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model,
                       const int32_t* d_pose_label, const float* d_pose_obs_total, int32_t num_poses,
                       const pcore_eval_params* params, const pcore_icp_params* icp, float* d_out_poses,
                       int32_t* d_out_iters, float* d_out_rc, float* d_out_oc, float* d_out_diff,
                       pcore_stream stream);

/* Planar (x, y, yaw) ICP of the 3-DoF search (ComputeGreedyCostsInParallelGPU with icp_type 0 and use_icp 1,
 * search_env.cpp:1843-1973: GetICPAdjustedPosesCPU -> GetICPAdjustedPose, 1198-1299, 6235-6396, a PCL ICP with
 * TransformationEstimation2D on the host between the two GPU passes).  The loop is the build's own spec modelled on
 * PCL's ("Planar ICP spec"); the defaults are the reference's settings. */
typedef struct pcore_planar_icp_params {
    int32_t max_iterations;         /* 20  (max_icp_iterations) */
    float   max_correspondence;     /* 0.05 m (icp_max_correspondence) */
    double  transformation_epsilon; /* 1e-8 */
    double  fitness_epsilon;        /* 1e-5 */
} pcore_planar_icp_params;

/* Render every pose at stage CLOUD (stride samples, 3-DoF source occlusion: the slots pcore_evaluate_icp feeds GICP)
 * and align each cloud to the observation -- its points in the order given to pcore_set_observation -- in the plane:
 * both are moved to the world frame by world_from_cam (HOST, 4 x 4 row-major float, each row left to right in float)
 * and only x, y and yaw move.  d_out_xform: N x 4 doubles (c, s, tx, ty), the cumulative world-frame transform
 * x' = c x - s y + tx, y' = s x + c y + ty; d_out_iters: estimation steps done; d_out_status: 0 = iteration cap,
 * 1 = transform threshold, 2 = absolute mse, 3 = relative mse, 4 = fewer than 3 correspondences (identity), 5 = empty
 * render (identity, 0 iterations); d_out_mse (nullable): the last iteration's mean squared correspondence distance (0
 * for status 4 and 5).  Only the 3-DoF cost types (0, 1) are accepted; there are no pose labels.  Every argument is
 * checked before the first launch.  The batch is split into equal chunks that fit a scratch budget of min(32 GiB, 40 %
 * of the free device memory) at 16 B per pose and stride sample.  The observation's world-frame copy and its
 * neighbour grid (cells >= 2 max_correspondence) are built on first use and kept while the observation, the matrix
 * bytes and the radius stay the same; a capturing stream that would need that build, or new scratch, gets
 * PCORE_E_STATE (run the call once before the capture). */
int pcore_icp_planar(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model, int32_t num_poses,
                     const pcore_eval_params* params, const float* world_from_cam,
                     const pcore_planar_icp_params* icp, double* d_out_xform, int32_t* d_out_iters,
                     int32_t* d_out_status, double* d_out_mse, pcore_stream stream);

/* Test hook (no reference counterpart): the planar ICP's estimation step (TransformationEstimation2D on raw sums,
 * DESIGN.md section 5) of n records of 10 doubles -- n, sum qx, sum qy, sum tx, sum ty, sum qx tx, sum qx ty,
 * sum qy tx, sum qy ty, sum d^2 -- into d_out (n x 4: c', s', tx', ty'), one thread each. */
int pcore_debug_planar_step(const double* d_sums, double* d_out, int32_t n, pcore_stream stream);

/* Test hook (no reference counterpart): the colour gate's CIEDE2000 distance (compute_costs.cuh:90-158) as the fused
 * cost kernel of cost_type 1 evaluates it on the device: n pairs of six floats (l1 a1 b1 l2 a2 b2) into d_out (n
 * doubles), one thread each. */
int pcore_debug_colour_distance(const float* d_lab_pairs, double* d_out, int32_t n, pcore_stream stream);

/* Test hook (no reference counterpart): the RGB -> Lab conversion that pcore_upload_meshes and
 * pcore_set_observation_colors store, of n colours (3 bytes each, in the order they are given there) into out_lab
 * (n x 3 floats: L a b).  Host only: both pointers are host memory and no device is needed. */
int pcore_debug_rgb2lab(const uint8_t* rgb, float* out_lab, int32_t n);

/* Point-to-plane ICP against a projective scene (cuda_icp: ICP_Point2Plane_cuda, icp.cu:157-218; Scene_projective,
 * depth_scene.h; get_normal, scene/common.cpp:17-107).  A correspondence is one projection and one gather from the
 * observed depth image: no neighbour search, no labels, no covariances.  The loop is the reference's, operation for
 * operation, with three build-owned choices (sum order, trigonometry, float-to-pixel conversion): DESIGN.md section 5,
 * "Point-to-plane ICP spec". */
typedef struct pcore_p2p_icp_params {
    int32_t max_iterations;     /* 30   (ICPConvergenceCriteria, icp.h:39-51) */
    float   relative_fitness;   /* 1e-5 */
    float   relative_rmse;      /* 1e-5 */
    float   max_dist_diff;      /* 0.1 m (Scene_projective, depth_scene.h:9) */
} pcore_p2p_icp_params;

/* Scene_projective's buffers of a depth image (int32 cm, read as uint32 for the points and saturated to uint16 for the
 * normals): d_out_pcd and d_out_normal, H x W x 3 floats each -- dep2pcd of every pixel, and the linemod normal (radius
 * 5, depth below 2000, difference threshold 50) where it is defined, zero elsewhere.  Needs only a context; the camera
 * is the arguments'. */
int pcore_scene_projective(pcore_ctx* ctx, const int32_t* d_depth_cm, int32_t width, int32_t height, float fx, float fy,
                           float cx, float cy, float* d_out_pcd, float* d_out_normal, pcore_stream stream);

/* Render every pose at stage CLOUD (stride samples; with d_pose_label the 6-DoF source occlusion of
 * pcore_evaluate_icp, with NULL the 3-DoF one) and align each cloud to the scene of the observation's source depth.
 * d_out_T: N x 16 row-major, the cumulative camera-frame transform; d_out_fitness: accepted points / points;
 * d_out_rmse: sqrt(sum of squared plane distances / accepted); d_out_iters: the iteration at which the loop returned
 * (an empty render: T = I, fitness 0, rmse 0, iteration 0); d_out_poses (nullable, N x 16): concatenate_transforms(T,
 * pose), the pose pcore_evaluate re-scores.  All cost types are accepted.  Every argument is checked before the first
 * launch.  The batch is split into equal chunks that fit a scratch budget of min(32 GiB, 40 % of the free device
 * memory) at 16 B per pose and stride sample.  The scene (32 B per pixel) is built on first use and kept while the
 * observation and the camera stay the same; a capturing stream that would need that build, or new scratch, gets
 * PCORE_E_STATE (run the call once before the capture). */
int pcore_icp_point2plane(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model,
                          const int32_t* d_pose_label, int32_t num_poses, const pcore_eval_params* params,
                          const pcore_p2p_icp_params* icp, float* d_out_T, float* d_out_fitness, float* d_out_rmse,
                          int32_t* d_out_iters, float* d_out_poses, pcore_stream stream);

/* Test hook (no reference counterpart): the same kernel over caller-made slots (segment i: d_xyzw + 4 i seg_stride,
 * d_seg_cnt[i] points of 4 floats, moved in place) and a caller-made scene (one float4 per pixel each). */
int pcore_debug_p2p_clouds(const float* d_xyzw, const int32_t* d_seg_cnt, int32_t seg_stride, int32_t num_segs,
                           const float* d_scene_pcd4, const float* d_scene_normal4, int32_t width, int32_t height,
                           float fx, float fy, float cx, float cy, const pcore_p2p_icp_params* icp, float* d_out_T,
                           float* d_out_fitness, float* d_out_rmse, int32_t* d_out_iters, pcore_stream stream);

/* Point-to-plane ICP against a nearest-neighbour scene (cuda_icp: ICP_Point2Plane_cuda over Scene_nn,
 * pcd_scene.h:48-137): each point is paired with the nearest scene point in 3-D, so the correspondence follows the
 * nearest surface across a depth edge where the projective scene pairs it with whatever its own pixel shows.  The
 * reference's kd-tree over the whole cloud is replaced by an exact search over the pixels within `window` of the
 * point's own pixel (the lowest pixel index wins on equal distances), which is the nearest neighbour of the whole
 * image whenever every pixel that can hold a point within max_dist_diff lies inside that window: DESIGN.md section 5,
 * "Nearest-neighbour scene".  The loop is pcore_icp_point2plane's.  The source depth is integer centimetres, so the
 * scene is quantised at the size of the default radius. */
typedef struct pcore_nn_icp_params {
    int32_t max_iterations;     /* 30 */
    float   relative_fitness;   /* 1e-5 */
    float   relative_rmse;      /* 1e-5 */
    float   max_dist_diff;      /* 0.01 m, the search radius (Scene_nn, pcd_scene.h:49); > 0 */
    int32_t window;             /* 32 pixels, the search window's half-width; 0 ... 128 */
} pcore_nn_icp_params;

/* pcore_icp_point2plane with the nearest-neighbour scene: the same arguments, outputs, scene cache, scratch budget
 * (PCORE_P2P_SCRATCH_BYTES), chunking and capture rule.  Every argument is checked before the first launch. */
int pcore_icp_point2plane_nn(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model,
                             const int32_t* d_pose_label, int32_t num_poses, const pcore_eval_params* params,
                             const pcore_nn_icp_params* icp, float* d_out_T, float* d_out_fitness, float* d_out_rmse,
                             int32_t* d_out_iters, float* d_out_poses, pcore_stream stream);

/* Test hook (no reference counterpart): pcore_debug_p2p_clouds over the nearest-neighbour scene.  The scene's points
 * must be dep2pcd of a centimetre depth image under the given camera (as pcore_scene_projective writes them): the
 * search skips pixels whose point cannot lie within the radius. */
int pcore_debug_p2p_nn_clouds(const float* d_xyzw, const int32_t* d_seg_cnt, int32_t seg_stride, int32_t num_segs,
                              const float* d_scene_pcd4, const float* d_scene_normal4, int32_t width, int32_t height,
                              float fx, float fy, float cx, float cy, const pcore_nn_icp_params* icp, float* d_out_T,
                              float* d_out_fitness, float* d_out_rmse, int32_t* d_out_iters, pcore_stream stream);

/* Test hook (no reference counterpart): stage CLOUD of every pose into caller-made slots, as the ICP entry points
 * render their source clouds -- pose i's points (x, y, z, 0) in the reference's compaction order (row-major stride
 * samples, compute_point_clouds.cuh:290-346) at d_out_xyzw + 4 i ws hs, their number in d_out_count[i]; ws = W / stride,
 * hs = ceil(H / stride).  params: stride, depth_factor and occlusion_threshold are used; d_pose_label as pcore_evaluate. */
int pcore_debug_render_clouds(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model,
                              const int32_t* d_pose_label, int32_t num_poses, const pcore_eval_params* params,
                              float* d_out_xyzw, int32_t* d_out_count, pcore_stream stream);

/* Stage "RENDER" / "DEBUG" images (renderer.cu:1594-1615): full-resolution int32 z-buffers (cm) with source
 * occlusion and INT_MAX -> 0 (image_render, image_renderer.cuh:336-496).  d_out_depth: N x H x W.
 * d_out_color (nullable): the reference's result_color -- three planes red, green, blue of N x H x W uint8 each,
 * concatenated -- holding each pixel's nearest triangle colour (the first triangle reaching the minimum depth,
 * as the serial z-test of image_renderer.cuh:146-159 keeps it; the tri_rgb of pcore_upload_meshes), black where
 * nothing is rendered or the source occludes the render (image_renderer.cuh:160-196). */
int pcore_render(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                 int32_t num_poses, float occlusion_threshold, int32_t* d_out_depth, uint8_t* d_out_color,
                 pcore_stream stream);

/* The composed state: every pose into ONE frame, the picture PrintStateGPU draws of the greedy state
 * (search_env.cpp:1718-1781: render_cuda_multi_unified("RENDER", ..., single_result_image = 1), image_renderer.cuh:
 * 262-275).  The reference's single image is racy and reads an empty source; the contract here is deterministic
 * ("Composed state").  With D_i, C_i what pcore_render returns for pose i alone (for occlude = 0:
 * against an all-zero source, no black-out at all):
 *   d_out_depth   H x W int32: the minimum D_i[p] over the poses with D_i[p] != 0, else 0
 *   d_out_owner   H x W int32 (nullable): the lowest i attaining it, else -1 -- a predicted instance mask
 *   d_out_color   3 x H x W uint8 (nullable), red / green / blue planes: C_owner[p], black without an owner
 *   d_out_visible num_poses int32 (nullable): the pixels each pose owns
 * A pose whose nearest fragment at a pixel has depth 0 (a NaN depth of a degenerate triangle, a surface within a
 * centimetre of the camera's plane) has D_i[p] = 0 and so is absent there: the poses behind it show.
 * occlude = 1 needs meshes, camera and observation (d_pose_label as in pcore_render); occlude = 0 needs meshes and a
 * camera only, and d_pose_label must be NULL.  num_poses * num_tris must not exceed 2^32 - 1 (the key of a pixel holds
 * pose * num_tris + triangle in 32 bits).  num_poses == 0 writes the empty frame.  Model ids outside the meshes render
 * nothing.  Asynchronous on `stream`, no host readback; every argument is checked before the first launch, and a
 * refused call writes nothing.  Per-context scratch of 8 B per pixel grows on first use. */
int pcore_render_scene(pcore_ctx* ctx, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                       int32_t num_poses, int32_t occlude, float occlusion_threshold, int32_t* d_out_depth,
                       uint8_t* d_out_color, int32_t* d_out_owner, int32_t* d_out_visible, pcore_stream stream);

/* Stage COST of composed states (no reference counterpart: PERCH's objective is a cost of the whole state, which the
 * reference's greedy GPU path dropped; DESIGN.md section 2, "State cost").  d_zs holds num_poses sampled z-buffers after
 * source occlusion, exactly what pcore_evaluate writes to d_dbg_zs (hs x ws int32 each; 0 = nothing of this pose here).
 * State s is the member list d_state_member[d_state_off[s] .. d_state_off[s + 1]) of indices into them.  Per sample the
 * minimum non-zero depth over the members wins and the lowest list position attaining it owns the sample; owned samples
 * of positive depth are the state's points (a negative minimum hides what is behind it and yields no point).  Each point
 * is unprojected as pcore_evaluate does and matched with the exact 1-NN (ties to the lowest index) against the observed
 * segment of d_pose_label[owner] -- an empty one for a label outside the segments -- or, for cost_type 0, against the
 * whole cloud (d_pose_label is then ignored and may be NULL); it is bad when d^2 > r^2.
 *   d_out_member_vis / _bad   num_members int32 each (nullable): the points / bad points every list entry owns
 *   d_out_rc / _oc / _diff    num_states floats each, pcore_evaluate's formulas over num = sum vis, bad = sum bad, expl =
 *                             the DISTINCT observed points that are the neighbour of a non-bad point of any member, and
 *                             tot = d_state_obs_total[s]; oc and diff are written as 0 when calc_obs_cost == 0
 * A one-member state with tot = pose_obs_total equals pcore_evaluate's costs of that pose bit for bit.  A member outside
 * [0, num_poses) contributes nothing; a duplicate member never owns a sample; a state without members has rc = -1; a
 * span that is not positive, or that leaves [0, num_members], is an empty state.  Spans of different states that overlap
 * leave the member outputs of the shared entries undefined (the states' costs stay defined).  Neither the members per state nor the
 * states are limited.  Needs a camera and an observation (PCORE_E_STATE otherwise), no meshes.  cost_type 1 and a stride
 * that does not divide the width get PCORE_E_INVALID_ARG.  num_states == 0 is a no-op.  Asynchronous on `stream`, no host
 * readback; every argument is checked before the first launch, and a refused call writes nothing.  While the observed
 * cloud has at most PCORE_STATE_LDS_OBS points the explained bitmap lives in the workgroup's LDS; above, in per-context
 * scratch that grows on first use (the growth changes pcore_generation; a capturing stream that would need it gets
 * PCORE_E_STATE). */
#define PCORE_STATE_LDS_OBS 131072
int pcore_evaluate_states(pcore_ctx* ctx, const int32_t* d_zs, int32_t num_poses, const int32_t* d_pose_label,
                          const int32_t* d_state_off, const int32_t* d_state_member, int32_t num_states,
                          const float* d_state_obs_total, const pcore_eval_params* params, float* d_out_rc,
                          float* d_out_oc, float* d_out_diff, int32_t* d_out_member_vis, int32_t* d_out_member_bad,
                          int32_t num_members, pcore_stream stream);

/* gpu_stats of render_cuda_multi_unified (model.h:24-27, filled at renderer.cu:1707 and 1739) for the last
 * pcore_evaluate_icp: icp_runtime = seconds of its GICP stage (source covariances + GICP launches, HIP events on
 * the call's stream -- this call waits for them); peak_memory_usage = the most device memory in use (MB,
 * hipMemGetInfo like print_cuda_memory_usage, cuda/utils.cuh:6-24) at a GICP stage since the last reset;
 * gicp_ms = the GICP launches alone; icp_chunks = chunks the batch ran in; gicp_iterations = the iterations the
 * poses report (d_out_iters summed), gicp_iterations_run = the iterations executed (fewer by the cycle exits),
 * gicp_cycle_exits = poses that left by the cycle exit.  reset != 0 restarts the peak. */
typedef struct pcore_gpu_stats {
    float icp_runtime;
    double peak_memory_usage;
    float gicp_ms;
    int32_t icp_chunks;
    int64_t gicp_iterations;
    int64_t gicp_iterations_run;
    int64_t gicp_cycle_exits;
} pcore_gpu_stats;
int pcore_get_stats(pcore_ctx* ctx, pcore_gpu_stats* out, int32_t reset);

/* LDS tile of the fused window launch (no reference counterpart: the reference renders whole frames; DESIGN.md
 * "Pose windows").  tier = the tier the next call starts from (wgs_per_cu[tier] workgroups per CU, a tile of
 * edge[tier] samples), tcap = the tile of the last launch; hist[b] = the poses of launch seq whose window held
 * more than edge[b-1] and at most edge[b] samples (hist[num_tiers]: more than edge[num_tiers-1]); chunked = its
 * poses scored in chunks of the tile.  seq numbers the context's launches from 1 (each launch publishes the counts
 * of the one before it); seq < 1: no counts yet.  Diagnostics only: the results never depend on the tile. */
#define PCORE_MAX_TILE_TIERS 8
typedef struct pcore_tile_info {
    int32_t num_tiers;
    int32_t tier;
    int32_t tcap;
    int32_t seq;
    int32_t edge[PCORE_MAX_TILE_TIERS];
    int32_t wgs_per_cu[PCORE_MAX_TILE_TIERS];
    int32_t hist[PCORE_MAX_TILE_TIERS + 1];
    int32_t chunked;
} pcore_tile_info;
int pcore_get_tile_info(pcore_ctx* ctx, pcore_tile_info* out);

/* Test hook (no reference counterpart): the GICP kernels' damped LM solve (H + lambda I) d = -b of n raw 28-term
 * systems (upper H row-major, b, error; d_sys n x 28, d_lambda n, d_out n x 6 doubles), one wave each, for the
 * parity test against the oracle's restatement of Eigen's pivoted LDLT. */
int pcore_debug_lm_solve(const double* d_sys, const double* d_lambda, double* d_out, int32_t n, pcore_stream stream);

/* Test hook (no reference counterpart): the GICP covariances of point segments by covariance_kernel (fast_gicp's
 * k-nearest-neighbour covariance with PLANE regularisation): d_xyzw = points as x, y, z, w floats;
 * segment s is points d_seg_off[s] .. + d_seg_cnt[s] (its own neighbour set); d_out_cov6 gets 6 doubles per point
 * (upper triangle, row-major).  1 <= k <= 16. */
int pcore_debug_covariances(const float* d_xyzw, const int32_t* d_seg_off, const int32_t* d_seg_cnt, int32_t num_segs,
                            int32_t k, double* d_out_cov6, pcore_stream stream);
/* Test hook (no reference counterpart): the k = 10 covariances of rendered-cloud slots (segment i: d_xyzw + 4 i
 * seg_stride, d_seg_cnt[i] points) by the threshold k-NN over each cloud's stride-s sample grid (camera fx, fy, cx, cy;
 * pcore_cov.h), falling back to the brute force where the grid does not allow it: bit-identical to
 * pcore_debug_covariances for any points. */
int pcore_debug_covariances_cloud(const float* d_xyzw, const int32_t* d_seg_cnt, int32_t seg_stride, int32_t num_segs,
                                  float fx, float fy, float cx, float cy, int32_t stride, double* d_out_cov6,
                                  pcore_stream stream);

/* GenerateSuccessorStates / GetStateImagesUnifiedGPU host work on the device (search_env.cpp:7056-7254,
 * 1535-1576), for the drop-in recognizer's states:
 *
 * pcore_count_within: IsValidPose's neighbour count (search_env.cpp:359-396, pcl::search::KdTree radiusSearch):
 * for every query i, the points of observed label segment d_labels[i] (as set by pcore_set_observation; a label
 * outside the segments counts 0) strictly within the radius -- float query and points, d_radius_sq[i] = float(r *
 * r), ((0 + dx^2) + dy^2) + dz^2 < r^2 in float.  d_queries: n x 3 float; d_out_counts: n int32.
 *
 * pcore_state_poses: the states' poses for the GPU search: for state i (x y z qx qy qz qw, double), cam_from_world
 * (HOST, 16 doubles row-major: inv(camera_pose * cam_to_body)) * ContPose::GetTransform (normalised quaternion,
 * object_state.cpp:83-97) * d_preprocess[d_model[i]] (16 doubles row-major per model, PreprocessModel), every
 * product summed in index order in double, then mat4x4::init_from_eigen(., 100) (model.h:89-107) into
 * d_out_poses (n x 16 float).  Model ids must lie in [0, num_models). */
int pcore_count_within(pcore_ctx* ctx, const float* d_queries, const int32_t* d_labels, const float* d_radius_sq,
                       int32_t n, int32_t* d_out_counts, pcore_stream stream);
int pcore_state_poses(pcore_ctx* ctx, const double* d_states, const int32_t* d_model, const double* cam_from_world,
                      const double* d_preprocess, int32_t num_models, int32_t n, float* d_out_poses,
                      pcore_stream stream);

/* Stage "CLOUD": compute_point_clouds (compute_point_clouds.cuh:188-367) over N z-buffers: stride mask,
 * pose-major / row / column compaction, unprojection.  xyz AoS (cap x 3).  d_label_mask (H x W) only
 * for num_poses == 1; d_pose_label gives the rendered-cloud label.  *out_count (HOST) = total points
 * (the call synchronises `stream`). */
int pcore_depth_to_cloud(pcore_ctx* ctx, const int32_t* d_depth, int32_t num_poses, int32_t width, int32_t height,
                         int32_t stride, float depth_factor, const uint8_t* d_label_mask,
                         const int32_t* d_pose_label, float* d_out_xyz, int32_t* d_out_pose, int32_t* d_out_label,
                         int32_t cap, int32_t* out_count, pcore_stream stream);

/* Stage "CLOUD" with the reference's two debug outputs as well (renderer.cu:1821-1847): d_color_planes = the
 * rendered colour planes (red, green, blue planes of N x H x W uint8 each -- pcore_render's d_out_color) and
 * d_out_color = each point's colour from them as three planes of `cap` bytes (depth_to_2d_cloud,
 * compute_point_clouds.cuh:163-165; the reference's plane stride is its point count, the same when cap equals it);
 * d_out_dc_index = result_dc_index (N x H x W int32): for every pixel the number of cloud points before it in pose /
 * row / column order, the reference's exclusive scan of the stride mask (compute_point_clouds.cuh:267-292).  Both
 * outputs are nullable; the rest is pcore_depth_to_cloud's. */
int pcore_depth_to_cloud_ex(pcore_ctx* ctx, const int32_t* d_depth, int32_t num_poses, int32_t width, int32_t height,
                            int32_t stride, float depth_factor, const uint8_t* d_label_mask, const int32_t* d_pose_label,
                            const uint8_t* d_color_planes, float* d_out_xyz, int32_t* d_out_pose, int32_t* d_out_label,
                            uint8_t* d_out_color, int32_t* d_out_dc_index, int32_t cap, int32_t* out_count,
                            pcore_stream stream);

/* Host selection of the reference moved on device: cost = (int)(rc + oc) (x86 conversion semantics),
 * skip invalid (-1/-2), keep |(int)rc - (int)oc| < 30, per-model minimum with strict '<' (lowest global
 * index wins ties) -- search_env.cpp:2022-2048, 2554-2566.  Result is folded into d_keys[num_models]
 * (int64, atomic min) as key = ((uint32)(cost ^ 0x80000000) << 31) | (index_base + i); initialise
 * d_keys to PCORE_KEY_NONE.  Keys from several batches / ranks combine with a MIN reduction
 * (RCCL all-reduce). */
#define PCORE_KEY_NONE ((int64_t)0x7fffffffffffffffLL)
int pcore_select(pcore_ctx* ctx, const float* d_rc, const float* d_oc, const int32_t* d_pose_model,
                 int32_t num_poses, int64_t index_base, int32_t num_models, int64_t* d_keys, pcore_stream stream);

/* The k best candidates per model instead of the minimum alone (no reference counterpart; the reference tracks the
 * pre-ICP ranking beside the post-ICP one, lowest_preicp_cost_per_object, search_env.cpp:2567-2572): every pose gets
 * exactly pcore_select's key.  Row m of d_topk (num_models x k int64, DEVICE) is a list of k keys in ascending order,
 * padded with PCORE_KEY_NONE; the caller initialises it to PCORE_KEY_NONE.  After the call row m holds the k smallest
 * keys of its previous content and the batch's keys of model m, ascending, so lists fold across batches (of disjoint
 * index ranges) as pcore_select's keys do.  Keys carry the global index: they are distinct and totally ordered, equal
 * costs order by lowest index first, and the result depends neither on scheduling nor on how the batch is cut nor on
 * the order in which batches are folded.  With k = 1 the row equals pcore_select's d_keys[m].  Model ids outside [0,
 * num_models) are ignored.  Lists of several ranks combine by taking the k smallest of their union.  Asynchronous on
 * `stream`, no host readback.  Every argument is checked before the first launch (pcore_select's checks, with a last global
 * index of at most 2^31 - 1, and 1 <= k <= PCORE_TOPK_MAX).  Per-context scratch for partial lists (at most 1024 x num_models x k keys) grows on first use; a
 * capturing stream that would need that growth gets PCORE_E_STATE (run the call once before the capture), and the
 * growth changes pcore_generation.  PCORE_TOPK_SLICE: the poses per partial list of a batch of at most 2^20 poses
 * (diagnostics and tests; the results never depend on it). */
#define PCORE_TOPK_MAX 64
#define PCORE_TOPK_SLICE 1024
int pcore_select_topk(pcore_ctx* ctx, const float* d_rc, const float* d_oc, const int32_t* d_pose_model,
                      int32_t num_poses, int64_t index_base, int32_t num_models, int32_t k,
                      int64_t* d_topk /* num_models x k, in/out */, pcore_stream stream);

/* ADD / ADD-S of estimated against ground-truth poses over one model's points -- the YCB harness
 * metric: compare_clouds (sbpl_perception/src/scripts/tools/fat_dataset/
 * fat_pose_image.py:2020-2139) and pose_error.add / adi (fat_dataset/lib/utils/pose_error.py:72-108).
 *   d_pts      n x 3 float model points (model frame, metres), device
 *   d_T_gt,    num_pairs x 16 double, row-major 4x4 object-to-camera transforms, device
 *   d_T_est
 *   d_add      num_pairs doubles: mean_i |T_gt p_i - T_est p_i|           (nullable)
 *   d_adds     num_pairs doubles: mean_i min_j |T_gt p_i - T_est p_j|     (nullable)
 * f64 arithmetic; the minimum is exact (no kd-tree approximation).  Needs only a context (no meshes /
 * camera / observation). */
int pcore_pose_distances(pcore_ctx* ctx, const float* d_pts, int32_t n, const double* d_T_gt, const double* d_T_est,
                         int32_t num_pairs, double* d_add, double* d_adds, pcore_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PCORE_H_ */
