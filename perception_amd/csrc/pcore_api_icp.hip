// pcore_api_icp.hip -- the staged-cloud driver (pcore_ctx.h, Staged) and the entry points built on it alone: the planar
// and the point-to-plane ICPs and their debug hooks.  pcore_evaluate_icp (pcore_api_eval.hip) uses the driver too.
#include "pcore_ctx.h"
#include "pcore_icp2d_math.h"
#include "pcore_p2p_math.h"
#include "pcore_prep.h"

#include <cmath>
#include <cstddef>
#include <cstring>

using namespace pcore;

namespace pcore {

int staged_slots(pcore_ctx* c, Staged& st) {
    if (const int rc = ensure_sampled(c, st.p->stride, st.s)) return rc;
    HIPC(c, reserve_gen(c, c->icp_cloud, (size_t)st.chunk * st.nsamp));
    HIPC(c, reserve_gen(c, c->icp_count, (size_t)st.chunk));
    st.cloud = c->icp_cloud.p;
    st.count = c->icp_count.p;
    fill_fused_args(c, st.p, st.a);
    return PCORE_OK;
}

// render_cloud_kernel, rastered through the fused launch's most-occupied tile (6 workgroups per CU; larger windows in
// chunks of it).  PCORE_FUSED_TCAP (test knob): a tile of that many samples.
hipError_t stage_chunk(pcore_ctx* c, Staged& st, int base, int n) {
    FusedArgs& a = st.a;
    a.poses = st.poses + (size_t)16 * base;
    a.pose_model = st.pose_model + base;
    a.pose_label = st.pose_label ? st.pose_label + base : nullptr;
    a.num_poses = n;
    a.cloud_out = st.cloud;
    a.cloud_count = st.count;
    a.cloud_cap = a.ws * a.hs;
    a.tcap = fused_tier_samples(0, a.ws, a.hs, 0, false, c->dinfo);
    if (const char* e = getenv("PCORE_FUSED_TCAP")) a.tcap = std::min(std::max(atoi(e), 1), a.ws * a.hs);
    if (a.tcap <= 0) a.tcap = a.ws * a.hs;
    return launch_render_cloud(a, st.s);
}

}  // namespace pcore

namespace {

// The checks of a staged call, in the order they are reported: the state, `bad` (the caller's own parameter checks: the
// message after "who: ", or nullptr), pose labels without a source mask, check_sampling (lds_hint ends its LDS message)
int staged_checks(pcore_ctx* c, Staged& st, const char* bad, const char* lds_hint) {
    const std::string pre = std::string(st.who) + ": ";
    if (!c->have_mesh || !c->have_cam || !c->have_obs)
        return fail(c, PCORE_E_STATE, pre + "meshes, camera and observation must be set first");
    if (bad) return fail(c, PCORE_E_INVALID_ARG, pre + bad);
    if (st.pose_label && !c->obs_has_mask) return fail(c, PCORE_E_INVALID_ARG, pre + "pose labels need a source mask");
    return check_sampling(c, st.who, st.p->stride, false, lds_hint, false, st.nsamp);
}

// What an ICP over staged slots (16 B a sample and a count per pose; `knob`: its scratch budget in bytes) does between
// its checks and its launches.  Its cache, named `what` and keyed by `serial` (the observation it was built from), is
// rebuilt by build() when stale; whatever has to be built or allocated is refused while the stream captures.
template <typename Build>
int staged_setup(pcore_ctx* c, Staged& st, const char* knob, const char* what, bool stale, uint64_t& serial, Build build) {
    HIPC(c, hipSetDevice(c->device));
    st.chunk = plan_chunks(st.num_poses, (size_t)st.nsamp * sizeof(float4) + sizeof(int32_t), knob, 0);
    const bool setup = stale || c->sampled_stride != st.p->stride || c->icp_cloud.n < (size_t)st.chunk * st.nsamp ||
                       c->icp_count.n < (size_t)st.chunk;
    if (const int cr = refuse_setup_in_capture(c, st.who, what, setup, st.s)) return cr;
    if (stale) {
        HIPC(c, hipStreamSynchronize(st.s));  // an earlier call on the stream may still read the old cache
        serial = 0;
        c->generation++;
        if (const int rc = build()) return rc;
        serial = c->obs_serial;
    }
    return staged_slots(c, st);
}

const char* planar_params_error(const pcore_eval_params* p, const pcore_planar_icp_params* pp, const float* world_from_cam) {
    if (p->cost_type != PCORE_COST_DEPTH_3DOF && p->cost_type != PCORE_COST_RGBD_3DOF)
        return "cost_type must be a 3-DoF one (0 or 1)";
    if (pp->max_iterations < 0) return "max_iterations must be >= 0";
    if (!std::isfinite(pp->max_correspondence) || pp->max_correspondence < 0.0f)
        return "max_correspondence must be finite and >= 0";
    if (std::isnan(pp->transformation_epsilon) || std::isnan(pp->fitness_epsilon)) return "NaN epsilon";
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(world_from_cam[i])) return "non-finite world_from_cam";
    return nullptr;
}

// In the templates below P is pcore_p2p_icp_params (the projective scene: nn = false, window 0) or pcore_nn_icp_params
// (nn = true, its window): the same fields but for the window.  The parameters' checks; nullptr when they hold.
template <typename P>
const char* p2p_params_error(const P& ip, int window, bool nn) {
    if (ip.max_iterations < 0) return "max_iterations must be >= 0";
    if (std::isnan(ip.relative_fitness) || ip.relative_fitness < 0.0f) return "relative_fitness must be >= 0";
    if (std::isnan(ip.relative_rmse) || ip.relative_rmse < 0.0f) return "relative_rmse must be >= 0";
    if (!nn && (std::isnan(ip.max_dist_diff) || ip.max_dist_diff < 0.0f)) return "max_dist_diff must be >= 0";
    if (nn && !(ip.max_dist_diff > 0.0f)) return "max_dist_diff must be > 0";
    if (window < 0 || window > p2p::kNnMaxWindow) return "window must be 0 ... 128";
    return nullptr;
}

// P2pArgs but for the batch's poses: the slots, the scene and its camera, the parameters, the outputs
template <typename P>
P2pArgs fill_p2p_args(float4* src, const int32_t* src_count, int src_cap, const float4* pcd, const float4* normal,
                      int width, int height, float fx, float fy, float cx, float cy, const P& ip, int window,
                      float* d_out_T, float* d_out_fitness, float* d_out_rmse, int32_t* d_out_iters) {
    P2pArgs g{};
    g.src = src; g.src_count = src_count; g.src_cap = src_cap;
    g.scene_pcd = pcd; g.scene_normal = normal;
    g.width = width; g.height = height;
    g.fx = fx; g.fy = fy; g.cx = cx; g.cy = cy;
    g.max_dist_diff = ip.max_dist_diff;
    g.rel_fitness = ip.relative_fitness;
    g.rel_rmse = ip.relative_rmse;
    g.max_iter = ip.max_iterations;
    g.window = window;
    g.out_T = d_out_T; g.out_fitness = d_out_fitness; g.out_rmse = d_out_rmse; g.out_iters = d_out_iters;
    return g;
}

// Point-to-plane ICP against the projective (nn = false) or the nearest-neighbour scene of the observation's source
// depth (ICP_Point2Plane_cuda, cuda_icp/icp.cu:157-218; Scene_nn, pcd_scene.h:48-137): stage CLOUD into per-pose slots,
// then the scene's kernel over the slots.  The scene buffers, their cache and rebuild keys, the scratch budget and the
// chunking are the same for both.  Every check comes before the first launch, so an invalid call writes nothing.
template <typename P>
int icp_point2plane_impl(pcore_ctx* c, const char* who, const float* d_poses, const int32_t* d_pose_model,
                         const int32_t* d_pose_label, int32_t num_poses, const pcore_eval_params* p, const P& ip,
                         int window, bool nn, float* d_out_T, float* d_out_fitness, float* d_out_rmse,
                         int32_t* d_out_iters, float* d_out_poses, pcore_stream stream) {
    Staged st{who, p, d_poses, d_pose_model, d_pose_label, num_poses, (hipStream_t)stream};
    const char* bad = p2p_params_error(ip, window, nn);
    if (p->cost_type != PCORE_COST_DEPTH_3DOF && p->cost_type != PCORE_COST_DEPTH_6DOF &&
        p->cost_type != PCORE_COST_RGBD_3DOF)
        bad = "unknown cost_type";
    else if (!bad && (num_poses < 0 || (num_poses > 0 && (!d_poses || !d_pose_model || !d_out_T || !d_out_fitness ||
                                                          !d_out_rmse || !d_out_iters))))
        bad = "null pose / output pointer";
    if (const int vr = staged_checks(c, st, bad, " (use a larger stride)")) return vr;
    if (num_poses == 0) return PCORE_OK;
    const pcore_camera& cam = c->cam;
    const int W = cam.width, H = cam.height;
    // the scene is kept while the observation, the image size and the bytes of fx, fy, cx, cy stay the same
    const bool stale = c->p2p_obs_serial != c->obs_serial ||
                       std::memcmp(&c->p2p_cam, &cam, offsetof(pcore_camera, proj)) != 0;
    const int rc = staged_setup(c, st, "PCORE_P2P_SCRATCH_BYTES", "the scene", stale, c->p2p_obs_serial, [&]() -> int {
        const size_t npx = (size_t)W * H;
        HIPC(c, dev_reserve(c->p2p_pcd, npx));
        HIPC(c, dev_reserve(c->p2p_normal, npx));
        HIPC(c, launch_p2p_scene(c->src_depth.p, W, H, cam.fx, cam.fy, cam.cx, cam.cy, c->p2p_pcd.p, c->p2p_normal.p,
                                 nullptr, nullptr, st.s));
        c->p2p_cam = cam;
        return PCORE_OK;
    });
    if (rc != PCORE_OK) return rc;
    P2pArgs g = fill_p2p_args(st.cloud, st.count, st.nsamp, c->p2p_pcd.p, c->p2p_normal.p, W, H, cam.fx, cam.fy, cam.cx,
                              cam.cy, ip, window, d_out_T, d_out_fitness, d_out_rmse, d_out_iters);
    g.poses_in = d_poses;
    g.poses_out = d_out_poses;
    return for_each_chunk(c, st, [&](int base, int n) -> int {
        g.pose_base = base;
        HIPC(c, nn ? launch_p2p_nn_icp(g, n, st.s) : launch_p2p_icp(g, n, st.s));
        return PCORE_OK;
    });
}

// the two debug hooks' body: the scene's kernel over caller-made slots and a caller-made scene
template <typename P>
int debug_p2p_clouds(const float* d_xyzw, const int32_t* d_seg_cnt, int32_t seg_stride, int32_t num_segs,
                     const float* d_scene_pcd4, const float* d_scene_normal4, int32_t width, int32_t height, float fx,
                     float fy, float cx, float cy, const P& ip, int window, bool nn, float* d_out_T,
                     float* d_out_fitness, float* d_out_rmse, int32_t* d_out_iters, pcore_stream stream) {
    if (p2p_params_error(ip, window, nn) || num_segs < 0 || seg_stride < 0 || width <= 0 || height <= 0 ||
        width > 16384 || height > 16384 || !d_scene_pcd4 || !d_scene_normal4 ||
        (num_segs > 0 && (!d_xyzw || !d_seg_cnt || !d_out_T || !d_out_fitness || !d_out_rmse || !d_out_iters)))
        return PCORE_E_INVALID_ARG;
    const P2pArgs g = fill_p2p_args((float4*)d_xyzw, d_seg_cnt, seg_stride, (const float4*)d_scene_pcd4,
                                    (const float4*)d_scene_normal4, width, height, fx, fy, cx, cy, ip, window, d_out_T,
                                    d_out_fitness, d_out_rmse, d_out_iters);
    const hipError_t e = nn ? launch_p2p_nn_icp(g, num_segs, (hipStream_t)stream)
                            : launch_p2p_icp(g, num_segs, (hipStream_t)stream);
    return e == hipSuccess ? PCORE_OK : PCORE_E_HIP;
}

}  // namespace

extern "C" {

// Planar ICP between the two passes of the 3-DoF search (GetICPAdjustedPosesCPU, search_env.cpp:1198-1299): stage
// CLOUD into per-pose slots (launch_render_cloud, as pcore_evaluate_icp's first step), then planar_icp_kernel over
// the slots.  Every check comes before the first launch, so an invalid call writes nothing.
int pcore_icp_planar(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model, int32_t num_poses,
                     const pcore_eval_params* p, const float* world_from_cam, const pcore_planar_icp_params* pp,
                     double* d_out_xform, int32_t* d_out_iters, int32_t* d_out_status, double* d_out_mse,
                     pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!p || !pp || !world_from_cam) return fail(c, PCORE_E_INVALID_ARG, "icp_planar: null parameters");
    Staged st{"icp_planar", p, d_poses, d_pose_model, nullptr, num_poses, (hipStream_t)stream};
    const char* bad = planar_params_error(p, pp, world_from_cam);
    if (!bad && (num_poses < 0 || (num_poses > 0 && (!d_poses || !d_pose_model || !d_out_xform || !d_out_iters ||
                                                     !d_out_status))))
        bad = "null pose / output pointer";
    if (const int vr = staged_checks(c, st, bad, " (use a larger stride)")) return vr;
    if (num_poses == 0) return PCORE_OK;
    // the world-frame grid is kept while the observation, the matrix's bytes and the radius stay the same
    const bool stale = c->planar_obs_serial != c->obs_serial ||
                       std::memcmp(c->planar_m, world_from_cam, sizeof(c->planar_m)) != 0 ||
                       std::memcmp(&c->planar_radius, &pp->max_correspondence, sizeof(float)) != 0;
    const int rc = staged_setup(c, st, "PCORE_ICP2D_SCRATCH_BYTES", "the world-frame grid", stale, c->planar_obs_serial,
                                [&]() -> int {
        const int n = (int)(c->obs_xyz_h.size() / 3);
        std::vector<float4> wp((size_t)n);
        for (int i = 0; i < n; i++) {
            float4 q;
            icp2d::to_world(world_from_cam, c->obs_xyz_h[3 * (size_t)i], c->obs_xyz_h[3 * (size_t)i + 1],
                            c->obs_xyz_h[3 * (size_t)i + 2], q.x, q.y, q.z);
            std::memcpy(&q.w, &i, 4);
            wp[i] = q;
        }
        std::vector<int32_t> cell_start;
        std::vector<float4> gpts;
        prep::build_grid(wp, pp->max_correspondence, c->planar_grid, cell_start, gpts);
        if (gpts.empty()) gpts.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        HIPC(c, dev_upload(c->planar_cell_start, cell_start));
        HIPC(c, dev_upload(c->planar_pts, gpts));
        std::memcpy(c->planar_m, world_from_cam, sizeof(c->planar_m));
        c->planar_radius = pp->max_correspondence;
        return PCORE_OK;
    });
    if (rc != PCORE_OK) return rc;
    PlanarArgs g{};
    g.src = st.cloud;
    g.src_count = st.count;
    g.src_cap = st.nsamp;
    for (int i = 0; i < 12; i++) g.m[i] = world_from_cam[i];
    g.grid = c->planar_grid;
    g.cell_start = c->planar_cell_start.p;
    g.grid_pts = c->planar_pts.p;
    g.r = pp->max_correspondence;
    g.r2 = pp->max_correspondence * pp->max_correspondence;
    g.max_iter = pp->max_iterations;
    g.eps_t = pp->transformation_epsilon;
    g.eps_fit = pp->fitness_epsilon;
    g.out_xform = d_out_xform;
    g.out_iters = d_out_iters;
    g.out_status = d_out_status;
    g.out_mse = d_out_mse;
    return for_each_chunk(c, st, [&](int base, int n) -> int {
        g.pose_base = base;
        HIPC(c, launch_planar_icp(g, n, st.s));
        return PCORE_OK;
    });
}

int pcore_debug_planar_step(const double* d_sums, double* d_out, int32_t n, pcore_stream stream) {
    if (n < 0 || (n > 0 && (!d_sums || !d_out))) return PCORE_E_INVALID_ARG;
    return launch_planar_step_test(d_sums, d_out, n, (hipStream_t)stream) == hipSuccess ? PCORE_OK : PCORE_E_HIP;
}

int pcore_scene_projective(pcore_ctx* c, const int32_t* d_depth_cm, int32_t width, int32_t height, float fx, float fy,
                           float cx, float cy, float* d_out_pcd, float* d_out_normal, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (width <= 0 || height <= 0 || width > 16384 || height > 16384)
        return fail(c, PCORE_E_INVALID_ARG, "scene_projective: bad image size");
    if (!d_depth_cm || !d_out_pcd || !d_out_normal)
        return fail(c, PCORE_E_INVALID_ARG, "scene_projective: null pointer");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, launch_p2p_scene(d_depth_cm, width, height, fx, fy, cx, cy, nullptr, nullptr, d_out_pcd, d_out_normal,
                             (hipStream_t)stream));
    return PCORE_OK;
}

int pcore_icp_point2plane(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                          int32_t num_poses, const pcore_eval_params* p, const pcore_p2p_icp_params* ip,
                          float* d_out_T, float* d_out_fitness, float* d_out_rmse, int32_t* d_out_iters,
                          float* d_out_poses, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!p || !ip) return fail(c, PCORE_E_INVALID_ARG, "icp_point2plane: null parameters");
    return icp_point2plane_impl(c, "icp_point2plane", d_poses, d_pose_model, d_pose_label, num_poses, p, *ip, 0,
                                false, d_out_T, d_out_fitness, d_out_rmse, d_out_iters, d_out_poses, stream);
}

int pcore_icp_point2plane_nn(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model,
                             const int32_t* d_pose_label, int32_t num_poses, const pcore_eval_params* p,
                             const pcore_nn_icp_params* ip, float* d_out_T, float* d_out_fitness, float* d_out_rmse,
                             int32_t* d_out_iters, float* d_out_poses, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!p || !ip) return fail(c, PCORE_E_INVALID_ARG, "icp_point2plane_nn: null parameters");
    return icp_point2plane_impl(c, "icp_point2plane_nn", d_poses, d_pose_model, d_pose_label, num_poses, p, *ip,
                                ip->window, true, d_out_T, d_out_fitness, d_out_rmse, d_out_iters, d_out_poses, stream);
}

int pcore_debug_p2p_clouds(const float* d_xyzw, const int32_t* d_seg_cnt, int32_t seg_stride, int32_t num_segs,
                           const float* d_scene_pcd4, const float* d_scene_normal4, int32_t width, int32_t height,
                           float fx, float fy, float cx, float cy, const pcore_p2p_icp_params* ip, float* d_out_T,
                           float* d_out_fitness, float* d_out_rmse, int32_t* d_out_iters, pcore_stream stream) {
    if (!ip) return PCORE_E_INVALID_ARG;
    return debug_p2p_clouds(d_xyzw, d_seg_cnt, seg_stride, num_segs, d_scene_pcd4, d_scene_normal4, width, height, fx,
                            fy, cx, cy, *ip, 0, false, d_out_T, d_out_fitness, d_out_rmse, d_out_iters, stream);
}

int pcore_debug_p2p_nn_clouds(const float* d_xyzw, const int32_t* d_seg_cnt, int32_t seg_stride, int32_t num_segs,
                              const float* d_scene_pcd4, const float* d_scene_normal4, int32_t width, int32_t height,
                              float fx, float fy, float cx, float cy, const pcore_nn_icp_params* ip, float* d_out_T,
                              float* d_out_fitness, float* d_out_rmse, int32_t* d_out_iters, pcore_stream stream) {
    if (!ip) return PCORE_E_INVALID_ARG;
    return debug_p2p_clouds(d_xyzw, d_seg_cnt, seg_stride, num_segs, d_scene_pcd4, d_scene_normal4, width, height, fx,
                            fy, cx, cy, *ip, ip->window, true, d_out_T, d_out_fitness, d_out_rmse, d_out_iters, stream);
}

// Test hook: stage CLOUD into caller-made slots (render_cloud_kernel as pcore_evaluate_icp, pcore_icp_planar and
// pcore_icp_point2plane launch it, without the covariances).  Every check comes before the launch.
int pcore_debug_render_clouds(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model,
                              const int32_t* d_pose_label, int32_t num_poses, const pcore_eval_params* p,
                              float* d_out_xyzw, int32_t* d_out_count, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!p) return fail(c, PCORE_E_INVALID_ARG, "debug_render_clouds: null parameters");
    Staged st{"debug_render_clouds", p, d_poses, d_pose_model, d_pose_label, num_poses, (hipStream_t)stream,
              (float4*)d_out_xyzw, d_out_count};
    const bool null_ptr = num_poses < 0 || (num_poses > 0 && (!d_poses || !d_pose_model || !d_out_xyzw || !d_out_count));
    if (const int vr = staged_checks(c, st, null_ptr ? "null pose / output pointer" : nullptr, "")) return vr;
    if (num_poses == 0) return PCORE_OK;
    HIPC(c, hipSetDevice(c->device));
    if (const int rc = ensure_sampled(c, p->stride, st.s)) return rc;
    fill_fused_args(c, p, st.a);
    HIPC(c, stage_chunk(c, st, 0, num_poses));
    return PCORE_OK;
}

}  // extern "C"
