// pcore_api.hip -- C ABI (include/pcore.h) of the MI355X pose-search core: the context's lifetime, the static inputs
// (mesh dedupe + vertex-ring streams, camera), the per-scene observation (label sort + neighbour grids; the arithmetic
// is pcore_prep.h's), and the parity stages' dispatch (clouds, render, select, states, metrics, debug hooks).  The
// per-batch path is pcore_api_eval.hip, the staged ICPs pcore_api_icp.hip.  Scratch grows monotonically.
#include "pcore_ctx.h"
#include "pcore_prep.h"
#include "pcore_streams.h"
#include "pcore_topk.h"

#include <climits>

using namespace pcore;

extern "C" {

int pcore_abi_version(void) { return PCORE_ABI_VERSION; }

int pcore_create(int device, pcore_ctx** out_ctx) {
    if (!out_ctx) return PCORE_E_INVALID_ARG;
    *out_ctx = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return PCORE_E_INVALID_ARG;
    pcore_ctx* c = new pcore_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess) {
        delete c;
        return PCORE_E_HIP;
    }
    // per-context (not function-static) launch constants: contexts on other devices or threads never share
    // or race on them
    DeviceInfo& d = c->dinfo;
    d.num_cus = std::max(1, c->prop.multiProcessorCount);
    d.lds_per_cu = c->prop.maxSharedMemoryPerMultiProcessor ? (size_t)c->prop.maxSharedMemoryPerMultiProcessor
                                                            : (size_t)160 * 1024;
    d.lds_granule = kLdsGranule;
    if (const char* e = getenv("PCORE_LDS_GRANULE")) d.lds_granule = (size_t)std::max(atoi(e), 4);  // A/B only
    int per_cu = 0;
    if (gicp_occupancy_per_cu(&per_cu) != hipSuccess) {
        delete c;
        return PCORE_E_HIP;
    }
    d.gicp_resident_wgs = std::max(1, per_cu) * d.num_cus;
    *out_ctx = c;
    return PCORE_OK;
}

uint64_t pcore_generation(const pcore_ctx* c) { return c ? c->generation : 0; }

void pcore_destroy(pcore_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;  // every member owns what it allocated (pcore_ctx.h)
}

const char* pcore_last_error(const pcore_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pcore_upload_meshes(pcore_ctx* c, const float* tri_xyz, const uint8_t* tri_rgb, int32_t num_tris,
                        const int32_t* tris_model_count, int32_t num_models) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!tri_xyz || num_tris <= 0 || !tris_model_count || num_models <= 0)
        return fail(c, PCORE_E_INVALID_ARG, "upload_meshes: empty mesh");
    long long acc = 0;
    for (int m = 0; m < num_models; m++) {
        if (tris_model_count[m] < 0) return fail(c, PCORE_E_INVALID_ARG, "upload_meshes: negative count");
        acc += tris_model_count[m];
    }
    if (acc != num_tris) return fail(c, PCORE_E_INVALID_ARG, "upload_meshes: sum(tris_model_count) != num_tris");
    HIPC(c, hipSetDevice(c->device));
    c->generation++;

    streams::Built sb;
    int chunks = kStreamChunks;
    if (const char* e = getenv("PCORE_STREAM_CHUNKS")) chunks = std::max(1, atoi(e));  // A/B knob
    int model_streams = kFusedWaves;
    if (const char* e = getenv("PCORE_MODEL_STREAMS")) model_streams = std::max(1, atoi(e));  // A/B knob
    std::vector<float4> box;
    std::vector<int32_t> slo(num_models), shi(num_models), tlo(num_models), thi(num_models);
    int t0 = 0;
    for (int m = 0; m < num_models; m++) {
        const int T = tris_model_count[m];
        tlo[m] = t0;
        thi[m] = t0 + T;
        const prep::ModelVerts mv = prep::dedupe_model(tri_xyz + (size_t)9 * t0, T);
        box.push_back(mv.bmin);
        box.push_back(mv.bmax);
        slo[m] = (int)sb.streams.size();
        streams::build_model(mv.tv, mv.vxyz, t0, model_streams, kVRing, kRefPasses, sb, chunks);
        shi[m] = (int)sb.streams.size();
        t0 += T;
    }
    // one padding step and one padding vertex pass after the last stream: the fused kernel prefetches the step and
    // the pass after the current ones unconditionally (within a model that is the next stream's first one)
    sb.stris.insert(sb.stris.end(), kStepSlots, streams::kSlotPadding);
    sb.sorig.insert(sb.sorig.end(), kStepSlots, 0u);
    sb.sverts.insert(sb.sverts.end(), kStepSlots, streams::F4{0.0f, 0.0f, 0.0f, 0.0f});
    HIPC(c, dev_upload(c->tris, tri_xyz, (size_t)9 * num_tris));
    HIPC(c, dev_upload(c->tri_lo, tlo));
    HIPC(c, dev_upload(c->tri_hi, thi));
    static_assert(sizeof(streams::F4) == sizeof(float4) && sizeof(streams::I4) == sizeof(int4), "stream layouts");
    HIPC(c, dev_upload(c->sverts, sb.sverts.data(), sb.sverts.size()));
    HIPC(c, dev_upload(c->stris, sb.stris));
    HIPC(c, dev_upload(c->streams, sb.streams.data(), sb.streams.size()));
    HIPC(c, dev_upload(c->stri_orig, sb.sorig));
    const prep::TriColours col = prep::tri_colours(tri_rgb, num_tris);
    HIPC(c, dev_upload(c->tri_lab, col.lab));
    HIPC(c, dev_upload(c->tri_rgb, col.packed));
    HIPC(c, dev_upload(c->model_st_lo, slo));
    HIPC(c, dev_upload(c->model_st_hi, shi));
    HIPC(c, dev_upload(c->model_box, box));
    c->num_models = num_models;
    c->num_tris = num_tris;
    c->have_mesh = true;
    return PCORE_OK;
}

int pcore_set_camera(pcore_ctx* c, const pcore_camera* cam) {
    if (!c || !cam) return PCORE_E_INVALID_ARG;
    if (cam->width <= 0 || cam->height <= 0 || cam->width > 16384 || cam->height > 16384)
        return fail(c, PCORE_E_INVALID_ARG, "set_camera: bad image size");
    HIPC(c, hipSetDevice(c->device));
    c->generation++;
    c->cam = *cam;
    HIPC(c, dev_upload(c->proj, cam->proj, 16));
    c->have_cam = true;
    c->have_obs = false;  // observation is tied to the image size
    c->sampled_stride = 0;
    return PCORE_OK;
}

int pcore_observed_cloud(pcore_ctx* c, const int32_t* d_depth, const uint8_t* d_label_mask, int32_t width,
                         int32_t height, int32_t stride, float depth_factor, float* d_out_xyz, int32_t* d_out_label,
                         int32_t cap, int32_t* out_count, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!c->have_cam) return fail(c, PCORE_E_STATE, "observed_cloud: camera not set");
    return pcore_depth_to_cloud(c, d_depth, 1, width, height, stride, depth_factor, d_label_mask, nullptr, d_out_xyz,
                                nullptr, d_out_label, cap, out_count, stream);
}

int pcore_observed_cloud_bounded(pcore_ctx* c, const int32_t* d_depth, const uint8_t* d_rgb, int32_t width,
                                 int32_t height, int32_t stride, float depth_factor, const float* cam_to_world,
                                 const double* bounds, float* d_out_xyz, uint8_t* d_out_rgb, int32_t cap,
                                 int32_t* out_count, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!c->have_cam) return fail(c, PCORE_E_STATE, "observed_cloud_bounded: camera not set");
    if (width <= 0 || height <= 0 || stride <= 0 || !d_depth || cap < 0 || (cap > 0 && !d_out_xyz) || !out_count ||
        (!cam_to_world) != (!bounds) || (d_out_rgb && !d_rgb))
        return fail(c, PCORE_E_INVALID_ARG, "observed_cloud_bounded: bad arguments");
    if (width % stride != 0) return fail(c, PCORE_E_INVALID_ARG, "observed_cloud_bounded: width % stride != 0");
    CloudBounds cb{};
    if (cam_to_world) {
        cb.on = 1;
        for (int i = 0; i < 12; i++) cb.m[i] = cam_to_world[i];
        for (int i = 0; i < 6; i++) cb.b[i] = (float)bounds[i];
        cb.cx = c->cam.cx;
        cb.cy = c->cam.cy;
        cb.fx = c->cam.fx;
        cb.fy = c->cam.fy;
        cb.depth_factor = depth_factor;
    }
    *out_count = 0;
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    HIPC(c, dev_reserve(c->scratch_counts, 1));
    HIPC(c, dev_reserve(c->scratch_offsets, 1));
    HIPC(c, dev_reserve(c->scratch_total, 1));
    HIPC(c, launch_cloud_count(d_depth, 1, width, height, stride, nullptr, cb, c->scratch_counts.p, s));
    HIPC(c, launch_exclusive_scan(c->scratch_counts.p, c->scratch_offsets.p, 1, c->scratch_total.p, s));
    HIPC(c, launch_cloud_write(d_depth, 1, width, height, stride, c->cam.cx, c->cam.cy, c->cam.fx, c->cam.fy,
                               depth_factor, nullptr, nullptr, c->scratch_offsets.p, d_out_xyz, nullptr, nullptr, cap,
                               cb, d_rgb, d_out_rgb, s));
    int32_t total = 0;
    HIPC(c, hipMemcpyAsync(&total, c->scratch_total.p, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    *out_count = total;
    return PCORE_OK;
}

int pcore_set_observation_colors(pcore_ctx* c, const uint8_t* d_obs_rgb, int32_t num_obs, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!c->have_obs) return fail(c, PCORE_E_STATE, "set_observation_colors: call pcore_set_observation first");
    if (num_obs != (int)c->obs_order.size() || (num_obs > 0 && !d_obs_rgb))
        return fail(c, PCORE_E_INVALID_ARG, "set_observation_colors: num_obs differs from the observation");
    HIPC(c, hipSetDevice(c->device));
    c->generation++;
    hipStream_t s = (hipStream_t)stream;
    std::vector<uint8_t> rgb((size_t)num_obs * 3);
    if (num_obs > 0) HIPC(c, hipMemcpyAsync(rgb.data(), d_obs_rgb, rgb.size(), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    std::vector<float4> labv(std::max(num_obs, 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int k = 0; k < num_obs; k++) labv[k] = prep::lab_of(&rgb[3 * (size_t)c->obs_order[k]]);
    HIPC(c, dev_upload(c->obs_lab, labv));
    c->have_obs_colours = true;
    return PCORE_OK;
}

int pcore_set_observation(pcore_ctx* c, const int32_t* d_src_depth_cm, const uint8_t* d_src_mask,
                          const float* d_obs_xyz, const int32_t* d_obs_label, int32_t num_obs,
                          float sensor_resolution, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!c->have_cam) return fail(c, PCORE_E_STATE, "set_observation: camera not set");
    if (!d_src_depth_cm || num_obs < 0 || (num_obs > 0 && !d_obs_xyz))
        return fail(c, PCORE_E_INVALID_ARG, "set_observation: bad arguments");
    if (!(sensor_resolution >= 0.0f)) return fail(c, PCORE_E_INVALID_ARG, "set_observation: bad sensor_resolution");
    HIPC(c, hipSetDevice(c->device));
    c->generation++;
    hipStream_t s = (hipStream_t)stream;
    const size_t npx = (size_t)c->cam.width * c->cam.height;
    HIPC(c, dev_reserve(c->src_depth, npx));
    HIPC(c, hipMemcpyAsync(c->src_depth.p, d_src_depth_cm, npx * 4, hipMemcpyDeviceToDevice, s));
    c->obs_has_mask = d_src_mask != nullptr;
    HIPC(c, dev_reserve(c->src_mask, npx));
    if (d_src_mask) HIPC(c, hipMemcpyAsync(c->src_mask.p, d_src_mask, npx, hipMemcpyDeviceToDevice, s));
    else HIPC(c, hipMemsetAsync(c->src_mask.p, 0, npx, s));

    // observed cloud -> host: stable label sort, neighbour grids, GICP targets (pcore_prep.h)
    std::vector<float> xyz((size_t)num_obs * 3);
    std::vector<int32_t> lab(num_obs, 0);
    if (num_obs > 0) {
        HIPC(c, hipMemcpyAsync(xyz.data(), d_obs_xyz, xyz.size() * 4, hipMemcpyDeviceToHost, s));
        if (d_obs_label) HIPC(c, hipMemcpyAsync(lab.data(), d_obs_label, lab.size() * 4, hipMemcpyDeviceToHost, s));
    }
    HIPC(c, hipStreamSynchronize(s));
    const prep::Sorted sorted = prep::sort_by_label(xyz, lab);
    const prep::Grids grids = prep::observation_grids(xyz, lab, sorted, sensor_resolution);
    const prep::Quads quads = prep::target_quads(sorted);
    c->obs_order = sorted.order;
    c->have_obs_colours = false;
    c->obs_xyz_h = xyz;  // pcore_icp_planar's targets, in the caller's order
    c->obs_serial++;
    // GICP targets and their segments; covariances are computed lazily per k
    HIPC(c, dev_upload(c->tgt, sorted.tgt));
    HIPC(c, dev_upload(c->seg_lo, sorted.lo));
    HIPC(c, dev_upload(c->seg_hi, sorted.hi));
    HIPC(c, dev_upload(c->seg_cnt, sorted.cnt));
    c->seg_lo_h = sorted.lo;
    c->seg_cnt_h = sorted.cnt;
    HIPC(c, dev_upload(c->tgt_quads, quads.quads));
    HIPC(c, dev_upload(c->seg_qoff, quads.qoff));
    c->num_obs = num_obs;
    c->max_seg = sorted.max_seg;
    c->cov_k_label = 0;
    c->cov_k_all = 0;
    HIPC(c, dev_upload(c->grids, grids.grids));
    HIPC(c, dev_upload(c->cell_start, grids.cell_start));
    HIPC(c, dev_upload(c->grid_pts, grids.pts));
    c->num_grids = sorted.num_labels;
    c->bitmap_words = std::max(1, (grids.max_count + 31) / 32);
    c->sampled_stride = 0;
    c->have_obs = true;
    return PCORE_OK;
}

int pcore_render(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                 int32_t num_poses, float occlusion_threshold, int32_t* d_out_depth, uint8_t* d_out_color,
                 pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!c->have_mesh || !c->have_cam || !c->have_obs)
        return fail(c, PCORE_E_STATE, "render: meshes, camera and observation must be set first");
    if (num_poses < 0 || (num_poses > 0 && (!d_poses || !d_pose_model || !d_out_depth)))
        return fail(c, PCORE_E_INVALID_ARG, "render: null pointer");
    if (d_pose_label && !c->obs_has_mask)
        return fail(c, PCORE_E_INVALID_ARG, "render: pose labels need a source mask");
    if (num_poses == 0) return PCORE_OK;
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int W = c->cam.width, H = c->cam.height;
    HIPC(c, launch_fill_i32(d_out_depth, INT_MAX, (size_t)num_poses * W * H, s));
    HIPC(c, launch_render_full(c->tris.p, c->num_tris, c->tri_lo.p, c->tri_hi.p, d_poses, d_pose_model, num_poses, W,
                               H, c->proj.p, d_out_depth, s));
    int32_t* tri_min = nullptr;
    if (d_out_color) {  // stage RENDER / DEBUG colour planes: the nearest triangle per pixel, second pass
        const size_t npx = (size_t)num_poses * W * H;
        HIPC(c, dev_reserve(c->render_tri, npx));
        tri_min = c->render_tri.p;
        HIPC(c, launch_fill_i32(tri_min, INT_MAX, npx, s));
        HIPC(c, launch_render_full_tri(c->tris.p, c->num_tris, c->tri_lo.p, c->tri_hi.p, d_poses, d_pose_model,
                                       num_poses, W, H, c->proj.p, d_out_depth, tri_min, s));
    }
    HIPC(c, launch_render_finalize(d_out_depth, c->src_depth.p, c->src_mask.p, d_pose_label, num_poses, W, H,
                                   occlusion_threshold, s, tri_min, d_out_color ? c->tri_rgb.p : nullptr, d_out_color));
    return PCORE_OK;
}

int pcore_render_scene(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                       int32_t num_poses, int32_t occlude, float occlusion_threshold, int32_t* d_out_depth,
                       uint8_t* d_out_color, int32_t* d_out_owner, int32_t* d_out_visible, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!c->have_mesh || !c->have_cam)
        return fail(c, PCORE_E_STATE, "render_scene: meshes and camera must be set first");
    if (occlude && !c->have_obs)
        return fail(c, PCORE_E_STATE, "render_scene: occlude needs an observation");
    if (num_poses < 0 || !d_out_depth || (num_poses > 0 && (!d_poses || !d_pose_model)))
        return fail(c, PCORE_E_INVALID_ARG, "render_scene: null pointer");
    if (d_pose_label && !occlude)
        return fail(c, PCORE_E_INVALID_ARG, "render_scene: pose labels are read only with occlude");
    if (d_pose_label && !c->obs_has_mask)
        return fail(c, PCORE_E_INVALID_ARG, "render_scene: pose labels need a source mask");
    // the key's low word is pose * num_tris + t, and all-ones stays the empty pixel's
    if ((uint64_t)num_poses * (uint64_t)c->num_tris > 0xffffffffull)
        return fail(c, PCORE_E_INVALID_ARG, "render_scene: num_poses * num_tris does not fit the key's 32 bits");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int W = c->cam.width, H = c->cam.height;
    const size_t npx = (size_t)W * H;
    HIPC(c, dev_reserve(c->scene_keys, npx));
    HIPC(c, hipMemsetAsync(c->scene_keys.p, 0xff, npx * sizeof(unsigned long long), s));
    if (d_out_visible && num_poses > 0) HIPC(c, hipMemsetAsync(d_out_visible, 0, (size_t)num_poses * 4, s));
    SceneArgs a{};
    a.tris = c->tris.p;
    a.tri_lo = c->tri_lo.p;
    a.tri_hi = c->tri_hi.p;
    a.num_tris = c->num_tris;
    a.num_models = c->num_models;
    a.poses = d_poses;
    a.pose_model = d_pose_model;
    a.pose_label = d_pose_label;
    a.num_poses = num_poses;
    a.width = W;
    a.height = H;
    a.proj = c->proj.p;
    a.src_depth = occlude ? c->src_depth.p : nullptr;
    a.src_mask = occlude ? c->src_mask.p : nullptr;
    a.occlude = occlude ? 1 : 0;
    a.occlusion_threshold = occlusion_threshold;
    a.keys = c->scene_keys.p;
    HIPC(c, launch_render_scene(a, s));
    HIPC(c, launch_scene_finalize(c->scene_keys.p, c->num_tris, num_poses, W, H, c->tri_rgb.p, d_out_depth, d_out_owner,
                                  d_out_color, d_out_visible, s));
    return PCORE_OK;
}

int pcore_debug_lm_solve(const double* d_sys, const double* d_lambda, double* d_out, int32_t n, pcore_stream stream) {
    if (n < 0 || (n > 0 && (!d_sys || !d_lambda || !d_out))) return PCORE_E_INVALID_ARG;
    return launch_lm_solve_test(d_sys, d_lambda, d_out, n, (hipStream_t)stream) == hipSuccess ? PCORE_OK : PCORE_E_HIP;
}

int pcore_debug_colour_distance(const float* d_lab_pairs, double* d_out, int32_t n, pcore_stream stream) {
    if (n < 0 || (n > 0 && (!d_lab_pairs || !d_out))) return PCORE_E_INVALID_ARG;
    return launch_colour_distance_test(d_lab_pairs, d_out, n, (hipStream_t)stream) == hipSuccess ? PCORE_OK : PCORE_E_HIP;
}

// Test hook: lab_of, the conversion pcore_upload_meshes and pcore_set_observation_colors store (host only).
int pcore_debug_rgb2lab(const uint8_t* rgb, float* out_lab, int32_t n) {
    if (n < 0 || (n > 0 && (!rgb || !out_lab))) return PCORE_E_INVALID_ARG;
    for (int32_t i = 0; i < n; i++) {
        const float4 v = prep::lab_of(rgb + 3 * (size_t)i);
        out_lab[3 * (size_t)i] = v.x;
        out_lab[3 * (size_t)i + 1] = v.y;
        out_lab[3 * (size_t)i + 2] = v.z;
    }
    return PCORE_OK;
}

int pcore_debug_covariances(const float* d_xyzw, const int32_t* d_seg_off, const int32_t* d_seg_cnt, int32_t num_segs,
                            int32_t k, double* d_out_cov6, pcore_stream stream) {
    if (num_segs < 0 || k <= 0 || k > 16 || (num_segs > 0 && (!d_xyzw || !d_seg_off || !d_seg_cnt || !d_out_cov6)))
        return PCORE_E_INVALID_ARG;
    return launch_covariances(reinterpret_cast<const float4*>(d_xyzw), d_seg_off, d_seg_cnt, 0, num_segs, k, d_out_cov6,
                              (hipStream_t)stream, INT_MAX) == hipSuccess ? PCORE_OK : PCORE_E_HIP;
}

int pcore_debug_covariances_cloud(const float* d_xyzw, const int32_t* d_seg_cnt, int32_t seg_stride, int32_t num_segs,
                                  float fx, float fy, float cx, float cy, int32_t stride, double* d_out_cov6,
                                  pcore_stream stream) {
    if (num_segs < 0 || seg_stride < 0 || stride <= 0 || (num_segs > 0 && (!d_xyzw || !d_seg_cnt || !d_out_cov6)))
        return PCORE_E_INVALID_ARG;
    return launch_covariances_cloud(reinterpret_cast<const float4*>(d_xyzw), d_seg_cnt, seg_stride, num_segs, fx, fy, cx,
                                    cy, stride, d_out_cov6, (hipStream_t)stream) == hipSuccess ? PCORE_OK : PCORE_E_HIP;
}

int pcore_depth_to_cloud(pcore_ctx* c, const int32_t* d_depth, int32_t num_poses, int32_t width, int32_t height,
                         int32_t stride, float depth_factor, const uint8_t* d_label_mask, const int32_t* d_pose_label,
                         float* d_out_xyz, int32_t* d_out_pose, int32_t* d_out_label, int32_t cap, int32_t* out_count,
                         pcore_stream stream) {
    return pcore_depth_to_cloud_ex(c, d_depth, num_poses, width, height, stride, depth_factor, d_label_mask,
                                   d_pose_label, nullptr, d_out_xyz, d_out_pose, d_out_label, nullptr, nullptr, cap,
                                   out_count, stream);
}

int pcore_depth_to_cloud_ex(pcore_ctx* c, const int32_t* d_depth, int32_t num_poses, int32_t width, int32_t height,
                            int32_t stride, float depth_factor, const uint8_t* d_label_mask, const int32_t* d_pose_label,
                            const uint8_t* d_color_planes, float* d_out_xyz, int32_t* d_out_pose, int32_t* d_out_label,
                            uint8_t* d_out_color, int32_t* d_out_dc_index, int32_t cap, int32_t* out_count,
                            pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (!c->have_cam) return fail(c, PCORE_E_STATE, "depth_to_cloud: camera not set");
    if (num_poses < 0 || width <= 0 || height <= 0 || stride <= 0 || !d_depth || cap < 0 ||
        (cap > 0 && !d_out_xyz) || !out_count || (d_out_color && !d_color_planes))
        return fail(c, PCORE_E_INVALID_ARG, "depth_to_cloud: bad arguments");
    if (width % stride != 0) return fail(c, PCORE_E_INVALID_ARG, "depth_to_cloud: width % stride != 0");
    if (d_label_mask && num_poses != 1)
        return fail(c, PCORE_E_INVALID_ARG, "depth_to_cloud: label mask needs num_poses == 1");
    *out_count = 0;
    if (num_poses == 0) return PCORE_OK;
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    HIPC(c, dev_reserve(c->scratch_counts, num_poses));
    HIPC(c, dev_reserve(c->scratch_offsets, num_poses));
    HIPC(c, dev_reserve(c->scratch_total, 1));
    const CloudBounds no_bounds{};
    HIPC(c, launch_cloud_count(d_depth, num_poses, width, height, stride, d_label_mask, no_bounds,
                               c->scratch_counts.p, s));
    HIPC(c, launch_exclusive_scan(c->scratch_counts.p, c->scratch_offsets.p, num_poses, c->scratch_total.p, s));
    HIPC(c, launch_cloud_write(d_depth, num_poses, width, height, stride, c->cam.cx, c->cam.cy, c->cam.fx, c->cam.fy,
                               depth_factor, d_label_mask, d_pose_label, c->scratch_offsets.p, d_out_xyz, d_out_pose,
                               d_out_label, cap, no_bounds, nullptr, nullptr, s, d_out_color ? d_color_planes : nullptr,
                               d_out_color));
    if (d_out_dc_index) {
        const size_t samples = (size_t)((width + stride - 1) / stride) * ((height + stride - 1) / stride);
        HIPC(c, dev_reserve(c->scratch_dc_pre, (size_t)num_poses * (samples + 1)));
        HIPC(c, launch_cloud_dc_index(d_depth, num_poses, width, height, stride, d_label_mask, c->scratch_offsets.p,
                                      c->scratch_dc_pre.p, d_out_dc_index, s));
    }
    int32_t total = 0;
    HIPC(c, hipMemcpyAsync(&total, c->scratch_total.p, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    *out_count = total;
    return PCORE_OK;
}

int pcore_select(pcore_ctx* c, const float* d_rc, const float* d_oc, const int32_t* d_pose_model, int32_t num_poses,
                 int64_t index_base, int32_t num_models, int64_t* d_keys, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (num_poses < 0 || num_models <= 0 || index_base < 0 || index_base + num_poses > 0x7fffffffLL ||
        (num_poses > 0 && (!d_rc || !d_oc || !d_pose_model || !d_keys)))
        return fail(c, PCORE_E_INVALID_ARG, "select: bad arguments");
    if (num_poses == 0) return PCORE_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, launch_select(d_rc, d_oc, d_pose_model, num_poses, index_base, num_models, d_keys, (hipStream_t)stream));
    return PCORE_OK;
}

int pcore_select_topk(pcore_ctx* c, const float* d_rc, const float* d_oc, const int32_t* d_pose_model, int32_t num_poses,
                      int64_t index_base, int32_t num_models, int32_t k, int64_t* d_topk, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    // pcore_select's checks; the last global index may be 2^31 - 1, all that the key's 31 index bits hold
    if (num_poses < 0 || num_models <= 0 || index_base < 0 || index_base + num_poses > 0x80000000LL ||
        (num_poses > 0 && (!d_rc || !d_oc || !d_pose_model || !d_topk)))
        return fail(c, PCORE_E_INVALID_ARG, "select_topk: bad arguments");
    if (k < 1 || k > PCORE_TOPK_MAX) return fail(c, PCORE_E_INVALID_ARG, "select_topk: k must lie in [1, PCORE_TOPK_MAX]");
    if (num_poses == 0) return PCORE_OK;
    hipStream_t s = (hipStream_t)stream;
    HIPC(c, hipSetDevice(c->device));
    const size_t need = (size_t)topk_slices(num_poses) * (size_t)num_models * (size_t)k;
    if (int rc = refuse_setup_in_capture(c, "select_topk", "the partial lists", c->topk_part.n < need || !c->topk_part.p, s))
        return rc;
    HIPC(c, reserve_gen(c, c->topk_part, need));
    HIPC(c, launch_select_topk(d_rc, d_oc, d_pose_model, num_poses, index_base, num_models, k, c->topk_part.p, d_topk, s));
    return PCORE_OK;
}

int pcore_count_within(pcore_ctx* c, const float* d_queries, const int32_t* d_labels, const float* d_radius_sq,
                       int32_t n, int32_t* d_out_counts, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (n < 0 || (n > 0 && (!d_queries || !d_labels || !d_radius_sq || !d_out_counts)))
        return fail(c, PCORE_E_INVALID_ARG, "count_within: null pointer");
    if (!c->have_obs) return fail(c, PCORE_E_STATE, "count_within: the observation must be set first");
    if (n == 0) return PCORE_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, launch_count_within(d_queries, d_labels, d_radius_sq, n, c->tgt.p, c->seg_lo.p, c->seg_hi.p,
                                c->num_obs > 0 ? c->num_grids : 0, d_out_counts, (hipStream_t)stream));
    return PCORE_OK;
}

int pcore_state_poses(pcore_ctx* c, const double* d_states, const int32_t* d_model, const double* cam_from_world,
                      const double* d_preprocess, int32_t num_models, int32_t n, float* d_out_poses,
                      pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (n < 0 || !cam_from_world || num_models <= 0 ||
        (n > 0 && (!d_states || !d_model || !d_preprocess || !d_out_poses)))
        return fail(c, PCORE_E_INVALID_ARG, "state_poses: bad arguments");
    if (n == 0) return PCORE_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, launch_state_poses(d_states, d_model, d_preprocess, cam_from_world, num_models, n, d_out_poses,
                               (hipStream_t)stream));
    return PCORE_OK;
}

int pcore_pose_distances(pcore_ctx* c, const float* d_pts, int32_t n, const double* d_T_gt, const double* d_T_est,
                         int32_t num_pairs, double* d_add, double* d_adds, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (n <= 0 || num_pairs < 0 || (num_pairs > 0 && (!d_pts || !d_T_gt || !d_T_est)))
        return fail(c, PCORE_E_INVALID_ARG, "pose_distances: need n > 0 points and pose pointers");
    if (num_pairs == 0 || (!d_add && !d_adds)) return PCORE_OK;
    if (num_pairs > 65535) return fail(c, PCORE_E_INVALID_ARG, "pose_distances: at most 65535 pairs per call");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, dev_reserve(c->metric_part, (size_t)2 * num_pairs * pose_dist_blocks(n)));
    HIPC(c, launch_pose_distances(d_pts, n, d_T_gt, d_T_est, num_pairs, c->metric_part.p, d_add, d_adds,
                                  (hipStream_t)stream));
    return PCORE_OK;
}

}  // extern "C"
