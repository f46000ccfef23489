// pcore_ctx.h -- the context behind include/pcore.h and what the host sources share (pcore_api.hip: lifetime, setup,
// clouds, render, select; pcore_api_eval.hip: the fused launch and pcore_evaluate_icp; pcore_api_icp.hip: the staged
// ICPs).  Private to them.  Every device and host allocation has an owner that frees it: `delete ctx` is the teardown.
#pragma once
#include "../../include/pcore.h"
#include "pcore_internal.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace pcore {

// Owners: device memory, host memory from hipHostMalloc, events.  Their destructors ignore HIP errors (nothing could
// be done about one) and run with the context's device current.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};
template <typename T>
struct DevBuf : NoCopy {
    T* p = nullptr;
    size_t n = 0;  // elements; 0 while p is null
    ~DevBuf() { if (p) (void)hipFree(p); }
};
template <typename T>
struct HostBuf : NoCopy {
    T* p = nullptr;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
};
struct Events : NoCopy {
    std::vector<hipEvent_t> v;
    ~Events() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
};

}  // namespace pcore

struct pcore_ctx {
    template <typename T> using DevBuf = pcore::DevBuf<T>;
    int device = 0;
    std::string err;
    hipDeviceProp_t prop{};
    pcore::DeviceInfo dinfo{};  // per-device launch constants, filled once in pcore_create
    uint64_t generation = 1;    // pcore_generation: bumped whenever captured state may change
    // mesh
    int num_models = 0;
    int num_tris = 0;
    DevBuf<float> tris;          // original triangle soup (parity render)
    DevBuf<int32_t> tri_lo, tri_hi;
    DevBuf<float4> sverts;       // vertex-ring streams (pcore_internal.h, kVRing)
    DevBuf<uint32_t> stris;
    DevBuf<int4> streams;
    DevBuf<int32_t> model_st_lo, model_st_hi;
    DevBuf<float4> model_box;  // FusedArgs::model_box
    DevBuf<uint32_t> tri_rgb;  // per original triangle: r | g << 8 | b << 16 (stage RENDER colour planes)
    bool have_mesh = false;
    // camera
    pcore_camera cam{};
    DevBuf<float> proj;
    bool have_cam = false;
    // observation
    DevBuf<int32_t> src_depth;
    DevBuf<uint8_t> src_mask;
    bool obs_has_mask = false;
    int sampled_stride = 0;
    DevBuf<int32_t> src_s;
    DevBuf<uint8_t> lab_s;
    DevBuf<pcore::LabelGrid> grids;
    DevBuf<int32_t> cell_start;
    DevBuf<float4> grid_pts;
    int num_grids = 0;
    int bitmap_words = 1;
    bool have_obs = false;
    // GICP targets: label-sorted observed points, segments [lo, hi) per label + the whole cloud
    int num_obs = 0;
    int max_seg = 0;
    DevBuf<float4> tgt;
    DevBuf<int32_t> seg_lo, seg_hi, seg_cnt;
    std::vector<int32_t> seg_lo_h, seg_cnt_h;  // host copies (grid covariance launches)
    DevBuf<float> tgt_quads;                   // GicpArgs::tgt_quads
    DevBuf<int32_t> seg_qoff;
    DevBuf<double> tgt_cov_label, tgt_cov_all;
    int cov_k_label = 0, cov_k_all = 0;
    // GICP scratch
    DevBuf<float4> icp_cloud;
    DevBuf<int32_t> icp_count;
    DevBuf<double> icp_cov;
    DevBuf<int32_t> icp_corr;   // GicpArgs::corr
    DevBuf<int32_t> scratch_dc_pre;  // stage CLOUD result_dc_index: per-pose sample prefixes
    DevBuf<int32_t> icp_corr_hist;  // GicpArgs::corr_hist
    DevBuf<double> icp_mahal;   // GicpArgs::mahal
    DevBuf<int32_t> icp_counter;                // GicpArgs::work_counter
    DevBuf<unsigned long long> icp_iter_stats;  // GicpArgs::iter_stats ([0..3]), zeroed per call
    // their copy in pinned host memory, made on the call's stream before each chunk's end event (pcore_get_stats reads
    // it after that event: no synchronous copy, which would wait for every blocking stream of the device)
    pcore::HostBuf<unsigned long long> icp_iter_stats_host;
    DevBuf<uint32_t> icp_order_keys;  // 2 x chunk keys (in, out)
    DevBuf<int32_t> icp_order_idx;    // 2 x chunk indices (in, out = GicpArgs::pose_order)
    DevBuf<unsigned char> icp_order_temp;
    // colour gate (cost_type 1)
    DevBuf<uint32_t> stri_orig;   // original triangle of every stream triangle slot
    DevBuf<float4> tri_lab;       // Lab per original triangle
    DevBuf<float4> obs_lab;       // Lab per observed point, label-sorted
    DevBuf<int32_t> colour_id;    // N x nsamp scratch of the fused kernel's colour id pass
    DevBuf<int32_t> fb_ctr;       // FusedArgs::fb_ctr
    DevBuf<int32_t> win_hist;     // FusedArgs::win_hist
    DevBuf<int32_t> fb_ctr_cap;   // the same for captured launches: counted into, never published or read
    DevBuf<int32_t> win_hist_cap;
    pcore::HostBuf<int32_t> fb_host;  // mapped host memory (FusedArgs::fb_host), host view
    int32_t* fb_dev = nullptr;    // the same, device view
    int32_t fb_seq = 0;           // sequence number of the last fused launch
    int32_t tile_key_seq = 0;     // first sequence number launched with the current tile configuration
    long long tile_key = -1;      // ws, hs, bitmap words, colour of the current tile configuration
    int tile_tier = pcore::kDefaultTier;
    int32_t tile_tcap = 0;        // tile (samples) of the last window launch
    bool tile_probed = false;     // the window probe has chosen a tier for the current tile key
    DevBuf<int32_t> win_probe;    // its histogram
    int32_t tile_edge[pcore::kTileTiers] = {};
    std::vector<int> obs_order;   // label-sorted position -> caller's observed index
    bool have_obs_colours = false;
    DevBuf<double> metric_part;  // ADD / ADD-S per-block partial sums
    // scratch (parity stages)
    DevBuf<int32_t> scratch_counts, scratch_offsets, scratch_total;
    DevBuf<int32_t> render_tri;  // stage RENDER colour: nearest triangle per pixel
    DevBuf<unsigned long long> scene_keys;  // pcore_render_scene: one (depth, pose, triangle) key per pixel
    // gpu_stats of the last pcore_evaluate_icp (pcore_get_stats): per chunk, events at the source covariances,
    // the GICP launch and its end on the call's stream; the peak device memory in use at a GICP stage
    pcore::Events icp_ev;
    int icp_ev_used = 0;
    double peak_mem_mb = 0.0;
    // planar ICP (pcore_icp_planar): the observation as set (host copy, caller's order), its world-frame copy and
    // neighbour grid, built on first use and kept while (observation, matrix bytes, radius) stay the same
    std::vector<float> obs_xyz_h;
    uint64_t obs_serial = 0;          // counts pcore_set_observation calls
    uint64_t planar_obs_serial = 0;   // the observation the grid below was built from (0: none)
    float planar_m[16] = {};
    float planar_radius = 0.0f;
    pcore::LabelGrid planar_grid{};
    DevBuf<int32_t> planar_cell_start;
    DevBuf<float4> planar_pts;
    // point-to-plane ICP (pcore_icp_point2plane): the projective scene of src_depth (a float4 point and a float4 normal
    // per pixel), built on first use and kept while the observation and the camera stay the same
    uint64_t p2p_obs_serial = 0;      // the observation the scene below was built from (0: none)
    pcore_camera p2p_cam{};
    DevBuf<float4> p2p_pcd, p2p_normal;
    DevBuf<int64_t> topk_part;  // pcore_select_topk: one partial list per (slice, model)
    DevBuf<uint32_t> state_bitmap;  // pcore_evaluate_states: explained bitmaps of clouds above PCORE_STATE_LDS_OBS
};

namespace pcore {

inline int fail(pcore_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPC(ctx, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, e_ == hipErrorOutOfMemory ? PCORE_E_OOM : PCORE_E_HIP,             \
                        std::string(#call) + ": " + hipGetErrorString(e_));                     \
    } while (0)

template <typename T>
hipError_t dev_free(DevBuf<T>& b) {
    hipError_t e = hipSuccess;
    if (b.p) e = hipFree(b.p);
    b.p = nullptr;
    b.n = 0;
    return e;
}

template <typename T>
hipError_t dev_reserve(DevBuf<T>& b, size_t n) {
    if (b.n >= n && b.p) return hipSuccess;
    hipError_t e = dev_free(b);
    if (e != hipSuccess) return e;
    e = hipMalloc(&b.p, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) b.n = n;
    return e;
}

// dev_reserve for scratch a captured graph points into: a reallocation invalidates such graphs
template <typename T>
hipError_t reserve_gen(pcore_ctx* c, DevBuf<T>& b, size_t n) {
    if (b.n >= n && b.p) return hipSuccess;
    c->generation++;
    return dev_reserve(b, n);
}

template <typename T>
hipError_t dev_upload(DevBuf<T>& b, const void* src, size_t n) {  // n elements of T, of any type with T's layout
    hipError_t e = dev_reserve(b, n);
    if (e == hipSuccess && n) e = hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
}
template <typename T>
hipError_t dev_upload(DevBuf<T>& b, const std::vector<T>& v) { return dev_upload(b, v.data(), v.size()); }

// A stream whose capture state cannot be queried (hipStreamIsCapturing fails, e.g. on the legacy stream while another
// stream captures in global mode) counts as capturing.
inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return cap != hipStreamCaptureStatusNone;
}

// `what` (or the scratch) has to be built or allocated first: none of it may happen while the stream captures
inline int refuse_setup_in_capture(pcore_ctx* c, const char* who, const char* what, bool setup, hipStream_t s) {
    if (setup && stream_capturing(s))
        return fail(c, PCORE_E_STATE, std::string(who) + ": " + what + " or the scratch would have to be built while the "
                                      "stream captures; run the call once before the capture");
    return PCORE_OK;
}

// The checks of a call that rasters the image sampled at `stride`, `who` prefixing the messages: the stride divides the
// width, the sampled image (ws x hs = nsamp samples, returned) fits the kernels' 12-bit sample coordinates and, whole, a
// workgroup's LDS (the overflow launch; `colour`: with the colour gate's tile).  `lds_hint` ends the LDS message; `need`
// appends the bytes it would take.
inline int check_sampling(pcore_ctx* c, const std::string& who, int stride, bool colour, const char* lds_hint, bool need,
                          int& nsamp) {
    const int W = c->cam.width, H = c->cam.height;
    if (stride <= 0 || W % stride != 0) return fail(c, PCORE_E_INVALID_ARG, who + ": width must be a multiple of stride");
    const int ws = W / stride, hs = (H + stride - 1) / stride;
    if (ws > 4095 || hs > 4095) return fail(c, PCORE_E_INVALID_ARG, who + ": sampled image too large");
    nsamp = ws * hs;
    const size_t lds = fused_lds_bytes(nsamp, c->bitmap_words, colour);
    if (lds > (size_t)c->prop.sharedMemPerBlock)
        return fail(c, PCORE_E_INVALID_ARG, who + ": sampled z-buffer does not fit in LDS" + lds_hint +
                                                (need ? "; need " + std::to_string(lds) + " B" : std::string()));
    return PCORE_OK;
}

// Poses per chunk of a batch whose poses each take `per_pose` bytes of scratch: equal chunks, as few as the budget allows
// (every chunk ends with the tail of its slowest pose): min(32 GiB, max(1 GiB, 40 % of the free device memory)), or what
// the caller's environment knob sets (test / A/B; at least 1, in units of 2^knob_shift bytes).
inline int plan_chunks(int num_poses, size_t per_pose, const char* knob, int knob_shift) {
    size_t budget = (size_t)32 << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
        budget = std::min(budget, std::max<size_t>((size_t)1 << 30, free_b / 5 * 2));
    if (const char* e = getenv(knob)) budget = (size_t)std::max(1LL, atoll(e)) << knob_shift;
    const int max_chunk = (int)std::min<size_t>(std::max<size_t>(1, budget / per_pose), 0x7fffffff);
    const int nchunks = (num_poses + max_chunk - 1) / max_chunk;
    return (num_poses + nchunks - 1) / nchunks;
}

// the source depth and mask sampled at `stride` (the callers' checks guarantee width % stride == 0)
inline int ensure_sampled(pcore_ctx* c, int stride, hipStream_t s) {
    if (c->sampled_stride == stride) return PCORE_OK;
    c->generation++;  // a captured graph would read a source sampled at another stride
    const int ws = c->cam.width / stride, hs = (c->cam.height + stride - 1) / stride;
    HIPC(c, dev_reserve(c->src_s, (size_t)ws * hs));
    HIPC(c, dev_reserve(c->lab_s, (size_t)ws * hs));
    HIPC(c, launch_sample_source(c->src_depth.p, c->src_mask.p, c->cam.width, c->cam.height, stride, c->src_s.p,
                                 c->lab_s.p, s));
    c->sampled_stride = stride;
    return PCORE_OK;
}

// a launch's FusedArgs but for its batch and outputs: the mesh, the camera, the sampled observation, the cost settings
inline void fill_fused_args(pcore_ctx* c, const pcore_eval_params* p, FusedArgs& a) {
    a = FusedArgs{};
    a.sverts = c->sverts.p;
    a.stris = c->stris.p;
    a.streams = c->streams.p;
    a.model_st_lo = c->model_st_lo.p;
    a.model_st_hi = c->model_st_hi.p;
    a.model_box = c->model_box.p;
    a.num_models = c->num_models;
    const float* pj = c->cam.proj;
    a.p00 = pj[0]; a.p01 = pj[1]; a.p02 = pj[2]; a.p03 = pj[3];
    a.p10 = pj[4]; a.p11 = pj[5]; a.p12 = pj[6]; a.p13 = pj[7];
    a.proj_sparse = (pj[1] == 0.0f && pj[3] == 0.0f && pj[4] == 0.0f && pj[7] == 0.0f) ? 1 : 0;
    a.width = c->cam.width;
    a.height = c->cam.height;
    a.stride = p->stride;
    a.ws = a.width / a.stride;
    a.hs = (a.height + a.stride - 1) / a.stride;
    a.cx = c->cam.cx; a.cy = c->cam.cy; a.fx = c->cam.fx; a.fy = c->cam.fy;
    a.depth_factor = p->depth_factor;
    a.src_s = c->src_s.p;
    a.lab_s = c->lab_s.p;
    a.grids = c->grids.p;
    a.cell_start = c->cell_start.p;
    a.grid_pts = c->grid_pts.p;
    a.num_grids = c->num_grids;
    a.bitmap_words = c->bitmap_words;
    a.r2 = p->sensor_resolution * p->sensor_resolution;  // renderer.cu:1877
    a.occlusion_threshold = p->occlusion_threshold;
    a.calc_obs = p->calc_obs_cost;
}

// A call that stages the clouds of its poses (stage CLOUD, render_cloud_kernel) into per-pose slots of the whole
// sampled image, chunk by chunk, and launches its own kernel over each chunk (pcore_api_icp.hip)
struct Staged {
    const char* who;
    const pcore_eval_params* p;
    const float* poses;
    const int32_t *pose_model, *pose_label;  // pose_label nullable
    int num_poses;
    hipStream_t s;
    float4* cloud = nullptr;   // the slots and their counts
    int32_t* count = nullptr;
    int nsamp = 0, chunk = 0;  // samples per slot (the checks set it); poses per chunk (plan_chunks)
    FusedArgs a{};
};
// the sampled source, the context's icp_cloud / icp_count grown to st.chunk slots (st.cloud, st.count), st.a
int staged_slots(pcore_ctx* c, Staged& st);
// stage CLOUD of the n poses from `base` into st.cloud
hipError_t stage_chunk(pcore_ctx* c, Staged& st, int base, int n);
// fn(base, n): the caller's launches over each staged chunk of n poses from `base`; PCORE_OK to go on
template <typename Fn>
int for_each_chunk(pcore_ctx* c, Staged& st, Fn&& fn) {
    for (int base = 0; base < st.num_poses; base += st.chunk) {
        const int n = std::min(st.chunk, st.num_poses - base);
        HIPC(c, stage_chunk(c, st, base, n));
        if (const int rc = fn(base, n)) return rc;
    }
    return PCORE_OK;
}

}  // namespace pcore
