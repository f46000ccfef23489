// pcore_api_eval.hip -- the per-batch path: pcore_evaluate / pcore_evaluate_select (the fused launch and its tile
// policy), pcore_evaluate_icp (GICP over staged clouds, then the re-score) and what reports on them (pcore_get_stats,
// pcore_get_tile_info).  No hidden allocations on evaluate / select once a batch size has been seen.
#include "pcore_ctx.h"

#include <cstring>

using namespace pcore;

namespace {

// the tier with the most workgroups per CU whose tile holds the windows of >= 99 % of the histogram's poses
int choose_tier(const int32_t* h, const int* edge, int fallback) {
    long long tot = 0;
    for (int b = 0; b <= kTileTiers; b++) tot += h[b];
    if (tot <= 0) return fallback;
    long long over = tot;  // windows above edge[t]
    for (int t = 0; t < kTileTiers; t++) {
        over -= h[t];
        if (edge[t] > 0 && over * 100 <= tot) return t;
    }
    return kTileTiers - 1;
}

// Tile of the fused window launch ("Pose windows"): choose_tier over the window histogram of the
// last launch that has published one with the same sampled image.  Until one has (the first call with a new
// image, or every call of a host that runs ahead of the GPU), the tier comes from a window probe of the
// first such batch: one small launch and a wait, once per sampled image.  Only the speed depends on the choice,
// never the results.
hipError_t set_fused_tiles(pcore_ctx* c, int num_poses, FusedArgs& a, hipStream_t s) {
    const bool colour = a.cid != nullptr;
    const int nsamp = a.ws * a.hs;
    hipError_t e;
    if (!c->fb_host.p) {
        if ((e = hipHostMalloc((void**)&c->fb_host.p, 16 * sizeof(int32_t), hipHostMallocMapped)) != hipSuccess) return e;
        std::memset(c->fb_host.p, 0, 16 * sizeof(int32_t));
        c->fb_host.p[kTileTiers + 2] = -1;
        if ((e = hipHostGetDevicePointer((void**)&c->fb_dev, c->fb_host.p, 0)) != hipSuccess) return e;
        if ((e = dev_reserve(c->fb_ctr, 2)) != hipSuccess) return e;
        if ((e = dev_reserve(c->win_hist, 2 * (kTileTiers + 1))) != hipSuccess) return e;
        // captured launches' own counters, allocated here: no allocation may happen while a stream captures
        if ((e = dev_reserve(c->fb_ctr_cap, 2)) != hipSuccess) return e;
        if ((e = dev_reserve(c->win_hist_cap, 2 * (kTileTiers + 1))) != hipSuccess) return e;
        if ((e = hipMemset(c->fb_ctr.p, 0, 2 * sizeof(int32_t))) != hipSuccess) return e;
        if ((e = hipMemset(c->win_hist.p, 0, 2 * (kTileTiers + 1) * sizeof(int32_t))) != hipSuccess) return e;
    }
    // A captured launch counts into buffers of its own that nothing publishes or reads: its replays can
    // never add to the parity histograms the eager launches publish: no window probe, no feedback.
    const bool capturing = stream_capturing(s);
    int edge[kTileTiers];
    for (int t = 0; t < kTileTiers; t++) edge[t] = fused_tier_samples(t, a.ws, a.hs, a.bitmap_words, colour, c->dinfo);
    const long long key = (((long long)a.ws * 4096 + a.hs) * 65536 + a.bitmap_words) * 2 + (colour ? 1 : 0);
    bool published = false;
    if (key != c->tile_key) {
        c->tile_key = key;
        c->tile_key_seq = c->fb_seq + 1;
        c->tile_tier = kDefaultTier;
        c->tile_probed = false;
    } else {
        volatile int32_t* fb = c->fb_host.p;
        const int32_t seq = fb[kTileTiers + 2];
        if (seq >= c->tile_key_seq && seq <= c->fb_seq) {
            int32_t h[kTileTiers + 1];
            for (int b = 0; b <= kTileTiers; b++) h[b] = fb[b];
            c->tile_tier = choose_tier(h, edge, c->tile_tier);
            published = true;
        }
    }
    const char* env_tier = getenv("PCORE_FUSED_TIER");  // A/B + test knob; >= kTileTiers: whole image
    if (!published && !c->tile_probed && !capturing && !env_tier && !getenv("PCORE_NO_WINDOW_PROBE")) {
        if ((e = dev_reserve(c->win_probe, kTileTiers + 1)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c->win_probe.p, 0, (kTileTiers + 1) * sizeof(int32_t), s)) != hipSuccess) return e;
        for (int t = 0; t < kTileTiers; t++) a.hist_edge[t] = edge[t];
        if ((e = launch_window_probe(a, c->win_probe.p, s)) != hipSuccess) return e;
        int32_t h[kTileTiers + 1];
        if ((e = hipMemcpyAsync(h, c->win_probe.p, sizeof(h), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        c->tile_tier = choose_tier(h, edge, c->tile_tier);
        c->tile_probed = true;
    }
    if (env_tier) c->tile_tier = std::min(std::max(atoi(env_tier), 0), kTileTiers);
    // tier kTileTiers (A/B knob only): the whole image
    a.tcap = c->tile_tier < kTileTiers && edge[c->tile_tier] > 0 ? edge[c->tile_tier] : nsamp;
    if (const char* env = getenv("PCORE_FUSED_TCAP"))  // test knob: a tile of this many samples (most poses overflow)
        a.tcap = std::min(std::max(atoi(env), 1), nsamp);
    for (int t = 0; t < kTileTiers; t++) a.hist_edge[t] = c->tile_edge[t] = edge[t];
    c->tile_tcap = a.tcap;
    a.fb_ctr = capturing ? c->fb_ctr_cap.p : c->fb_ctr.p;
    a.win_hist = capturing ? c->win_hist_cap.p : c->win_hist.p;
    a.fb_host = capturing ? nullptr : c->fb_dev;
    a.fb_seq = ++c->fb_seq;
    a.fb_par = a.fb_seq & 1;
    return hipSuccess;
}

// Every check pcore_evaluate makes before it launches anything.  pcore_evaluate_icp runs the same checks up
// front, so an invalid call fails before it writes any output.
int validate_eval(pcore_ctx* c, const char* who, const float* d_poses, const int32_t* d_pose_model,
                  const int32_t* d_pose_label, const float* d_pose_obs_total, int32_t num_poses,
                  const pcore_eval_params* p, const float* d_out_rc, const float* d_out_oc, const float* d_out_diff,
                  int& nsamp) {
    const std::string w(who);
    if (!c->have_mesh || !c->have_cam || !c->have_obs)
        return fail(c, PCORE_E_STATE, w + ": meshes, camera and observation must be set first");
    if (num_poses < 0 || (num_poses > 0 && (!d_poses || !d_pose_model || !d_out_rc)))
        return fail(c, PCORE_E_INVALID_ARG, w + ": null pose / output pointer");
    if (p->cost_type != PCORE_COST_DEPTH_3DOF && p->cost_type != PCORE_COST_DEPTH_6DOF &&
        p->cost_type != PCORE_COST_RGBD_3DOF)
        return fail(c, PCORE_E_INVALID_ARG, w + ": unknown cost_type");
    if (p->cost_type == PCORE_COST_RGBD_3DOF && (d_pose_label || !c->have_obs_colours))
        return fail(c, PCORE_E_INVALID_ARG,
                    w + ": cost_type 1 is 3-DoF (no pose labels) and needs pcore_set_observation_colors");
    if (num_poses == 0) return PCORE_OK;
    if (p->cost_type == PCORE_COST_DEPTH_6DOF && (!d_pose_label || !c->obs_has_mask))
        return fail(c, PCORE_E_INVALID_ARG, w + ": cost_type 2 needs pose labels and a source mask");
    if (p->calc_obs_cost && (!d_pose_obs_total || !d_out_oc || !d_out_diff))
        return fail(c, PCORE_E_INVALID_ARG, w + ": calc_obs_cost needs pose_obs_total and oc/diff outputs");
    // the overflow launch holds the whole sampled image in LDS (the GICP cloud launch needs less: no bitmap)
    return check_sampling(c, w, p->stride, p->cost_type == PCORE_COST_RGBD_3DOF, " (use a larger stride)", true, nsamp);
}

int evaluate_impl(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                  const float* d_pose_obs_total, int32_t num_poses, const pcore_eval_params* p, float* d_out_rc,
                  float* d_out_oc, float* d_out_diff, int32_t* d_dbg_zs, int64_t* d_keys, int64_t index_base,
                  int32_t num_models, pcore_stream stream) {
    if (!c || !p) return PCORE_E_INVALID_ARG;
    int nsamp = 0;
    const int vr = validate_eval(c, "evaluate", d_poses, d_pose_model, d_pose_label, d_pose_obs_total, num_poses, p,
                                 d_out_rc, d_out_oc, d_out_diff, nsamp);
    if (vr != PCORE_OK || num_poses == 0) return vr;
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = ensure_sampled(c, p->stride, s)) return rc;

    FusedArgs a{};
    fill_fused_args(c, p, a);
    a.poses = d_poses;
    a.pose_model = d_pose_model;
    a.pose_label = (p->cost_type == PCORE_COST_DEPTH_6DOF) ? d_pose_label : nullptr;
    a.pose_obs_total = d_pose_obs_total;
    a.num_poses = num_poses;
    a.out_rc = d_out_rc;
    a.out_oc = d_out_oc;
    a.out_diff = d_out_diff;
    a.dbg_zs = d_dbg_zs;
    if (p->cost_type == PCORE_COST_RGBD_3DOF) {
        a.stri_orig = c->stri_orig.p;
        a.tri_lab = c->tri_lab.p;
        a.obs_lab = c->obs_lab.p;
        a.colour_thr = p->color_distance_threshold;
        HIPC(c, reserve_gen(c, c->colour_id, (size_t)num_poses * nsamp));
        a.cid = c->colour_id.p;
    }
    if (const char* e = getenv("PCORE_DEBUG_SKIP")) a.dbg_skip = atoi(e);
    a.sel_keys = d_keys;
    a.sel_base = index_base;
    a.sel_models = num_models;
    HIPC(c, set_fused_tiles(c, num_poses, a, s));
    HIPC(c, launch_fused_cost(a, s));
    return PCORE_OK;
}

}  // namespace

extern "C" {

int pcore_evaluate(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                   const float* d_pose_obs_total, int32_t num_poses, const pcore_eval_params* p, float* d_out_rc,
                   float* d_out_oc, float* d_out_diff, int32_t* d_dbg_zs, pcore_stream stream) {
    return evaluate_impl(c, d_poses, d_pose_model, d_pose_label, d_pose_obs_total, num_poses, p, d_out_rc, d_out_oc,
                         d_out_diff, d_dbg_zs, nullptr, 0, 0, stream);
}

int pcore_evaluate_select(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model,
                          const int32_t* d_pose_label, const float* d_pose_obs_total, int32_t num_poses,
                          const pcore_eval_params* p, float* d_out_rc, float* d_out_oc, float* d_out_diff,
                          int64_t index_base, int32_t num_models, int64_t* d_keys, pcore_stream stream) {
    if (!c) return PCORE_E_INVALID_ARG;
    if (num_models <= 0 || index_base < 0 || index_base + num_poses > 0x7fffffffLL || (num_poses > 0 && !d_keys))
        return fail(c, PCORE_E_INVALID_ARG, "evaluate_select: bad selection arguments");
    return evaluate_impl(c, d_poses, d_pose_model, d_pose_label, d_pose_obs_total, num_poses, p, d_out_rc, d_out_oc,
                         d_out_diff, nullptr, d_keys, index_base, num_models, stream);
}

int pcore_evaluate_icp(pcore_ctx* c, const float* d_poses, const int32_t* d_pose_model, const int32_t* d_pose_label,
                       const float* d_pose_obs_total, int32_t num_poses, const pcore_eval_params* p,
                       const pcore_icp_params* ip, float* d_out_poses, int32_t* d_out_iters, float* d_out_rc,
                       float* d_out_oc, float* d_out_diff, pcore_stream stream) {
    if (!c || !p || !ip) return PCORE_E_INVALID_ARG;
    if (ip->k_correspondences <= 0 || ip->k_correspondences > 16 || ip->max_iterations < 0)
        return fail(c, PCORE_E_INVALID_ARG, "evaluate_icp: k_correspondences must be in [1, 16]");
    if (ip->cycle_exit_window < 0)
        return fail(c, PCORE_E_INVALID_ARG, "evaluate_icp: cycle_exit_window must be >= 0");
    if (num_poses > 0 && !d_out_poses) return fail(c, PCORE_E_INVALID_ARG, "evaluate_icp: null d_out_poses");
    if (p->cost_type != PCORE_COST_DEPTH_3DOF && p->cost_type != PCORE_COST_DEPTH_6DOF)
        return fail(c, PCORE_E_INVALID_ARG, "evaluate_icp: cost_type must be 0 or 2");
    // everything the final pcore_evaluate (the re-score) checks, before any chunk writes an output
    const bool six = p->cost_type == PCORE_COST_DEPTH_6DOF;
    hipStream_t s = (hipStream_t)stream;
    Staged st{"evaluate_icp", p, d_poses, d_pose_model, six ? d_pose_label : nullptr, num_poses, s};
    const int vr = validate_eval(c, st.who, d_poses, d_pose_model, d_pose_label, d_pose_obs_total, num_poses, p,
                                 d_out_rc, d_out_oc, d_out_diff, st.nsamp);
    if (vr != PCORE_OK || num_poses == 0) return vr;
    HIPC(c, hipSetDevice(c->device));
    if (const int rc = ensure_sampled(c, p->stride, s)) return rc;
    const int nsamp = st.nsamp, k = ip->k_correspondences;
    // target covariances, once per (observation, k): of the nl label segments (6-DoF) or of the whole cloud, segment nl
    const int nl = c->num_grids;
    DevBuf<double>& tcov = six ? c->tgt_cov_label : c->tgt_cov_all;
    int& tcov_k = six ? c->cov_k_label : c->cov_k_all;
    if (tcov_k != k) {
        const int seg0 = six ? 0 : nl, nseg = six ? nl : 1;
        HIPC(c, dev_reserve(tcov, (size_t)6 * std::max(c->num_obs, 1)));
        HIPC(c, launch_covariances(c->tgt.p, c->seg_lo.p + seg0, c->seg_cnt.p + seg0, 0, nseg, k, tcov.p, s, kGridNNMin));
        HIPC(c, launch_covariances_grid(c->tgt.p, c->seg_lo_h.data() + seg0, c->seg_cnt_h.data() + seg0, nseg, seg0,
                                        c->grids.p, c->cell_start.p, c->grid_pts.p, k, tcov.p, s));
        tcov_k = k;
    }
    // GICP scratch per pose: nsamp cloud slots (16 B) + covariances (48 B) + the iteration's correspondences (4 B)
    // and Mahalanobis matrices (48 B), and gicp_kernel's correspondence history: kCorrHist sets of up to hist_cap points
    // (C3's rendered clouds hold <= 467 of 4,800 samples; larger clouds search every iteration).  Up to 32 GiB is one
    // chunk for 100k poses at 640x480 / stride 8; on C3 (50k poses) one chunk instead of two saves ~5 ms of a 37 ms step.
    const int hist_cap = std::min(nsamp, kCorrHistCap);
    const size_t per_pose = (size_t)nsamp * 116 + (size_t)kCorrHist * hist_cap * 4;
    const int chunk = st.chunk = plan_chunks(num_poses, per_pose, "PCORE_ICP_SCRATCH_GIB", 30);
    if (const int rc = staged_slots(c, st)) return rc;
    HIPC(c, dev_reserve(c->icp_cov, (size_t)6 * chunk * nsamp));
    HIPC(c, dev_reserve(c->icp_corr, (size_t)chunk * nsamp));
    const bool use_hist = !getenv("PCORE_GICP_NO_HIST");  // A/B knob (same results)
    if (use_hist) HIPC(c, dev_reserve(c->icp_corr_hist, (size_t)chunk * kCorrHist * hist_cap));
    HIPC(c, dev_reserve(c->icp_mahal, (size_t)6 * chunk * nsamp));
    HIPC(c, dev_reserve(c->icp_counter, 1));
    HIPC(c, dev_reserve(c->icp_iter_stats, 4));
    if (!c->icp_iter_stats_host.p)
        HIPC(c, hipHostMalloc((void**)&c->icp_iter_stats_host.p, 4 * sizeof(unsigned long long), hipHostMallocDefault));
    HIPC(c, dev_reserve(c->icp_order_keys, (size_t)2 * chunk));
    HIPC(c, dev_reserve(c->icp_order_idx, (size_t)2 * chunk));
    const size_t order_temp = gicp_order_temp_bytes(chunk);
    HIPC(c, dev_reserve(c->icp_order_temp, order_temp));
    // gpu_stats (renderer.cu:1707, 1739): device memory in use at the GICP stage, events around it per chunk
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        c->peak_mem_mb = std::max(c->peak_mem_mb, (double)(total_b - free_b) / 1024.0 / 1024.0);
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    HIPC(c, hipStreamIsCapturing(s, &cap_status));
    const bool timed = cap_status == hipStreamCaptureStatusNone;
    c->icp_ev_used = 0;
    HIPC(c, hipMemsetAsync(c->icp_iter_stats.p, 0, 4 * sizeof(unsigned long long), s));
    while (timed && c->icp_ev.v.size() < (size_t)3 * ((num_poses + chunk - 1) / chunk)) {
        hipEvent_t e;
        HIPC(c, hipEventCreate(&e));
        c->icp_ev.v.push_back(e);
    }
    GicpArgs g{};
    g.src = st.cloud;
    g.src_count = st.count;
    g.src_cov = c->icp_cov.p;
    g.corr = c->icp_corr.p;
    g.mahal = c->icp_mahal.p;
    g.corr_hist = use_hist ? c->icp_corr_hist.p : nullptr;
    g.corr_hist_cap = hist_cap;
    g.src_cap = nsamp;
    g.tgt = c->tgt.p;
    g.tgt_cov = tcov.p;
    g.seg_lo = c->seg_lo.p;
    g.seg_hi = c->seg_hi.p;
    g.num_segs = nl;
    g.whole_seg = nl;
    g.pose_label = st.pose_label;
    g.poses_in = d_poses;
    g.poses_out = d_out_poses;
    g.iters_out = d_out_iters;
    g.max_iter = ip->max_iterations;
    g.rot_eps = ip->rotation_epsilon;
    g.trans_eps = ip->transformation_epsilon;
    g.work_counter = c->icp_counter.p;
    g.cycle_window = ip->cycle_exit_window;
    g.iter_stats = c->icp_iter_stats.p;
    g.tgt_quads = c->tgt_quads.p;
    g.seg_qoff = c->seg_qoff.p;
    g.grids = c->grids.p;
    g.cell_start = c->cell_start.p;
    g.grid_pts = c->grid_pts.p;
    // the GICP kernel instance with the grid search only when some segment the poses can use is large (gicp_pose:
    // use_grid = nt > kGridNNMin with grids present); 6-DoF poses use their label's segment, 3-DoF the whole cloud
    bool grid_needed = false;
    if (c->grids.p)
        for (int L = six ? 0 : nl; L < (six ? nl : nl + 1); L++)
            grid_needed = grid_needed || segment_uses_grid(c->seg_cnt_h[L], true);
    const int rc = for_each_chunk(c, st, [&](int base, int n) -> int {
        hipEvent_t* ev = timed ? c->icp_ev.v.data() + 3 * c->icp_ev_used : nullptr;
        if (ev) HIPC(c, hipEventRecord(ev[0], s));
        // the clouds' covariances: k = 10 by the threshold k-NN over each cloud's sample grid (pcore_cov.h), other k
        // by the brute force; bit-identical
        if (k == 10)
            HIPC(c, launch_covariances_cloud(st.cloud, st.count, nsamp, n, st.a.fx, st.a.fy, st.a.cx, st.a.cy, p->stride,
                                             c->icp_cov.p, s));
        else
            HIPC(c, launch_covariances(st.cloud, nullptr, st.count, nsamp, n, k, c->icp_cov.p, s));
        g.pose_base = base;
        g.pose_order = nullptr;
        if (!getenv("PCORE_GICP_INDEX_ORDER")) {  // A/B knob: the queue in index order
            HIPC(c, launch_gicp_order(g, n, c->icp_order_keys.p, c->icp_order_keys.p + chunk, c->icp_order_idx.p,
                                      c->icp_order_idx.p + chunk, c->icp_order_temp.p, order_temp, s));
            g.pose_order = c->icp_order_idx.p + chunk;
        }
        if (ev) HIPC(c, hipEventRecord(ev[1], s));
        HIPC(c, launch_gicp(g, n, c->dinfo, s, grid_needed));
        if (ev) {  // the counters so far (the last chunk's copy holds the call's totals), then the chunk's end
            HIPC(c, hipMemcpyAsync(c->icp_iter_stats_host.p, c->icp_iter_stats.p, 4 * sizeof(unsigned long long),
                                   hipMemcpyDeviceToHost, s));
            HIPC(c, hipEventRecord(ev[2], s));
            c->icp_ev_used++;
        }
        return PCORE_OK;
    });
    if (rc != PCORE_OK) return rc;
    // re-render and re-score the adjusted poses (renderer.cu:1757-1907)
    return pcore_evaluate(c, d_out_poses, d_pose_model, d_pose_label, d_pose_obs_total, num_poses, p, d_out_rc,
                          d_out_oc, d_out_diff, nullptr, stream);
}

int pcore_get_stats(pcore_ctx* c, pcore_gpu_stats* out, int32_t reset) {
    if (!c || !out) return PCORE_E_INVALID_ARG;
    HIPC(c, hipSetDevice(c->device));
    double icp_ms = 0.0, gicp_ms = 0.0;
    for (int i = 0; i < c->icp_ev_used; i++) {
        hipEvent_t* ev = c->icp_ev.v.data() + 3 * i;
        HIPC(c, hipEventSynchronize(ev[2]));
        float a = 0.0f, b = 0.0f;
        HIPC(c, hipEventElapsedTime(&a, ev[0], ev[2]));
        HIPC(c, hipEventElapsedTime(&b, ev[1], ev[2]));
        icp_ms += a;
        gicp_ms += b;
    }
    out->icp_runtime = (float)(icp_ms * 1e-3);
    out->peak_memory_usage = c->peak_mem_mb;
    out->gicp_ms = (float)gicp_ms;
    out->icp_chunks = c->icp_ev_used;
    unsigned long long it[4] = {0ull, 0ull, 0ull, 0ull};
    if (c->icp_ev_used > 0 && c->icp_iter_stats_host.p)  // the last chunk's end event (after its copy) has completed
        for (int i = 0; i < 4; i++) it[i] = c->icp_iter_stats_host.p[i];
    if (it[3] != 0)
        return fail(c, PCORE_E_HIP, "evaluate_icp: " + std::to_string(it[3]) +
                                        " poses needed the grid search in the GICP instance without it");
    out->gicp_iterations = (int64_t)it[0];
    out->gicp_iterations_run = (int64_t)it[1];
    out->gicp_cycle_exits = (int64_t)it[2];
    if (reset) c->peak_mem_mb = 0.0;
    return PCORE_OK;
}

int pcore_get_tile_info(pcore_ctx* c, pcore_tile_info* out) {
    if (!c || !out) return PCORE_E_INVALID_ARG;
    static_assert(kTileTiers <= PCORE_MAX_TILE_TIERS, "pcore_tile_info holds the tiers");
    std::memset(out, 0, sizeof(*out));
    out->num_tiers = kTileTiers;
    out->tier = c->tile_tier;
    out->tcap = c->tile_tcap;
    out->seq = -1;
    for (int t = 0; t < kTileTiers; t++) {
        out->edge[t] = c->tile_edge[t];
        out->wgs_per_cu[t] = tier_wgs(t);
    }
    if (c->fb_host.p) {
        const volatile int32_t* fb = c->fb_host.p;
        for (int b = 0; b <= kTileTiers; b++) out->hist[b] = fb[b];
        out->chunked = fb[kTileTiers + 1];
        out->seq = fb[kTileTiers + 2];
    }
    return PCORE_OK;
}

}  // extern "C"
