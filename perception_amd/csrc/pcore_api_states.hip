// pcore_api_states.hip -- pcore_evaluate_states: the checks and the launch of stage COST over composed states
// (pcore_state_cost.hip; DESIGN.md section 2, "State cost").
#include "pcore_ctx.h"

using namespace pcore;

extern "C" {

int pcore_evaluate_states(pcore_ctx* c, const int32_t* d_zs, int32_t num_poses, const int32_t* d_pose_label,
                          const int32_t* d_state_off, const int32_t* d_state_member, int32_t num_states,
                          const float* d_state_obs_total, const pcore_eval_params* p, float* d_out_rc,
                          float* d_out_oc, float* d_out_diff, int32_t* d_out_member_vis, int32_t* d_out_member_bad,
                          int32_t num_members, pcore_stream stream) {
    if (!c || !p) return PCORE_E_INVALID_ARG;
    const std::string w("evaluate_states");
    if (!c->have_cam || !c->have_obs) return fail(c, PCORE_E_STATE, w + ": camera and observation must be set first");
    if (p->cost_type != PCORE_COST_DEPTH_3DOF && p->cost_type != PCORE_COST_DEPTH_6DOF)
        return fail(c, PCORE_E_INVALID_ARG, w + ": cost_type must be 0 or 2 (the sampled z-buffers carry no colour ids)");
    if (num_states < 0 || num_poses < 0 || num_members < 0)
        return fail(c, PCORE_E_INVALID_ARG, w + ": negative count");
    if (p->stride <= 0 || c->cam.width % p->stride != 0)
        return fail(c, PCORE_E_INVALID_ARG, w + ": width must be a multiple of stride");
    if (num_states == 0) return PCORE_OK;
    if (!d_state_off || !d_out_rc || (num_members > 0 && !d_state_member) ||
        (num_members > 0 && num_poses > 0 && !d_zs))
        return fail(c, PCORE_E_INVALID_ARG, w + ": null state / z-buffer / output pointer");
    const bool six = p->cost_type == PCORE_COST_DEPTH_6DOF;
    if (six && num_poses > 0 && !d_pose_label) return fail(c, PCORE_E_INVALID_ARG, w + ": cost_type 2 needs pose labels");
    if (p->calc_obs_cost && (!d_state_obs_total || !d_out_oc || !d_out_diff))
        return fail(c, PCORE_E_INVALID_ARG, w + ": calc_obs_cost needs state_obs_total and oc/diff outputs");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;

    StateCostArgs a{};
    a.zs = d_zs;
    a.num_poses = num_poses;
    a.pose_label = six ? d_pose_label : nullptr;
    a.state_off = d_state_off;
    a.state_member = d_state_member;
    a.num_states = num_states;
    a.num_members = num_members;
    a.state_obs_total = d_state_obs_total;
    a.stride = p->stride;
    a.ws = c->cam.width / p->stride;
    a.hs = (c->cam.height + p->stride - 1) / p->stride;
    a.cx = c->cam.cx; a.cy = c->cam.cy; a.fx = c->cam.fx; a.fy = c->cam.fy;
    a.depth_factor = p->depth_factor;
    a.grids = c->grids.p;
    a.cell_start = c->cell_start.p;
    a.grid_pts = c->grid_pts.p;
    a.seg_lo = c->seg_lo.p;
    a.num_grids = c->num_grids;
    a.bitmap_words = std::max(1, (c->num_obs + 31) / 32);
    a.r2 = p->sensor_resolution * p->sensor_resolution;  // renderer.cu:1877
    a.calc_obs = p->calc_obs_cost;
    a.out_rc = d_out_rc;
    a.out_oc = d_out_oc;
    a.out_diff = d_out_diff;
    a.out_member_vis = d_out_member_vis;
    a.out_member_bad = d_out_member_bad;
    if (c->num_obs > PCORE_STATE_LDS_OBS) {  // the explained bitmap does not fit the workgroup's LDS
        const size_t need = (size_t)state_cost_scratch_blocks(num_states, c->dinfo) * a.bitmap_words;
        if (const int rc = refuse_setup_in_capture(c, "evaluate_states", "the bitmap scratch",
                                                   !(c->state_bitmap.p && c->state_bitmap.n >= need), s))
            return rc;
        HIPC(c, reserve_gen(c, c->state_bitmap, need));
        a.scratch_bitmap = c->state_bitmap.p;
    }
    // list positions beyond the kernel's LDS histogram are counted in place
    if (d_out_member_vis && num_members > 0) HIPC(c, hipMemsetAsync(d_out_member_vis, 0, (size_t)num_members * 4, s));
    if (d_out_member_bad && num_members > 0) HIPC(c, hipMemsetAsync(d_out_member_bad, 0, (size_t)num_members * 4, s));
    HIPC(c, launch_state_cost(a, c->dinfo, s));
    return PCORE_OK;
}

}  // extern "C"
