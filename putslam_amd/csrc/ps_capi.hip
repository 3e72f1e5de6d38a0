// ps_capi.hip -- the device translation unit of libputslam_hip.so (include/putslam_hip.h): every kernel header and every launch.
// PsContext itself -- stream, scratch arena, option table, stop-table builders, timing record -- lives in ps_context.cpp /
// ps_internal.h, host-only; so do the batch queue and the environment default.
// There is no CPU fallback anywhere in this file: every entry point launches HIP kernels or fails with a negative PsStatus.
//
// Top to bottom: the shared host glue (ps_glue.h), the pair pipeline (the plan of a call with its schedule and stages, one header
// per subject), the VO entry point, then every further feature as ONE header (its kernels, then its host glue and entry points) in
// dependency order, and psi_kernel_attributes last.
#include "ps_block.h" // namespace psdev: the work-group and wave primitives
#include "ps_internal.h"
#include "ps_glue.h"

#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace psdev;

#include "ps_ransac_stage.h" // kernels 3 + 4 (ps_score_value.h, ps_score_pass.h / _fast.h / _euclid.h, ps_select_refit.h): Plan, make_plan, prepare_score, run_ransac_stage; ps_ransac_rigid3d
#include "ps_match_stage.h"  // kernels 1 + 2 (ps_matcher_mfma.h): run_match_stage; ps_match_hamming256
#include "ps_diag.h"         // ps_debug_*: the parity tests' diagnostics (no reference counterpart)
#include "ps_geometry.h"     // ps_umeyama_f32 / ps_kabsch_f64 / ps_keypoints2Dto3D / ps_remove_image_distortion / ps_points3Dto2D

static_assert(kPsReorderMargin == kReorderMargin && kPsReorderTopMax == kReorderTopMax, "ps_internal.h mirrors ps_score_pass.h");
static_assert(kPlanBlock == kBlock && kPlanPrefixFixed == kPrefixFixed && kPlanPrefixAdaptive == kPrefixAdaptive && kPlanStages == kStages,
              "ps_score_plan.h mirrors ps_block.h / ps_score_pass.h");

extern "C" {

// ---------------------------------------------------------------------------------------------
// the 72-byte per-pair record of the multi-GPU gather (include/putslam_hip.h: ps_pack_records_device)
namespace {
__global__ void ps_pack_records_kernel(const float *__restrict__ pose, const PsRansacStats *__restrict__ stats, int valid, int pairs,
                                       float *__restrict__ rec)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= pairs) return;
    float *r = rec + (size_t)p * PS_RECORD_FLOATS;
    if (p < valid) {
        for (int i = 0; i < 16; ++i) r[i] = pose[(size_t)p * 16 + i];
        r[16] = (float)stats[p].numInliers;
        r[17] = (float)stats[p].numMatchesIn;
    } else {
        for (int i = 0; i < PS_RECORD_FLOATS; ++i) r[i] = 0.0f;
    }
}
} // namespace

int ps_pack_records_device(PsContext *ctx, void *hipStream, const float *pose, const PsRansacStats *stats, int valid, int pairs,
                           float *records)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (pairs < 0 || valid < 0 || valid > pairs || (pairs > 0 && !records) || (valid > 0 && (!pose || !stats)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_pack_records_device: bad argument");
    if (pairs == 0) return PS_OK;
    hipStream_t st = hipStream ? (hipStream_t)hipStream : ctx->stream;
    hipLaunchKernelGGL(ps_pack_records_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, pose, stats, valid, pairs, records);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// ---------------------------------------------------------------------------------------------
int ps_vo_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                       const PsFrameSet *frames, const int32_t *pairs, int P, const PsPairResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!frames || !out || P < 0 || (P > 0 && !pairs)) return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_device: bad argument");
    if (P == 0) return PS_OK;
    if (!frames->desc || !frames->pts || !frames->nkpts || frames->maxKpts < 1 || frames->maxKpts > PS_MAX_KPTS)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_device: bad frame set");
    if (!out->matches || !out->numMatches || !out->inlierMask || !out->pose || !out->stats)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_device: null output");
    FrameStrides strides; // (checked here, before anything is planned or allocated; run_match_stage resolves them for its launches)
    rc = frame_strides(ctx, *frames, true, true, "ps_vo_pairs_device", strides);
    if (rc) return rc;
    if (cfg && cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "explicit sample streams are per call, not per batch");
    const int cap = frames->maxKpts;
    Plan pl;
    rc = make_plan(ctx, params, cfg, K, cap, cap, pl);
    if (rc) return rc;
    begin_timed_call(ctx);
    HandoffGuard handoffGuard{ctx}; // (prepare_score below may already queue a clearing: the guard stands before it)
    rc = prepare_score(ctx, pl, P, cap, false, true, frames->desc);
    if (rc) return rc;
    rc = run_match_stage(ctx, *frames, pairs, P, &pl, out->matches, out->numMatches, 0);
    if (rc) return rc;
    return run_ransac_stage(ctx, pl, P, cap, out->matches, out->numMatches, cap, out->pose, out->inlierMask, out->stats, 2);
}

} // extern "C"

// The further features, each header its kernels and then its host side, in dependency order
#include "ps_stream_push.h"  // ps_vo_stream_create / _push: the synchronous streaming form
#include "ps_stream_async.h" // ... and the pipelined one, on the PsVoStream of the former
#include "ps_map_match.h"    // map_sweep<F, D>, its launcher and entry bodies; ps_match_xyz_device / ps_map_pairs_device (the plan and the stages above)
#include "ps_dbscan.h"       // ps_dbscan_thin(_device)
#include "ps_exclusion.h"    // ps_exclude(_device) and the three rules (DBScan's bound)
#include "ps_map_view.h"     // ps_map_views_device / ps_frame_levels_device
#include "ps_loop_closure.h" // ps_pose_sets_device / ps_loop_pairs_device (the plan and the stages above)
#include "ps_match_l2.h"     // ps_match_l2_f32 / ps_match_l2_device / ps_vo_pairs_l2_device (the plan and the stages above)
#include "ps_map_match_l2.h" // the float policy of ps_map_match.h: ps_match_xyz_l2_f32 / ps_match_xyz_l2_device / ps_map_pairs_l2_device (ps_match_l2.h too)
#include "ps_map_store_f32.h" // ps_map_views_l2_device / ps_pose_sets_l2_device / ps_loop_pairs_l2_device (ps_map_view.h, ps_loop_closure.h, ps_match_l2.h)
#include "ps_klt.h"          // ps_klt_pyramids_* / ps_klt_track_device / ps_klt_select_device / ps_perform_tracking (ps_exclusion.h's bound)
#include "ps_fast.h"         // ps_fast_detector_* / ps_detect_features(_device) (the PsImageSet rule of all three: ps_glue.h, ps_image_rule.h)
#include "ps_orb.h"          // ps_orb_pyramids_* / ps_describe_features(_device) (ps_fast.h's stable counting sort)
#include "ps_orb_detect.h"   // ps_orb_detector_* / ps_orb_detect_frames / ps_detect_features_orb (ps_fast.h's tile body, ps_orb.h's levels)
#include "ps_frame_assembly.h" // ps_gather_keypoints / ps_assemble_frames / ps_front_end_* (the launches of ps_dbscan.h, ps_orb.h, ps_orb_detect.h)
#include "ps_track_vo.h"     // ps_ransac_match_lists / ps_assemble_tracked / ps_track_vo_pairs (the plan and the stages above, ps_klt.h's launches, ps_frame_assembly.h's body)
#include "ps_uncertainty.h"  // ps_feature_uncertainty / ps_measurement_edges / ps_compute_normals / ps_compute_rgb_gradients / ps_information_matrices (ps_frame_assembly.h's back-projection)
#include "ps_patches.h"      // ps_patch_models / ps_patch_align / ps_compute_patch(_gradient) / ps_optimize_location(s) (ps_image_rule.h's set rule)
#include "ps_track_close.h"  // ps_track_candidates / ps_track_close_* (ps_exclusion.h's predicate, ps_map_view.h's level rule, the launches of ps_orb.h and ps_frame_assembly.h)

// Launch attributes of the kernels that need them (ps_internal.h; called once per context).
extern "C" void psi_kernel_attributes(void)
{
    // the cross-check kernel keeps best[q] for up to PS_MAX_KPTS queries in LDS (64 KiB of the CU's 160 KiB)
    for (const void *k : {reinterpret_cast<const void *>(&ps_crosscheck_prep<true>), reinterpret_cast<const void *>(&ps_crosscheck_prep<false>),
                          reinterpret_cast<const void *>(&ps_crosscheck_prep<true, 1024>), reinterpret_cast<const void *>(&ps_crosscheck_prep<false, 1024>)})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, PS_MAX_KPTS * 4);
    dbscan_kernel_attributes();
    exclusion_kernel_attributes();
    l2_kernel_attributes();
    klt_kernel_attributes();
    patch_kernel_attributes();
}
