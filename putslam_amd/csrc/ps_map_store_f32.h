// ps_map_store_f32.h -- the resident feature map with FLOAT descriptor rows (SURF / SIFT): ps_map_views_l2_device,
// ps_pose_sets_l2_device, ps_loop_pairs_l2_device (include/putslam_hip.h).  The reference runs the same code
// for both descriptor kinds:
//   Matcher::matchXYZ (src/Matcher/matcher.cpp:675-679)                      copies whatever cv::Mat row the chosen observation holds,
//   Matcher::matchFeatureLoopClosure (src/Matcher/matcher.cpp:802-861)       pushes ext.descriptor rows into a Mat, performMatching,
//   MatcherOpenCV (src/Matcher/matcherOpenCV.cpp:100-102)                    which for SURF / SIFT is BFMatcher(NORM_L2, true).
// Everything that depends on the store's index arrays alone is shared with the binary path: ps_view_select / ps_view_emit
// (ps_map_view.h), ps_pose_table / _count / _scan / _emit, ps_loop_gate / ps_loop_verdict (ps_loop_closure.h), run_l2_match
// (ps_match_l2.h).  The two emit kernels are instantiated without their 32-byte descriptor store and record the observation of
// every output row instead (obsIdx, or the context's scratch when the caller keeps none).
//
// The one new kernel is the row gather.  An emit thread storing its own 256- or 512-byte row would have 64 lanes writing 64
// different rows: every store instruction touches 64 cache lines.  ps_gather_rows_f32 walks (set, row < nkpts[set]) and lets a
// whole wavefront copy ONE row at a time, lane k the k-th unit of the row, from obsDesc + obs x stride to the output row:
// consecutive lanes, consecutive addresses, both ways.  The unit is 16 bytes where both bases and both strides are multiples of
// 16 and dim is a multiple of 4 (dense SURF / SIFT rows), else a 32-bit word; the host decides once and picks the
// instantiation -- no run-time choice inside the loop.  Rows are moved as words, never through float arithmetic.  nkpts is 0
// for an overflowed or invalid set, so no row of such a set is written; no LDS, no scratch memory.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ps_glue.h"
#include "ps_loop_closure.h"
#include "ps_map_view.h"
#include "ps_match_l2.h"

namespace psdev {

constexpr int kGatherBlock = 256;
constexpr int kGatherWaves = kGatherBlock / 64;
constexpr int kGatherRows = 32; // rows a work-group copies: eight a wave

struct GatherArgs {
    const uint32_t *src;    // obsDesc
    size_t srcRowWords;     // 32-bit words between the store's rows
    int numObs, dim;
    const int32_t *obsIdx;  // [sets][maxKpts]: the observation of every output row
    const int32_t *nkpts;   // [sets]
    int maxKpts, chunks;    // work-groups per set
    uint32_t *dst;
    size_t dstRowWords, dstSetWords;
};

// grid sets x chunks.  VEC: 16-byte units (the host has checked both bases, both strides and dim).
template <bool VEC> __global__ __launch_bounds__(kGatherBlock) void ps_gather_rows_f32(GatherArgs a)
{
    const int lane = (int)threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int s = (int)blockIdx.x / a.chunks, c = (int)blockIdx.x - s * a.chunks;
    int n = a.nkpts[s];
    n = n < 0 ? 0 : (n > a.maxKpts ? a.maxKpts : n);
    const int r0 = c * kGatherRows;
    if (r0 >= n) return; // (the whole work-group)
    const int r1 = r0 + kGatherRows < n ? r0 + kGatherRows : n;
    const int32_t *__restrict__ oi = a.obsIdx + (size_t)s * a.maxKpts;
    uint32_t *__restrict__ set = a.dst + (size_t)s * a.dstSetWords;
    for (int r = r0 + w; r < r1; r += kGatherWaves) {
        const int o = oi[r]; // (one address for the wave)
        if (o < 0 || o >= a.numObs) continue; // (cannot happen for a row the emit kernel wrote: nothing outside the store is read)
        const uint32_t *__restrict__ from = a.src + (size_t)o * a.srcRowWords;
        uint32_t *__restrict__ to = set + (size_t)r * a.dstRowWords;
        if (VEC) {
            const uint4 *__restrict__ from4 = reinterpret_cast<const uint4 *>(from);
            uint4 *__restrict__ to4 = reinterpret_cast<uint4 *>(to);
            for (int k = lane; k < (a.dim >> 2); k += 64) to4[k] = from4[k];
        } else {
            for (int k = lane; k < a.dim; k += 64) to[k] = from[k];
        }
    }
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the checks and the launches
namespace {

// THE RULE of a PsMapStoreF32's rows (include/putslam_hip.h); rowBytes = the resolved stride
int check_store_f32(PsContext *ctx, const PsMapStoreF32 &st, const char *who, size_t &rowBytes)
{
    const std::string w(who);
    if (st.dim < 1) return fail(ctx, PS_ERR_BAD_ARG, (w + ": store.dim < 1").c_str());
    if (st.dim > PS_MAX_L2_DIM) return fail(ctx, PS_ERR_UNSUPPORTED, (w + ": more than PS_MAX_L2_DIM elements per descriptor").c_str());
    rowBytes = st.obsDescRowStride ? st.obsDescRowStride : (size_t)st.dim * 4;
    if ((rowBytes & 3) != 0 || rowBytes < (size_t)st.dim * 4 || ((uintptr_t)st.obsDesc & 3) != 0)
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": obsDescRowStride must be a multiple of 4 and >= dim x 4, obsDesc 4-byte aligned").c_str());
    return PS_OK;
}

// The observation of every output row: the caller's obsIdx, or the context's block of 4 x sets x maxKpts bytes
int gather_obs_block(PsContext *ctx, int32_t *callers, int sets, int maxKpts, int32_t *&out)
{
    out = callers;
    if (callers) return PS_OK;
    PS_ENSURE(ctx->gatherObs, (size_t)sets * maxKpts * sizeof(int32_t));
    out = (int32_t *)ctx->gatherObs.p;
    return PS_OK;
}

// The gather of `sets` sets behind an emit kernel that recorded obsIdx on the same stream
int run_gather_rows(PsContext *ctx, const char *who, const PsMapStoreF32 &st, size_t srcRowBytes, const PsFrameSetF32 &fs,
                    const L2Strides &strides, int sets, const int32_t *obsIdx)
{
    if (st.numObs == 0) return PS_OK; // (no observation, no member, no row)
    GatherArgs g{};
    g.src = (const uint32_t *)st.obsDesc;
    g.srcRowWords = srcRowBytes / 4;
    g.numObs = st.numObs;
    g.dim = st.dim;
    g.obsIdx = obsIdx;
    g.nkpts = fs.nkpts;
    g.maxKpts = fs.maxKpts;
    g.chunks = (fs.maxKpts + kGatherRows - 1) / kGatherRows;
    g.dst = (uint32_t *)fs.desc;
    g.dstRowWords = (size_t)strides.rowFloats;
    g.dstSetWords = strides.frameFloats;
    if ((long long)sets * g.chunks > (long long)INT_MAX)
        return fail(ctx, PS_ERR_UNSUPPORTED, (std::string(who) + ": sets x row chunks exceeds the grid").c_str());
    const bool vec = (st.dim & 3) == 0 && ((uintptr_t)st.obsDesc & 15) == 0 && (srcRowBytes & 15) == 0 && ((uintptr_t)fs.desc & 15) == 0 &&
                     ((g.dstRowWords * 4) & 15) == 0 && ((g.dstSetWords * 4) & 15) == 0;
    HandoffGuard handoffGuard{ctx};
    const dim3 grid((unsigned)sets * (unsigned)g.chunks), block(kGatherBlock);
    if (vec) hipLaunchKernelGGL(ps_gather_rows_f32<true>, grid, block, 0, ctx->stream, g);
    else hipLaunchKernelGGL(ps_gather_rows_f32<false>, grid, block, 0, ctx->stream, g);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_map_store_f32(void) { return sizeof(PsMapStoreF32); }
size_t ps_abi_sizeof_map_view_out_f32(void) { return sizeof(PsMapViewOutF32); }
size_t ps_abi_sizeof_pose_set_out_f32(void) { return sizeof(PsPoseSetOutF32); }
size_t ps_abi_sizeof_loop_batch_f32(void) { return sizeof(PsLoopBatchF32); }

int ps_map_views_l2_device(PsContext *ctx, const PsMapStoreF32 *store, const PsMapViewRequest *req, const PsMapViewOutF32 *out)
{
    const char *who = "ps_map_views_l2_device";
    int rc = bind(ctx);
    if (rc) return rc;
    if (!store || !req || !out) return fail(ctx, PS_ERR_BAD_ARG, "ps_map_views_l2_device: null store, request or output block");
    rc = check_view_call(ctx, who, store, req);
    if (rc || req->V == 0) return rc;
    size_t rowBytes = 0;
    rc = check_store_f32(ctx, *store, who, rowBytes);
    if (rc) return rc;
    rc = check_view_request(ctx, who, store->numPoses, req, out);
    if (rc) return rc;
    L2Strides strides;
    rc = check_l2_frames(ctx, out->views, true, "ps_map_views_l2_device: output views", strides);
    if (rc) return rc;
    if (out->views.dim != store->dim) return fail(ctx, PS_ERR_BAD_ARG, "ps_map_views_l2_device: views.dim differs from store.dim");
    if (out->views.numFrames < req->V) return fail(ctx, PS_ERR_BAD_ARG, "ps_map_views_l2_device: the output set has fewer than V views");
    TimingOff toff(ctx);
    ViewArgs a{};
    fill_view_args(a, store, req, out);
    a.ptsStride = strides.ptsFloats;
    rc = gather_obs_block(ctx, out->obsIdx, req->V, out->views.maxKpts, a.obsIdx);
    if (rc) return rc;
    rc = run_view_chain<false>(ctx, who, a, req->V);
    if (rc) return rc;
    return run_gather_rows(ctx, who, *store, rowBytes, out->views, strides, req->V, a.obsIdx);
}

int ps_pose_sets_l2_device(PsContext *ctx, const PsMapStoreF32 *store, const PsPoseSetRequest *req, const PsPoseSetOutF32 *out)
{
    const char *who = "ps_pose_sets_l2_device";
    int rc = bind(ctx);
    if (rc) return rc;
    if (!store || !req || !out) return fail(ctx, PS_ERR_BAD_ARG, "ps_pose_sets_l2_device: null store, request or output block");
    if (store->numFeatures < 0 || store->numObs < 0 || store->numPoses < 0 || req->S < 0)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_pose_sets_l2_device: a negative count (numFeatures, numObs, numPoses, S)");
    if (req->S > PS_LOOP_MAX_SETS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_pose_sets_l2_device: more than PS_LOOP_MAX_SETS sets");
    L2Strides strides;
    rc = check_l2_frames(ctx, out->sets, true, "ps_pose_sets_l2_device: output sets", strides);
    if (rc) return rc;
    rc = check_pose_call(ctx, who, store, req, out);
    if (rc) return rc;
    size_t rowBytes = 0;
    rc = check_store_f32(ctx, *store, who, rowBytes);
    if (rc) return rc;
    if (out->sets.dim != store->dim) return fail(ctx, PS_ERR_BAD_ARG, "ps_pose_sets_l2_device: sets.dim differs from store.dim");
    TimingOff toff(ctx);
    if (req->S == 0) { // nothing but the empty set
        PS_HIP(hipMemsetAsync((void *)out->sets.nkpts, 0, sizeof(int32_t), ctx->stream));
        return PS_OK;
    }
    PoseSetArgs a{};
    fill_pose_args(a, store, req, out);
    a.ptsStride = strides.ptsFloats;
    rc = gather_obs_block(ctx, out->obsIdx, req->S, out->sets.maxKpts, a.obsIdx);
    if (rc) return rc;
    rc = run_pose_chain<false>(ctx, a);
    if (rc) return rc;
    return run_gather_rows(ctx, who, *store, rowBytes, out->sets, strides, req->S, a.obsIdx);
}

int ps_loop_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                            const PsLoopBatchF32 *b, const PsLoopResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    L2Strides strides;
    return loop_pairs_body(
        ctx, "ps_loop_pairs_l2_device", params, cfg, K, b, out,
        [&](const PsFrameSetF32 &fs) { return check_l2_frames(ctx, fs, true, "ps_loop_pairs_l2_device: sets", strides); },
        [&](const int32_t *eff, int L, const Plan &pl) {
            return run_l2_match(ctx, b->sets, strides, eff, L, &pl, out->pair.matches, out->pair.numMatches, 0);
        });
}

} // extern "C"
