// ps_track_vo.h -- the tracking VO step without a host step (include/putslam_hip.h: "The tracking VO step"; Matcher::trackKLT,
// matcher.cpp:147-211): the estimator over caller-supplied device-resident match lists, the rows a tracked frame leaves, and the
// queue of launches that is the whole step.  Part of the device translation unit (ps_capi.hip), after ps_klt.h and
// ps_frame_assembly.h, whose launches and checks it uses.  The record builder ps_prep_match_lists stands in ps_pair_records.h
// beside the single-pair kernel it shares its body with.
#pragma once

namespace psdev {

// what ps_assemble_tracked_rows needs beside its arrays
struct TrackedArgs {
    DistArgs dist;
    double scale;
    const uint8_t *depth;       // frame 0 of the set
    size_t rowStride, frameStride;
    const int32_t *frame;       // pair p reads depth frame frame[p * frameStep + frameOff]
    int frameStep, frameOff;
    int rows, cols, numFrames, cap;
};

// Output row j of pair p from tracked point i = keptIdx[p][j]: its position, the undistorted one, the 3-D point read from the
// pair's depth frame, and the previous rows' columns carried by index.  One thread per output row, a grid of row blocks x pairs,
// no LDS.
__global__ __launch_bounds__(kBlock) void ps_assemble_tracked_rows(TrackedArgs a, const float2 *__restrict__ nextPts,
                                                                   const int32_t *__restrict__ keptIdx, const int32_t *__restrict__ numKept,
                                                                   PsTrackedCarry c, PsTrackedRows o)
{
    const int p = (int)blockIdx.y, j = (int)(blockIdx.x * kBlock + threadIdx.x);
    const int n = numKept[p];
    const bool ok = n >= 0 && n <= a.cap;
    if (j == 0) o.counts[p] = ok ? n : -1;
    if (!ok || j >= n) return;
    const size_t base = (size_t)p * (size_t)a.cap, to = base + (size_t)j;
    const int i = keptIdx[to];
    const bool in = i >= 0 && i < a.cap;
    const size_t from = base + (size_t)(in ? i : 0);
    float2 pt = make_float2(0.f, 0.f), q = pt;
    float X = 0.f, Y = 0.f, Z = 0.f;
    if (in) {
        pt = nextPts[from];
        const int g = a.frame[(size_t)p * (size_t)a.frameStep + (size_t)a.frameOff];
        const bool have = g >= 0 && g < a.numFrames;
        undistort_and_back_project(pt, a.dist, a.scale, have ? a.depth + (size_t)g * a.frameStride : (const uint8_t *)nullptr, a.rowStride,
                                   a.rows, a.cols, q, X, Y, Z);
    }
    o.pts[3 * to] = X;
    o.pts[3 * to + 1] = Y;
    o.pts[3 * to + 2] = Z;
    reinterpret_cast<float2 *>(o.xy)[to] = pt;
    if (o.xyUndist) reinterpret_cast<float2 *>(o.xyUndist)[to] = q;
    if (o.angle) o.angle[to] = in ? c.angle[from] : 0.f;
    if (o.response) o.response[to] = in ? c.response[from] : 0.f;
    if (o.octave) o.octave[to] = in ? c.octave[from] : 0;
    if (o.detDist) o.detDist[to] = in ? c.detDist[from] : 0.0;
}

} // namespace psdev

// Host side: the checks, the launches and the entry points
namespace {

// a group of point sets as ps_ransac_match_lists takes it; `a` resolved
int point_sets_check(PsContext *ctx, const PsPointSets *s, const char *who, PointSetsArgs &a)
{
    if (!s || !s->pts || !s->counts || s->numSets < 1 || s->capacity < 1)
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null point sets or array, numSets or capacity < 1").c_str());
    const size_t dense = (size_t)s->capacity * 12, stride = s->setStride ? s->setStride : dense;
    if ((stride & 3) != 0 || stride < dense || stride / 4 > (size_t)INT_MAX)
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": setStride must be a multiple of 4, >= capacity x 12 and below 8 GiB").c_str());
    a.pts = s->pts;
    a.counts = s->counts;
    a.numSets = s->numSets;
    a.capacity = s->capacity;
    a.strideFloats = (int)(stride / 4);
    return PS_OK;
}

struct MatchListsCall {
    Plan pl;
    PointSetsArgs prev{}, cur{};
};

// everything of ps_ransac_match_lists that can refuse, for P > 0: nothing is queued
int match_lists_check(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K, const PsPointSets *prev,
                      const PsPointSets *cur, const PsDMatch *matches, const int32_t *numMatches, int cap, uint8_t *mask, float *pose,
                      PsRansacStats *stats, MatchListsCall &c)
{
    static const char *who = "ps_ransac_match_lists";
    if (!matches || !numMatches || !mask || !pose || !stats) return fail(ctx, PS_ERR_BAD_ARG, "ps_ransac_match_lists: null array or output");
    if (cap < 1 || cap > (1 << 22)) return fail(ctx, PS_ERR_BAD_ARG, "ps_ransac_match_lists: cap must lie in 1 .. 1 << 22");
    int rc = point_sets_check(ctx, prev, who, c.prev);
    if (rc) return rc;
    rc = point_sets_check(ctx, cur, who, c.cur);
    if (rc) return rc;
    if (cur->capacity > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_ransac_match_lists: capacity of the current sets above PS_MAX_KPTS");
    if (cfg && cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "explicit sample streams are per call, not per batch");
    return make_plan(ctx, params, cfg, K, cap, cur->capacity, c.pl);
}

// everything of the chain that can still refuse or grow the scratch, for a checked call: the scoring stage's decisions (prepare_score
// may refuse a batch and may queue a clearing of its own scratch: the caller's HandoffGuard stands before it) and every block the
// launches below use.  Nothing of the caller's is touched here.
int match_lists_prepare(PsContext *ctx, MatchListsCall &c, const PsDMatch *matches, int P, int cap)
{
    int rc = prepare_score(ctx, c.pl, P, cap, false, true, matches);
    if (rc) return rc;
    PS_ENSURE(ctx->mvalid, (size_t)P * sizeof(int32_t));
    PS_ENSURE(ctx->cmax, (size_t)P * sizeof(float2));
    PS_ENSURE(ctx->sMatches, (size_t)P * cap * sizeof(PsDMatch)); // the lists kernel 4 reads: train indices it may follow, or -1
    PS_ENSURE(ctx->sMisc2, (size_t)P * sizeof(int32_t));         // ... and their counts
    PS_ENSURE(ctx->idxList, (size_t)P * cap * sizeof(int32_t));  // (run_ransac_stage's)
    return ensure_records(ctx, (size_t)P, (size_t)cap);
}

// the chain for a prepared call: ps_prep_match_lists, then kernels 3 + 4 as map_pairs_body queues them
int match_lists_launch(PsContext *ctx, MatchListsCall &c, const int32_t *pairs, const PsDMatch *matches, const int32_t *numMatches, int P,
                       int cap, uint8_t *mask, float *pose, PsRansacStats *stats)
{
    PsDMatch *clean = (PsDMatch *)ctx->sMatches.p;
    int32_t *numClean = (int32_t *)ctx->sMisc2.p;
    tick(ctx, 1, false);
    hipLaunchKernelGGL(ps_prep_match_lists, dim3((unsigned)P), dim3(kBlock), 0, ctx->stream, c.prev, c.cur, pairs, matches, numMatches, c.pl.pa,
                       rec_ptrs(ctx, c.pl.score), (int32_t *)ctx->mvalid.p, (float2 *)ctx->cmax.p, clean, numClean);
    tick(ctx, 1, true);
    PS_HIP(hipGetLastError());
    return run_ransac_stage(ctx, c.pl, P, cap, clean, numClean, cap, pose, mask, stats, 2);
}

// geometry and the depth set as ps_assemble_tracked takes them; `a` resolved except for the pair's frame
int tracked_check(PsContext *ctx, const PsFrameGeometry *g, const PsDepthSet *depth, int P, int capacity, const PsTrackedCarry *carry,
                  const PsTrackedRows *out, const char *who, TrackedArgs &a)
{
    const auto msg = [who](const char *what) { return std::string(who) + what; };
    int rc = rows_grid_check(ctx, P, capacity, who);
    if (rc) return rc;
    if (!g || !depth || !out) return fail(ctx, PS_ERR_BAD_ARG, msg(": null geometry, depth set or output rows").c_str());
    if (!out->xy || !out->pts || !out->counts) return fail(ctx, PS_ERR_BAD_ARG, msg(": rows xy, pts and counts are required").c_str());
    const PsTrackedCarry none{};
    const PsTrackedCarry &c = carry ? *carry : none;
    if (!c.angle != !out->angle || !c.response != !out->response || !c.octave != !out->octave || !c.detDist != !out->detDist)
        return fail(ctx, PS_ERR_BAD_ARG, msg(": angle, response, octave and detDist are carried as pairs: both or neither").c_str());
    size_t view = 0;
    if (!depth_set_strides(*depth, a.rowStride, a.frameStride, view))
        return fail(ctx, PS_ERR_BAD_ARG, msg(": depth set: rows and cols in 1 .. 8192, even strides, rowStride at least a row, frameStride at least a view").c_str());
    if (depth->numFrames < 0 || (P > 0 && depth->numFrames > 0 && !depth->pixels))
        return fail(ctx, PS_ERR_BAD_ARG, msg(": depth set: numFrames < 0 or null pixels").c_str());
    for (int i = 0; i < 5; ++i) a.dist.k[i] = g->dist5[i];
    a.dist.fx = g->K[0];
    a.dist.fy = g->K[4];
    a.dist.cx = g->K[2];
    a.dist.cy = g->K[5];
    a.scale = g->depthImageScale;
    a.depth = reinterpret_cast<const uint8_t *>(depth->pixels);
    a.rows = depth->rows;
    a.cols = depth->cols;
    a.numFrames = depth->numFrames;
    a.cap = capacity;
    return PS_OK;
}

int tracked_launch(PsContext *ctx, const TrackedArgs &a, const float *nextPts, const int32_t *keptIdx, const int32_t *numKept, int P,
                   const PsTrackedCarry *carry, const PsTrackedRows &out)
{
    hipLaunchKernelGGL(ps_assemble_tracked_rows, rows_grid(P, a.cap), dim3(kBlock), 0, ctx->stream, a, reinterpret_cast<const float2 *>(nextPts),
                       keptIdx, numKept, carry ? *carry : PsTrackedCarry{}, out);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_point_sets(void) { return sizeof(PsPointSets); }
size_t ps_abi_sizeof_tracked_carry(void) { return sizeof(PsTrackedCarry); }
size_t ps_abi_sizeof_tracked_rows(void) { return sizeof(PsTrackedRows); }
size_t ps_abi_sizeof_track_vo_params(void) { return sizeof(PsTrackVoParams); }
size_t ps_abi_sizeof_track_vo_in(void) { return sizeof(PsTrackVoIn); }
size_t ps_abi_sizeof_track_vo_out(void) { return sizeof(PsTrackVoOut); }

int ps_ransac_match_lists(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K, const PsPointSets *prev,
                          const PsPointSets *cur, const int32_t *pairs, const PsDMatch *matches, const int32_t *numMatches, int P, int cap,
                          const PsPairResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (P < 0 || !out || !prev || !cur || !params || !cfg) return fail(ctx, PS_ERR_BAD_ARG, "ps_ransac_match_lists: null argument or P < 0");
    if (P == 0) return PS_OK;
    MatchListsCall c;
    rc = match_lists_check(ctx, params, cfg, K, prev, cur, matches, numMatches, cap, out->inlierMask, out->pose, out->stats, c);
    if (rc) return rc;
    begin_timed_call(ctx);
    HandoffGuard handoffGuard{ctx}; // (prepare_score may already queue a clearing: the guard stands before it)
    rc = match_lists_prepare(ctx, c, matches, P, cap);
    if (rc) return rc;
    return match_lists_launch(ctx, c, pairs, matches, numMatches, P, cap, out->inlierMask, out->pose, out->stats);
}

int ps_assemble_tracked(PsContext *ctx, const PsFrameGeometry *geometry, const PsDepthSet *depth, const int32_t *depthFrame,
                        const float *nextPts, const int32_t *keptIdx, const int32_t *numKept, int P, int capacity,
                        const PsTrackedCarry *carry, const PsTrackedRows *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TrackedArgs a{};
    rc = tracked_check(ctx, geometry, depth, P, capacity, carry, out, "ps_assemble_tracked", a);
    if (rc) return rc;
    if (P == 0) return PS_OK;
    if (!depthFrame || !nextPts || !keptIdx || !numKept) return fail(ctx, PS_ERR_BAD_ARG, "ps_assemble_tracked: null array");
    a.frame = depthFrame;
    a.frameStep = 1;
    a.frameOff = 0;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return tracked_launch(ctx, a, nextPts, keptIdx, numKept, P, carry, *out);
}

int ps_track_vo_pairs(PsContext *ctx, const PsKltPyramids *pyr, const PsKltParams *klt, const PsTrackVoParams *tp,
                      const PsRansacParams *params, const PsRansacConfig *cfg, const PsFrameGeometry *geometry, const PsDepthSet *depth,
                      const PsTrackVoIn *in, int P, int capacity, const PsTrackVoOut *out)
{
    static const char *who = "ps_track_vo_pairs";
    int rc = bind(ctx);
    if (rc) return rc;
    if (!tp || !in || !out || !params || !cfg || P < 0) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pairs: null argument or P < 0");
    if (tp->removeTooCloseFeatures != 0)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_vo_pairs: removeTooCloseFeatures is not restated -- the reference leaves the matches' "
                                             "trainIdx un-renumbered after erasing features (matcher.cpp:960-963); run ps_exclude_device instead");
    if (const char *why = klt_params_error(klt)) return fail(ctx, PS_ERR_BAD_ARG, why);
    if (!pyr || pyr->device != ctx->device || klt->winSize != pyr->W)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pairs: null or foreign pyramid set, or a winSize other than the set's");
    TrackedArgs a{};
    rc = tracked_check(ctx, geometry, depth, P, capacity, &in->prev, &out->rows, who, a);
    if (rc) return rc;
    if (P == 0) return PS_OK;
    if (!in->pairs || !in->prevXY || !in->prevPts || !in->prevCounts || !out->nextPts || !out->status || !out->err || !out->matches ||
        !out->numMatches || !out->keptIdx)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pairs: null array");
    const PsPointSets prev{in->prevPts, in->prevCounts, P, capacity, 0}, cur{out->rows.pts, out->rows.counts, P, capacity, 0};
    MatchListsCall c;
    rc = match_lists_check(ctx, params, cfg, geometry->K, &prev, &cur, out->matches, out->numMatches, capacity, out->inlierMask, out->pose,
                           out->stats, c);
    if (rc) return rc;
    if ((long long)P * (long long)capacity > (long long)INT_MAX)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_vo_pairs: pairs x capacity beyond 2^31");
    a.frame = in->depthFrame ? in->depthFrame : in->pairs;
    a.frameStep = in->depthFrame ? 1 : 2;
    a.frameOff = in->depthFrame ? 0 : 1;
    begin_timed_call(ctx);
    HandoffGuard handoffGuard{ctx};
    // what the estimator can refuse (a batch too long to score completely, an allocation) is found before the first launch: an error
    // leaves the outputs untouched
    rc = match_lists_prepare(ctx, c, out->matches, P, capacity);
    if (rc) return rc;
    rc = klt_track_launch(ctx, pyr, *klt, in->pairs, in->prevXY, in->prevCounts, P, capacity, out->nextPts, out->status, out->err);
    if (rc) return rc;
    rc = klt_select_launch(ctx, out->nextPts, out->status, out->err, in->prevCounts, P, capacity, tp->trackingErrorThreshold,
                           tp->minimalReprojDistanceNewTrackingFeatures, out->matches, out->numMatches, out->rows.xy, out->keptIdx);
    if (rc) return rc;
    rc = tracked_launch(ctx, a, out->nextPts, out->keptIdx, out->numMatches, P, &in->prev, out->rows);
    if (rc) return rc;
    return match_lists_launch(ctx, c, nullptr, out->matches, out->numMatches, P, capacity, out->inlierMask, out->pose, out->stats);
}

int ps_track_vo_pair(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, const uint16_t *depth, int rows, int cols, int channels,
                     size_t rowStride, size_t depthStep, const PsKltParams *klt, const PsTrackVoParams *tp, const PsRansacParams *params,
                     const PsRansacConfig *cfg, const PsFrameGeometry *geometry, const PsTrackVoIn *in, int n, const PsTrackVoOut *out,
                     int *numKept)
{
    static const char *who = "ps_track_vo_pair";
    int rc = bind(ctx);
    if (rc) return rc;
    if (const char *why = klt_params_error(klt)) return fail(ctx, PS_ERR_BAD_ARG, why);
    rc = klt_shape_error(ctx, rows, cols, channels, klt->winSize, klt->maxLevels, who);
    if (rc) return rc;
    rowStride = image_row_stride(cols, channels, rowStride);
    if (!prevImg || !nextImg || !depth || !in || !out || !numKept || !tp || rowStride == 0 || n < 0 || !out->pose || !out->stats ||
        (n > 0 && (!in->prevXY || !in->prevPts || !out->nextPts || !out->matches || !out->keptIdx || !out->inlierMask)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pair: null array, negative count or a row stride below a row");
    if (n > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_vo_pair: more than PS_MAX_KPTS points");
    // what the device form would refuse, before anything is allocated or uploaded
    if (!params || !cfg || !geometry) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pair: null params, config or geometry");
    if (tp->removeTooCloseFeatures != 0)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_vo_pair: removeTooCloseFeatures is not restated -- the reference leaves the matches' "
                                             "trainIdx un-renumbered after erasing features (matcher.cpp:960-963); run ps_exclude instead");
    {
        Plan probe;
        rc = make_plan(ctx, params, cfg, geometry->K, n > 0 ? n : 1, n > 0 ? n : 1, probe); // (usedPairs, numHypotheses, the estimator)
        if (rc) return rc;
    }
    if (cfg && cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pair: explicit sample streams are ps_ransac_rigid3d's");
    const PsTrackedCarry &pc = in->prev;
    const PsTrackedRows &orow = out->rows;
    if (n > 0 && ((orow.angle && !pc.angle) || (orow.response && !pc.response) || (orow.octave && !pc.octave) || (orow.detDist && !pc.detDist)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pair: a carried column is wanted without its previous rows");
    PsDepthSet ds{};
    ds.pixels = depth; // (the host array: checked for NULL only; the device copy is named below)
    ds.rowStride = depthStep;
    ds.numFrames = 1;
    ds.rows = rows;
    ds.cols = cols;
    size_t dRow = 0, dFrame = 0, dView = 0;
    if (!depth_set_strides(ds, dRow, dFrame, dView)) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_vo_pair: an odd depth step or one below a row");
    TimingOff toff(ctx);
    PsKltPyramids *pyr = nullptr;
    rc = ps_klt_pyramids_create(ctx, rows, cols, channels, klt->winSize, klt->maxLevels, 2, &pyr);
    if (rc) return rc;
    const HandleOwner<PsKltPyramids> own(pyr, ps_klt_pyramids_destroy);
    const size_t imgBytes = image_bytes(rows, cols, channels, rowStride), N = (size_t)(n > 0 ? n : 1);
    // one block: two images | the depth view | pairs[2], count, depth frame | the previous rows | everything PsTrackVoOut names
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes, 16); // (the previous image, at 0)
    const size_t oImg1 = lay.take<uint8_t>(imgBytes, 16), oDepth = lay.take<uint16_t>(dView / 2, 16), oHead = lay.take<int32_t>(4, 16),
                 oPrevXY = lay.take<float2>(N), oPrevPts = lay.take<float>(3 * N), oPAng = lay.take<float>(N), oPResp = lay.take<float>(N),
                 oPOct = lay.take<int32_t>(N), oPDist = lay.take<double>(N);
    const size_t oNext = lay.take<float2>(N, 16), oErr = lay.take<float>(N), oNum = lay.take<int32_t>(1), oMatches = lay.take<PsDMatch>(N, 8),
                 oKeptIdx = lay.take<int32_t>(N), oXy = lay.take<float2>(N), oUn = lay.take<float2>(N), oPts = lay.take<float>(3 * N),
                 oCount = lay.take<int32_t>(1), oAng = lay.take<float>(N), oResp = lay.take<float>(N), oOct = lay.take<int32_t>(N),
                 oDist = lay.take<double>(N), oPose = lay.take<float>(16), oStats = lay.take<PsRansacStats>(1, 8),
                 oMask = lay.take<uint8_t>(N), oStatus = lay.take<uint8_t>(N), total = lay.total;
    const DeviceBlock blk(total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    const int32_t head[4] = {0, 1, n, 0};
    PS_HIP(hipMemcpyAsync(d, prevImg, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oImg1, nextImg, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oDepth, depth, dView, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oHead, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    const auto up = [&](size_t off, const void *from, size_t bytes) {
        return (from && n > 0) ? hipMemcpyAsync(d + off, from, (size_t)n * bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
    };
    PS_HIP(up(oPrevXY, in->prevXY, 8));
    PS_HIP(up(oPrevPts, in->prevPts, 12));
    PS_HIP(up(oPAng, pc.angle, 4));
    PS_HIP(up(oPResp, pc.response, 4));
    PS_HIP(up(oPOct, pc.octave, 4));
    PS_HIP(up(oPDist, pc.detDist, 8));
    if (klt->flags & PS_KLT_USE_INITIAL_FLOW) PS_HIP(up(oNext, out->nextPts, 8));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (head[] and pageable sources leave scope / may change)
    rc = klt_build_launch(ctx, pyr, (const uint8_t *)d, rowStride, oImg1, 2, 0);
    if (rc) return rc;
    PsTrackVoIn din{};
    din.pairs = (const int32_t *)(d + oHead);
    din.depthFrame = (const int32_t *)(d + oHead) + 3;
    din.prevXY = (const float *)(d + oPrevXY);
    din.prevPts = (const float *)(d + oPrevPts);
    din.prevCounts = (const int32_t *)(d + oHead) + 2;
    din.prev.angle = pc.angle ? (const float *)(d + oPAng) : nullptr;
    din.prev.response = pc.response ? (const float *)(d + oPResp) : nullptr;
    din.prev.octave = pc.octave ? (const int32_t *)(d + oPOct) : nullptr;
    din.prev.detDist = pc.detDist ? (const double *)(d + oPDist) : nullptr;
    PsTrackVoOut dout{};
    dout.nextPts = (float *)(d + oNext);
    dout.status = (uint8_t *)(d + oStatus);
    dout.err = (float *)(d + oErr);
    dout.matches = (PsDMatch *)(d + oMatches);
    dout.numMatches = (int32_t *)(d + oNum);
    dout.keptIdx = (int32_t *)(d + oKeptIdx);
    dout.rows.xy = (float *)(d + oXy);
    dout.rows.xyUndist = (float *)(d + oUn);
    dout.rows.pts = (float *)(d + oPts);
    dout.rows.counts = (int32_t *)(d + oCount);
    dout.rows.angle = pc.angle ? (float *)(d + oAng) : nullptr;
    dout.rows.response = pc.response ? (float *)(d + oResp) : nullptr;
    dout.rows.octave = pc.octave ? (int32_t *)(d + oOct) : nullptr;
    dout.rows.detDist = pc.detDist ? (double *)(d + oDist) : nullptr;
    dout.inlierMask = (uint8_t *)(d + oMask);
    dout.pose = (float *)(d + oPose);
    dout.stats = (PsRansacStats *)(d + oStats);
    PsDepthSet dds = ds;
    dds.pixels = (const uint16_t *)(d + oDepth);
    rc = ps_track_vo_pairs(ctx, pyr, klt, tp, params, cfg, geometry, &dds, &din, 1, (int)N, &dout);
    if (rc) return rc;
    std::vector<char> back(total - oNext);
    PS_HIP(hipMemcpyAsync(back.data(), d + oNext, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const auto at = [&](size_t off) { return back.data() + (off - oNext); }; // (the block's offsets, seen from the downloaded part)
    int32_t k = 0;
    std::memcpy(&k, at(oNum), 4);
    if (k < 0 || k > n) return fail(ctx, PS_ERR_HIP, "ps_track_vo_pair: the device returned an impossible count");
    const auto take = [&](void *to, size_t off, size_t bytes, int count) { if (to && count > 0) std::memcpy(to, at(off), (size_t)count * bytes); };
    take(out->nextPts, oNext, 8, n);
    take(out->status, oStatus, 1, n);
    take(out->err, oErr, 4, n);
    take(out->matches, oMatches, 16, k);
    take(out->keptIdx, oKeptIdx, 4, k);
    take(orow.xy, oXy, 8, k);
    take(orow.xyUndist, oUn, 8, k);
    take(orow.pts, oPts, 12, k);
    take(orow.angle, oAng, 4, k);
    take(orow.response, oResp, 4, k);
    take(orow.octave, oOct, 4, k);
    take(orow.detDist, oDist, 8, k);
    take(out->inlierMask, oMask, 1, k);
    take(out->pose, oPose, 4, 16);
    take(out->stats, oStats, sizeof(PsRansacStats), 1);
    if (out->numMatches) *out->numMatches = k;
    if (orow.counts) *orow.counts = k;
    *numKept = k;
    return PS_OK;
}

} // extern "C"
