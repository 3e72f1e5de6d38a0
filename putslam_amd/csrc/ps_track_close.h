// ps_track_close.h -- the second half of the tracking VO step without a host step (include/putslam_hip.h: "Closing the tracking VO
// step"; Matcher::trackKLT, matcher.cpp:213-381): the refill merge with the predicted level of every merged row, the description at
// that level, and the gather of the rows the description kept.  Part of the device translation unit (ps_capi.hip), after
// ps_exclusion.h (the merge predicate), ps_map_view.h (the level rule), ps_orb.h (the description's launches), ps_frame_assembly.h
// (the candidates' launches) and ps_track_vo.h.  DESIGN.md section 8.15.
//
// Shape: four launches on one stream.
//  1. ps_track_merge_rows, one work-group per pair: the candidates pass in tiles of 256, one per thread.  A tile is first swept
//     against the tracked rows and the candidates accepted before it (both staged through LDS 256 at a time: every thread reads
//     every entry), then resolved against itself -- the least undecided candidate of the tile is accepted, every undecided thread
//     near it rejects its own, one barrier a step, at most one step per accepted candidate -- and its accepted candidates are
//     appended to the list in LDS (u16 indices) by a ballot prefix.  Then every merged row is copied out with its level.
//  2. + 3. ps_orb_place and ps_orb_describe (ps_orb.h) on the merged rows with the level as octave.
//  4. ps_close_tracked_rows, one thread per output row: the gather by keptIdx.
#pragma once

namespace psdev {

constexpr int kTcBlock = 256;
constexpr int kTcWaves = kTcBlock / 64;
static_assert(PS_EXCL_MAX_CAND <= 0xFFFF, "u16 indices of the accepted candidates");

// the columns of a block of rows, read only: a pair's (a frame's) rows lie `cap` apart
struct TcRowsIn {
    const float2 *xy, *un;
    const float *pts, *angle, *response;
    const int32_t *octave;
    const double *detDist;
    const int32_t *counts;
    int cap;
};
// ... and of a block that is written; level / src: the handle's merged block only
struct TcRowsOut {
    float2 *xy, *un;
    float *pts, *angle, *response;
    int32_t *octave;
    double *detDist;
    int32_t *level, *src, *counts;
    int cap;
};

struct TcShared {
    float2 tile[kTcBlock]; // 256 positions of the set a tile is swept against
    float2 own[kTcBlock];  // the tile's own positions
    int mins[2][kTcWaves];
    int wsum[kTcWaves];
};

PS_D ExPt tc_point(float2 q) { return ExPt{0.f, 0.f, 0.f, q.x, q.y}; }

// thread `tid`'s candidate `a` against entries 0 .. lim-1 of the staged tile
PS_D bool tc_sweep_tile(const PsExclusionRule &rule, const TcShared &sh, int lim, const ExPt &a)
{
    bool hit = false;
    for (int kk = 0; kk < lim; ++kk) hit = hit || ex_near(rule, tc_point(sh.tile[kk]), a);
    return hit;
}

// merged row `to` from row `s` of `r`, with its predicted level: curDist is matcher.cpp:287-290 as compiled -- float products,
// float sums left to right, the float root, widened (ps_assemble_rows' detDist arithmetic, not Vector3f::norm's order)
PS_D void tc_emit(const TcRowsIn &r, size_t s, const LevelBlock *__restrict__ levels, const TcRowsOut &m, size_t to, int src)
{
    const float x = r.pts[3 * s], y = r.pts[3 * s + 1], z = r.pts[3 * s + 2];
    const int oc = r.octave[s];
    const double dd = r.detDist[s];
    const float cur = ps_sqrt((x * x + y * y) + z * z);
    m.xy[to] = r.xy[s];
    m.un[to] = r.un[s];
    m.pts[3 * to] = x;
    m.pts[3 * to + 1] = y;
    m.pts[3 * to + 2] = z;
    m.angle[to] = r.angle[s];
    m.response[to] = r.response[s];
    m.octave[to] = oc;
    m.detDist[to] = dd;
    m.level[to] = level_octave_ok(oc) ? level_rule(levels, oc, dd, (double)cur) : -1;
    m.src[to] = src;
}

// One work-group per pair: mergeTrackedFeatures (matcher.cpp:97-130) where the refill is due and candidates are given, then the
// predicted level (:281-301) of every merged row.  acc[]: dynamic LDS, c.cap u16 -- the accepted candidates in order.
__global__ __launch_bounds__(kTcBlock) void ps_track_merge_rows(PsExclusionRule rule, int minimalTracked, TcRowsIn t, TcRowsIn c, int candFrames,
                                                                const int32_t *__restrict__ candFrame,
                                                                const LevelBlock *__restrict__ levels, TcRowsOut m,
                                                                int32_t *__restrict__ refill)
{
    extern __shared__ __align__(16) unsigned char tcLds[];
    __shared__ TcShared sh;
    uint16_t *acc = reinterpret_cast<uint16_t *>(tcLds);
    const int p = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = t.counts[p];
    if (n < 0 || n > t.cap) { // (uniform over the work-group, like every branch on n, nc and na below)
        if (tid == 0) m.counts[p] = -1;
        return;
    }
    const bool due = n < minimalTracked;
    const int f = (due && c.counts != nullptr && candFrame != nullptr) ? candFrame[p] : -1;
    const bool has = f >= 0 && f < candFrames;
    const int nc = has ? c.counts[f] : 0;
    if (nc < 0 || nc > c.cap) {
        if (tid == 0) m.counts[p] = -1;
        return;
    }
    if (tid == 0) refill[p] = due ? (has ? 1 : 2) : 0;
    const size_t tb = (size_t)p * (size_t)t.cap, cb = (size_t)(has ? f : 0) * (size_t)c.cap;
    int na = 0, step = 0;
    for (int i0 = 0; i0 < nc; i0 += kTcBlock) {
        const int i = i0 + tid;
        const bool valid = i < nc;
        const float2 q = c.un[cb + (size_t)(valid ? i : i0)];
        const ExPt a = tc_point(q);
        bool blocked = false;
        for (int k0 = 0; k0 < n; k0 += kTcBlock) { // ... against the tracked rows
            if (k0 + tid < n) sh.tile[tid] = t.un[tb + (size_t)(k0 + tid)];
            __syncthreads();
            if (__ballot(valid && !blocked) != 0ull) blocked = blocked || tc_sweep_tile(rule, sh, min(kTcBlock, n - k0), a);
            __syncthreads();
        }
        for (int k0 = 0; k0 < na; k0 += kTcBlock) { // ... against the candidates appended by the tiles before
            if (k0 + tid < na) sh.tile[tid] = c.un[cb + (size_t)acc[k0 + tid]];
            __syncthreads();
            if (__ballot(valid && !blocked) != 0ull) blocked = blocked || tc_sweep_tile(rule, sh, min(kTcBlock, na - k0), a);
            __syncthreads();
        }
        // ... and the tile against itself, greedy in index order
        sh.own[tid] = q;
        bool und = valid && !blocked, accepted = false;
        for (;;) {
            const unsigned long long bc = __ballot(und);
            if (lane == 0) sh.mins[step & 1][w] = bc ? w * 64 + (__ffsll((long long)bc) - 1) : INT_MAX;
            __syncthreads();
            int seed = INT_MAX;
#pragma unroll
            for (int k = 0; k < kTcWaves; ++k) seed = min(seed, sh.mins[step & 1][k]);
            ++step; // (the other half of mins[] is written next: no second barrier)
            if (seed == INT_MAX) break;
            if (tid == seed) {
                accepted = true;
                und = false;
            } else if (und && ex_near(rule, tc_point(sh.own[seed]), a)) {
                und = false;
            }
        }
        const unsigned long long bk = __ballot(accepted);
        if (lane == 0) sh.wsum[w] = __popcll(bk);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < kTcWaves; ++k) {
            before += k < w ? sh.wsum[k] : 0;
            tot += sh.wsum[k];
        }
        if (accepted) acc[na + before + __popcll(bk & ((1ull << lane) - 1ull))] = (uint16_t)i;
        na += tot;
        __syncthreads(); // (acc[], and own[] / wsum[] free for the next tile)
    }
    const int total = n + na; // (at most t.cap + c.cap, which the host holds to m.cap)
    const size_t mb = (size_t)p * (size_t)m.cap;
    for (int j = tid; j < total; j += kTcBlock) {
        if (j < n) {
            tc_emit(t, tb + (size_t)j, levels, m, mb + (size_t)j, j);
        } else {
            const int i = (int)acc[j - n];
            tc_emit(c, cb + (size_t)i, levels, m, mb + (size_t)j, t.cap + i);
        }
    }
    if (tid == 0) m.counts[p] = total;
}

// Output row j < numKept[p] of pair p is merged row keptIdx[p][j] (ps_orb_place's: always a merged row); counts[p] = numKept[p],
// -1 where the pair was refused.  One thread per output row, a grid of row blocks x pairs, no LDS.
__global__ __launch_bounds__(kBlock) void ps_close_tracked_rows(TcRowsOut m, const int32_t *__restrict__ keptIdx,
                                                                const int32_t *__restrict__ numKept, TcRowsOut o, int32_t *__restrict__ srcIdx)
{
    const int p = (int)blockIdx.y, j = (int)(blockIdx.x * kBlock + threadIdx.x);
    const int n = numKept[p];
    const bool ok = n >= 0 && n <= m.cap;
    if (j == 0) o.counts[p] = ok ? n : -1;
    if (!ok || j >= n) return;
    const size_t base = (size_t)p * (size_t)m.cap, to = base + (size_t)j;
    const int i = keptIdx[to];
    if (i < 0 || i >= m.cap) return;
    const size_t from = base + (size_t)i;
    o.xy[to] = m.xy[from];
    o.un[to] = m.un[from];
    o.pts[3 * to] = m.pts[3 * from];
    o.pts[3 * to + 1] = m.pts[3 * from + 1];
    o.pts[3 * to + 2] = m.pts[3 * from + 2];
    o.angle[to] = m.angle[from];
    o.response[to] = m.response[from];
    o.octave[to] = m.octave[from];
    o.detDist[to] = m.detDist[from];
    srcIdx[to] = m.src[from];
}

} // namespace psdev

// Host side: the handle, the checks, the launches and the entry points
struct PsTrackClose {
    int device = 0;
    int maxPairs = 0, maxRows = 0;
    char *block = nullptr; // every array below
    float *xy = nullptr, *un = nullptr, *pts = nullptr, *angle = nullptr, *response = nullptr;
    double *detDist = nullptr;
    int32_t *octave = nullptr, *level = nullptr, *src = nullptr, *count = nullptr, *keptIdx = nullptr, *numKept = nullptr;
};

namespace {

bool tracked_rows_complete(const PsTrackedRows &r)
{
    return r.xy && r.xyUndist && r.pts && r.counts && r.angle && r.response && r.octave && r.detDist;
}

TcRowsOut tc_rows_out(const PsTrackedRows &r, int cap)
{
    return TcRowsOut{reinterpret_cast<float2 *>(r.xy), reinterpret_cast<float2 *>(r.xyUndist), r.pts, r.angle, r.response, r.octave, r.detDist,
                     nullptr, nullptr, r.counts, cap};
}

enum { kTcPassMerge = 1, kTcPassPlace = 2, kTcPassDescribe = 4, kTcPassClose = 8, kTcPassAll = 15 };

// the checks and the launches of ps_track_close_pairs; passes: which of the four launches are queued (the diagnostic's mask)
int track_close_call(PsContext *ctx, PsTrackClose *tc, const PsOrbPyramids *pyr, const int32_t *slots, const PsTrackCloseParams *tp,
                     const PsTrackedRows *tracked, const PsTrackCandidates *cand, const int32_t *candFrame, int P, int capacity,
                     int outCapacity, const PsTrackCloseOut *out, int passes, const char *who)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!tc || tc->device != ctx->device || !tp || !tracked || !out || P < 0 || P > tc->maxPairs)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pairs: null argument, another device's handle, or P outside 0 .. the handle's maxPairs");
    if (tp->removeTooCloseFeatures != 0)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_close_pairs: removeTooCloseFeatures is not restated -- the reference leaves the matches' "
                                             "trainIdx un-renumbered after erasing features (matcher.cpp:960-963, reached from :274-277 too)");
    if (capacity < 1) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pairs: capacity < 1");
    if (cand && (cand->numFrames < 1 || cand->capacity < 1 || !cand->xy || !cand->xyUndist || !cand->pts || !cand->angle || !cand->response ||
                 !cand->octave || !cand->detDist || !cand->counts || !candFrame))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pairs: candidates need every column, counts, numFrames and capacity >= 1, and candFrame");
    if (cand && cand->capacity > PS_EXCL_MAX_CAND) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_close_pairs: candidate capacity above PS_EXCL_MAX_CAND");
    if (outCapacity > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_close_pairs: outCapacity above PS_MAX_KPTS");
    const long long need = (long long)capacity + (cand ? cand->capacity : 0);
    if ((long long)outCapacity < need || outCapacity > tc->maxRows)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pairs: outCapacity must hold capacity + the candidates' capacity and not exceed the handle's maxRows");
    if (!tracked_rows_complete(*tracked)) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pairs: the tracked rows need every column (the level rule reads octave and detDist, the merge xyUndist)");
    if (!out->desc || !out->srcIdx || !out->refill || !tracked_rows_complete(out->rows))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pairs: desc, srcIdx, refill and every column of the closed rows are required");
    rc = orb_describe_check(ctx, pyr, slots, tc->xy, tc->angle, tc->level, tc->count, P, outCapacity, out->desc, tc->keptIdx, tc->numKept, who);
    if (rc) return rc;
    if (P == 0) return PS_OK;
    PsExclusionRule rule;
    if (ps_exclusion_rule_merge_tracked(tp->minimalReprojDistanceNewTrackingFeatures, &rule) != PS_OK)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pairs: the merge rule");
    TimingOff toff(ctx);
    rc = ensure_level_block(ctx);
    if (rc) return rc;
    const TcRowsIn t{reinterpret_cast<const float2 *>(tracked->xy), reinterpret_cast<const float2 *>(tracked->xyUndist), tracked->pts, tracked->angle,
                     tracked->response, tracked->octave, tracked->detDist, tracked->counts, capacity};
    TcRowsIn c{};
    c.cap = 1;
    if (cand)
        c = TcRowsIn{reinterpret_cast<const float2 *>(cand->xy), reinterpret_cast<const float2 *>(cand->xyUndist), cand->pts, cand->angle,
                     cand->response, cand->octave, cand->detDist, cand->counts, cand->capacity};
    const TcRowsOut m{reinterpret_cast<float2 *>(tc->xy), reinterpret_cast<float2 *>(tc->un), tc->pts, tc->angle, tc->response, tc->octave,
                      tc->detDist, tc->level, tc->src, tc->count, outCapacity};
    HandoffGuard handoffGuard{ctx};
    if (passes & kTcPassMerge)
        hipLaunchKernelGGL(ps_track_merge_rows, dim3((unsigned)P), dim3(kTcBlock), (size_t)c.cap * sizeof(uint16_t), ctx->stream, rule,
                       (int)tp->minimalTrackedFeatures, t, c, cand ? cand->numFrames : 0, cand ? candFrame : (const int32_t *)nullptr,
                       (const LevelBlock *)ctx->levelTab.p, m, out->refill);
    PS_HIP(hipGetLastError());
    rc = orb_describe_launch(ctx, pyr, slots, tc->xy, tc->angle, tc->level, tc->count, P, outCapacity, out->desc, tc->keptIdx, tc->numKept,
                             ((passes & kTcPassPlace) ? kOrbPassPlace : 0) | ((passes & kTcPassDescribe) ? kOrbPassDescribe : 0));
    if (rc) return rc;
    if (passes & kTcPassClose)
        hipLaunchKernelGGL(ps_close_tracked_rows, rows_grid(P, outCapacity), dim3(kBlock), 0, ctx->stream, m, (const int32_t *)tc->keptIdx,
                       (const int32_t *)tc->numKept, tc_rows_out(out->rows, outCapacity), out->srcIdx);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_track_candidates(void) { return sizeof(PsTrackCandidates); }
size_t ps_abi_sizeof_track_close_params(void) { return sizeof(PsTrackCloseParams); }
size_t ps_abi_sizeof_track_close_out(void) { return sizeof(PsTrackCloseOut); }

int ps_track_candidates(PsContext *ctx, PsFrontEnd *fe, const PsImageSet *images, const PsDepthSet *depth, const PsFrameGeometry *geometry,
                        int capacity, const PsFrameRowsOut *out)
{
    static const char *who = "ps_track_candidates";
    int rc = bind(ctx);
    if (rc) return rc;
    if (capacity > PS_DBSCAN_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_candidates: capacity above PS_DBSCAN_MAX_KPTS");
    size_t row = 0, frame = 0;
    rc = check_image_set(ctx, fe, &PsFrontEnd::maxFrames, images, 0, who, row, frame);
    if (rc) return rc;
    AssembleArgs a{};
    rc = assemble_check(ctx, geometry, depth, 0, images->numFrames, out, true, false, who, a);
    if (rc) return rc;
    if (!out->xy || !out->xyUndist || !out->angle || !out->response || !out->octave || !out->detDist)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_candidates: xy, xyUndist, angle, response, octave and detDist are all required");
    if (depth->numFrames != images->numFrames || depth->rows != fe->rows || depth->cols != fe->cols)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_candidates: the depth set's numFrames, rows and cols must be the images'");
    if (capacity < 1 || capacity < fe->need || capacity > fe->rowCap)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_candidates: capacity must hold what a frame can emit and not exceed max(1, maximalTrackedFeatures)");
    const int F = images->numFrames;
    if (F == 0) return PS_OK;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    const OrbDetPlan pl = orbdet_plan(fe->det, fe->params.detect);
    rc = orbdet_launch(ctx, fe->det, images->pixels, row, frame, F, pl, capacity, fe->xy0, fe->resp0, fe->ang0, fe->oct0, fe->cnt0, kOrbDetPassAll);
    if (rc) return rc;
    rc = dbscan_launch(ctx, fe->xy0, fe->oct0, fe->cnt0, 0, F, capacity, fe->params.DBScanEps, kFrontEndMinPts, kFrontEndFromCluster, fe->thinIdx,
                       fe->thinN);
    if (rc) return rc;
    PsFrameRowsOut o = *out; // the key points' own columns are the detector's, gathered by DBScan's keptIdx
    o.angleIn = fe->ang0;
    o.responseIn = fe->resp0;
    o.octaveIn = fe->oct0;
    return assemble_launch(ctx, a, fe->xy0, fe->thinIdx, fe->thinN, F, capacity, o);
}

int ps_track_close_create(PsContext *ctx, int maxPairs, int maxRows, PsTrackClose **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_create: null out");
    *out = nullptr;
    if (maxPairs < 1 || maxPairs > kImageMaxFrames || maxRows < 1)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_create: maxPairs must lie in 1 .. 65535, maxRows at least 1");
    if (maxRows > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_close_create: maxRows above PS_MAX_KPTS");
    HandleOwner<PsTrackClose> own(new PsTrackClose, ps_track_close_destroy);
    PsTrackClose *tc = own.get();
    tc->device = ctx->device;
    tc->maxPairs = maxPairs;
    tc->maxRows = maxRows;
    const size_t Pm = (size_t)maxPairs, N = Pm * (size_t)maxRows;
    BlockLayout lay;
    const size_t oDist = lay.take<double>(N, 16), oXy = lay.take<float2>(N, 16), oUn = lay.take<float2>(N, 16), oPts = lay.take<float>(3 * N, 16),
                 oAng = lay.take<float>(N, 16), oResp = lay.take<float>(N, 16), oOct = lay.take<int32_t>(N, 16), oLev = lay.take<int32_t>(N, 16),
                 oSrc = lay.take<int32_t>(N, 16), oKept = lay.take<int32_t>(N, 16), oCount = lay.take<int32_t>(Pm, 16),
                 oNumKept = lay.take<int32_t>(Pm, 16);
    hipError_t e = hipMalloc((void **)&tc->block, lay.total);
    if (e == hipSuccess) e = hipMemset(tc->block, 0, lay.total);
    if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_track_close_create: hipMalloc", e);
    char *b = tc->block;
    tc->detDist = (double *)(b + oDist), tc->xy = (float *)(b + oXy), tc->un = (float *)(b + oUn), tc->pts = (float *)(b + oPts);
    tc->angle = (float *)(b + oAng), tc->response = (float *)(b + oResp), tc->octave = (int32_t *)(b + oOct), tc->level = (int32_t *)(b + oLev);
    tc->src = (int32_t *)(b + oSrc), tc->keptIdx = (int32_t *)(b + oKept), tc->count = (int32_t *)(b + oCount);
    tc->numKept = (int32_t *)(b + oNumKept);
    *out = own.release();
    return PS_OK;
}

void ps_track_close_destroy(PsTrackClose *tc)
{
    if (!tc) return;
    (void)hipSetDevice(tc->device);
    if (tc->block) (void)hipFree(tc->block); // (hipFree waits for the device: queued work that uses the handle has finished)
    delete tc;
}

int ps_track_close_pairs(PsContext *ctx, PsTrackClose *tc, const PsOrbPyramids *pyr, const int32_t *slots, const PsTrackCloseParams *tp,
                         const PsTrackedRows *tracked, const PsTrackCandidates *cand, const int32_t *candFrame, int P, int capacity,
                         int outCapacity, const PsTrackCloseOut *out)
{
    return track_close_call(ctx, tc, pyr, slots, tp, tracked, cand, candFrame, P, capacity, outCapacity, out, kTcPassAll, "ps_track_close_pairs");
}

int ps_debug_track_close_passes(PsContext *ctx, PsTrackClose *tc, const PsOrbPyramids *pyr, const int32_t *slots, const PsTrackCloseParams *tp,
                                const PsTrackedRows *tracked, const PsTrackCandidates *cand, const int32_t *candFrame, int P, int capacity,
                                int outCapacity, const PsTrackCloseOut *out, int passes)
{
    return track_close_call(ctx, tc, pyr, slots, tp, tracked, cand, candFrame, P, capacity, outCapacity, out, passes, "ps_debug_track_close_passes");
}

int ps_track_close_pair(PsContext *ctx, const uint8_t *img, const uint16_t *depth, int rows, int cols, int channels, size_t rowStride,
                        size_t depthStep, const PsFrontEndParams *params, const int8_t *pattern1024, const PsFrameGeometry *geometry,
                        const PsTrackCloseParams *tp, const PsTrackedRows *tracked, int n, uint8_t *desc, const PsTrackedRows *out,
                        int32_t *srcIdx, int cap, int *nout, int *refill)
{
    static const char *who = "ps_track_close_pair";
    int rc = bind(ctx);
    if (rc) return rc;
    rc = image_shape_error(ctx, rows, cols, channels, who);
    if (rc) return rc;
    rowStride = image_row_stride(cols, channels, rowStride);
    if (!img || !depth || !geometry || !tp || !tracked || !out || !nout || !refill || rowStride == 0 || n < 0 || cap < 0 ||
        (n > 0 && (!tracked->xy || !tracked->xyUndist || !tracked->pts || !tracked->angle || !tracked->response || !tracked->octave ||
                   !tracked->detDist)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pair: null argument, negative count or cap, a row stride below a row, or a tracked column absent");
    if (n > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_close_pair: more than PS_MAX_KPTS rows");
    if (tp->removeTooCloseFeatures != 0)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_close_pair: removeTooCloseFeatures is not restated (ps_track_close_pairs)");
    PsDepthSet ds{};
    ds.pixels = depth; // (the host array: checked for NULL only; the device copy is named below)
    ds.rowStride = depthStep;
    ds.numFrames = 1;
    ds.rows = rows;
    ds.cols = cols;
    size_t dRow = 0, dFrame = 0, dView = 0;
    if (!depth_set_strides(ds, dRow, dFrame, dView)) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pair: an odd depth step or one below a row");
    TimingOff toff(ctx);
    PsFrontEnd *fe = nullptr; // (the detector for the sandbox, and the pyramids the rows are described in)
    rc = ps_front_end_create(ctx, rows, cols, channels, params, pattern1024, 1, &fe);
    if (rc) return rc;
    const HandleOwner<PsFrontEnd> own(fe, ps_front_end_destroy);
    const bool due = n < tp->minimalTrackedFeatures; // (the device decides the same from the count it is given)
    const size_t N = (size_t)(n > 0 ? n : 1), room = (size_t)(fe->need > 1 ? fe->need : 1), M = N + (due ? room : 0);
    if (M > (size_t)PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_track_close_pair: rows + candidates above PS_MAX_KPTS");
    PsTrackClose *tc = nullptr;
    rc = ps_track_close_create(ctx, 1, (int)M, &tc);
    if (rc) return rc;
    const HandleOwner<PsTrackClose> ownTc(tc, ps_track_close_destroy);
    const size_t imgBytes = image_bytes(rows, cols, channels, rowStride);
    // one block: the image | the depth view | slot, count, candFrame | the tracked rows | the candidates | everything PsTrackCloseOut names
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes, 16);
    const size_t oDepth = lay.take<uint16_t>(dView / 2, 16), oHead = lay.take<int32_t>(4, 16), oTDist = lay.take<double>(N), oTXy = lay.take<float2>(N),
                 oTUn = lay.take<float2>(N), oTPts = lay.take<float>(3 * N), oTAng = lay.take<float>(N), oTResp = lay.take<float>(N),
                 oTOct = lay.take<int32_t>(N), oCDist = lay.take<double>(room), oCXy = lay.take<float2>(room), oCUn = lay.take<float2>(room),
                 oCPts = lay.take<float>(3 * room), oCAng = lay.take<float>(room), oCResp = lay.take<float>(room), oCOct = lay.take<int32_t>(room),
                 oCN = lay.take<int32_t>(1);
    const size_t oCount = lay.take<int32_t>(2, 16), oDist = lay.take<double>(M), oXy = lay.take<float2>(M), oUn = lay.take<float2>(M),
                 oPts = lay.take<float>(3 * M), oAng = lay.take<float>(M), oResp = lay.take<float>(M), oOct = lay.take<int32_t>(M),
                 oSrc = lay.take<int32_t>(M), oDesc = lay.take<uint8_t>(32 * M, 16), total = lay.total;
    const DeviceBlock blk(total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    const int32_t head[4] = {0, n, 0, 0};
    PS_HIP(hipMemcpyAsync(d, img, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oDepth, depth, dView, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oHead, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    const auto up = [&](size_t off, const void *from, size_t bytes) {
        return n > 0 ? hipMemcpyAsync(d + off, from, (size_t)n * bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
    };
    PS_HIP(up(oTXy, tracked->xy, 8));
    PS_HIP(up(oTUn, tracked->xyUndist, 8));
    PS_HIP(up(oTPts, tracked->pts, 12));
    PS_HIP(up(oTAng, tracked->angle, 4));
    PS_HIP(up(oTResp, tracked->response, 4));
    PS_HIP(up(oTOct, tracked->octave, 4));
    PS_HIP(up(oTDist, tracked->detDist, 8));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (head[] and pageable sources leave scope / may change)
    PsImageSet is{};
    is.pixels = (const uint8_t *)d;
    is.rowStride = rowStride;
    is.numFrames = 1;
    is.rows = rows;
    is.cols = cols;
    is.channels = channels;
    PsDepthSet dds = ds;
    dds.pixels = (const uint16_t *)(d + oDepth);
    PsTrackCandidates cs{};
    if (due) {
        PsFrameRowsOut co{};
        co.pts = (float *)(d + oCPts);
        co.nkpts = (int32_t *)(d + oCN);
        co.xy = (float *)(d + oCXy);
        co.xyUndist = (float *)(d + oCUn);
        co.angle = (float *)(d + oCAng);
        co.response = (float *)(d + oCResp);
        co.octave = (int32_t *)(d + oCOct);
        co.detDist = (double *)(d + oCDist);
        rc = ps_track_candidates(ctx, fe, &is, &dds, geometry, (int)room, &co);
        if (rc) return rc;
        cs = PsTrackCandidates{co.xy, co.xyUndist, co.pts, co.angle, co.response, co.octave, co.detDist, co.nkpts, 1, (int32_t)room};
    }
    rc = ps_orb_pyramids_build_device(ctx, fe->pyr, &is, 0);
    if (rc) return rc;
    const int32_t *dhead = (const int32_t *)(d + oHead);
    const PsTrackedRows dt{(float *)(d + oTXy), (float *)(d + oTUn), (float *)(d + oTPts), (int32_t *)(d + oHead) + 1, (float *)(d + oTAng),
                           (float *)(d + oTResp), (int32_t *)(d + oTOct), (double *)(d + oTDist)};
    PsTrackCloseOut dout{};
    dout.desc = (uint8_t *)(d + oDesc);
    dout.rows = PsTrackedRows{(float *)(d + oXy), (float *)(d + oUn), (float *)(d + oPts), (int32_t *)(d + oCount), (float *)(d + oAng),
                              (float *)(d + oResp), (int32_t *)(d + oOct), (double *)(d + oDist)};
    dout.srcIdx = (int32_t *)(d + oSrc);
    dout.refill = (int32_t *)(d + oCount) + 1;
    rc = ps_track_close_pairs(ctx, tc, fe->pyr, dhead, tp, &dt, due ? &cs : nullptr, due ? dhead + 2 : nullptr, 1, (int)N, (int)M, &dout);
    if (rc) return rc;
    std::vector<char> back(total - oCount);
    PS_HIP(hipMemcpyAsync(back.data(), d + oCount, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    int32_t kr[2] = {0, 0};
    std::memcpy(kr, back.data(), 8);
    if (kr[0] < 0 || (size_t)kr[0] > M) return fail(ctx, PS_ERR_HIP, "ps_track_close_pair: the device returned an impossible count");
    *nout = kr[0];
    *refill = kr[1];
    if (kr[0] > cap) return fail(ctx, PS_ERR_BAD_ARG, "ps_track_close_pair: cap is too small (*nout = required)");
    const size_t k = (size_t)kr[0];
    const auto take = [&](void *to, size_t off, size_t bytes) { if (to && k > 0) std::memcpy(to, back.data() + (off - oCount), k * bytes); };
    take(out->xy, oXy, 8);
    take(out->xyUndist, oUn, 8);
    take(out->pts, oPts, 12);
    take(out->angle, oAng, 4);
    take(out->response, oResp, 4);
    take(out->octave, oOct, 4);
    take(out->detDist, oDist, 8);
    take(srcIdx, oSrc, 4);
    take(desc, oDesc, 32);
    if (out->counts) *out->counts = kr[0];
    return PS_OK;
}

} // extern "C"
