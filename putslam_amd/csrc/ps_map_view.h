// ps_map_view.h -- map views built on the device from a feature map that is resident in HBM (ps_map_views_device /
// ps_frame_levels_device, include/putslam_hip.h).  Per view and candidate feature, what the reference's host
// does between getCovisibleFeatures and matchXYZ:
//   FeaturesMap::findNearestFrame (src/Map/featuresMap.cpp:528-563)            the observation with the least viewing angle,
//   PUTSLAM::removeMapFeaturesWithoutGoodObservationAngle (PUTSLAM.cpp:932-950) dropped if that angle is too large,
//   PUTSLAM::moveMapFeaturesToLocalCordinateSystem (PUTSLAM.cpp:28-51)          position in the camera frame + projection,
//   Matcher::matchXYZ (src/Matcher/matcher.cpp:675-692,700-701)                 predicted level, float position, descriptor.
// No device log / pow / acos: the angle of a (historical pose, current pose) pair comes from a host-filled table, the level is a
// count of host-found thresholds x passes (LevelBlock), T[o] = pow(1.2, o) is a host-filled table.  What is left is exact double
// arithmetic (the translation unit is built with -ffp-contract=off; f64 divide and sqrt are correctly rounded), a gather and an
// ordered compaction.
//
// Shape: two launches on one stream, grid V x chunks, one candidate per thread, 256 candidates a chunk (ps_map_sweep / ps_map_emit's).
//   ps_view_select  steps 1 - 3 and the octave check: the kept flags of a chunk as four ballot words and their count.
//   ps_view_emit    sums the chunk counts of its view (the total, and the part before its own chunk: the order does not depend on
//                   which chunk ran first), then evaluates its kept candidates once more -- this time with the level -- and writes
//                   their rows.  The second evaluation re-reads 4 + 8 bytes an observation, mostly from L2; parking the
//                   intermediate results instead would move 60 bytes a candidate slot out and back and size the context's
//                   scratch with V x candidates (4 GiB for 64 views of a 2^20-feature store).
// The view's angle table is staged through LDS when it has at most kViewAngleLds poses (template parameter: no run-time choice
// between an LDS and a global pointer inside the walk, which hipcc has turned into FLAT loads before).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "ps_device_math.h"
#include "ps_glue.h"

namespace psdev {

constexpr int kViewBlock = 256;
constexpr int kViewWaves = kViewBlock / 64;
constexpr int kViewAngleLds = 2048; // poses whose angles are staged: 16 KiB
constexpr int kLevelOctaves = PS_LEVEL_OCTAVE_MAX - PS_LEVEL_OCTAVE_MIN + 1;

// the constant block the context fills once: ps_level_thresholds' t[k], then T[o] = pow(1.2, o)
struct LevelBlock {
    double t[7];
    double pw[kLevelOctaves];
};

PS_D bool level_octave_ok(int octave) { return octave >= PS_LEVEL_OCTAVE_MIN && octave <= PS_LEVEL_OCTAVE_MAX; }

// THE LEVEL RULE (include/putslam_hip.h): x = (T[octave] * detDist) / curDist, level = #{k : x >= t[k]} if x is finite, else 0
PS_D int level_rule(const LevelBlock *__restrict__ lb, int octave, double detDist, double curDist)
{
    const double x = (lb->pw[octave - PS_LEVEL_OCTAVE_MIN] * detDist) / curDist;
    if (!(fabs(x) <= DBL_MAX)) return 0; // NaN, +-inf
    int level = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) level += x >= lb->t[k] ? 1 : 0;
    return level;
}

struct ViewArgs {
    // the store
    const double *pos;
    const int32_t *obsStart, *obsPose;
    const uint4 *obsDesc;
    const int32_t *obsOctave;
    const double *obsDetDist;
    int numFeatures, numObs, numPoses;
    // the request
    const double *camInv, *poseAngle;
    const int32_t *cand, *candCounts;
    double maxAngle, fx, fy, cx, cy, imageW, imageH;
    int slots; // candidate slots per view: candCapacity, or numFeatures when cand is null
    int flags;
    // the outputs
    uint4 *desc;
    float *pts;
    int32_t *nkpts;
    int maxKpts, descStride /* uint4 */, ptsStride /* floats */;
    int32_t *mapLevel, *viewCount, *featIdx, *obsIdx;
    double *posCam, *uv, *angle;
    // scratch
    const LevelBlock *levels;
    int32_t *bad;                // [V], cleared before the launches
    int32_t *chunkCount;         // [V][chunks]
    unsigned long long *keptMask; // [V][chunks][4]
    int chunks;
};

struct ViewRow {
    int obs, level;
    double p0, p1, p2, u, v, angle;
};

// Steps 1 - 4 for feature f of view v (M = the view's camInv, ang = its angle table: LDS if STAGED).  Returns whether the feature
// is emitted; bad is set for a malformed observation range, a pose id outside the table or an emitted feature's octave outside
// the level table.  LEVEL = false leaves out step 4's arithmetic (r.level is not set).
template <bool LEVEL>
PS_D bool view_eval(const ViewArgs &a, const double *__restrict__ M, const double *ang, int f, ViewRow &r, bool &bad)
{
    const int s = a.obsStart[f], e = a.obsStart[f + 1];
    if (s < 0 || e < s || e > a.numObs) {
        bad = true;
        return false;
    }
    double best = 10.0; // featuresMap.cpp:537
    int chosen = -1;
    for (int o = s; o < e; ++o) {
        const int q = a.obsPose[o];
        if (q < 0 || q >= a.numPoses) {
            bad = true;
            continue;
        }
        const double an = ang[q];
        if (an < best) { // :552 (strict; a NaN is never chosen)
            best = an;
            chosen = o;
        }
    }
    if (chosen < 0 || best > a.maxAngle) return false; // :558-561, PUTSLAM.cpp:940
    const double x = a.pos[3 * (size_t)f], y = a.pos[3 * (size_t)f + 1], z = a.pos[3 * (size_t)f + 2];
    r.p0 = ((M[0] * x + M[4] * y) + M[8] * z) + M[12]; // PUTSLAM.cpp:38-40
    r.p1 = ((M[1] * x + M[5] * y) + M[9] * z) + M[13];
    r.p2 = ((M[2] * x + M[6] * y) + M[10] * z) + M[14];
    double u = ((a.fx * r.p0) / r.p2) + a.cx, v = ((a.fy * r.p1) / r.p2) + a.cy; // depthSensorModel.cpp:20
    if (u < 0 || u > a.imageW || v < 0 || v > a.imageH || r.p2 < 0.8 || r.p2 > 6.0) u = v = -1.0; // :21-23
    if ((a.flags & PS_VIEW_REQUIRE_VISIBLE) && u == -1.0) return false; // featuresMap.cpp:474
    r.u = u;
    r.v = v;
    r.obs = chosen;
    r.angle = best;
    const int octave = a.obsOctave[chosen];
    if (!level_octave_ok(octave)) {
        bad = true;
        return true;
    }
    if (LEVEL) {
        const double curDist = sqrt((r.p0 * r.p0 + r.p1 * r.p1) + r.p2 * r.p2); // matcher.cpp:685-687
        r.level = level_rule(a.levels, octave, a.obsDetDist[chosen], curDist);
    }
    return true;
}

// candidates of view v: -1 for a count outside 0 .. slots
PS_D int view_candidates(const ViewArgs &a, int v)
{
    const int n = a.cand ? a.candCounts[v] : a.numFeatures;
    return (n < 0 || n > a.slots) ? -1 : n;
}

template <bool STAGED> PS_D const double *view_stage_angles(const ViewArgs &a, int v, double *sAng)
{
    const double *__restrict__ g = a.poseAngle + (size_t)v * a.numPoses;
    if (!STAGED) return g;
    for (int q = (int)threadIdx.x; q < a.numPoses; q += kViewBlock) sAng[q] = g[q];
    __syncthreads();
    return sAng;
}

template <bool STAGED> __global__ __launch_bounds__(kViewBlock) void ps_view_select(ViewArgs a)
{
    __shared__ double sAng[STAGED ? kViewAngleLds : 1];
    __shared__ int sCnt[kViewWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int v = (int)blockIdx.x / a.chunks, c = (int)blockIdx.x - v * a.chunks;
    const size_t blk = (size_t)v * a.chunks + c;
    const int n = view_candidates(a, v);
    const int i0 = c * kViewBlock;
    if (n < 0 || i0 >= n) { // (the whole work-group)
        if (tid == 0) {
            a.chunkCount[blk] = 0;
            if (n < 0 && c == 0) a.bad[v] = 1;
        }
        return;
    }
    const double *ang = view_stage_angles<STAGED>(a, v, sAng);
    const double *__restrict__ M = a.camInv + (size_t)v * 16;
    const int i = i0 + tid;
    bool keep = false, bad = false;
    if (i < n) {
        const int f = a.cand ? a.cand[(size_t)v * a.slots + i] : i;
        if (f < 0 || f >= a.numFeatures) {
            bad = true;
        } else {
            ViewRow r;
            keep = view_eval<false>(a, M, ang, f, r, bad);
        }
    }
    const unsigned long long bk = __ballot(keep);
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&a.bad[v], 1);
    if (lane == 0) {
        a.keptMask[blk * kViewWaves + w] = bk;
        sCnt[w] = __popcll(bk);
    }
    __syncthreads();
    if (tid == 0) a.chunkCount[blk] = (sCnt[0] + sCnt[1]) + (sCnt[2] + sCnt[3]);
}

// DESC = false (the float-row store, ps_map_store_f32.h): the row's 32 descriptor bytes are left out -- obsIdx, which is then
// always given, names the observation and ps_gather_rows_f32 copies its row afterwards.
template <bool STAGED, bool DESC = true> __global__ __launch_bounds__(kViewBlock) void ps_view_emit(ViewArgs a)
{
    __shared__ double sAng[STAGED ? kViewAngleLds : 1];
    __shared__ int sPre[kViewWaves], sTot[kViewWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int v = (int)blockIdx.x / a.chunks, c = (int)blockIdx.x - v * a.chunks;
    const size_t blk = (size_t)v * a.chunks + c;
    const int n = view_candidates(a, v);
    const bool invalid = n < 0 || a.bad[v] != 0;
    // the view's count, and the part of it in the chunks before this one
    int pre = 0, tot = 0;
    if (!invalid) {
        const int32_t *__restrict__ cc = a.chunkCount + (size_t)v * a.chunks;
        const int used = (n + kViewBlock - 1) / kViewBlock; // (later chunks hold zeros)
        for (int k = tid; k < used; k += kViewBlock) {
            const int x = cc[k];
            tot += x;
            pre += k < c ? x : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            pre += __shfl_down(pre, o, 64);
            tot += __shfl_down(tot, o, 64);
        }
        if (lane == 0) {
            sPre[w] = pre;
            sTot[w] = tot;
        }
        __syncthreads();
        pre = (sPre[0] + sPre[1]) + (sPre[2] + sPre[3]);
        tot = (sTot[0] + sTot[1]) + (sTot[2] + sTot[3]);
    }
    const bool over = tot > a.maxKpts;
    if (c == 0 && tid == 0) {
        a.viewCount[v] = invalid ? INT_MIN : (over ? -tot : tot);
        a.nkpts[v] = (invalid || over) ? 0 : tot;
    }
    const int i0 = c * kViewBlock;
    if (invalid || over || i0 >= n) return; // (the whole work-group)
    const double *ang = view_stage_angles<STAGED>(a, v, sAng);
    const double *__restrict__ M = a.camInv + (size_t)v * 16;
    const unsigned long long *__restrict__ km = a.keptMask + blk * kViewWaves;
    int row = pre;
    for (int k = 0; k < w; ++k) row += __popcll(km[k]);
    const unsigned long long mine = km[w];
    if (!((mine >> lane) & 1ull)) return;
    row += __popcll(mine & ((1ull << lane) - 1ull));
    const int i = i0 + tid;
    const int f = a.cand ? a.cand[(size_t)v * a.slots + i] : i;
    ViewRow r;
    bool bad = false;
    if (!view_eval<true>(a, M, ang, f, r, bad) || bad || row >= a.maxKpts) return; // (what the select pass kept is kept again)
    const size_t o = (size_t)v * a.maxKpts + row;
    if (DESC) {
        uint4 *__restrict__ d = a.desc + (size_t)v * a.descStride + 2 * (size_t)row;
        d[0] = a.obsDesc[2 * (size_t)r.obs];
        d[1] = a.obsDesc[2 * (size_t)r.obs + 1];
    }
    float *__restrict__ p = a.pts + (size_t)v * a.ptsStride + 3 * (size_t)row;
    p[0] = (float)r.p0; // matcher.cpp:700-701
    p[1] = (float)r.p1;
    p[2] = (float)r.p2;
    a.mapLevel[o] = r.level;
    if (a.featIdx) a.featIdx[o] = f;
    if (a.obsIdx) a.obsIdx[o] = r.obs;
    if (a.posCam) {
        a.posCam[3 * o] = r.p0;
        a.posCam[3 * o + 1] = r.p1;
        a.posCam[3 * o + 2] = r.p2;
    }
    if (a.uv) {
        a.uv[2 * o] = r.u;
        a.uv[2 * o + 1] = r.v;
    }
    if (a.angle) a.angle[o] = r.angle;
}

// matcher.cpp:639-652 for the keypoints of a frame set: one keypoint per thread, grid numFrames x chunks
__global__ __launch_bounds__(kViewBlock) void ps_frame_levels(const float *__restrict__ pts, const int32_t *__restrict__ nkpts,
                                                               int maxKpts, int ptsStride, int chunks,
                                                               const int32_t *__restrict__ octave, const double *__restrict__ detDist,
                                                               const LevelBlock *__restrict__ levels, int32_t *__restrict__ curLevel)
{
    const int f = (int)blockIdx.x / chunks, i = ((int)blockIdx.x - f * chunks) * kViewBlock + (int)threadIdx.x;
    int n = nkpts[f];
    n = n < 0 ? 0 : (n > maxKpts ? maxKpts : n);
    if (i >= n) return;
    const float *__restrict__ p = pts + (size_t)f * ptsStride + 3 * (size_t)i;
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    const float nrm = sqrtf(p0 * p0 + (p1 * p1 + p2 * p2)); // Vector3f::norm, :644
    const size_t o = (size_t)f * maxKpts + i;
    const int oc = octave[o];
    curLevel[o] = level_octave_ok(oc) ? level_rule(levels, oc, detDist[o], (double)nrm) : -1;
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the level block, the checks and the launches
namespace {

// the level rule's constant block, uploaded once per context (the one synchronising step, like a scratch block's first growth)
int ensure_level_block(PsContext *ctx)
{
    if (ctx->levelTab.p) return PS_OK;
    static LevelBlock host; // (filled identically by every caller: psi_level_tables computes once per process)
    if (psi_level_tables(host.t, host.pw) != PS_OK)
        return fail(ctx, PS_ERR_UNSUPPORTED, "level thresholds: the host's log is not monotone around a switching point of ceil(log(x) / log(1.2))");
    PS_ENSURE(ctx->levelTab, sizeof(LevelBlock));
    hipError_t e = hipMemcpyAsync(ctx->levelTab.p, &host, sizeof(LevelBlock), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        release(ctx->levelTab);
        return fail(ctx, PS_ERR_HIP, "level thresholds: upload", e);
    }
    return PS_OK;
}

// What ps_map_views_device and ps_map_views_l2_device (ps_map_store_f32.h) share on the host side: the two store structs differ
// in obsDesc alone, the two output blocks in `views` alone.
// The argument rules that do not concern the descriptor rows or the output set; PS_OK with V == 0 left to the caller.
template <class Store> int check_view_call(PsContext *ctx, const char *who, const Store *store, const PsMapViewRequest *req)
{
    const std::string w(who);
    if (store->numFeatures < 0 || store->numObs < 0 || store->numPoses < 0 || req->V < 0)
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": a negative count (numFeatures, numObs, numPoses, V)").c_str());
    if (req->V == 0) return PS_OK;
    if (!store->obsStart || (store->numFeatures > 0 && !store->pos) ||
        (store->numObs > 0 && (!store->obsPose || !store->obsDesc || !store->obsOctave || !store->obsDetDist)))
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": null array in the store").c_str());
    return PS_OK;
}

template <class Out> int check_view_request(PsContext *ctx, const char *who, int numPoses, const PsMapViewRequest *req, const Out *out)
{
    const std::string w(who);
    if (!req->camInv || (numPoses > 0 && !req->poseAngle)) return fail(ctx, PS_ERR_BAD_ARG, (w + ": null camInv or poseAngle").c_str());
    if (req->cand && (!req->candCounts || req->candCapacity < 0))
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": a candidate list needs candCounts and candCapacity >= 0").c_str());
    if (!out->mapLevel || !out->viewCount) return fail(ctx, PS_ERR_BAD_ARG, (w + ": null mapLevel or viewCount").c_str());
    return PS_OK;
}

// The store's index arrays, the request and the side arrays of a checked call (descriptor rows and the output set: the caller's)
template <class Store, class Out> void fill_view_args(ViewArgs &a, const Store *store, const PsMapViewRequest *req, const Out *out)
{
    a.pos = store->pos; a.obsStart = store->obsStart; a.obsPose = store->obsPose;
    a.obsOctave = store->obsOctave; a.obsDetDist = store->obsDetDist;
    a.numFeatures = store->numFeatures; a.numObs = store->numObs; a.numPoses = store->numPoses;
    a.camInv = req->camInv; a.poseAngle = req->poseAngle; a.cand = req->cand; a.candCounts = req->candCounts;
    a.maxAngle = req->maxAngle; a.fx = req->fx; a.fy = req->fy; a.cx = req->cx; a.cy = req->cy;
    a.imageW = req->imageW; a.imageH = req->imageH;
    a.slots = req->cand ? req->candCapacity : store->numFeatures;
    a.flags = req->flags;
    a.nkpts = (int32_t *)out->views.nkpts; a.pts = (float *)out->views.pts;
    a.maxKpts = out->views.maxKpts;
    a.mapLevel = out->mapLevel; a.viewCount = out->viewCount; a.featIdx = out->featIdx; a.obsIdx = out->obsIdx;
    a.posCam = out->posCam; a.uv = out->uv; a.angle = out->angle;
}

// The level block, the scratch and the two launches for V views.  DESC = false: ps_view_emit leaves the descriptor rows out.
template <bool DESC> int run_view_chain(PsContext *ctx, const char *who, ViewArgs &a, int V)
{
    const int chunks = a.slots > 0 ? (a.slots + kViewBlock - 1) / kViewBlock : 1;
    if ((long long)V * chunks > (long long)INT_MAX)
        return fail(ctx, PS_ERR_UNSUPPORTED, (std::string(who) + ": V x candidate chunks exceeds the grid").c_str());
    int rc = ensure_level_block(ctx);
    if (rc) return rc;
    const size_t groups = (size_t)V * chunks;
    PS_ENSURE(ctx->viewChunks, groups * (kViewWaves * 8 + 4) + (size_t)V * 4);
    HandoffGuard handoffGuard{ctx}; // (the context's scratch is in use until the launches have run)
    a.levels = (const LevelBlock *)ctx->levelTab.p;
    a.keptMask = (unsigned long long *)ctx->viewChunks.p;
    a.chunkCount = (int32_t *)(a.keptMask + groups * kViewWaves);
    a.bad = a.chunkCount + groups;
    a.chunks = chunks;
    PS_HIP(hipMemsetAsync(a.bad, 0, (size_t)V * 4, ctx->stream));
    const dim3 grid((unsigned)groups), block(kViewBlock);
    const bool staged = a.numPoses <= kViewAngleLds;
    if (staged) hipLaunchKernelGGL(ps_view_select<true>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(ps_view_select<false>, grid, block, 0, ctx->stream, a);
    PS_HIP(hipGetLastError());
    if (staged) hipLaunchKernelGGL((ps_view_emit<true, DESC>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((ps_view_emit<false, DESC>), grid, block, 0, ctx->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_map_store(void) { return sizeof(PsMapStore); }
size_t ps_abi_sizeof_map_view_request(void) { return sizeof(PsMapViewRequest); }
size_t ps_abi_sizeof_map_view_out(void) { return sizeof(PsMapViewOut); }

int ps_map_views_device(PsContext *ctx, const PsMapStore *store, const PsMapViewRequest *req, const PsMapViewOut *out)
{
    const char *who = "ps_map_views_device";
    int rc = bind(ctx);
    if (rc) return rc;
    if (!store || !req || !out) return fail(ctx, PS_ERR_BAD_ARG, "ps_map_views_device: null store, request or output block");
    rc = check_view_call(ctx, who, store, req);
    if (rc || req->V == 0) return rc;
    if (((uintptr_t)store->obsDesc & 15) != 0) return fail(ctx, PS_ERR_BAD_ARG, "ps_map_views_device: obsDesc must be 16-byte aligned");
    rc = check_view_request(ctx, who, store->numPoses, req, out);
    if (rc) return rc;
    FrameStrides strides;
    rc = check_frame_set(ctx, out->views, "ps_map_views_device: output views", strides);
    if (rc) return rc;
    if (out->views.numFrames < req->V) return fail(ctx, PS_ERR_BAD_ARG, "ps_map_views_device: the output set has fewer than V views");
    TimingOff toff(ctx);
    ViewArgs a{};
    fill_view_args(a, store, req, out);
    a.obsDesc = (const uint4 *)store->obsDesc;
    a.desc = (uint4 *)out->views.desc;
    a.descStride = strides.descUint4();
    a.ptsStride = strides.ptsFloats();
    return run_view_chain<true>(ctx, who, a, req->V);
}

int ps_frame_levels_device(PsContext *ctx, const PsFrameSet *frames, const int32_t *octave, const double *detDist, int32_t *curLevel)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!frames || !octave || !detDist || !curLevel || frames->numFrames < 0)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_frame_levels_device: null argument or numFrames < 0");
    if (frames->numFrames == 0) return PS_OK;
    if (!frames->pts || !frames->nkpts || frames->maxKpts < 1)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_frame_levels_device: null pts / nkpts or maxKpts < 1");
    if (frames->maxKpts > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_frame_levels_device: more than PS_MAX_KPTS keypoints per frame");
    FrameStrides strides; // (no descriptors are read: desc may be null, and its stride is not looked at)
    rc = frame_strides(ctx, *frames, false, true, "ps_frame_levels_device", strides);
    if (rc) return rc;
    const int chunks = (frames->maxKpts + kViewBlock - 1) / kViewBlock;
    if ((long long)frames->numFrames * chunks > (long long)INT_MAX)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_frame_levels_device: numFrames x chunks exceeds the grid");
    TimingOff toff(ctx);
    rc = ensure_level_block(ctx);
    if (rc) return rc;
    HandoffGuard handoffGuard{ctx};
    hipLaunchKernelGGL(ps_frame_levels, dim3((unsigned)frames->numFrames * (unsigned)chunks), dim3(kViewBlock), 0, ctx->stream,
                       frames->pts, frames->nkpts, frames->maxKpts, strides.ptsFloats(), chunks, octave, detDist,
                       (const LevelBlock *)ctx->levelTab.p, curLevel);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

} // extern "C"
