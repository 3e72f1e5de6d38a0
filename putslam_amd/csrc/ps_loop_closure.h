// ps_loop_closure.h -- loop-closure candidates verified in one batch from the resident feature map (ps_pose_sets_device /
// ps_loop_pairs_device, include/putslam_hip.h).  What the reference's loop-closure thread does per candidate:
//   FeaturesMap::loopClosure (src/Map/featuresMap.cpp:733-873)               the two gates, the copy of every feature seen from
//                                                                            either pose, the threshold on the returned ratio,
//   Matcher::matchFeatureLoopClosure (src/Matcher/matcher.cpp:802-861)       each feature's descriptor and point3D AS OBSERVED FROM
//                                                                            THAT POSE, performMatching, RANSAC, the repack.
// The store is feature-major; a pose's feature set is its inversion.  Shape of ps_pose_sets_device: four launches on one stream,
// one feature per thread, 256 features a chunk.
//   ps_pose_table   one work-group: head[q] = the last set that names pose q, next[s] = the previous set with the same pose (a pose
//                   listed twice is a chain); no atomics -- every thread scans the S pose ids in LDS.
//   ps_pose_count   grid chunks.  A thread walks its feature's observations, follows the chain of each observation's pose and sets
//                   its bit in an LDS bitmap [S][256 bits] (LDS atomic-or: idempotent, no order); the chunk's member count of
//                   every set goes to chunkCount[chunk][s].
//   ps_pose_scan    grid S.  One work-group per set turns its column of chunk counts into exclusive offsets (a block scan over
//                   256 chunks a trip) and writes setCount / nkpts.
//   ps_pose_emit    grid chunks.  Rebuilds the bitmap, and every member writes its row at offset + popcount of the bits below its
//                   own: ascending feature index whatever order the chunks ran in.
// The store's observation index (obsStart, obsPose) is read twice, descriptors and points once per member, whatever S is.  The
// bitmap always lies in LDS and the table always in global memory: no run-time choice between the two inside a loop (ps_map_view.h).
// ps_loop_pairs_device adds a gate kernel in front of ps_vo_pairs_device's stages and a verdict kernel behind them.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ps_glue.h"
#include "ps_block.h" // block_scan_int, block_scan_flag
#include "ps_ransac_stage.h"

namespace psdev {

constexpr int kPoseBlock = 256;
constexpr int kPoseWords = kPoseBlock / 32; // bitmap words per set and chunk
constexpr int kPoseTableBlock = PS_LOOP_MAX_SETS;

struct PoseSetArgs {
    // the store and the request
    const int32_t *obsStart, *obsPose;
    const uint4 *obsDesc;
    const double *obsPoint3D;
    int numFeatures, numObs, numPoses;
    const int32_t *poses;
    int S;
    // the outputs
    uint4 *desc;
    float *pts;
    int32_t *nkpts;
    int maxKpts, descStride /* uint4 */, ptsStride /* floats */;
    int32_t *setCount, *featIdx, *obsIdx;
    // scratch
    int32_t *bad;        // [1], cleared before the launches: a malformed observation range somewhere in the store
    int32_t *next;       // [S]
    int32_t *head;       // [numPoses], -1 before ps_pose_table
    int32_t *chunkCount; // [chunks][S]: counts, then (ps_pose_scan) exclusive offsets
    int chunks;
};

__global__ __launch_bounds__(kPoseTableBlock) void ps_pose_table(const int32_t *__restrict__ poses, int S, int numPoses,
                                                                 int32_t *__restrict__ head, int32_t *__restrict__ next)
{
    __shared__ int sPose[kPoseTableBlock];
    const int s = (int)threadIdx.x;
    if (s < S) sPose[s] = poses[s];
    __syncthreads();
    if (s >= S) return;
    const int q = sPose[s];
    if (q < 0 || q >= numPoses) { // (names no pose: ps_pose_scan reports it)
        next[s] = -1;
        return;
    }
    int prev = -1;
    bool later = false;
    for (int k = 0; k < S; ++k) {
        const bool same = sPose[k] == q;
        prev = (same && k < s) ? k : prev;
        later |= same && k > s;
    }
    next[s] = prev;
    if (!later) head[q] = s;
}

// The bits of feature f (this thread's) in the chunk's bitmap; false for a malformed observation range.
PS_D bool pose_mark(const PoseSetArgs &a, unsigned *bm, int f)
{
    const int tid = (int)threadIdx.x;
    const int s = a.obsStart[f], e = a.obsStart[f + 1];
    if (s < 0 || e < s || e > a.numObs) return false;
    for (int o = s; o < e; ++o) {
        const int q = a.obsPose[o];
        if (q < 0 || q >= a.numPoses) continue; // (belongs to no set)
        for (int k = a.head[q]; k >= 0; k = a.next[k]) atomicOr(&bm[k * kPoseWords + (tid >> 5)], 1u << (tid & 31));
    }
    return true;
}

PS_D void pose_clear(unsigned *bm, int S)
{
    for (int i = (int)threadIdx.x; i < S * kPoseWords; i += kPoseBlock) bm[i] = 0u;
    __syncthreads();
}

__global__ __launch_bounds__(kPoseBlock) void ps_pose_count(PoseSetArgs a)
{
    extern __shared__ __align__(16) unsigned s_bm[]; // [S][kPoseWords]
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    pose_clear(s_bm, a.S);
    const int f = c * kPoseBlock + tid;
    const bool bad = f < a.numFeatures && !pose_mark(a, s_bm, f);
    if (__ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(a.bad, 1);
    __syncthreads();
    for (int s = tid; s < a.S; s += kPoseBlock) {
        const uint4 lo = *reinterpret_cast<const uint4 *>(s_bm + s * kPoseWords);
        const uint4 hi = *reinterpret_cast<const uint4 *>(s_bm + s * kPoseWords + 4);
        a.chunkCount[(size_t)c * a.S + s] = ((__popc(lo.x) + __popc(lo.y)) + (__popc(lo.z) + __popc(lo.w))) +
                                            ((__popc(hi.x) + __popc(hi.y)) + (__popc(hi.z) + __popc(hi.w)));
    }
}

__global__ __launch_bounds__(kPoseBlock) void ps_pose_scan(PoseSetArgs a)
{
    __shared__ int s_wsum[kPoseBlock / 64];
    const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int q = a.poses[s];
    const bool invalid = q < 0 || q >= a.numPoses || a.bad[0] != 0; // (the whole work-group)
    int carry = 0;
    if (!invalid) {
        for (int c0 = 0; c0 < a.chunks; c0 += kPoseBlock) {
            const int c = c0 + tid;
            const size_t cell = (size_t)(c < a.chunks ? c : 0) * a.S + s;
            const int v = c < a.chunks ? a.chunkCount[cell] : 0;
            int sum;
            const int ex = block_scan_int<kPoseBlock>(v, sum, s_wsum);
            if (c < a.chunks) a.chunkCount[cell] = carry + ex;
            carry += sum;
        }
    }
    if (tid == 0) {
        const bool over = carry > a.maxKpts;
        a.setCount[s] = invalid ? INT_MIN : (over ? -carry : carry);
        a.nkpts[s] = (invalid || over) ? 0 : carry;
        if (s == 0) a.nkpts[a.S] = 0; // the empty set
    }
}

// DESC = false (the float-row store, ps_map_store_f32.h): the 32 descriptor bytes are left out; obsIdx is then always given
template <bool DESC = true> __global__ __launch_bounds__(kPoseBlock) void ps_pose_emit(PoseSetArgs a)
{
    extern __shared__ __align__(16) unsigned s_bm[];
    if (a.bad[0] != 0) return; // (the whole grid)
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    pose_clear(s_bm, a.S);
    const int f = c * kPoseBlock + tid;
    const bool live = f < a.numFeatures && pose_mark(a, s_bm, f);
    __syncthreads();
    if (!live) return;
    const int w = tid >> 5;
    const unsigned below = (1u << (tid & 31)) - 1u;
    const int s0 = a.obsStart[f], e = a.obsStart[f + 1];
    for (int o = s0; o < e; ++o) {
        const int q = a.obsPose[o];
        if (q < 0 || q >= a.numPoses) continue;
        int k = a.head[q];
        if (k < 0) continue;
        bool first = true; // (a malformed store may hold the pose twice: the first observation is the member's)
        for (int p = s0; p < o; ++p) first &= a.obsPose[p] != q;
        if (!first) continue;
        for (; k >= 0; k = a.next[k]) {
            const int n = a.setCount[k];
            if (n < 0 || n > a.maxKpts) continue; // overflowed: no row of it is written
            const unsigned *bm = s_bm + k * kPoseWords;
            int row = a.chunkCount[(size_t)c * a.S + k];
#pragma unroll
            for (int j = 0; j < kPoseWords; ++j) row += j < w ? __popc(bm[j]) : (j == w ? __popc(bm[j] & below) : 0);
            if (row < 0 || row >= n) continue;
            if (DESC) {
                uint4 *__restrict__ d = a.desc + (size_t)k * a.descStride + 2 * (size_t)row;
                d[0] = a.obsDesc[2 * (size_t)o];
                d[1] = a.obsDesc[2 * (size_t)o + 1];
            }
            float *__restrict__ p = a.pts + (size_t)k * a.ptsStride + 3 * (size_t)row;
            p[0] = (float)a.obsPoint3D[3 * (size_t)o]; // matcher.cpp:819-821
            p[1] = (float)a.obsPoint3D[3 * (size_t)o + 1];
            p[2] = (float)a.obsPoint3D[3 * (size_t)o + 2];
            const size_t at = (size_t)k * a.maxKpts + row;
            if (a.featIdx) a.featIdx[at] = f;
            if (a.obsIdx) a.obsIdx[at] = o;
        }
    }
}

// ---- the verifier's two kernels
struct LoopArgs {
    const int32_t *setCount, *featIdx, *pairs;
    int L, S, minFeatures, maxKpts;
    double threshold;
    int32_t *eff; // [L][2] effective pairs
    const PsDMatch *matches;
    const int32_t *numMatches;
    const uint8_t *inlierMask;
    const PsRansacStats *stats;
    double *ratio;
    int32_t *closed, *numPaired, *pairedRows, *pairedFeat;
};

enum { kLoopRun = 0, kLoopGated = 1, kLoopInvalid = 2 };

// featuresMap.cpp:776-779 (strict) and matcher.cpp:830
PS_D int loop_state(const LoopArgs &a, int l)
{
    const int s0 = a.pairs[2 * l], s1 = a.pairs[2 * l + 1];
    if (s0 < 0 || s0 >= a.S || s1 < 0 || s1 >= a.S) return kLoopInvalid;
    const int n0 = a.setCount[s0], n1 = a.setCount[s1];
    if (n0 < 0 || n1 < 0) return kLoopInvalid;
    if (n0 <= a.minFeatures || n1 <= a.minFeatures || n0 < 10 || n1 < 10) return kLoopGated;
    return kLoopRun;
}

__global__ __launch_bounds__(kBlock) void ps_loop_gate(LoopArgs a)
{
    const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (l >= a.L) return;
    const bool run = loop_state(a, l) == kLoopRun;
    a.eff[2 * l] = run ? a.pairs[2 * l] : a.S;
    a.eff[2 * l + 1] = run ? a.pairs[2 * l + 1] : a.S;
}

// One work-group per candidate: the final inliers in match order (matcher.cpp:853-857), the ratio and the verdict
__global__ __launch_bounds__(kBlock) void ps_loop_verdict(LoopArgs a)
{
    __shared__ int s_wsum[kBlock / 64];
    const int l = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int state = loop_state(a, l);
    int n = state == kLoopRun ? a.numMatches[l] : 0;
    n = n < 0 ? 0 : (n > a.maxKpts ? a.maxKpts : n);
    const int s0 = state == kLoopRun ? a.pairs[2 * l] : 0, s1 = state == kLoopRun ? a.pairs[2 * l + 1] : 0;
    const size_t row0 = (size_t)l * a.maxKpts;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += kBlock) {
        const int i = i0 + tid;
        const bool in = i < n && a.inlierMask[row0 + i] != 0;
        int total;
        const int pos = block_scan_flag<kBlock>(in, total, s_wsum);
        if (in) {
            const PsDMatch m = a.matches[row0 + i];
            const size_t o = 2 * (row0 + base + pos);
            a.pairedRows[o] = m.queryIdx;
            a.pairedRows[o + 1] = m.trainIdx;
            if (a.pairedFeat) {
                a.pairedFeat[o] = a.featIdx[(size_t)s0 * a.maxKpts + m.queryIdx];
                a.pairedFeat[o + 1] = a.featIdx[(size_t)s1 * a.maxKpts + m.trainIdx];
            }
        }
        base += total;
    }
    if (tid == 0) {
        double r = 0.0; // gated: both reference gates leave matchingRatio = 0
        if (state == kLoopRun) r = n == 0 ? -1.0 : a.stats[l].pointInlierRatio; // matcher.cpp:838-839, :859
        a.ratio[l] = r;
        a.closed[l] = (state != kLoopInvalid && r > a.threshold) ? 1 : 0; // featuresMap.cpp:806 (false for a NaN)
        a.numPaired[l] = state == kLoopInvalid ? INT_MIN : base;
    }
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the checks and the launches.  ps_map_store_f32.h runs the same
// chains for a store of float rows: the two store structs differ in obsDesc alone, the two batches in `sets` alone.
namespace {

// The argument rules of a pose-set call that do not concern the descriptor rows or the output set
template <class Store, class Out>
int check_pose_call(PsContext *ctx, const char *who, const Store *store, const PsPoseSetRequest *req, const Out *out)
{
    const std::string w(who);
    const int S = req->S;
    if (out->sets.numFrames < S + 1) return fail(ctx, PS_ERR_BAD_ARG, (w + ": the output set has fewer than S + 1 frames").c_str());
    if (S > 0 && (!req->poses || !out->setCount)) return fail(ctx, PS_ERR_BAD_ARG, (w + ": null poses or setCount").c_str());
    if (S > 0 && (!store->obsStart || (store->numObs > 0 && (!store->obsPose || !store->obsDesc || !req->obsPoint3D))))
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": null array in the store, or null obsPoint3D").c_str());
    return PS_OK;
}

template <class Store, class Out> void fill_pose_args(PoseSetArgs &a, const Store *store, const PsPoseSetRequest *req, const Out *out)
{
    a.obsStart = store->obsStart; a.obsPose = store->obsPose;
    a.obsPoint3D = req->obsPoint3D;
    a.numFeatures = store->numFeatures; a.numObs = store->numObs; a.numPoses = store->numPoses;
    a.poses = req->poses; a.S = req->S;
    a.pts = (float *)out->sets.pts; a.nkpts = (int32_t *)out->sets.nkpts;
    a.maxKpts = out->sets.maxKpts;
    a.setCount = out->setCount; a.featIdx = out->featIdx; a.obsIdx = out->obsIdx;
}

// The scratch and the four launches for S >= 1 sets.  DESC = false: ps_pose_emit leaves the descriptor rows out.
template <bool DESC> int run_pose_chain(PsContext *ctx, PoseSetArgs &a)
{
    const int S = a.S;
    const int chunks = (a.numFeatures + kPoseBlock - 1) / kPoseBlock;
    const size_t fixedInts = 4 + (size_t)S + (size_t)a.numPoses; // bad (padded) | next | head
    PS_ENSURE(ctx->poseSets, (fixedInts + (size_t)chunks * S) * sizeof(int32_t));
    HandoffGuard handoffGuard{ctx}; // (the context's scratch is in use until the launches have run)
    a.bad = (int32_t *)ctx->poseSets.p;
    a.next = a.bad + 4;
    a.head = a.next + S;
    a.chunkCount = a.head + a.numPoses;
    a.chunks = chunks;
    PS_HIP(hipMemsetAsync(a.bad, 0, 4 * sizeof(int32_t), ctx->stream));
    if (a.numPoses > 0) PS_HIP(hipMemsetAsync(a.head, 0xFF, (size_t)a.numPoses * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(ps_pose_table, dim3(1), dim3(kPoseTableBlock), 0, ctx->stream, a.poses, S, a.numPoses, a.head, a.next);
    PS_HIP(hipGetLastError());
    const size_t lds = (size_t)S * kPoseWords * sizeof(unsigned); // 32 KiB at PS_LOOP_MAX_SETS
    if (chunks > 0) {
        hipLaunchKernelGGL(ps_pose_count, dim3((unsigned)chunks), dim3(kPoseBlock), lds, ctx->stream, a);
        PS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ps_pose_scan, dim3((unsigned)S), dim3(kPoseBlock), 0, ctx->stream, a);
    PS_HIP(hipGetLastError());
    if (chunks > 0) {
        hipLaunchKernelGGL(ps_pose_emit<DESC>, dim3((unsigned)chunks), dim3(kPoseBlock), lds, ctx->stream, a);
        PS_HIP(hipGetLastError());
    }
    return PS_OK;
}

// ps_loop_pairs_device / ps_loop_pairs_l2_device: checkSets(b->sets) holds the rule of the batch's frame set, match(eff, L, pl)
// runs the matcher of its descriptor kind on the effective pairs.
template <class Batch, class Check, class Match>
int loop_pairs_body(PsContext *ctx, const char *who, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                    const Batch *b, const PsLoopResults *out, Check checkSets, Match match)
{
    const std::string w(who);
    if (!b || !out || b->L < 0) return fail(ctx, PS_ERR_BAD_ARG, (w + ": null batch or results, or L < 0").c_str());
    if (b->L == 0) return PS_OK;
    if (b->S < 0 || !b->pairs || !b->setCount) return fail(ctx, PS_ERR_BAD_ARG, (w + ": S < 0, null pairs or setCount").c_str());
    int rc = checkSets(b->sets); // (checked here, before anything is planned or allocated)
    if (rc) return rc;
    if ((long long)b->sets.numFrames < (long long)b->S + 1)
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": the frame set has fewer than S + 1 frames (the empty set is frame S)").c_str());
    const PsPairResults &pr = out->pair;
    if (!pr.matches || !pr.numMatches || !pr.inlierMask || !pr.pose || !pr.stats || !out->ratio || !out->closed || !out->numPaired ||
        !out->pairedRows)
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": null output").c_str());
    if (out->pairedFeat && !b->featIdx) return fail(ctx, PS_ERR_BAD_ARG, (w + ": pairedFeat needs featIdx").c_str());
    if (cfg && cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "explicit sample streams are per call, not per batch");
    const int L = b->L, cap = b->sets.maxKpts;
    Plan pl;
    rc = make_plan(ctx, params, cfg, K, cap, cap, pl);
    if (rc) return rc;
    begin_timed_call(ctx);
    HandoffGuard handoffGuard{ctx}; // (prepare_score below may already queue a clearing: the guard stands before it)
    PS_ENSURE(ctx->loopPairs, (size_t)L * 2 * sizeof(int32_t));
    LoopArgs a{};
    a.setCount = b->setCount; a.featIdx = b->featIdx; a.pairs = b->pairs;
    a.L = L; a.S = b->S; a.minFeatures = b->minNumberOfFeaturesLC; a.maxKpts = cap;
    a.threshold = b->matchingRatioThresholdLC;
    a.eff = (int32_t *)ctx->loopPairs.p;
    a.matches = pr.matches; a.numMatches = pr.numMatches; a.inlierMask = pr.inlierMask; a.stats = pr.stats;
    a.ratio = out->ratio; a.closed = out->closed; a.numPaired = out->numPaired;
    a.pairedRows = out->pairedRows; a.pairedFeat = out->pairedFeat;
    hipLaunchKernelGGL(ps_loop_gate, dim3((unsigned)((L + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, a);
    PS_HIP(hipGetLastError());
    rc = prepare_score(ctx, pl, L, cap, false, true, b->sets.desc);
    if (rc) return rc;
    rc = match(a.eff, L, pl);
    if (rc) return rc;
    rc = run_ransac_stage(ctx, pl, L, cap, pr.matches, pr.numMatches, cap, pr.pose, pr.inlierMask, pr.stats, 2);
    if (rc) return rc;
    hipLaunchKernelGGL(ps_loop_verdict, dim3((unsigned)L), dim3(kBlock), 0, ctx->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_pose_set_request(void) { return sizeof(PsPoseSetRequest); }
size_t ps_abi_sizeof_pose_set_out(void) { return sizeof(PsPoseSetOut); }
size_t ps_abi_sizeof_loop_batch(void) { return sizeof(PsLoopBatch); }
size_t ps_abi_sizeof_loop_results(void) { return sizeof(PsLoopResults); }

int ps_pose_sets_device(PsContext *ctx, const PsMapStore *store, const PsPoseSetRequest *req, const PsPoseSetOut *out)
{
    const char *who = "ps_pose_sets_device";
    int rc = bind(ctx);
    if (rc) return rc;
    if (!store || !req || !out) return fail(ctx, PS_ERR_BAD_ARG, "ps_pose_sets_device: null store, request or output block");
    if (store->numFeatures < 0 || store->numObs < 0 || store->numPoses < 0 || req->S < 0)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_pose_sets_device: a negative count (numFeatures, numObs, numPoses, S)");
    if (req->S > PS_LOOP_MAX_SETS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_pose_sets_device: more than PS_LOOP_MAX_SETS sets");
    FrameStrides strides;
    rc = check_frame_set(ctx, out->sets, "ps_pose_sets_device: output sets", strides);
    if (rc) return rc;
    rc = check_pose_call(ctx, who, store, req, out);
    if (rc) return rc;
    if (((uintptr_t)store->obsDesc & 15) != 0) return fail(ctx, PS_ERR_BAD_ARG, "ps_pose_sets_device: obsDesc must be 16-byte aligned");
    TimingOff toff(ctx);
    if (req->S == 0) { // nothing but the empty set
        PS_HIP(hipMemsetAsync((void *)out->sets.nkpts, 0, sizeof(int32_t), ctx->stream));
        return PS_OK;
    }
    PoseSetArgs a{};
    fill_pose_args(a, store, req, out);
    a.obsDesc = (const uint4 *)store->obsDesc;
    a.desc = (uint4 *)out->sets.desc;
    a.descStride = strides.descUint4();
    a.ptsStride = strides.ptsFloats();
    return run_pose_chain<true>(ctx, a);
}

int ps_loop_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                         const PsLoopBatch *b, const PsLoopResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    return loop_pairs_body(
        ctx, "ps_loop_pairs_device", params, cfg, K, b, out,
        [&](const PsFrameSet &fs) {
            FrameStrides strides; // (run_match_stage resolves them again for its launches)
            return check_frame_set(ctx, fs, "ps_loop_pairs_device: sets", strides);
        },
        [&](const int32_t *eff, int L, const Plan &pl) {
            return run_match_stage(ctx, b->sets, eff, L, &pl, out->pair.matches, out->pair.numMatches, 0);
        });
}

} // extern "C"
