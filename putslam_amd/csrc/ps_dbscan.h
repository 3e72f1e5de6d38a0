// ps_dbscan.h -- DBScan::run (reference src/Matcher/dbscan.cpp) as one work-group per frame: keypoint thinning between
// detection and description (matcher.cpp:459-461 and the three other call sites).
//
// What the reference computes, read closely:
//  * neighbours: (double)(float)sqrt((double)dx*dx + (double)dy*dy) < eps with dx, dy float differences.  The float products
//    are exact in double and the sum rounds once, so the predicate is  s < sstar  for the least double sstar whose rounded root
//    reaches eps (dbscan_bound below, host side): no device sqrt.  A NaN makes every predicate false, itself included.
//  * main loop in ascending index: an unvisited point counts ALL its neighbours (itself and visited ones included); below
//    minPts it becomes noise, else it seeds a cluster whose list is expanded.
//  * expansion: an unvisited x of the list is visited and collects its UNVISITED neighbours (x itself excluded); at least minPts
//    of them are appended.  Only a point that was still unlabelled joins the cluster: noise is never relabelled.
//  * duplicates in the list are no-ops, so a deduplicated FIFO reproduces the processing order; connected components of the
//    eps-graph never interact, so each one is replayed on its own in ascending index order.
//  * keep: noise, and the first featuresFromCluster members of a cluster in index order; an input octave of -5 is removed.
//
// Shape: the work-group finds the components with a union-find over all pairs (LDS atomics, roots = least index), replays the
// small ones one per lane and the large ones cooperatively (every "collect the neighbours" step is a work-group pass with an
// ordered append through ballots), then writes the survivors' indices in ascending order.  Per-point state lives in LDS, 20 bytes
// a point: PS_DBSCAN_MAX_KPTS points per frame.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ps_block.h" // uf_find / uf_union (here at work-group scope: comp[] lies in LDS)
#include "ps_glue.h"

namespace psdev {

constexpr int kDbBlock = 1024;
constexpr int kDbWaves = kDbBlock / 64;
constexpr int kDbChunks = (PS_DBSCAN_MAX_KPTS + kDbBlock - 1) / kDbBlock; // points per thread, at most
constexpr int kDbLaneMax = 32;                                             // components this small are replayed by one lane
constexpr int kDbBigMax = PS_DBSCAN_MAX_KPTS / (kDbLaneMax + 1) + 1;       // components larger than that, at most
static_assert(kDbChunks * kDbWaves == 128, "db_scan_counts: two entries per lane of one wave");
// lab[] while replaying: >= 0 = visited, member of the cluster seeded by that index; then these
constexpr int kDbNoise = -1, kDbUnvisited = -2, kDbQueued = -3;
constexpr uint16_t kDbEnd = 0xFFFF;

// dynamic LDS of one frame of `cap` points: xy float2, comp int, lab int, nxt u16, qn u16
__host__ __device__ inline size_t dbscan_lds_bytes(int cap) { return (size_t)cap * 20; }

__device__ __forceinline__ bool db_nb(float2 a, float2 b, double sstar)
{
    const float dx = a.x - b.x, dy = a.y - b.y;
    const double s = (double)dx * (double)dx + (double)dy * (double)dy;
    return s < sstar;
}

// wave 0: sRed[j][w] (per-wave counts of chunk j) -> exclusive prefix in (j, w) order; *total = the sum
__device__ __forceinline__ void db_scan_counts(int *sRed, int *total)
{
    const int lane = (int)threadIdx.x & 63;
    const int v0 = sRed[2 * lane], v1 = sRed[2 * lane + 1];
    int inc = v0 + v1;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    const int exc = inc - v0 - v1;
    sRed[2 * lane] = exc;
    sRed[2 * lane + 1] = exc + v0;
    if (lane == 63) *total = inc;
}

struct DbShared {
    int red[kDbChunks * kDbWaves];
    int cnt[kDbWaves];
    int mins[kDbWaves];
    int tot[2];
    int nBig;
    int big[kDbBigMax];
};

// One cooperative step on component r for point x: counts x's neighbours among the component's members -- all of them but x
// (seed step, `all`: x itself too if it is its own neighbour) or the unvisited ones other than x (expansion) -- and, if the
// count reaches minPts, appends the unqueued unvisited ones to q[tail...] in ascending index and marks them queued.  The thread
// that owns x then marks it visited: lab[x] = seed (seed step: x itself, or noise if the count stays below minPts).  Returns the
// number appended; every thread returns the same.  Ends with a barrier.
__device__ __forceinline__ int db_coop_step(const float2 *xy, const int *comp, int *lab, uint16_t *q, int n, int r, int x,
                                            int seed, bool all, double sstar, int minPts, int tail, DbShared &sh)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float2 p = xy[x];
    unsigned bits = 0;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < kDbChunks; ++j) {
        const int k = j * kDbBlock + tid;
        bool c = false, a = false;
        if (k < n && k >= r && comp[k] == r) {
            if (k == x) {
                c = all && db_nb(p, p, sstar);
            } else if (db_nb(p, xy[k], sstar)) {
                const int l = lab[k];
                c = all || l <= kDbUnvisited;
                a = l == kDbUnvisited;
            }
        }
        const unsigned long long bc = __ballot(c), ba = __ballot(a);
        cnt += __popcll(bc);
        if (lane == 0) sh.red[j * kDbWaves + w] = __popcll(ba);
        bits |= (a ? 1u : 0u) << j;
    }
    if (lane == 0) sh.cnt[w] = cnt;
    __syncthreads();
    if (w == 0) {
        db_scan_counts(sh.red, &sh.tot[1]);
        if (lane == 0) {
            int t = 0;
            for (int i = 0; i < kDbWaves; ++i) t += sh.cnt[i];
            sh.tot[0] = t;
        }
    }
    __syncthreads();
    const bool core = sh.tot[0] >= minPts;
    const int added = core ? sh.tot[1] : 0;
#pragma unroll
    for (int j = 0; j < kDbChunks; ++j) {
        const bool a = (bits >> j) & 1u;
        const unsigned long long ba = __ballot(a);
        if (a && core) {
            const int k = j * kDbBlock + tid;
            q[tail + sh.red[j * kDbWaves + w] + __popcll(ba & ((1ull << lane) - 1ull))] = (uint16_t)k;
            lab[k] = kDbQueued;
        }
    }
    if (tid == x % kDbBlock) lab[x] = all ? (core ? x : kDbNoise) : seed;
    __syncthreads();
    return added;
}

// Lane replay of component r (members linked in ascending order through nxt[], m <= kDbLaneMax of them).
__device__ __forceinline__ void db_lane_replay(const float2 *xy, int *lab, const uint16_t *nxt, uint16_t *qn, int r, double sstar, int minPts)
{
    for (int i = r; i != kDbEnd; i = nxt[i]) {
        if (lab[i] != kDbUnvisited) continue;
        const float2 pi = xy[i];
        int cnt = 0;
        for (int k = r; k != kDbEnd; k = nxt[k]) cnt += db_nb(pi, xy[k], sstar) ? 1 : 0;
        if (cnt < minPts) {
            lab[i] = kDbNoise;
            continue;
        }
        lab[i] = i;
        int head = kDbEnd, tail = kDbEnd;
        for (int k = r; k != kDbEnd; k = nxt[k])
            if (lab[k] == kDbUnvisited && db_nb(pi, xy[k], sstar)) {
                lab[k] = kDbQueued;
                qn[k] = kDbEnd;
                if (tail == kDbEnd) head = k; else qn[tail] = (uint16_t)k;
                tail = k;
            }
        while (head != kDbEnd) {
            const int x = head;
            head = qn[x];
            if (head == kDbEnd) tail = kDbEnd;
            lab[x] = i;
            const float2 px = xy[x];
            int c = 0;
            for (int k = r; k != kDbEnd; k = nxt[k]) c += (lab[k] <= kDbUnvisited && db_nb(px, xy[k], sstar)) ? 1 : 0;
            if (c < minPts) continue;
            for (int k = r; k != kDbEnd; k = nxt[k])
                if (lab[k] == kDbUnvisited && db_nb(px, xy[k], sstar)) {
                    lab[k] = kDbQueued;
                    qn[k] = kDbEnd;
                    if (tail == kDbEnd) head = k; else qn[tail] = (uint16_t)k;
                    tail = k;
                }
        }
    }
}

// One work-group per frame f: xy [frames][cap] float2, octave [frames][cap] (may be null), counts [frames] (null: every frame
// holds n0 points).  Writes keptIdx[f][0 .. nkept[f]) in ascending order; a count outside [0, cap] gives nkept[f] = -1.
__global__ __launch_bounds__(kDbBlock) void ps_dbscan_kernel(const float2 *__restrict__ xyIn, const int32_t *__restrict__ octave,
                                                             const int32_t *__restrict__ counts, int n0, int cap, double sstar,
                                                             int minPts, int ffc, int32_t *__restrict__ keptIdx,
                                                             int32_t *__restrict__ nkept)
{
    extern __shared__ __align__(16) unsigned char dbLds[];
    __shared__ DbShared sh;
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = counts ? counts[f] : n0;
    if (n < 0 || n > cap) {
        if (tid == 0) nkept[f] = -1;
        return;
    }
    float2 *xy = reinterpret_cast<float2 *>(dbLds);
    int *comp = reinterpret_cast<int *>(dbLds + (size_t)cap * 8);
    int *lab = reinterpret_cast<int *>(dbLds + (size_t)cap * 12);
    uint16_t *nxt = reinterpret_cast<uint16_t *>(dbLds + (size_t)cap * 16);
    uint16_t *qn = reinterpret_cast<uint16_t *>(dbLds + (size_t)cap * 18);
    const float2 *src = xyIn + (size_t)f * cap;
    for (int i = tid; i < n; i += kDbBlock) {
        xy[i] = src[i];
        comp[i] = i;
        lab[i] = 0;
    }
    if (tid == 0) sh.nBig = 0;
    __syncthreads();

    // 1. components: every pair once, the lanes of a wave read the same partner (LDS broadcast)
    for (int i0 = w * 64; i0 < n; i0 += kDbBlock) {
        const int i = i0 + lane;
        const float2 pi = xy[i < n ? i : i0];
        for (int k = i0 + 1; k < n; ++k) {
            const float2 pk = xy[k];
            if (i < k && i < n && db_nb(pi, pk, sstar)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(comp, i, k);
        }
    }
    __syncthreads();
    // Flatten.  uf_find's path-halving stores may land late and put a non-root ancestor back into comp[x] after x's own root
    // was written there, so the roots go to lab[] first (every find still ends at the true root: a stale store only ever writes
    // an ancestor) and are copied into comp[] after a barrier.  From here on comp[i] is the least index of i's component.
    for (int i = tid; i < n; i += kDbBlock) lab[i] = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(comp, i);
    __syncthreads();
    for (int i = tid; i < n; i += kDbBlock) {
        comp[i] = lab[i];
        lab[i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kDbBlock) atomicAdd(&lab[comp[i]], 1);
    __syncthreads();
    for (int r = tid; r < n; r += kDbBlock)
        if (comp[r] == r) {
            const int m = lab[r];
            qn[r] = (uint16_t)m;
            if (m > kDbLaneMax) sh.big[atomicAdd(&sh.nBig, 1)] = r;
        }
    __syncthreads();
    for (int i = tid; i < n; i += kDbBlock) lab[i] = kDbUnvisited;
    __syncthreads();

    // 2. small components, one lane each: link the members in ascending order, replay
    for (int r = tid; r < n; r += kDbBlock) {
        if (comp[r] != r) continue;
        const int m = qn[r];
        if (m > kDbLaneMax) continue;
        int prev = r;
        for (int k = r + 1, got = 1; got < m && k < n; ++k)
            if (comp[k] == r) {
                nxt[prev] = (uint16_t)k;
                prev = k;
                ++got;
            }
        nxt[prev] = kDbEnd;
        db_lane_replay(xy, lab, nxt, qn, r, sstar, minPts);
    }
    __syncthreads();

    // 3. large components, cooperatively; qn[] is the FIFO now
    const int nBig = sh.nBig;
    for (int b = 0; b < nBig; ++b) {
        const int r = sh.big[b];
        int cur = r;
        for (;;) {
            // the next unvisited member in index order seeds a step of the main loop
            int best = INT_MAX;
#pragma unroll
            for (int j = 0; j < kDbChunks; ++j) {
                const int k = j * kDbBlock + tid;
                const bool c = k < n && k >= cur && comp[k] == r && lab[k] == kDbUnvisited;
                const unsigned long long bc = __ballot(c);
                if (bc && best == INT_MAX) best = j * kDbBlock + w * 64 + (__ffsll((long long)bc) - 1);
            }
            if (lane == 0) sh.mins[w] = best;
            __syncthreads();
            int seed = INT_MAX;
            for (int i = 0; i < kDbWaves; ++i) seed = min(seed, sh.mins[i]);
            __syncthreads();
            if (seed == INT_MAX) break;
            int tail = db_coop_step(xy, comp, lab, qn, n, r, seed, seed, true, sstar, minPts, 0, sh);
            for (int head = 0; head < tail; ++head) // x leaves the queue visited, a member of the seed's cluster
                tail += db_coop_step(xy, comp, lab, qn, n, r, (int)qn[head], seed, false, sstar, minPts, tail, sh);
            cur = seed + 1;
        }
    }
    __syncthreads();

    // 4. keep rule, then the survivors in ascending order
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < kDbChunks; ++j) {
        const int x = j * kDbBlock + tid;
        bool keep = false;
        if (x < n) {
            const int L = lab[x];
            if (L < 0) {
                keep = true;
            } else if (ffc > 0) {
                int c = 0;
                for (int y = L; y < x && c < ffc; ++y) c += lab[y] == L ? 1 : 0;
                keep = c < ffc;
            }
            if (octave && octave[(size_t)f * cap + x] == -5) keep = false;
        }
        const unsigned long long bk = __ballot(keep);
        if (lane == 0) sh.red[j * kDbWaves + w] = __popcll(bk);
        bits |= (keep ? 1u : 0u) << j;
    }
    __syncthreads();
    if (w == 0) db_scan_counts(sh.red, &sh.tot[1]);
    __syncthreads();
    int32_t *out = keptIdx + (size_t)f * cap;
#pragma unroll
    for (int j = 0; j < kDbChunks; ++j) {
        const bool keep = (bits >> j) & 1u;
        const unsigned long long bk = __ballot(keep);
        if (keep) out[sh.red[j * kDbWaves + w] + __popcll(bk & ((1ull << lane) - 1ull))] = j * kDbBlock + tid;
    }
    if (tid == 0) nkept[f] = sh.tot[1];
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the bound, the launch and the entry points
namespace {

// the least double s with (double)(float)sqrt(s) >= eps; the rounded root is monotone in s
double dbscan_bound(double eps)
{
    if (!(eps > 0.0)) return 0.0; // also NaN: nothing is a neighbour
    return least_double_where([eps](double s) { return (double)(float)std::sqrt(s) >= eps; });
}

int dbscan_launch(PsContext *ctx, const float *xy, const int32_t *octave, const int32_t *counts, int n0, int frames, int cap,
                  double eps, int minPts, int ffc, int32_t *keptIdx, int32_t *nkept)
{
    hipLaunchKernelGGL(ps_dbscan_kernel, dim3((unsigned)frames), dim3(kDbBlock), dbscan_lds_bytes(cap), ctx->stream,
                       reinterpret_cast<const float2 *>(xy), octave, counts, n0, cap, dbscan_bound(eps), minPts, ffc, keptIdx,
                       nkept);
    PS_HIP(hipGetLastError());
    return PS_OK;
}
} // namespace

static void dbscan_kernel_attributes()
{
    // 20 bytes of per-point state per keypoint
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ps_dbscan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dbscan_lds_bytes(PS_DBSCAN_MAX_KPTS));
}

extern "C" {

double ps_debug_dbscan_bound(double eps) { return dbscan_bound(eps); }

int ps_dbscan_thin(PsContext *ctx, const float *xy, size_t xyStride, const int32_t *octave, size_t octaveStride, int n,
                   double eps, int minPts, int featuresFromCluster, int32_t *keptIdx, int *nkept)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (nkept) *nkept = 0;
    if (xyStride == 0) xyStride = 8;
    if (octaveStride == 0) octaveStride = 4;
    if (!nkept || n < 0 || n > PS_DBSCAN_MAX_KPTS || xyStride < 8 || octaveStride < 4 || (n > 0 && (!xy || !keptIdx)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_dbscan_thin: bad argument (n must lie in 0 .. PS_DBSCAN_MAX_KPTS, strides >= 8 / 4 bytes)");
    if (n == 0) return PS_OK;
    std::vector<float> hxy((size_t)n * 2);
    const char *pxy = reinterpret_cast<const char *>(xy);
    for (int i = 0; i < n; ++i) std::memcpy(&hxy[(size_t)i * 2], pxy + (size_t)i * xyStride, 8);
    std::vector<int32_t> hoct;
    if (octave) {
        hoct.resize((size_t)n);
        const char *po = reinterpret_cast<const char *>(octave);
        for (int i = 0; i < n; ++i) std::memcpy(&hoct[(size_t)i], po + (size_t)i * octaveStride, 4);
    }
    PS_ENSURE(ctx->sMisc0, (size_t)n * 8);
    if (octave) PS_ENSURE(ctx->sMisc1, (size_t)n * 4);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 4);
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, hxy.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (octave) PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, hoct.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    rc = dbscan_launch(ctx, (const float *)ctx->sMisc0.p, octave ? (const int32_t *)ctx->sMisc1.p : nullptr, nullptr, n, 1, n, eps,
                       minPts, featuresFromCluster, (int32_t *)ctx->sMisc2.p, (int32_t *)ctx->sNumM.p);
    if (rc) return rc;
    int32_t nk = 0;
    PS_HIP(hipMemcpyAsync(&nk, ctx->sNumM.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipMemcpyAsync(keptIdx, ctx->sMisc2.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    *nkept = nk;
    return PS_OK;
}

int ps_dbscan_thin_device(PsContext *ctx, const float *xy, const int32_t *octave, const int32_t *counts, int frames, int capacity,
                          double eps, int minPts, int featuresFromCluster, int32_t *keptIdx, int32_t *nkept)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (frames < 0 || (frames > 0 && (capacity < 1 || capacity > PS_DBSCAN_MAX_KPTS || !xy || !counts || !keptIdx || !nkept)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_dbscan_thin_device: bad argument (capacity must lie in 1 .. PS_DBSCAN_MAX_KPTS)");
    if (frames == 0) return PS_OK;
    return dbscan_launch(ctx, xy, octave, counts, 0, frames, capacity, eps, minPts, featuresFromCluster, keptIdx, nkept);
}

} // extern "C"
