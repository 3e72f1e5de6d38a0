// ps_exclusion.h -- the spatial-exclusion filters of the per-frame front end: features that lie too close to features already
// held are rejected.  Three reference loops, one rule (PsExclusionRule, include/putslam_hip.h):
//  * PUTSLAM::chooseFeaturesToAddToMap + removeCloseFeatures (src/PUTSLAM/PUTSLAM.cpp:53-178): greedy in index order against the
//    visible map features and the candidates accepted before, 3-D (float norm) or 2-D (DBScan's predicate), depth gate, cap;
//  * Matcher::mergeTrackedFeatures (src/Matcher/matcher.cpp:97-130): greedy, 2-D only (double root), no gate, no cap;
//  * Matcher::removeTooCloseFeatures (matcher.cpp:886-974): j goes iff ANY earlier i is near it, removed or not.
// Every predicate is decided as  squared sum < bound  with the bound found on the host (no device sqrt); a NaN makes it false.
//
// Shape: three launches on one stream.
//  1. ps_excl_sweep<0>: candidates x existing set, the existing set staged through LDS in tiles of 256, the tile range split
//     over blockIdx.z where the batch is small; writes flag[j] = 1 for a candidate that is blocked or fails the depth gate.
//     The all-earlier rule runs the same sweep once more against the candidates themselves (<1>: k < j) and is done.
//  2. ps_excl_sweep<2>: every pair of unflagged candidates once; a near pair is joined in a union-find in global memory whose
//     roots are the least index of their tree (ps_block.h's lock-free form, DBScan's, at agent scope).  Connected components of the
//     conflict graph never interact: the greedy choice of one does not depend on another.
//  3. ps_excl_resolve, one work-group per frame: components of up to 32 members are replayed one per lane in index order; larger
//     ones cooperatively -- the least undecided index is accepted, every thread rejects its own undecided members near it, one
//     barrier a step, at most one step per accepted member (dense blob: one step; chain of n: n / 2 steps).  Then the cap by a
//     prefix count and the survivors by a stable compaction.  Per-point state lives in LDS, 11 bytes a candidate.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ps_block.h" // uf_union (here at agent scope)
#include "ps_dbscan.h"
#include "ps_device_math.h"
#include "ps_glue.h"

namespace psdev {

constexpr int kExTile = 256; // threads of a sweep work-group = candidates per chunk = entries of an LDS tile
constexpr int kExBlock = 1024;
constexpr int kExWaves = kExBlock / 64;
constexpr int kExChunks = PS_EXCL_MAX_CAND / kExBlock; // candidates per thread of the resolving work-group, at most
constexpr int kExLaneMax = 32;                          // components this small are replayed by one lane
constexpr int kExBigMax = PS_EXCL_MAX_CAND / (kExLaneMax + 1) + 1;
constexpr uint16_t kExEnd = 0xFFFF;
static_assert(PS_EXCL_MAX_CAND % kExBlock == 0 && PS_EXCL_MAX_CAND < 0xFFFF, "u16 links, whole chunks");
static_assert(kExChunks * kExWaves == 128, "db_scan_counts: two entries per lane of one wave");
// st[]: undecided, accepted, rejected (also: flagged by the sweep)
constexpr uint8_t kExUndecided = 0, kExAccepted = 1, kExRejected = 2;

// dynamic LDS of ps_excl_resolve for `cap` candidates: comp int, aux int, nxt u16, st u8
__host__ __device__ inline size_t excl_lds_bytes(int cap) { return (size_t)cap * 11; }

struct ExPt {
    float x, y, z, u, v;
};

__device__ __forceinline__ ExPt ex_load(const float *__restrict__ p3, const float *__restrict__ p2, int i)
{
    ExPt p = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (p3) {
        p.x = p3[3 * i];
        p.y = p3[3 * i + 1];
        p.z = p3[3 * i + 2];
    }
    if (p2) {
        p.u = p2[2 * i];
        p.v = p2[2 * i + 1];
    }
    return p;
}

// near3 || near2 of the rule.  F32: Eigen's (a - b).norm() on Vector3f, the sum in the order ps_map_match.h uses; F64: the
// doubles of the float differences, summed left to right (matcher.cpp:905-908); 2-D: cv::norm's exact double products.
__device__ __forceinline__ bool ex_near(const PsExclusionRule &r, const ExPt &a, const ExPt &b)
{
    bool hit = false;
    if (r.form3 != PS_EXCL_NONE) {
        const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z;
        if (r.form3 == PS_EXCL_F32) {
            const float s = d0 * d0 + (d1 * d1 + d2 * d2);
            hit = (double)s < r.bound3;
        } else {
            const double x = (double)d0, y = (double)d1, z = (double)d2;
            const double s = x * x + y * y + z * z;
            hit = s < r.bound3;
        }
    }
    if (r.form2 != PS_EXCL_NONE) {
        const float du = a.u - b.u, dv = a.v - b.v;
        const double s = (double)du * (double)du + (double)dv * (double)dv;
        hit = hit || s < r.bound2;
    }
    return hit;
}

// Work-group (chunk c of frame f, split z): the 256 candidates c * 256 ... against
//   MODE 0: the existing set of the frame             -> flag (also: depth gate; par[i] = i)
//   MODE 1: every earlier candidate                   -> flag
//   MODE 2: every earlier unflagged candidate         -> union, for unflagged candidates
// Tiles t = z, z + zsplit, ... of the other set pass through LDS.  A frame whose counts lie outside their capacity is left alone.
template <int MODE>
__global__ __launch_bounds__(kExTile) void ps_excl_sweep(PsExclusionRule rule, const float *__restrict__ cand3,
                                                         const float *__restrict__ cand2, const int32_t *__restrict__ candCounts,
                                                         int n0, int capC, const float *__restrict__ ex3,
                                                         const float *__restrict__ ex2, const int32_t *__restrict__ exCounts, int m0,
                                                         int capE, int chunks, uint8_t *__restrict__ flags, int32_t *__restrict__ par)
{
    __shared__ float4 s3[kExTile];
    __shared__ float2 s2[kExTile];
    __shared__ uint8_t sF[kExTile];
    const int tid = (int)threadIdx.x;
    const int f = (int)blockIdx.x / chunks, c = (int)blockIdx.x % chunks, zsplit = (int)gridDim.z;
    const int n = candCounts ? candCounts[f] : n0, m = exCounts ? exCounts[f] : m0;
    if (n < 0 || n > capC || m < 0 || m > capE) return;
    const int i0 = c * kExTile, i = i0 + tid;
    if (i0 >= n) return;
    const bool valid = i < n;
    const float *__restrict__ a3 = cand3 ? cand3 + (size_t)f * capC * 3 : nullptr;
    const float *__restrict__ a2 = cand2 ? cand2 + (size_t)f * capC * 2 : nullptr;
    const float *__restrict__ b3 = MODE == 0 ? (ex3 ? ex3 + (size_t)f * capE * 3 : nullptr) : a3;
    const float *__restrict__ b2 = MODE == 0 ? (ex2 ? ex2 + (size_t)f * capE * 2 : nullptr) : a2;
    uint8_t *__restrict__ flg = flags + (size_t)f * capC;
    int32_t *__restrict__ pr = par ? par + (size_t)f * capC : nullptr;
    const int kEnd = MODE == 0 ? m : (n < i0 + kExTile ? n : i0 + kExTile);
    const ExPt a = ex_load(a3, a2, valid ? i : i0);
    bool hit = false;     // MODE 0 / 1: flagged
    bool active = valid;  // takes part in the tests
    if (MODE == 0) {
        if (rule.depthGate && !((double)a.z > rule.depthMin && (double)a.z < rule.depthMax)) hit = true;
        if (blockIdx.z == 0 && valid && pr) pr[i] = i;
    }
    if (MODE == 2) active = valid && flg[i] == 0;
    for (int t = (int)blockIdx.z; t * kExTile < kEnd; t += zsplit) {
        const int k = t * kExTile + tid;
        if (k < kEnd) {
            const ExPt b = ex_load(b3, b2, k);
            s3[tid] = make_float4(b.x, b.y, b.z, 0.f);
            s2[tid] = make_float2(b.u, b.v);
            if (MODE == 2) sF[tid] = flg[k];
        }
        __syncthreads();
        const int lim = kEnd - t * kExTile < kExTile ? kEnd - t * kExTile : kExTile;
        if (__ballot(active && !(MODE != 2 && hit)) != 0ull) { // (wave-uniform: a wave with nothing left to decide skips the tile)
            for (int kk = 0; kk < lim; ++kk) {
                if (MODE == 2 && sF[kk]) continue;
                const float4 q3 = s3[kk];
                const float2 q2 = s2[kk];
                const ExPt b = {q3.x, q3.y, q3.z, q2.x, q2.y};
                const bool nr = active && (MODE == 0 || t * kExTile + kk < i) && ex_near(rule, b, a);
                if (MODE == 2) {
                    if (nr) uf_union<__HIP_MEMORY_SCOPE_AGENT>(pr, i, t * kExTile + kk); // (par[] is shared by the work-groups of a frame)
                } else {
                    hit = hit || nr;
                }
            }
        }
        __syncthreads();
    }
    if (MODE != 2 && valid && hit) flg[i] = 1;
}

struct ExShared {
    int red[kExChunks * kExWaves];
    int mins[2][kExWaves];
    int tot;
    int nBig;
    int big[kExBigMax];
};

// One work-group per frame: flags + union-find of the sweeps -> keptIdx[f][0 .. nkept[f]) ascending; nkept[f] = -1 for a frame
// whose counts lie outside their capacity.
__global__ __launch_bounds__(kExBlock) void ps_excl_resolve(PsExclusionRule rule, const float *__restrict__ cand3,
                                                            const float *__restrict__ cand2, const int32_t *__restrict__ candCounts,
                                                            int n0, int capC, const int32_t *__restrict__ exCounts, int m0, int capE,
                                                            const uint8_t *__restrict__ flags, const int32_t *__restrict__ par,
                                                            int32_t *__restrict__ keptIdx, int32_t *__restrict__ nkept)
{
    extern __shared__ __align__(16) unsigned char exLds[];
    __shared__ ExShared sh;
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = candCounts ? candCounts[f] : n0, m = exCounts ? exCounts[f] : m0;
    if (n < 0 || n > capC || m < 0 || m > capE) {
        if (tid == 0) nkept[f] = -1;
        return;
    }
    int *comp = reinterpret_cast<int *>(exLds);
    int *aux = reinterpret_cast<int *>(exLds + (size_t)capC * 4);
    uint16_t *nxt = reinterpret_cast<uint16_t *>(exLds + (size_t)capC * 8);
    uint8_t *st = exLds + (size_t)capC * 10;
    const float *__restrict__ a3 = cand3 ? cand3 + (size_t)f * capC * 3 : nullptr;
    const float *__restrict__ a2 = cand2 ? cand2 + (size_t)f * capC * 2 : nullptr;
    const uint8_t *__restrict__ flg = flags + (size_t)f * capC;
    const bool greedy = rule.mode == PS_EXCL_GREEDY;

    if (greedy) {
        const int32_t *__restrict__ pr = par + (size_t)f * capC;
        // the sweeps have finished: the forest is stable, plain loads find the roots
        for (int i = tid; i < n; i += kExBlock) {
            const bool blocked = flg[i] != 0;
            int r = -1;
            if (!blocked) {
                r = i;
                for (int p = pr[r]; p != r; p = pr[r]) r = p;
            }
            comp[i] = r;
            st[i] = blocked ? kExRejected : kExUndecided;
            aux[i] = 0;
        }
        if (tid == 0) sh.nBig = 0;
        __syncthreads();
        for (int i = tid; i < n; i += kExBlock)
            if (comp[i] >= 0) atomicAdd(&aux[comp[i]], 1);
        __syncthreads();
        // small components, one lane each: link the members in ascending order, replay the greedy loop
        for (int r = tid; r < n; r += kExBlock) {
            if (comp[r] != r) continue;
            const int cnt = aux[r];
            if (cnt == 1) {
                st[r] = kExAccepted;
                continue;
            }
            if (cnt > kExLaneMax) {
                sh.big[atomicAdd(&sh.nBig, 1)] = r;
                continue;
            }
            int prev = r;
            for (int k = r + 1, got = 1; got < cnt && k < n; ++k)
                if (comp[k] == r) {
                    nxt[prev] = (uint16_t)k;
                    prev = k;
                    ++got;
                }
            nxt[prev] = kExEnd;
            for (int i = r; i != kExEnd; i = nxt[i]) {
                if (st[i] != kExUndecided) continue;
                st[i] = kExAccepted;
                const ExPt pi = ex_load(a3, a2, i);
                for (int k = nxt[i]; k != kExEnd; k = nxt[k])
                    if (st[k] == kExUndecided && ex_near(rule, pi, ex_load(a3, a2, k))) st[k] = kExRejected;
            }
        }
        __syncthreads();
        // large components, cooperatively: every thread keeps its own candidates in registers and decides only those
        const int nBig = sh.nBig;
        if (nBig > 0) {
            ExPt own[kExChunks];
#pragma unroll
            for (int j = 0; j < kExChunks; ++j) {
                const int k = j * kExBlock + tid;
                own[j] = ex_load(a3, a2, k < n ? k : 0);
            }
            int step = 0;
            for (int b = 0; b < nBig; ++b) {
                const int r = sh.big[b];
                unsigned und = 0; // own undecided members of the component
#pragma unroll
                for (int j = 0; j < kExChunks; ++j) {
                    const int k = j * kExBlock + tid;
                    if (k < n && comp[k] == r) und |= 1u << j;
                }
                for (;;) {
                    int best = INT_MAX;
#pragma unroll
                    for (int j = 0; j < kExChunks; ++j) {
                        const unsigned long long bc = __ballot((und >> j) & 1u);
                        if (bc && best == INT_MAX) best = j * kExBlock + w * 64 + (__ffsll((long long)bc) - 1);
                    }
                    if (lane == 0) sh.mins[step & 1][w] = best;
                    __syncthreads();
                    int seed = INT_MAX;
                    for (int i = 0; i < kExWaves; ++i) seed = min(seed, sh.mins[step & 1][i]);
                    ++step; // (the other half of mins[] is written next: no second barrier)
                    if (seed == INT_MAX) break;
                    const ExPt ps = ex_load(a3, a2, seed);
#pragma unroll
                    for (int j = 0; j < kExChunks; ++j) {
                        if (!((und >> j) & 1u)) continue;
                        const int k = j * kExBlock + tid;
                        if (k == seed) {
                            st[k] = kExAccepted;
                            und &= ~(1u << j);
                        } else if (ex_near(rule, ps, own[j])) {
                            st[k] = kExRejected;
                            und &= ~(1u << j);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }

    // the cap by a prefix count, the survivors in ascending order
    const int room = rule.maxKeep < 0 ? INT_MAX : rule.maxKeep;
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < kExChunks; ++j) {
        const int k = j * kExBlock + tid;
        const bool keep = k < n && (greedy ? st[k] == kExAccepted : flg[k] == 0);
        const unsigned long long bk = __ballot(keep);
        if (lane == 0) sh.red[j * kExWaves + w] = __popcll(bk);
        bits |= (keep ? 1u : 0u) << j;
    }
    __syncthreads();
    if (w == 0) db_scan_counts(sh.red, &sh.tot);
    __syncthreads();
    int32_t *out = keptIdx + (size_t)f * capC;
#pragma unroll
    for (int j = 0; j < kExChunks; ++j) {
        const bool keep = (bits >> j) & 1u;
        const unsigned long long bk = __ballot(keep);
        const int pos = sh.red[j * kExWaves + w] + __popcll(bk & ((1ull << lane) - 1ull));
        if (keep && pos < room) out[pos] = j * kExBlock + tid;
    }
    if (tid == 0) nkept[f] = sh.tot < room ? sh.tot : room;
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the bounds, the rules, the launches and the entry points
namespace {

// the least double s with sqrt(s) >= d (dbscan_bound without the rounding to float)
double sqrt_bound_f64(double d)
{
    if (!(d > 0.0)) return 0.0; // also NaN: nothing passes
    return least_double_where([d](double s) { return std::sqrt(s) >= d; });
}

const char *exclusion_rule_error(const PsExclusionRule *r)
{
    if (!r) return "null rule";
    if (r->form3 != PS_EXCL_NONE && r->form3 != PS_EXCL_F32 && r->form3 != PS_EXCL_F64) return "rule: unknown form3";
    if (r->form2 != PS_EXCL_NONE && r->form2 != PS_EXCL_F64) return "rule: unknown form2";
    if (r->mode != PS_EXCL_GREEDY && r->mode != PS_EXCL_ALL_EARLIER) return "rule: unknown mode";
    return nullptr;
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// the three launches; flags / par: frames x capC scratch of the context.  n0 / m0 stand in for null counts.
int exclusion_launch(PsContext *ctx, const PsExclusionRule &rule, const float *cand3, const float *cand2, const int32_t *candCounts,
                     int n0, int capC, const float *ex3, const float *ex2, const int32_t *exCounts, int m0, int capE, int frames,
                     int32_t *keptIdx, int32_t *nkept)
{
    const bool greedy = rule.mode == PS_EXCL_GREEDY;
    PS_ENSURE(ctx->exFlag, (size_t)frames * capC);
    if (greedy) PS_ENSURE(ctx->exPar, (size_t)frames * capC * sizeof(int32_t));
    uint8_t *flags = (uint8_t *)ctx->exFlag.p;
    int32_t *par = greedy ? (int32_t *)ctx->exPar.p : nullptr;
    PS_HIP(hipMemsetAsync(flags, 0, (size_t)frames * capC, ctx->stream));
    const int chunks = ceil_div(capC, kExTile);
    const long long groups = (long long)frames * chunks;
    // a small batch splits the other set's tiles over blockIdx.z until a thousand work-groups are in flight
    const int want = groups >= 1024 ? 1 : (int)ceil_div(1024, (int)groups);
    const int tilesE = ceil_div(capE > 0 ? capE : 1, kExTile);
    const int zE = want < tilesE ? want : tilesE, zC = want < chunks ? want : chunks;
    const dim3 block(kExTile);
    hipLaunchKernelGGL(ps_excl_sweep<0>, dim3((unsigned)groups, 1, (unsigned)zE), block, 0, ctx->stream, rule, cand3, cand2,
                       candCounts, n0, capC, ex3, ex2, exCounts, m0, capE, chunks, flags, par);
    PS_HIP(hipGetLastError());
    if (greedy)
        hipLaunchKernelGGL(ps_excl_sweep<2>, dim3((unsigned)groups, 1, (unsigned)zC), block, 0, ctx->stream, rule, cand3, cand2,
                           candCounts, n0, capC, ex3, ex2, exCounts, m0, capE, chunks, flags, par);
    else
        hipLaunchKernelGGL(ps_excl_sweep<1>, dim3((unsigned)groups, 1, (unsigned)zC), block, 0, ctx->stream, rule, cand3, cand2,
                           candCounts, n0, capC, ex3, ex2, exCounts, m0, capE, chunks, flags, par);
    PS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ps_excl_resolve, dim3((unsigned)frames), dim3(kExBlock), greedy ? excl_lds_bytes(capC) : 0, ctx->stream, rule,
                       cand3, cand2, candCounts, n0, capC, exCounts, m0, capE, (const uint8_t *)flags, (const int32_t *)par, keptIdx,
                       nkept);
    PS_HIP(hipGetLastError());
    return PS_OK;
}
} // namespace

static void exclusion_kernel_attributes()
{
    // 11 bytes of per-candidate state
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ps_excl_resolve), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)excl_lds_bytes(PS_EXCL_MAX_CAND));
}

extern "C" {

size_t ps_abi_sizeof_exclusion_rule(void) { return sizeof(PsExclusionRule); }

double ps_sqrt_bound_f64(double d) { return sqrt_bound_f64(d); }

int ps_exclusion_rule_new_map_features(double minEuclideanDistanceOfFeatures, double minImageDistanceOfFeatures,
                                       int maxOnceFeatureAdd, PsExclusionRule *rule)
{
    if (!rule) return PS_ERR_BAD_ARG;
    // the thresholds arrive through float parameters (PUTSLAM.cpp:101) and are compared as doubles (:62,68)
    const double dE = (double)(float)minEuclideanDistanceOfFeatures, dI = (double)(float)minImageDistanceOfFeatures;
    *rule = PsExclusionRule{};
    rule->bound3 = (double)sq_bound_f32(dE);
    rule->bound2 = dbscan_bound(dI);
    rule->depthMin = 0.8;
    rule->depthMax = 6.0;
    rule->form3 = PS_EXCL_F32;
    rule->form2 = PS_EXCL_F64;
    rule->mode = PS_EXCL_GREEDY;
    rule->maxKeep = maxOnceFeatureAdd > 0 ? maxOnceFeatureAdd : 0;
    rule->depthGate = 1;
    return PS_OK;
}

int ps_exclusion_rule_merge_tracked(double minimalReprojDistanceNewTrackingFeatures, PsExclusionRule *rule)
{
    if (!rule) return PS_ERR_BAD_ARG;
    *rule = PsExclusionRule{};
    rule->bound2 = sqrt_bound_f64(minimalReprojDistanceNewTrackingFeatures);
    rule->form3 = PS_EXCL_NONE;
    rule->form2 = PS_EXCL_F64;
    rule->mode = PS_EXCL_GREEDY;
    rule->maxKeep = -1;
    return PS_OK;
}

int ps_exclusion_rule_too_close(double minimalEuclidDistanceNewTrackingFeatures, double minimalReprojDistanceNewTrackingFeatures,
                                PsExclusionRule *rule)
{
    if (!rule) return PS_ERR_BAD_ARG;
    *rule = PsExclusionRule{};
    rule->bound3 = sqrt_bound_f64(minimalEuclidDistanceNewTrackingFeatures);
    rule->bound2 = sqrt_bound_f64(minimalReprojDistanceNewTrackingFeatures);
    rule->form3 = PS_EXCL_F64;
    rule->form2 = PS_EXCL_F64;
    rule->mode = PS_EXCL_ALL_EARLIER;
    rule->maxKeep = -1;
    return PS_OK;
}

int ps_exclude(PsContext *ctx, const PsExclusionRule *rule, const float *cand3, const float *cand2, int n, const float *exist3,
               const float *exist2, int m, int32_t *keptIdx, int *nkept)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (const char *why = exclusion_rule_error(rule)) return fail(ctx, PS_ERR_BAD_ARG, why);
    if (!nkept || n < 0 || m < 0) return fail(ctx, PS_ERR_BAD_ARG, "ps_exclude: bad argument (null nkept or a negative count)");
    if (n > PS_EXCL_MAX_CAND || m > PS_MAX_KPTS)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_exclude: more than PS_EXCL_MAX_CAND candidates or PS_MAX_KPTS existing features");
    const bool need3 = rule->form3 != PS_EXCL_NONE, need2 = rule->form2 != PS_EXCL_NONE;
    if (n > 0 && (!keptIdx || ((need3 || rule->depthGate) && !cand3) || (need2 && !cand2)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_exclude: null candidate array or keptIdx");
    if (n > 0 && m > 0 && ((need3 && !exist3) || (need2 && !exist2)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_exclude: null array of existing features");
    if (n == 0) {
        *nkept = 0;
        return PS_OK;
    }
    TimingOff toff(ctx);
    const bool up3 = cand3 && (need3 || rule->depthGate), e3 = m > 0 && need3, e2 = m > 0 && need2;
    if (up3) PS_ENSURE(ctx->sMisc0, (size_t)n * 12);
    if (need2) PS_ENSURE(ctx->sMisc1, (size_t)n * 8);
    if (e3) PS_ENSURE(ctx->sDesc, (size_t)m * 12);
    if (e2) PS_ENSURE(ctx->sMatches, (size_t)m * 8);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 4);
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    if (up3) PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, cand3, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    if (need2) PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, cand2, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (e3) PS_HIP(hipMemcpyAsync(ctx->sDesc.p, exist3, (size_t)m * 12, hipMemcpyHostToDevice, ctx->stream));
    if (e2) PS_HIP(hipMemcpyAsync(ctx->sMatches.p, exist2, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = exclusion_launch(ctx, *rule, up3 ? (const float *)ctx->sMisc0.p : nullptr, need2 ? (const float *)ctx->sMisc1.p : nullptr,
                          nullptr, n, n, e3 ? (const float *)ctx->sDesc.p : nullptr, e2 ? (const float *)ctx->sMatches.p : nullptr,
                          nullptr, m, m, 1, (int32_t *)ctx->sMisc2.p, (int32_t *)ctx->sNumM.p);
    if (rc) return rc;
    int32_t nk = 0;
    std::vector<int32_t> kept((size_t)n);
    PS_HIP(hipMemcpyAsync(&nk, ctx->sNumM.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipMemcpyAsync(kept.data(), ctx->sMisc2.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    if (nk < 0 || nk > n) return fail(ctx, PS_ERR_HIP, "ps_exclude: the device returned an impossible count");
    std::memcpy(keptIdx, kept.data(), (size_t)nk * 4);
    *nkept = nk;
    return PS_OK;
}

int ps_exclude_device(PsContext *ctx, const PsExclusionRule *rule, const float *cand3, const float *cand2,
                      const int32_t *candCounts, int candCapacity, const float *exist3, const float *exist2,
                      const int32_t *existCounts, int existCapacity, int frames, int32_t *keptIdx, int32_t *nkept)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (const char *why = exclusion_rule_error(rule)) return fail(ctx, PS_ERR_BAD_ARG, why);
    if (frames < 0 || candCapacity < 1 || existCapacity < 0)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_exclude_device: bad argument (frames >= 0, candCapacity >= 1, existCapacity >= 0)");
    if (candCapacity > PS_EXCL_MAX_CAND || existCapacity > PS_MAX_KPTS)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_exclude_device: candCapacity above PS_EXCL_MAX_CAND or existCapacity above PS_MAX_KPTS");
    if (frames == 0) return PS_OK;
    const bool need3 = rule->form3 != PS_EXCL_NONE, need2 = rule->form2 != PS_EXCL_NONE;
    if (!candCounts || !keptIdx || !nkept || ((need3 || rule->depthGate) && !cand3) || (need2 && !cand2))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_exclude_device: null candidate array, counts or output");
    if (existCapacity > 0 && (!existCounts || (need3 && !exist3) || (need2 && !exist2)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_exclude_device: null array of existing features");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx}; // (the context's scratch is in use until the launches have run)
    return exclusion_launch(ctx, *rule, (need3 || rule->depthGate) ? cand3 : nullptr, need2 ? cand2 : nullptr, candCounts, 0,
                            candCapacity, existCapacity > 0 && need3 ? exist3 : nullptr, existCapacity > 0 && need2 ? exist2 : nullptr,
                            existCapacity > 0 ? existCounts : nullptr, 0, existCapacity, frames, keptIdx, nkept);
}

} // extern "C"
