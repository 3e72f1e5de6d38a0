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
//     roots are the least index of their tree (the lock-free form of ps_dbscan.h at agent scope).  Connected components of the
//     conflict graph never interact: the greedy choice of one does not depend on another.
//  3. ps_excl_resolve, one work-group per frame: components of up to 32 members are replayed one per lane in index order; larger
//     ones cooperatively -- the least undecided index is accepted, every thread rejects its own undecided members near it, one
//     barrier a step, at most one step per accepted member (dense blob: one step; chain of n: n / 2 steps).  Then the cap by a
//     prefix count and the survivors by a stable compaction.  Per-point state lives in LDS, 11 bytes a candidate.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ps_dbscan.h"
#include "putslam_hip.h"

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

// union-find in global memory, shared by the work-groups of a frame; every root is the least index of its tree
__device__ __forceinline__ int ex_find(int32_t *par, int x)
{
    int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        const int g = __hip_atomic_load(&par[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g != p) __hip_atomic_store(&par[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // path halving
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void ex_union(int32_t *par, int a, int b)
{
    for (;;) {
        a = ex_find(par, a);
        b = ex_find(par, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(&par[b], b, a);
        if (old == b) return;
        b = old; // b was hooked meanwhile: retry from where it went
    }
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
                    if (nr) ex_union(pr, i, t * kExTile + kk);
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
