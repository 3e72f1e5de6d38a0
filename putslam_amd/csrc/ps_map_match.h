// ps_map_match.h -- guided map matching: Matcher::matchXYZ (reference src/Matcher/matcher.cpp:694-746) for P (map view, frame)
// pairs of a device-resident batch in two launches, no host step, for 32-byte binary rows (ps_match_xyz_device /
// ps_map_pairs_device, include/putslam_hip.h) and, through ps_map_match_l2.h, for SURF / SIFT float rows; the host-pointer
// forms (ps_match_xyz here, ps_match_xyz_l2_f32 there) stage one pair and take the same two launches (match_xyz_host).
// The rule, per map feature j:
//   candidate i : |mapPos[j] - curPos[i]| < sphereRadius (float norm against a double radius, exact
//                 squared-domain bound) and |predictedLevel[i] - level[j]| <= 1          (:699-711)
//   value(i)    : popcount of the per-byte SATURATING difference mapDesc[j] - curDesc[i]
//                 (cv::Mat subtraction of CV_8U + NORM_HAMMING, :719-721 -- not XOR Hamming; float rows: ps_map_match_l2.h)
//   best        : smallest value, first index on ties                                      (:714-727)
//   accepted    : acceptRatio * value <= best (double)                                     (:734-746)
// and the output is ordered by (j, i) like the reference's push_back loop.
//
//   map_sweep<F, D>   THE sweep, once, for a descriptor policy D; the kernels ps_map_sweep<F> (MapBinRows, below) and
//                     ps_map_sweep_l2<F> (MapL2Rows, ps_map_match_l2.h) are its two instantiations.
//                     Grid P x chunks, a chunk = 4 waves x F map features.  The frame's positions and levels pass through LDS
//                     once per work-group, 1024 keypoints at a time; a wave holds its F features in scalar registers, so one LDS
//                     read serves F sphere tests.  Candidates are rare (0 - 3 per feature at the first try of the retry ladder,
//                     up to 14 at the tenth): a feature's candidates (i, value bits) are appended in ballot order -- ascending
//                     i -- to a stash of kMapStash entries in LDS, and best / ratio / emit work on that list.  A feature with
//                     more candidates than the stash holds is swept again from global memory (map_resweep).  The chunk's accepted matches, ordered by (j, i), go to a place in the pair's row of a
//                     staging block that the chunk reserves with ONE atomic add; (start, count) are kept per chunk.
//   ps_map_emit       grid P.  Scans the pair's chunk counts and moves the chunks to the output row in chunk order -- the
//                     (j, i) order of the reference's push_back loop whatever order the chunks ran in -- and, in the same pass
//                     over the matches, does what ps_prep_from_matches does for one pair: depth filter, ordered compaction,
//                     scoring records, bounds, the scoring stage's counters cleared.
// A pair whose count exceeds the row capacity reports -(count) and is handed to RANSAC with no matches.
//
// A descriptor policy D holds what a candidate's VALUE is, and nothing of the decomposition:
//   D::Args                      the kernel's argument block: MapArgs m, then the descriptor pointers and strides
//   D(args, view, frame)         the rows of the pair's map view and frame
//   D::Best, D::none()           what a lane keeps per feature across the tile loop
//   hit(j, i, best)              inside the rare hit branch: the value bits stashed beside i (binary: the value, evaluated
//                                there; float: nothing yet -- a row is 256 - 2048 B and is not touched there)
//   values<F>(lists, cnt, jw)    the value phase of the wave's F lists between the tile loop and best / ratio (binary: none)
//   best_value(best, list, cnt, s)  bestVal of a feature with cnt > 0 candidates
//   value(j, i)                  one lane, one candidate, from global memory: map_resweep's value
#pragma once
#include "ps_block.h" // the integer and flag scans, wave minima
#include "ps_glue.h"
#include "ps_pair_records.h" // PrepArgs, RecPtrs, PairRecords
#include "ps_ransac_stage.h" // Plan, make_plan, prepare_score, ensure_records, rec_ptrs, run_ransac_stage

namespace psdev {

constexpr int kMapBlock = 256;  // 4 waves
constexpr int kMapWaves = kMapBlock / 64;
constexpr int kMapTile = 1024;  // keypoints staged per trip: 16 KiB of LDS
constexpr int kMapStash = 16;   // candidates kept per map feature

// What the decomposition and ps_map_emit read (the descriptors are the policies')
struct MapArgs {
    const float *mapPts, *curPts;     // frame sets' points
    const int32_t *mapN, *curN;       // ... keypoint counts
    const int32_t *mapLevel, *curLevel; // [numFrames][maxKpts]
    int mapFrames, curFrames, mapCap, curCap;
    int mapPtsStride, curPtsStride;   // floats between frames
    const int32_t *pairs;             // P x (map view, frame)
    float radiusBound;
    double acceptRatio;
    const float *radiusPer;           // P or null
    const double *ratioPer;           // P or null
    int maxMatches;                   // row capacity
    int chunks;                       // chunks per pair = ceil(mapCap / chunk size)
    int chunkFeatures;                // 4 x F
    PsDMatch *tmp;                    // [P][maxMatches] staging rows
    int32_t *tmpCount;                // [P] matches reserved so far (cleared before the sweep)
    int32_t *chunkStart, *chunkCount; // [P][chunks]
};

// keypoints of a view / frame a pair may touch: 0 for an index outside the set, counts clamped to the row capacity
PS_D int map_count(const int32_t *__restrict__ n, int frame, int frames, int cap)
{
    if (frame < 0 || frame >= frames) return 0;
    const int v = n[frame];
    return v < 0 ? 0 : (v > cap ? cap : v);
}

// One map feature against the pair's frame: what a sweep from global memory needs
struct MapSphere {
    float mx, my, mz;
    int lj, j;
    const float *__restrict__ curPos;
    const int32_t *__restrict__ curLevel;
    int ncur;
    float radiusBound;
    double acceptRatio;
};

enum MapResweep { kMapLeast, kMapCount, kMapWrite };

// One wave, one map feature, the whole frame from global memory, a lane evaluating d.value(j, i) per candidate.
//   kMapLeast: returns the bits of the least non-NaN value among the candidates (+inf's bits if there is none);
//   kMapCount / kMapWrite: the number of candidates within the accept ratio of bestVal, ascending i; kMapWrite emits them from
//   out[0] on.
template <MapResweep MODE, class D> PS_D uint32_t map_resweep(const D &d, const MapSphere &s, float bestVal, PsDMatch *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    uint32_t n = 0, least = 0x7F800000u;
    for (int i0 = 0; i0 < s.ncur; i0 += 64) {
        const int i = i0 + lane;
        bool acc = false;
        float value = 0.f;
        if (i < s.ncur) {
            const float d0 = s.mx - s.curPos[3 * i], d1 = s.my - s.curPos[3 * i + 1], d2 = s.mz - s.curPos[3 * i + 2];
            const float sum = d0 * d0 + (d1 * d1 + d2 * d2);
            const int li = s.curLevel[i];
            if (sum < s.radiusBound && li - 1 <= s.lj && s.lj <= li + 1) {
                value = d.value(s.j, i);
                if (MODE == kMapLeast) {
                    if (value == value && __float_as_uint(value) < least) least = __float_as_uint(value);
                } else {
                    acc = s.acceptRatio * (double)value <= (double)bestVal;
                }
            }
        }
        if (MODE != kMapLeast) {
            const unsigned long long bal = __ballot(acc);
            if (MODE == kMapWrite && acc) {
                PsDMatch m;
                m.queryIdx = s.j;
                m.trainIdx = i;
                m.imgIdx = -1; // default-constructed cv::DMatch (matcher.cpp:741)
                m.distance = value;
                out[n + __popcll(bal & ((1ull << lane) - 1ull))] = m;
            }
            n += __popcll(bal);
        }
    }
    return MODE == kMapLeast ? wave_min_u32(least) : n;
}

template <int F, class D> PS_D void map_sweep(const typename D::Args &b)
{
    constexpr int CH = kMapWaves * F;
    const MapArgs &a = b.m;
    __shared__ uint4 s_tile[kMapTile];
    __shared__ uint2 s_stash[CH * kMapStash]; // (i, the value's float bits)
    __shared__ int s_n[CH];
    __shared__ int s_start;
    const int p = blockIdx.x / a.chunks, c = blockIdx.x - p * a.chunks;
    const int view = a.pairs[2 * p], frame = a.pairs[2 * p + 1];
    const int nmap = map_count(a.mapN, view, a.mapFrames, a.mapCap);
    const int ncur = map_count(a.curN, frame, a.curFrames, a.curCap);
    const int j0 = c * CH;
    if (j0 >= nmap || ncur == 0) { // (the whole work-group)
        if (threadIdx.x == 0) {
            a.chunkStart[(size_t)p * a.chunks + c] = 0;
            a.chunkCount[(size_t)p * a.chunks + c] = 0;
        }
        return;
    }
    const float radiusBound = a.radiusPer ? a.radiusPer[p] : a.radiusBound;
    const double acceptRatio = a.ratioPer ? a.ratioPer[p] : a.acceptRatio;
    const float *__restrict__ mapPos = a.mapPts + (size_t)view * a.mapPtsStride;
    const int32_t *__restrict__ mapLevel = a.mapLevel + (size_t)view * a.mapCap;
    const float *__restrict__ curPos = a.curPts + (size_t)frame * a.curPtsStride;
    const int32_t *__restrict__ curLevel = a.curLevel + (size_t)frame * a.curCap;
    const D d(b, view, frame);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long below = (1ull << lane) - 1ull;
    const int jw = j0 + w * F;                          // the wave's first feature
    uint2 *const lists = s_stash + w * F * kMapStash; // ... and its F lists

    // the wave's F map features: wave-uniform (a feature beyond the view gets a NaN position: no test passes)
    float mx[F], my[F], mz[F];
    int lj[F], cnt[F];
    typename D::Best best[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const int j = jw + f;
        const bool has = j < nmap;
        const int jc = has ? j : nmap - 1;
        mx[f] = has ? mapPos[3 * jc] : __builtin_nanf("");
        my[f] = mapPos[3 * jc + 1];
        mz[f] = mapPos[3 * jc + 2];
        lj[f] = mapLevel[jc];
        cnt[f] = 0;
        best[f] = D::none();
    }

    for (int t0 = 0; t0 < ncur; t0 += kMapTile) {
        const int nt = ncur - t0 < kMapTile ? ncur - t0 : kMapTile;
        __syncthreads(); // (the previous tile has been read)
        for (int i = threadIdx.x; i < nt; i += kMapBlock) {
            const int g = t0 + i;
            s_tile[i] = make_uint4(__float_as_uint(curPos[3 * g]), __float_as_uint(curPos[3 * g + 1]),
                                   __float_as_uint(curPos[3 * g + 2]), (uint32_t)curLevel[g]);
        }
        __syncthreads();
        for (int i0 = 0; i0 < nt; i0 += 64) {
            const int i = i0 + lane;
            const bool inb = i < nt;
            const uint4 q = s_tile[inb ? i : nt - 1];
            const float px = __uint_as_float(q.x), py = __uint_as_float(q.y), pz = __uint_as_float(q.z);
            const int li = (int)q.w;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const float d0 = mx[f] - px, d1 = my[f] - py, d2 = mz[f] - pz;
                const float s = d0 * d0 + (d1 * d1 + d2 * d2); // the reference's rounding (no contraction)
                const bool hit = inb && s < radiusBound && li - 1 <= lj[f] && lj[f] <= li + 1;
                const unsigned long long bal = __ballot(hit);
                if (bal != 0ull) { // (rare; wave-uniform)
                    if (hit) {
                        const int g = t0 + i;
                        const uint32_t bits = d.hit(jw + f, g, best[f]);
                        const int pos = cnt[f] + __popcll(bal & below);
                        if (pos < kMapStash) lists[f * kMapStash + pos] = make_uint2((uint32_t)g, bits);
                    }
                    cnt[f] += __popcll(bal);
                }
            }
        }
    }
    __syncthreads(); // the stash is complete
    d.template values<F>(lists, cnt, jw);

    // best / ratio over the short list (or further sweeps), the feature's accepted count
    const auto sphere = [&](int f) { return MapSphere{mx[f], my[f], mz[f], lj[f], jw + f, curPos, curLevel, ncur, radiusBound, acceptRatio}; };
    unsigned long long accMask[F];
    float bestVal[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        accMask[f] = 0ull;
        bestVal[f] = 0.f;
        int n = 0;
        if (cnt[f] > 0) {
            bestVal[f] = d.best_value(best[f], lists + f * kMapStash, cnt[f], sphere(f));
            if (cnt[f] <= kMapStash) {
                bool acc = false;
                if (lane < cnt[f]) acc = acceptRatio * (double)__uint_as_float(lists[f * kMapStash + lane].y) <= (double)bestVal[f];
                accMask[f] = __ballot(acc);
                n = __popcll(accMask[f]);
            } else {
                n = (int)map_resweep<kMapCount>(d, sphere(f), bestVal[f], nullptr);
            }
        }
        if (lane == 0) s_n[w * F + f] = n;
    }
    __syncthreads();
    int total = 0, before = 0; // accepted matches of the chunk / of the features in front of this wave's
    for (int k = 0; k < CH; ++k) {
        const int n = s_n[k];
        if (k < w * F) before += n;
        total += n;
    }
    if (threadIdx.x == 0) {
        const int start = total > 0 ? atomicAdd(&a.tmpCount[p], total) : 0;
        s_start = start;
        a.chunkStart[(size_t)p * a.chunks + c] = start;
        a.chunkCount[(size_t)p * a.chunks + c] = total;
    }
    __syncthreads();
    const int start = s_start;
    // the pair overflows its row (ps_map_emit reports it from the total): nothing of it is kept
    if (total == 0 || start < 0 || start > a.maxMatches - total) return;
    PsDMatch *__restrict__ out = a.tmp + (size_t)p * a.maxMatches + start + before;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        if (cnt[f] == 0) continue;
        if (cnt[f] <= kMapStash) {
            if ((accMask[f] >> lane) & 1ull) {
                const uint2 e = lists[f * kMapStash + lane];
                PsDMatch m;
                m.queryIdx = jw + f;
                m.trainIdx = (int)e.x;
                m.imgIdx = -1; // default-constructed cv::DMatch (matcher.cpp:741)
                m.distance = __uint_as_float(e.y);
                out[__popcll(accMask[f] & below)] = m;
            }
            out += __popcll(accMask[f]);
        } else {
            out += map_resweep<kMapWrite>(d, sphere(f), bestVal[f], out);
        }
    }
}

// popcount of the per-byte saturating difference a - b of two 32-byte rows
PS_D uint32_t satdiff_popc256(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    const uint32_t aw[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const uint32_t bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int d = (int)((aw[w] >> (8 * k)) & 0xFFu) - (int)((bw[w] >> (8 * k)) & 0xFFu);
            d = d < 0 ? 0 : d;
            v += (uint32_t)__popc((unsigned)d);
        }
    return v;
}

// The binary policy: 32-byte rows, the value is the popcount of the difference -- cheap enough to evaluate inside the hit branch,
// where each lane also keeps its least (value << 32 | i), so that bestVal is one wave minimum.
struct MapBinArgs {
    MapArgs m;
    const uint4 *mapDesc, *curDesc;   // frame sets' descriptors
    int mapDescStride, curDescStride; // uint4 between frames
};

struct MapBinRows {
    using Args = MapBinArgs;
    using Best = unsigned long long; // per lane: least (value, i) among the candidates it has seen
    const uint4 *__restrict__ mapDesc, *__restrict__ curDesc;

    PS_D MapBinRows(const Args &b, int view, int frame)
        : mapDesc(b.mapDesc + (size_t)view * b.mapDescStride), curDesc(b.curDesc + (size_t)frame * b.curDescStride)
    {
    }
    PS_D static Best none() { return ~0ull; }
    PS_D uint32_t popc(int j, int i) const { return satdiff_popc256(mapDesc[2 * j], mapDesc[2 * j + 1], curDesc[2 * i], curDesc[2 * i + 1]); }
    PS_D uint32_t hit(int j, int i, Best &best) const
    {
        const uint32_t v = popc(j, i);
        const Best key = ((Best)v << 32) | (unsigned)i;
        best = key < best ? key : best;
        return __float_as_uint((float)v);
    }
    template <int F> PS_D void values(uint2 *, const int (&)[F], int) const {}
    PS_D float best_value(Best best, const uint2 *, int, const MapSphere &) const { return (float)(uint32_t)(wave_min_u64(best) >> 32); }
    PS_D float value(int j, int i) const { return (float)popc(j, i); }
};

template <int F> __global__ __launch_bounds__(kMapBlock) void ps_map_sweep(MapBinArgs b) { map_sweep<F, MapBinRows>(b); }

// One work-group per pair: the chunks' matches in (j, i) order, the signed and the clamped count, and (REC) the scoring
// records of the depth-valid ones as ps_prep_from_matches builds them for a single pair.
template <bool REC, int BLOCK>
__global__ __launch_bounds__(BLOCK) void ps_map_emit(MapArgs a, PrepArgs pa, RecPtrs rec, PsDMatch *__restrict__ matches,
                                                     int32_t *__restrict__ numMatches, int32_t *__restrict__ numClamped,
                                                     int32_t *__restrict__ mvalid, float2 *__restrict__ cmaxOut)
{
    extern __shared__ __align__(16) int s_off[]; // chunks + 1 exclusive offsets
    __shared__ int s_wsum[(REC ? 2 : 1) * (BLOCK / 64)]; // (the one-barrier flag scan of the record stage takes two sets)
    __shared__ float2 s_red[BLOCK / 64];
    const int p = blockIdx.x;
    const int view = a.pairs[2 * p], frame = a.pairs[2 * p + 1];
    const int nmap = map_count(a.mapN, view, a.mapFrames, a.mapCap);
    const int total = a.tmpCount[p];
    const bool over = total < 0 || total > a.maxMatches;
    const int m = over ? 0 : total;
    const int chunks = m > 0 ? (nmap + a.chunkFeatures - 1) / a.chunkFeatures : 0;
    const int32_t *__restrict__ cStart = a.chunkStart + (size_t)p * a.chunks;
    const int32_t *__restrict__ cCount = a.chunkCount + (size_t)p * a.chunks;
    int carry = 0;
    for (int c0 = 0; c0 < chunks; c0 += BLOCK) {
        const int c = c0 + threadIdx.x;
        const int v = c < chunks ? cCount[c] : 0;
        int sum;
        const int ex = block_scan_int<BLOCK>(v, sum, s_wsum);
        if (c < chunks) s_off[c] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) s_off[chunks] = carry; // (= m)
    __syncthreads();
    const PsDMatch *__restrict__ tmp = a.tmp + (size_t)p * a.maxMatches;
    PsDMatch *__restrict__ out = matches + (size_t)p * a.maxMatches;
    const float *__restrict__ prev = a.mapPts + (size_t)(m > 0 ? view : 0) * a.mapPtsStride;
    const float *__restrict__ cur = a.curPts + (size_t)(m > 0 ? frame : 0) * a.curPtsStride;
    PairRecords pr(pa, rec, p, REC);
    int trip = 0;
    for (int i0 = 0; i0 < m; i0 += BLOCK, ++trip) {
        const int i = i0 + threadIdx.x;
        float px = 0, py = 0, pz = 0, cx_ = 0, cy_ = 0, cz_ = 0;
        int q = 0, t = 0;
        bool ok = false;
        if (i < m) {
            // the chunk that holds output position i: the last one whose offset is <= i (empty chunks share an offset)
            int lo = 0, hi = chunks; // s_off[lo] <= i < s_off[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid] <= i) lo = mid;
                else hi = mid;
            }
            const PsDMatch mt = tmp[cStart[lo] + (i - s_off[lo])];
            out[i] = mt;
            q = mt.queryIdx;
            t = mt.trainIdx;
            if (REC) {
                px = prev[3 * q]; py = prev[3 * q + 1]; pz = prev[3 * q + 2];
                cx_ = cur[3 * t]; cy_ = cur[3 * t + 1]; cz_ = cur[3 * t + 2];
                ok = match_depth_ok(px, py, pz, cx_, cy_, cz_);
            }
        }
        if (REC) {
            int vtotal;
            const int vpos = block_scan_flag<BLOCK, false>(ok, vtotal, s_wsum, trip);
            pr.add(ok, vpos, vtotal, i, q, t, px, py, pz, cx_, cy_, cz_);
        }
    }
    if (REC) pr.finish<BLOCK>(s_red, mvalid, cmaxOut);
    if (threadIdx.x == 0) {
        numMatches[p] = over ? -total : total;
        if (numClamped) numClamped[p] = m;
    }
}

} // namespace psdev

// Host side: Matcher::matchXYZ, matcher.cpp:606-798, for a device-resident batch.  Part of the device translation unit, on the
// plan and the stages of ps_ransac_stage.h (Plan, make_plan, prepare_score, ensure_records, rec_ptrs, run_ransac_stage).
// A batch KIND names what differs between PsMapBatch and PsMapBatchF32 -- Batch, Args (the policy's argument block), what (the
// prefix of the messages), sweeps() (the kernel per F) and sets(ctx, b, l): the rule of the two frame sets, which leaves the
// descriptor arguments and the point strides of a batch that passed in l -- and, for the host-pointer form, Elem (what a row is
// made of), host_rows (the rule of dim and of the row pitches, with the entry's own texts) and set_dim.  MapBinKind is below,
// MapL2Kind in ps_map_match_l2.h.
namespace {

// Map features per wave of the sweep: eight when that still gives every CU several work-groups, fewer for a handful of pairs
// (ten pairs of 2000 features, one frame's retry ladder: four per wave, 1250 work-groups).
int map_features_per_wave(int P, int mapCap)
{
    for (int f = 8; f > 1; f >>= 1)
        if ((long long)P * ((mapCap + kMapWaves * f - 1) / (kMapWaves * f)) >= 1024) return f;
    return 1;
}

template <class Args> struct MapSweeps { void (*f1)(Args), (*f2)(Args), (*f4)(Args), (*f8)(Args); };

template <class Kind> int check_map_batch(PsContext *ctx, const typename Kind::Batch *b, typename Kind::Args &l)
{
    const std::string w(Kind::what);
    if (!b || b->P < 0) return fail(ctx, PS_ERR_BAD_ARG, (w + ": null batch or P < 0").c_str());
    if (b->P == 0) return PS_OK;
    if (!b->pairs || !b->mapLevel || !b->curLevel) return fail(ctx, PS_ERR_BAD_ARG, (w + ": null pairs / mapLevel / curLevel").c_str());
    if (int rc = Kind::sets(ctx, *b, l)) return rc;
    if (b->maxMatches < 1) return fail(ctx, PS_ERR_BAD_ARG, (w + ": maxMatches must lie in 1 .. 1 << 22").c_str());
    if (b->maxMatches > (1 << 22)) return fail(ctx, PS_ERR_UNSUPPORTED, (w + ": maxMatches must lie in 1 .. 1 << 22").c_str());
    return PS_OK;
}

// The two launches for a checked batch (l as check_map_batch left it); pl = null: matches only.  numClamped (device, P, or
// null) receives max(numMatches[p], 0), what kernel 4 is given.
template <class Kind>
int run_map_match(PsContext *ctx, const typename Kind::Batch &b, typename Kind::Args l, const Plan *pl, PsDMatch *dMatches,
                  int32_t *dNumMatches, int32_t **numClamped, int slot0)
{
    const int P = b.P, F = map_features_per_wave(P, b.maps.maxKpts), CH = kMapWaves * F;
    MapArgs &a = l.m;
    a.mapPts = b.maps.pts; a.curPts = b.frames.pts;
    a.mapN = b.maps.nkpts; a.curN = b.frames.nkpts;
    a.mapLevel = b.mapLevel; a.curLevel = b.curLevel;
    a.mapFrames = b.maps.numFrames; a.curFrames = b.frames.numFrames;
    a.mapCap = b.maps.maxKpts; a.curCap = b.frames.maxKpts;
    a.pairs = b.pairs;
    a.radiusBound = b.radiusBound; a.acceptRatio = b.acceptRatio;
    a.radiusPer = b.radiusBoundPerPair; a.ratioPer = b.acceptRatioPerPair;
    a.maxMatches = b.maxMatches;
    a.chunks = (a.mapCap + CH - 1) / CH;
    a.chunkFeatures = CH;
    // scratch: the staging rows, then [P] reserved | [P] clamped | [P][chunks] start | [P][chunks] count
    PS_ENSURE(ctx->sMatches, (size_t)P * b.maxMatches * sizeof(PsDMatch));
    PS_ENSURE(ctx->sMisc2, ((size_t)2 * P + (size_t)2 * P * a.chunks) * sizeof(int32_t));
    if (pl) {
        PS_ENSURE(ctx->mvalid, (size_t)P * sizeof(int32_t));
        PS_ENSURE(ctx->cmax, (size_t)P * sizeof(float2));
        int rc = ensure_records(ctx, (size_t)P, (size_t)b.maxMatches);
        if (rc != PS_OK) return rc;
    }
    a.tmp = (PsDMatch *)ctx->sMatches.p;
    a.tmpCount = (int32_t *)ctx->sMisc2.p;
    int32_t *clamped = a.tmpCount + P;
    a.chunkStart = clamped + P;
    a.chunkCount = a.chunkStart + (size_t)P * a.chunks;
    if (numClamped) *numClamped = clamped;
    PS_HIP(hipMemsetAsync(a.tmpCount, 0, (size_t)P * sizeof(int32_t), ctx->stream));
    tick(ctx, slot0, false);
    const dim3 grid((unsigned)P * (unsigned)a.chunks), block(kMapBlock);
    const MapSweeps<typename Kind::Args> sweeps = Kind::sweeps();
    switch (F) {
    case 8: hipLaunchKernelGGL(sweeps.f8, grid, block, 0, ctx->stream, l); break;
    case 4: hipLaunchKernelGGL(sweeps.f4, grid, block, 0, ctx->stream, l); break;
    case 2: hipLaunchKernelGGL(sweeps.f2, grid, block, 0, ctx->stream, l); break;
    default: hipLaunchKernelGGL(sweeps.f1, grid, block, 0, ctx->stream, l); break;
    }
    tick(ctx, slot0, true);
    PS_HIP(hipGetLastError());
    tick(ctx, slot0 + 1, false);
    const size_t lds = ((size_t)a.chunks + 1) * sizeof(int32_t);
    const bool wide = P <= kWidePairs; // a handful of pairs: 1024-thread work-groups shorten the per-pair serial walk
    const PrepArgs pa = pl ? pl->pa : PrepArgs{};
    const RecPtrs rp = pl ? rec_ptrs(ctx, pl->score) : RecPtrs{};
    int32_t *mv = (int32_t *)ctx->mvalid.p;
    float2 *cmx = (float2 *)ctx->cmax.p;
    if (pl) {
        if (wide) hipLaunchKernelGGL((ps_map_emit<true, 1024>), dim3((unsigned)P), dim3(1024), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
        else hipLaunchKernelGGL((ps_map_emit<true, kBlock>), dim3((unsigned)P), dim3(kBlock), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
    } else {
        if (wide) hipLaunchKernelGGL((ps_map_emit<false, 1024>), dim3((unsigned)P), dim3(1024), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
        else hipLaunchKernelGGL((ps_map_emit<false, kBlock>), dim3((unsigned)P), dim3(kBlock), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
    }
    tick(ctx, slot0 + 1, true);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// ps_match_xyz_device / ps_match_xyz_l2_device
template <class Kind>
int match_xyz_body(PsContext *ctx, const char *who, const typename Kind::Batch *b, PsDMatch *matches, int32_t *numMatches)
{
    int rc = bind(ctx);
    if (rc) return rc;
    typename Kind::Args l{};
    rc = check_map_batch<Kind>(ctx, b, l);
    if (rc) return rc;
    if (b->P == 0) return PS_OK;
    if (!matches || !numMatches) return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null output").c_str());
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return run_map_match<Kind>(ctx, *b, l, nullptr, matches, numMatches, nullptr, 0);
}

// ps_map_pairs_device / ps_map_pairs_l2_device
template <class Kind>
int map_pairs_body(PsContext *ctx, const char *who, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                   const typename Kind::Batch *b, const PsPairResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    typename Kind::Args l{};
    rc = check_map_batch<Kind>(ctx, b, l);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null output").c_str());
    if (b->P == 0) return PS_OK;
    if (!out->matches || !out->numMatches || !out->inlierMask || !out->pose || !out->stats)
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null output").c_str());
    if (cfg && cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "explicit sample streams are per call, not per batch");
    const int P = b->P, cap = b->maxMatches;
    Plan pl;
    rc = make_plan(ctx, params, cfg, K, cap, b->frames.maxKpts, pl);
    if (rc) return rc;
    begin_timed_call(ctx);
    HandoffGuard handoffGuard{ctx}; // (prepare_score below may already queue a clearing: the guard stands before it)
    rc = prepare_score(ctx, pl, P, cap, false, true, b->maps.desc);
    if (rc) return rc;
    int32_t *clamped = nullptr;
    rc = run_map_match<Kind>(ctx, *b, l, &pl, out->matches, out->numMatches, &clamped, 0);
    if (rc) return rc;
    return run_ransac_stage(ctx, pl, P, cap, out->matches, clamped, cap, out->pose, out->inlierMask, out->stats, 2);
}

// ps_match_xyz / ps_match_xyz_l2_f32: host arrays, rows of dim Kind::Elem.  One pair is staged in the context's scratch and
// goes through the batch's check and launches; a negative count from the device is the needed capacity.
template <class Kind>
int match_xyz_host(PsContext *ctx, const std::string &who, const float *mapPos, const typename Kind::Elem *mapDesc, size_t mapDescStep,
                   const int32_t *mapLevel, int nmap, const float *curPos, const typename Kind::Elem *curDesc, size_t curDescStep,
                   const int32_t *curLevel, int ncur, int dim, double sphereRadius, double acceptRatio, PsDMatch *out, int cap, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    if (nout) *nout = 0;
    if (!nout || nmap < 0 || ncur < 0 || cap < 0 || dim < 1 || (cap > 0 && !out) || (nmap > 0 && (!mapPos || !mapDesc || !mapLevel)) ||
        (ncur > 0 && (!curPos || !curDesc || !curLevel)))
        return fail(ctx, PS_ERR_BAD_ARG, (who + ": bad argument").c_str());
    const size_t row = (size_t)dim * sizeof(typename Kind::Elem);
    rc = Kind::host_rows(ctx, dim, (nmap > 0 && mapDescStep < row) || (ncur > 0 && curDescStep < row));
    if (rc) return rc;
    if (nmap > PS_MAX_KPTS || ncur > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, (who + ": more than PS_MAX_KPTS rows").c_str());
    if (nmap == 0 || ncur == 0) return PS_OK;
    const int devCap = cap < 1 ? 1 : (cap > (1 << 22) ? (1 << 22) : cap);
    PS_ENSURE(ctx->sMisc0, (size_t)nmap * 12);
    PS_ENSURE(ctx->sMisc1, (size_t)ncur * 12);
    PS_ENSURE(ctx->sDesc, (size_t)(nmap + ncur) * row);
    PS_ENSURE(ctx->sNk, (size_t)(nmap + ncur + 4) * sizeof(int32_t));
    PS_ENSURE(ctx->sMask, (size_t)devCap * sizeof(PsDMatch)); // (the device rows of `out`: sMatches is the batch's staging)
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    uint8_t *dDesc = (uint8_t *)ctx->sDesc.p;
    int32_t *dLvl = (int32_t *)ctx->sNk.p, *dMeta = dLvl + nmap + ncur;
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, mapPos, (size_t)nmap * 12, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, curPos, (size_t)ncur * 12, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc, row, mapDesc, mapDescStep, row, (size_t)nmap, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc + (size_t)nmap * row, row, curDesc, curDescStep, row, (size_t)ncur, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(dLvl, mapLevel, (size_t)nmap * 4, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(dLvl + nmap, curLevel, (size_t)ncur * 4, hipMemcpyHostToDevice, ctx->stream));
    const int32_t hostMeta[4] = {nmap, ncur, 0, 0}; // the two counts, the pair (view 0, frame 0)
    PS_HIP(hipMemcpyAsync(dMeta, hostMeta, sizeof hostMeta, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // hostMeta goes out of scope
    typename Kind::Batch b{};
    b.maps.desc = (const typename Kind::Elem *)dDesc; b.maps.pts = (const float *)ctx->sMisc0.p; b.maps.nkpts = dMeta;
    b.maps.numFrames = 1; b.maps.maxKpts = nmap;
    b.frames.desc = (const typename Kind::Elem *)(dDesc + (size_t)nmap * row); b.frames.pts = (const float *)ctx->sMisc1.p; b.frames.nkpts = dMeta + 1;
    b.frames.numFrames = 1; b.frames.maxKpts = ncur;
    Kind::set_dim(b, dim);
    b.mapLevel = dLvl; b.curLevel = dLvl + nmap;
    b.pairs = dMeta + 2;
    b.P = 1;
    b.maxMatches = devCap;
    b.radiusBound = sq_bound_f32(sphereRadius); // (float)norm < (double)radius  <=>  squared sum < bound
    b.acceptRatio = acceptRatio;
    typename Kind::Args l{};
    rc = check_map_batch<Kind>(ctx, &b, l);
    if (rc) return rc;
    rc = run_map_match<Kind>(ctx, b, l, nullptr, (PsDMatch *)ctx->sMask.p, (int32_t *)ctx->sNumM.p, nullptr, 0);
    if (rc) return rc;
    int32_t n = 0;
    PS_HIP(hipMemcpyAsync(&n, ctx->sNumM.p, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const int total = n < 0 ? -n : n;
    *nout = total;
    if (total > cap) return fail(ctx, PS_ERR_BAD_ARG, (who + ": output capacity too small (*nout = needed)").c_str());
    if (total > 0) {
        PS_HIP(hipMemcpyAsync(out, ctx->sMask.p, (size_t)total * sizeof(PsDMatch), hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PS_OK;
}

struct MapBinKind {
    using Batch = PsMapBatch;
    using Args = MapBinArgs;
    using Elem = uint8_t;
    static constexpr const char *what = "map batch";
    static int host_rows(PsContext *ctx, int, bool shortPitch)
    {
        return shortPitch ? fail(ctx, PS_ERR_UNSUPPORTED, "descriptor rows must be 32 bytes (ORB/LDB)") : PS_OK;
    }
    static void set_dim(Batch &, int) {}
    static MapSweeps<Args> sweeps() { return {ps_map_sweep<1>, ps_map_sweep<2>, ps_map_sweep<4>, ps_map_sweep<8>}; }
    static int sets(PsContext *ctx, const Batch &b, Args &l)
    {
        FrameStrides maps, frames;
        if (int rc = check_frame_set(ctx, b.maps, "map batch: map views", maps)) return rc;
        if (int rc = check_frame_set(ctx, b.frames, "map batch: frames", frames)) return rc;
        l.m.mapPtsStride = maps.ptsFloats(); l.m.curPtsStride = frames.ptsFloats();
        l.mapDesc = (const uint4 *)b.maps.desc; l.curDesc = (const uint4 *)b.frames.desc;
        l.mapDescStride = maps.descUint4(); l.curDescStride = frames.descUint4();
        return PS_OK;
    }
};

} // namespace

extern "C" {

float ps_map_sphere_bound(double sphereRadius) { return sq_bound_f32(sphereRadius); }

size_t ps_abi_sizeof_map_batch(void) { return sizeof(PsMapBatch); }

int ps_match_xyz(PsContext *ctx, const float *mapPos, const uint8_t *mapDesc, size_t mapDescStep, const int32_t *mapLevel,
                 int nmap, const float *curPos, const uint8_t *curDesc, size_t curDescStep, const int32_t *curLevel, int ncur,
                 double sphereRadius, double acceptRatio, PsDMatch *out, int cap, int *nout)
{
    return match_xyz_host<MapBinKind>(ctx, "ps_match_xyz", mapPos, mapDesc, mapDescStep, mapLevel, nmap, curPos, curDesc, curDescStep, curLevel,
                                      ncur, PS_DESC_BYTES, sphereRadius, acceptRatio, out, cap, nout);
}

int ps_match_xyz_device(PsContext *ctx, const PsMapBatch *b, PsDMatch *matches, int32_t *numMatches)
{
    return match_xyz_body<MapBinKind>(ctx, "ps_match_xyz_device", b, matches, numMatches);
}

int ps_map_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                        const PsMapBatch *b, const PsPairResults *out)
{
    return map_pairs_body<MapBinKind>(ctx, "ps_map_pairs_device", params, cfg, K, b, out);
}

} // extern "C"
