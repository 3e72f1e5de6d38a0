// ps_select_refit.h -- kernel 4 of the pair pipeline: the replay of the sequential best-model rule over the counts kernel 3 left,
// the inliers of the selected hypothesis, the refit on them (wave-level Umeyama) and the final inliers.
//
// Kernel 4  ps_select_refit    replay of the sequential best-model rule, refit, final inliers
//
// The launch is run_ransac_stage's (ps_ransac_stage.h), which also sizes the dynamic LDS.
#pragma once
#include "ps_block.h" // kBlock, phase_stamp, block_scan_flag
#include "ps_device_math.h"
#include "ps_score_value.h" // ModelArgs, load_model / gen_model, ScoreConsts, inlier_test

#include "../../include/putslam_hip.h"

namespace psdev {

// ------------------------------------------------------------------------------------------
// Wave-level N-point Umeyama (refit, RANSAC.cpp:153): the canonical summation order is
// 64 strided partials (lane l takes elements l, l+64, ...) and a stride-1,2,4,..,32 tree.
// getter(j, src[3], dst[3]) yields the j-th correspondence.  All 64 lanes return the model.
// ------------------------------------------------------------------------------------------
// (the strides 1 .. 8 stay inside a row of 16 lanes: DPP row shifts, no trip through the LDS crossbar; the partial sums the
// result depends on -- lanes that are multiples of twice the stride -- read what __shfl_down would hand them; strides 16 and
// 32 combine the four row sums, read as scalars: (r0 + r16) + (r32 + r48), the tree's own association)
PS_D float wave_tree_sum(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x101, 0xF, 0xF, false));
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x102, 0xF, 0xF, false));
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x104, 0xF, 0xF, false));
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x108, 0xF, 0xF, false));
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
    const float r16 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r32 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
    const float r48 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r16) + (r32 + r48);
#else
    return v;
#endif
}

// The correspondences come from two places: j < split through getA (kernel 4: operands parked in LDS), the rest through getB
// (global memory).  Two loops, not one getter with a branch inside: the compiler merged the branch's two sources into generic
// pointers and FLAT loads (four per trip, waited for together: 350 cycles a trip) -- and, before that, into arrays in scratch
// memory (600 cycles a trip; the two passes were 8 of kernel 4's 26 us for a single pair).  A getter yields
// u = (src.x, src.y, src.z, dst.x), v = (dst.y, dst.z, -, -).  The LDS loop requests the lane's next element before it adds
// the current one; each lane still adds its elements in ascending order.
template <typename GetA, typename GetB> PS_D bool wave_umeyama(int k, int split, GetA getA, GetB getB, Rigid &mdl)
{
    const int lane = threadIdx.x & 63;
    const float one_over_n = 1.0f / (float)k;
    const int k1 = k < split ? k : split;
    // the lane's first element behind the split: the smallest j = lane (mod 64) with j >= k1
    const int jB = lane + (((k1 > lane ? k1 - lane : 0) + 63) >> 6 << 6);
    float ss[3] = {0.0f, 0.0f, 0.0f}, ds[3] = {0.0f, 0.0f, 0.0f};
    auto add1 = [&](const float4 &u, const float4 &v) {
        ss[0] = ss[0] + u.x; ss[1] = ss[1] + u.y; ss[2] = ss[2] + u.z;
        ds[0] = ds[0] + u.w; ds[1] = ds[1] + v.x; ds[2] = ds[2] + v.y;
    };
    {
        float4 u, v, un, vn;
        if (lane < k1) getA(lane, u, v);
        for (int j = lane; j < k1; j += 64) {
            if (j + 64 < k1) getA(j + 64, un, vn);
            add1(u, v);
            u = un;
            v = vn;
        }
        for (int j = jB; j < k; j += 64) {
            getB(j, u, v);
            add1(u, v);
        }
    }
    float sm[3], dm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sm[c] = wave_tree_sum(ss[c]) * one_over_n;
        dm[c] = wave_tree_sum(ds[c]) * one_over_n;
    }
    float acc[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[r][c] = 0.0f;
    auto add2 = [&](const float4 &u, const float4 &v) {
        const float s[3] = {u.x, u.y, u.z}, d[3] = {u.w, v.x, v.y};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[r][c] = acc[r][c] + (d[r] - dm[r]) * (s[c] - sm[c]);
    };
    {
        float4 u, v, un, vn;
        if (lane < k1) getA(lane, u, v);
        for (int j = lane; j < k1; j += 64) {
            if (j + 64 < k1) getA(j + 64, un, vn);
            add2(u, v);
            u = un;
            v = vn;
        }
        for (int j = jB; j < k; j += 64) {
            getB(j, u, v);
            add2(u, v);
        }
    }
    float sigma[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) sigma[r][c] = one_over_n * wave_tree_sum(acc[r][c]);
    bool ok = umeyama_finish(sigma, sm, dm, mdl);
    if (!ok) set_identity(mdl);
    return ok;
}

struct SelectArgs {
    int estimator;       // PsEstimator
    int mode;            // RANSAC::ERROR_VERSION
    int H, cap;
    int minMatches;      // minimalNumberOfMatches (RANSAC) or 8 (USAC_wrapper.cpp:120)
    int iter0;           // initial trip limit: min(computeRANSACIteration(0.20), H) or min(850000, H)
    double minRatio;     // minimalInlierRatioThreshold
    const float *ransacTab;  // non-increasing; ransacTab[k] = smallest ratio r with iterations(r) <= k
    int ransacTabN;
    float ransacTiny;        // ratios <= this make the reference's quotient -inf (limit 0)
    const double *usacTab;   // non-increasing; usacTab[k] = smallest p with stopping(p) <= k+1
    int usacTabN;
    int trainRange;      // train indices are < trainRange (size of the uniqueness bitmaps, 0 = skip)
    int stageCap;        // inlier correspondences staged in LDS for the refit and the re-selection (8 words each)
};

// First k of [0, n) with !(x < tab[k]) -- n if there is none -- for a non-increasing table, found by the whole wavefront: every
// lane probes one of 64 evenly spaced entries and the ballot narrows the range 64-fold per step (850 000 entries: four
// dependent loads instead of a binary search's twenty, 0.5 us each from a cold table).  Wave-uniform arguments and result.
template <typename T> PS_D int table_first_not_below(const T *__restrict__ tab, int n, T x)
{
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const int kq = lo + lane * step;
        const bool valid = kq < hi;
        const bool below = valid && (x < tab[valid ? kq : lo]);
        const int t = __popcll(__ballot(below));     // the probes that are still "below" form a prefix of the lanes
        const int nvalid = __popcll(__ballot(valid));
        const int nlo = t > 0 ? lo + (t - 1) * step + 1 : lo;
        const int nhi = t < nvalid ? lo + t * step : hi;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}
// min(Kcap, computeRANSACIteration(r)) through the host-built threshold table (RANSAC.cpp:450-461).
PS_D int ransac_limit(const SelectArgs &a, float r)
{
    if (r <= a.ransacTiny) return 0;
    return table_first_not_below<float>(a.ransacTab, a.ransacTabN, r); // first k with r >= tab[k]
}
// min(H, updateStandardStopping(inliers, M, 3)) through the host-built table (USAC.h:944-971).
PS_D int usac_limit(const SelectArgs &a, unsigned c, unsigned M)
{
    double n_in = 1.0, n_pts = 1.0;
#pragma unroll
    for (unsigned i = 0; i < 3; ++i) {
        n_in *= (double)(unsigned)(c - i);
        n_pts *= (double)(unsigned)(M - i);
    }
    double pgood = n_in / n_pts;
    const int lo = table_first_not_below<double>(a.usacTab, a.usacTabN, pgood);
    int stop = lo + 1;
    return stop < a.H ? stop : a.H;
}

PS_D void store_pose(float *pose, const Rigid &m)
{
    // column-major 4x4 (Eigen::Matrix4f storage)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int r = 0; r < 3; ++r) pose[4 * c + r] = m.R[r][c];
        pose[4 * c + 3] = 0.0f;
    }
    pose[12] = m.t[0]; pose[13] = m.t[1]; pose[14] = m.t[2]; pose[15] = 1.0f;
}

// ------------------------------------------------------------------------------------------
// Kernel 4.  One workgroup per pair:
//  (1) replay of the sequential selection over counts[0..H): strict '>' first-best with the
//      adaptive trip limit (RANSAC.cpp:87,438-455 / USAC.h:326,409-414,498-509) or plain arg-max;
//  (2) inliers of the selected hypothesis, in match order;
//  (3) Umeyama refit on them and the Euclidean re-selection (RANSAC.cpp:152-158);
//  (4) ratio gate (RANSAC.cpp:161-164 / USAC_wrapper.cpp:139-141), pointInlierRatio (RANSAC.h:56-66).
// The phases are the functions below, force-inlined; the kernel holds the LDS and the order.
// ------------------------------------------------------------------------------------------

// ---- (1) the three replays: each returns the selected hypothesis (-1: none), its count and the trips the schedule ran ----
struct Selection {
    int bestIdx, bestCount, trips;
};

// RANSAC in the reference's own regime (at most 487 iterations): counts and stop table fit a wavefront's registers (select_wave)
PS_D bool wave_replay(const SelectArgs &a) { return a.estimator == PS_EST_RANSAC && a.H <= 8 * 64 && a.ransacTabN <= 8 * 64; }

// The fixed schedule: plain arg-max, the first index on ties.
template <int BLOCK>
PS_D Selection select_fixed(const SelectArgs &a, const int32_t *__restrict__ cnts, unsigned long long *s_red, int *s_sel)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long key = 0ull;
    auto take = [&](int i, int c) {
        unsigned long long kk = ((unsigned long long)(unsigned)c << 32) | (0xFFFFFFFFu - (unsigned)i);
        key = kk > key ? kk : key;
    };
    int i = tid;
    for (; i + 7 * BLOCK < a.H; i += 8 * BLOCK) { // eight loads in flight: the counts come from another launch (HBM latency)
        int c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = cnts[i + u * BLOCK];
#pragma unroll
        for (int u = 0; u < 8; ++u) take(i + u * BLOCK, c[u]);
    }
    for (; i < a.H; i += BLOCK) take(i, cnts[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long other = __shfl_down(key, o, 64);
        key = other > key ? other : key;
    }
    if (lane == 0) s_red[wv] = key;
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = s_red[0];
        for (int i = 1; i < BLOCK / 64; ++i) b = s_red[i] > b ? s_red[i] : b;
        int c = (int)(b >> 32);
        s_sel[0] = c > 0 ? (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFu)) : -1;
        s_sel[1] = c;
        s_sel[2] = a.H;
    }
    __syncthreads();
    return {s_sel[0], s_sel[1], s_sel[2]};
}

// Every wavefront replays the schedule by itself, counts and stop table in registers (eight of each per lane, index = 64 u +
// lane), a round = eight ballots and scalar code.  No barrier, no table search through memory: the work-group form below spends
// 0.8 us per record on its dependent table loads alone (3.9 of the single pair's 91 us, profiles/r04g).  Needs wave_replay(a).
PS_D Selection select_wave(const SelectArgs &a, const int32_t *__restrict__ cnts, int M)
{
    const int lane = threadIdx.x & 63;
    int c[8];
    float tb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int idx = u * 64 + lane;
        c[u] = idx < a.H ? cnts[idx] : 0;
        tb[u] = idx < a.ransacTabN ? a.ransacTab[idx] : 0.0f;
    }
    int pos = 0, limit = a.iter0, best = 0, bIdx = -1;
    for (;;) {
        int fIdx = -1, fCnt = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = u * 64 + lane;
            const unsigned long long mk = __ballot(idx >= pos && idx < limit && c[u] > best);
            if (fIdx < 0 && mk != 0ull) { // the first index in [pos, limit) that beats the best
                const int l = __ffsll((long long)mk) - 1;
                fIdx = u * 64 + l;
                fCnt = __builtin_amdgcn_readlane(c[u], l);
            }
        }
        if (fIdx < 0) break;
        bIdx = fIdx;
        best = fCnt;
        pos = bIdx + 1;
        const float r = (float)best / (float)M; // ratio as RANSAC.cpp:280
        // ransac_limit(): the first k with r >= tab[k] of a non-increasing table = the number of k with r < tab[k]
        int lim = 0;
        if (!(r <= a.ransacTiny)) {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                lim += __popcll(__ballot(u * 64 + lane < a.ransacTabN && r < tb[u]));
        }
        limit = lim;
    }
    return {bIdx, best, (bIdx + 1 > limit) ? bIdx + 1 : limit};
}

// Sequential replay by the work-group (USAC; RANSAC beyond the wave form's tables).  State changes only at "records" (count >
// best so far), so the workgroup repeatedly finds the first index in [pos, limit) that beats the best.
// The range is searched in windows that double (2 Ki, 4 Ki, ... indices; eight loads of a thread in flight): the
// first record lies a few indices behind `pos` as a rule, and a thread that had no hit of its own used to walk the
// whole range alone, one dependent load at a time -- under USAC's initial limit of 850 000 that was 480 us for a
// single pair (profiles/r04g/single_pair_schedules.txt).  A window never reaches beyond `limit`: the same indices
// are read as before (counts beyond the trip limit may be stale under the staged scoring).
template <int BLOCK>
PS_D Selection select_block(const SelectArgs &a, const int32_t *__restrict__ cnts, int M, unsigned long long *s_red, int *s_sel)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int pos = 0, limit = a.iter0, best = 0, bIdx = -1;
    for (;;) {
        unsigned f = 0xFFFFFFFFu;
        int span = 8 * BLOCK;
        for (int w0 = pos; w0 < limit;) {
            const int w1 = (limit - w0 > span) ? w0 + span : limit;
            unsigned found = 0xFFFFFFFFu;
            for (int i0 = w0 + tid; i0 < w1 && found == 0xFFFFFFFFu; i0 += 8 * BLOCK) {
                int c[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + u * BLOCK;
                    c[u] = i < w1 ? cnts[i] : (int)0x80000000;
                }
#pragma unroll
                for (int u = 7; u >= 0; --u)
                    if (c[u] > best) found = (unsigned)(i0 + u * BLOCK); // (descending: the smallest index stays)
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                unsigned other = __shfl_down(found, o, 64);
                found = other < found ? other : found;
            }
            if (lane == 0) s_red[wv] = found;
            __syncthreads();
            f = (unsigned)s_red[0];
            for (int i = 1; i < BLOCK / 64; ++i) f = (unsigned)s_red[i] < f ? (unsigned)s_red[i] : f;
            __syncthreads();
            if (f != 0xFFFFFFFFu) break;
            w0 = w1;
            if (span < 512 * BLOCK) span *= 2;
        }
        if (f == 0xFFFFFFFFu) break;
        bIdx = (int)f;
        best = cnts[bIdx];
        pos = bIdx + 1;
        if (a.estimator == PS_EST_USAC)
            limit = usac_limit(a, (unsigned)best, (unsigned)M);
        else
            limit = ransac_limit(a, (float)best / (float)M); // ratio as RANSAC.cpp:280
    }
    if (tid == 0) {
        s_sel[0] = bIdx;
        s_sel[1] = best;
        s_sel[2] = (bIdx + 1 > limit) ? bIdx + 1 : limit;
    }
    __syncthreads();
    return {s_sel[0], s_sel[1], s_sel[2]};
}

// ---- (2) the inliers of model mdl (inv: its inverse, for the reprojection metrics) among the pair's M records, in match
// order: their indices to list[], the first stageCap of them -- the refit's and the re-selection's operands -- parked in LDS
// while they are in registers.  fetch(i, A, B, C) reads record i; the first trip's (cA, cB, cC) are the caller's, every later
// trip fetches the next one's before its scan.  Returns their number.
template <int BLOCK, class Fetch>
PS_D int inlier_pass(const SelectArgs &a, const ScoreConsts &k, const Rigid &mdl, const Rigid &inv, int M, Fetch fetch, float4 cA,
                     float4 cB, float4 cC, int32_t *__restrict__ list, float *s_stage, int *s_wsum)
{
    const int tid = threadIdx.x;
    int kin = 0, trip = 0;
    for (int i0 = 0; i0 < M; i0 += BLOCK, ++trip) {
        const int i = i0 + tid;
        float4 nA, nB, nC;
        fetch(i + BLOCK, nA, nB, nC);
        const float4 A = cA, B = cB, C = cC;
        bool in = false;
        if (i < M) {
            switch (a.mode) {
            case PS_EUCLIDEAN_ERROR: in = inlier_test<PS_EUCLIDEAN_ERROR>(mdl, inv, k, A, B, C); break;
            case PS_ADAPTIVE_ERROR: in = inlier_test<PS_ADAPTIVE_ERROR>(mdl, inv, k, A, B, C); break;
            case PS_REPROJECTION_ERROR: in = inlier_test<PS_REPROJECTION_ERROR>(mdl, inv, k, A, B, C); break;
            case PS_EUCLIDEAN_AND_REPROJECTION_ERROR:
                in = inlier_test<PS_EUCLIDEAN_AND_REPROJECTION_ERROR>(mdl, inv, k, A, B, C);
                break;
            default: in = false; break;
            }
        }
        int total;
        int pos = block_scan_flag<BLOCK, false>(in, total, s_wsum, trip);
        if (in) {
            const int slot = kin + pos;
            list[slot] = i;
            if (slot < a.stageCap) { // the refit's and the re-selection's operands, parked in LDS while they are in registers
                float *d = s_stage + 8 * slot;
                reinterpret_cast<float4 *>(d)[0] = make_float4(B.x, B.y, B.z, A.x);
                reinterpret_cast<float4 *>(d)[1] = make_float4(A.y, A.z, A.w, __int_as_float(i));
            }
        }
        kin += total;
        cA = nA; cB = nB; cC = nC;
    }
    __syncthreads(); // list / staged points visible to the whole workgroup
    return kin;
}

// ---- pointInlierRatio (RANSAC.h:56-66) needs the unique trainIdx among ALL input matches and among the final inliers: two
// bitmaps over the train indices in LDS (bits: 2 * words, cleared by the caller), each lane counting the bits it set first.
struct TrainTally {
    uint32_t *bits;
    int words, trainRange;
    const PsDMatch *mm; // the pair's input matches
    int nIn;
    uint8_t *mask;      // ... and the caller's inlier flags
    int ua = 0, ui = 0;

    PS_D void all_matches(int first, int stride)
    {
        for (int i = first; i < nIn; i += stride) {
            const int t = mm[i].trainIdx;
            if (t >= 0 && t < trainRange) {
                const uint32_t bit = 1u << (t & 31);
                const uint32_t old = atomicOr(&bits[t >> 5], bit);
                ua += (old & bit) ? 0 : 1;
            }
        }
    }
    // a final inlier: its flag in the caller's mask and -- pointInlierRatio's numerator (RANSAC.h:56-66) -- its train index
    // in the second bitmap, where it is found (round 3 walked all input matches once more for this and read the mask back)
    PS_D void note_inlier(const int4 &d) // d = (index in the match list, queryIdx, trainIdx, 0)
    {
        mask[d.x] = 1;
        if (d.z >= 0 && d.z < trainRange) {
            const uint32_t bit = 1u << (d.z & 31);
            const uint32_t old = atomicOr(&bits[words + (d.z >> 5)], bit);
            ui += (old & bit) ? 0 : 1;
        }
    }
    // one LDS atomic per wave and tally (the compiler's own form walks the 64 lanes one by one)
    PS_D void reduce(int *s_uniq)
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ua += __shfl_down(ua, o, 64);
            ui += __shfl_down(ui, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&s_uniq[0], ua);
            atomicAdd(&s_uniq[1], ui);
        }
    }
};

// ---- (3) refit on the kin best inliers (wave 0; the other wavefronts tally the input matches meanwhile: the refit's serial
// Umeyama + Jacobi-SVD chain is 14 of this kernel's 35 us for a single pair, profiles/r03e/latency_stamps.json), then the
// re-selection with the Euclid/adaptive rule under the refitted model, which replaces mdl.  Returns the final inliers' number.
template <int BLOCK>
PS_D int refit_reselect(const SelectArgs &a, const ScoreConsts &k, int kin, bool accepted, const float4 *__restrict__ recA,
                        const float4 *__restrict__ recB, const int4 *__restrict__ recD, size_t rbase, const int32_t *list,
                        const float *s_stage, Rigid &s_model, int *s_wsum, unsigned long long *stamps, TrainTally &tally, Rigid &mdl,
                        const Rigid &inv)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (wv != 0) tally.all_matches(tid - 64, BLOCK - 64);
    if (wv == 0) {
        Rigid ref;
        wave_umeyama(kin, a.stageCap,
                     [&](int j, float4 &u, float4 &v) { // parked by the inlier pass
                         const float4 *q = reinterpret_cast<const float4 *>(s_stage + 8 * j);
                         u = q[0];
                         v = q[1];
                     },
                     [&](int j, float4 &u, float4 &v) { // more inliers than the LDS holds: from the records
                         const int i = list[j];
                         const float4 A = recA[rbase + i], B = recB[rbase + i];
                         u = make_float4(B.x, B.y, B.z, A.x);
                         v = make_float4(A.y, A.z, 0.0f, 0.0f);
                     },
                     ref);
        if (lane == 0) s_model = ref;
    }
    __syncthreads();
    phase_stamp(stamps, 7); // (3a) refit: wave-level Umeyama + Jacobi SVD
    mdl = s_model;
    // (two loops, one per source of the operands: a branch inside one loop was compiled into generic pointers and FLAT
    // loads; the order of the matches does not matter here)
    int nfinal = 0;
    auto reselect = [&](const float4 &A, const float4 &B, int i) {
        const bool in = inlier_test<PS_EUCLIDEAN_ERROR>(mdl, inv, k, A, B, A); // s < A.w : plain or adaptive bound
        if (in && accepted) tally.note_inlier(recD[rbase + i]);
        nfinal += in ? 1 : 0;
    };
    const int kLds = kin < a.stageCap ? kin : a.stageCap;
    for (int j = tid; j < kLds; j += BLOCK) { // parked by the inlier pass
        const float4 *q = reinterpret_cast<const float4 *>(s_stage + 8 * j);
        const float4 u = q[0], v = q[1];
        reselect(make_float4(u.w, v.x, v.y, v.z), make_float4(u.x, u.y, u.z, 0.0f), __float_as_int(v.w));
    }
    for (int j = a.stageCap + tid; j < kin; j += BLOCK) {
        const int i = list[j];
        reselect(recA[rbase + i], recB[rbase + i], i);
    }
    { // (each lane counted its own: one exchange at the end instead of a scan per trip)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nfinal += __shfl_down(nfinal, o, 64);
        if (lane == 0) s_wsum[wv] = nfinal;
        __syncthreads();
        nfinal = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) nfinal += s_wsum[w];
    }
    return accepted ? nfinal : 0; // identity + inliers cleared (RANSAC.cpp:161-164)
}

// USAC: no refit (USAC_wrapper.cpp:204-222 commented out); the loop's inliers are returned even
// when the ratio gate replaces the pose by identity (USAC_wrapper.cpp:139-141).
template <int BLOCK>
PS_D int usac_inliers(int kin, const int4 *__restrict__ recD, size_t rbase, const int32_t *list, TrainTally &tally)
{
    const int tid = threadIdx.x;
    for (int j = tid; j < kin; j += BLOCK) tally.note_inlier(recD[rbase + list[j]]);
    tally.all_matches(tid, BLOCK);
    return kin;
}

template <int BLOCK = kBlock>
__global__ __launch_bounds__(BLOCK) void ps_select_refit(const float4 *__restrict__ recA,
                                                          const float4 *__restrict__ recB,
                                                          const float4 *__restrict__ recC,
                                                          const int4 *__restrict__ recD,
                                                          const int32_t *__restrict__ mvalid,
                                                          const int32_t *__restrict__ counts,
                                                          const PsDMatch *__restrict__ matches,
                                                          const int32_t *__restrict__ numMatches, int matchStride,
                                                          ModelArgs ma, ScoreConsts k, SelectArgs a,
                                                          int32_t *__restrict__ idxList, float *__restrict__ poseOut,
                                                          uint8_t *__restrict__ maskOut,
                                                          PsRansacStats *__restrict__ statsOut,
                                                          unsigned long long *__restrict__ stamps,
                                                          const unsigned *__restrict__ bailDev, unsigned *__restrict__ bailHost)
{
    phase_stamp(stamps, 4);
    // the staged scoring's "nothing to gain" counters (ps_stage_reorder) on their way to the host's policy: two plain stores
    // into mapped host memory by one thread of the launch that follows every stage (nobody waits for them)
    if (bailHost != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        bailHost[0] = bailDev[0];
        bailHost[1] = bailDev[1];
    }
    extern __shared__ __align__(16) uint32_t s_bits[]; // two bitmaps over train indices: 2 * ceil(trainRange/32) words
    __shared__ int s_wsum[2 * (BLOCK / 64)];
    __shared__ unsigned long long s_red[BLOCK / 64];
    __shared__ int s_sel[4];
    __shared__ Rigid s_model;
    __shared__ int s_uniq[2];

    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    const int words = (a.trainRange + 31) >> 5;
    // [stageCap][8]: cur xyz (src), prev xyz (dst), the match's Euclidean bound, its index among the depth-valid matches
    float *s_stage = reinterpret_cast<float *>(s_bits + ((2 * words + 3) & ~3));
    const int M = mvalid[p];
    const int nIn = numMatches[p];
    const size_t rbase = (size_t)p * a.cap;
    const int32_t *cnts = counts + (size_t)p * a.H;
    uint8_t *mask = maskOut + (size_t)p * matchStride;
    int32_t *list = idxList + rbase;

    for (int i = tid; i < nIn; i += BLOCK) mask[i] = 0;

    const bool run = !(M < a.minMatches || M < 3);
    // The inlier pass' first records do not depend on the selection: their loads (written by another launch: HBM latency)
    // are in flight while the schedule is replayed; every later trip fetches the next one's before its scan.
    const bool needInv = (a.mode == PS_REPROJECTION_ERROR || a.mode == PS_EUCLIDEAN_AND_REPROJECTION_ERROR);
    const bool needC = needInv;
    float4 cA, cB, cC;
    auto fetch = [&](int i, float4 &A, float4 &B, float4 &C) {
        A = B = C = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < M) {
            A = recA[rbase + i];
            B = recB[rbase + i];
            if (needC) C = recC[rbase + i];
        }
    };
    if (run) fetch(tid, cA, cB, cC);

    Selection sel{-1, 0, 0};
    if (run)
        sel = a.estimator == PS_EST_FIXED ? select_fixed<BLOCK>(a, cnts, s_red, s_sel)
              : wave_replay(a)            ? select_wave(a, cnts, M)
                                          : select_block<BLOCK>(a, cnts, M, s_red, s_sel);

    phase_stamp(stamps, 5); // (1) selection replayed
    // ---- (2) inliers of the selected hypothesis ----
    Rigid mdl, inv;
    set_identity(mdl);
    set_identity(inv);
    int kin = 0;
    if (run && sel.bestIdx >= 0) {
        if (ma.models && sel.bestIdx < ma.modelH)
            load_model(ma, (size_t)p * ma.modelH + sel.bestIdx, mdl); // parked by kernel 3 (an invalid sample parks the identity)
        else
            gen_model(recA, recB, rbase, (uint32_t)M, ma, base_seed(ma) + (uint64_t)p, (uint32_t)sel.bestIdx, mdl);
        if (needInv) inverse_rigid_general(mdl, inv);
        kin = inlier_pass<BLOCK>(a, k, mdl, inv, M, fetch, cA, cB, cC, list, s_stage, s_wsum);
    }

    phase_stamp(stamps, 6); // (2) winner's model, inlier pass, ordered compaction
    const float ratioF = run ? (float)sel.bestCount / (float)M : 0.0f;
    const double ratioD = (double)ratioF;
    bool accepted = run && !(ratioD < a.minRatio);
    int nfinal = 0;

    // The tally of ALL input matches does not depend on the refit: the other wavefronts build it while wave 0 runs the refit.
    for (int i = tid; i < 2 * words; i += BLOCK) s_bits[i] = 0u;
    if (tid == 0) s_uniq[0] = s_uniq[1] = 0;
    __syncthreads();
    TrainTally tally{s_bits, words, a.trainRange, matches + (size_t)p * matchStride, nIn, mask};
    if (run && a.estimator != PS_EST_USAC)
        nfinal = refit_reselect<BLOCK>(a, k, kin, accepted, recA, recB, recD, rbase, list, s_stage, s_model, s_wsum, stamps, tally, mdl, inv);
    else if (run)
        nfinal = usac_inliers<BLOCK>(kin, recD, rbase, list, tally);
    else
        tally.all_matches(tid, BLOCK);

    phase_stamp(stamps, 8); // (3b) Euclidean re-selection, mask, (4) unique trainIdx among the final inliers
    tally.reduce(s_uniq);
    __syncthreads();

    if (tid == 0) {
        Rigid out = mdl;
        if (!accepted) set_identity(out);
        store_pose(poseOut + (size_t)p * 16, out);
        PsRansacStats st;
        st.numMatchesIn = nIn;
        st.numMatchesValid = M;
        st.bestHypothesis = sel.bestIdx;
        st.bestInlierCount = sel.bestCount;
        st.iterationsRun = sel.trips;
        st.numInliers = nfinal;
        st.accepted = accepted ? 1 : 0;
        st.bestInlierRatio = ratioF;
        st.pointInlierRatio = (double)s_uniq[1] / (double)s_uniq[0];
        statsOut[p] = st;
    }
    phase_stamp(stamps, 9); // (4) pointInlierRatio, pose and statistics stored
}

} // namespace psdev
