// ps_pair_records.h -- the record stage of a frame pair, once: what every route into RANSAC leaves behind for kernels 3 and 4.
// A route walks the pair's match list in order, drops the matches whose points fail the depth filter (RANSAC.cpp:65-74),
// compacts the survivors in order and hands each to PairRecords, which writes the scoring records (write_records), keeps
// the pair's bounds and, at the end, writes the valid count and the bounds and clears the scoring stage's counters.
// The routes: ps_crosscheck_prep (ps_match_stage.h), ps_l2_crosscheck (ps_match_l2.h), ps_map_emit (ps_map_match.h) and the
// caller's lists below (ps_prep_from_matches, ps_prep_match_lists).  A route keeps only what is its own: how it finds match
// i, its compaction scan, and how it writes matches / numMatches.
#pragma once

#include "ps_block.h"
#include "ps_device_math.h"

#include "../../include/putslam_hip.h"

namespace psdev {

struct PrepArgs {
    float fx, fy, cx, cy;   // camera matrix entries (cv::Mat CV_32FC1, RGBD.cpp:93-96)
    double thrE;            // inlierThresholdEuclidean
    int mode;               // RANSAC::ERROR_VERSION
    int cap;
    int ptsStride;          // floats between consecutive frames' point blocks (PsFrameSet::ptsFrameStride / 4; cap * 3 when dense)
    int32_t *zeroCounts;    // optional: the first zeroH counts of every pair (row stride zeroStride) to clear for kernel 3's
    int zeroH;              // split-range atomics (saves a memset launch)
    int zeroStride;
    int32_t *zeroSurvA, *zeroSurvB; // optional: per-pair survivor counters of the staged scoring to clear (ps_score_pass.h)
    int skipE, skipF;       // the reprojection kernels' record forms no launch of this call will read (RecPtrs::E / ::F)
};

// Where kernel 2 puts the records of the depth-valid matches (scratch arena, [P][cap] each unless noted).
struct RecPtrs {
    float4 *A;  // prev xyz + squared Euclid bound
    float4 *B;  // cur xyz, w = 1
    float4 *C;  // projections of prev and cur (realOld u v, realNew u v)
    int4 *D;    // (index in the match list, queryIdx, trainIdx, 0)
    float4 *E;  // offsets c - real of the decision-exact scoring paths: (cx - uOld, cx - uNew, cy - vOld, cy - vNew)
#ifdef PS_STREAM_DIAG
    float4 *S;  // -DPS_STREAM_DIAG builds only: a shadow block kernel 2 writes every record a second time into (7 x 16 B per match;
                // nothing reads it): doubles kernel 2's write traffic for the A/B of profiles/r06*/records_traffic_ab.txt
#endif
    float2 *F;  // the fast scoring kernel's packed match record for large launches, 40 B = 5 float2 per match, laid out as
                // the SGPR pairs its packed instructions take (one s_load_dwordx8 + one dwordx2, no repacking; 8 B less
                // scalar-cache footprint per match than prev + cur + offsets):
                // (cur.x, prev.x) (cur.y, prev.y) (cur.z, prev.z) (cx - uOld, cx - uNew) (cy - vOld, cy - vNew)
    float *G;   // the Euclidean fast scoring kernel's pair-interleaved record (ps_score_euclid.h), [P][ceil(cap/2)][12 or 16]:
                // match 2k in the even floats, match 2k+1 in the odd ones; null unless that kernel will run (it then
                // replaces E and F, which only the reprojection kernels read)
};

// Builds the records of depth-valid match number v of pair p; returns the largest |offset| of E.
// `fixedBound` = sq_bound_f32(inlierThresholdEuclidean), the same for every match unless the mode is ADAPTIVE (the caller
// computes it once: the exact squared-domain bound costs two or three square roots).
PS_D float write_records(const PrepArgs &a, const RecPtrs &r, int p, int v, int srcIdx, int q, int t, float px, float py,
                         float pz, float cx_, float cy_, float cz_, float fixedBound)
{
    // Euclid rule of RANSAC.cpp:268-272: thr = inlierThresholdEuclidean (* prev.z in ADAPTIVE mode),
    // turned into its exact squared-domain bound.
    const float bound = a.mode == PS_ADAPTIVE_ERROR ? sq_bound_f32(a.thrE * (double)pz) : fixedBound;
    const size_t slot = (size_t)p * a.cap + (size_t)v;
    r.A[slot] = make_float4(px, py, pz, bound);
    r.B[slot] = make_float4(cx_, cy_, cz_, 1.0f);
    r.D[slot] = make_int4(srcIdx, q, t, 0);
    // the projections (four divisions) are read by the reprojection metrics only
    const bool euclidOnly = a.mode == PS_EUCLIDEAN_ERROR || a.mode == PS_ADAPTIVE_ERROR;
    float ou = 0.0f, ov = 0.0f, nu = 0.0f, nv = 0.0f;
    if (!euclidOnly) {
        project(px, py, pz, a.fx, a.fy, a.cx, a.cy, ou, ov);    // realOld  (RANSAC.cpp:357-358)
        project(cx_, cy_, cz_, a.fx, a.fy, a.cx, a.cy, nu, nv); // realNew  (RANSAC.cpp:352-353)
        r.C[slot] = make_float4(ou, ov, nu, nv);
    }
    if (r.G != nullptr) {
        // Euclidean metrics: the pair-interleaved operands of ps_ransac_score_euclid; errorVersion 4 normalises the match
        // by its own depth (the adaptive threshold thr * prev.z becomes the constant thr, ps_score_euclid.h)
        const bool adaptive = a.mode == PS_ADAPTIVE_ERROR;
        const int rf = adaptive ? 16 : 12;
        float *g = r.G + ((size_t)p * (size_t)((a.cap + 1) >> 1) + (size_t)(v >> 1)) * rf + (v & 1);
        if (adaptive) {
            const float w = 1.0f / pz;
            g[0] = cx_ * w; g[2] = cy_ * w; g[4] = cz_ * w; g[6] = w;
            g[8] = px * w; g[10] = py * w; g[12] = pz * w; g[14] = 0.0f;
        } else {
            g[0] = cx_; g[2] = cy_; g[4] = cz_;
            g[6] = px; g[8] = py; g[10] = pz;
        }
        return 0.0f;
    }
    if (euclidOnly) return 0.0f;
    // offsets of the decision-exact scoring paths (ps_score_fast.h): predicted - real = quotient + (c - real)
    // (laid out as the two v_pk_fma_f32 operand pairs: u offsets of both directions, then v offsets)
    const float4 e = make_float4(a.cx - ou, a.cx - nu, a.cy - ov, a.cy - nv);
    if (!a.skipE) r.E[slot] = e;
    if (!a.skipF) {
        float2 *f = r.F + 5 * slot;
        f[0] = make_float2(cx_, px); f[1] = make_float2(cy_, py); f[2] = make_float2(cz_, pz);
        f[3] = make_float2(e.x, e.y); f[4] = make_float2(e.z, e.w);
    }
#ifdef PS_STREAM_DIAG
    if (r.S != nullptr) { // (diagnostic build: every record once more, into a block nothing reads)
        float4 *sh = r.S + 7 * slot;
        sh[0] = make_float4(px, py, pz, bound); sh[1] = make_float4(cx_, cy_, cz_, 1.0f); sh[2] = make_float4(ou, ov, nu, nv);
        sh[3] = make_float4((float)srcIdx, (float)q, (float)t, 0.0f); sh[4] = make_float4(cx_, px, cy_, py);
        sh[5] = make_float4(cz_, pz, e.x, e.y); sh[6] = make_float4(e.z, e.w, 0.0f, 0.0f);
    }
#endif
    // (a NaN offset reports an infinite bound: the decision-exact kernels then leave the pair to the value-exact code)
    const bool num = e.x == e.x && e.y == e.y && e.z == e.z && e.w == e.w;
    return num ? fmaxf(fmaxf(fabsf(e.x), fabsf(e.y)), fmaxf(fabsf(e.z), fabsf(e.w))) : INFINITY;
}

// An odd number of depth-valid matches leaves the second half of the last pair record unwritten: it repeats the first
// (finite, inside the pair's bounds; the scoring kernel does not count it).  Called by one thread after the records of
// the pair are visible to it.
PS_D void finish_pair_records(const PrepArgs &a, const RecPtrs &r, int p, int M)
{
    if (r.G == nullptr || !(M & 1)) return;
    const int rf = a.mode == PS_ADAPTIVE_ERROR ? 16 : 12;
    float *g = r.G + ((size_t)p * (size_t)((a.cap + 1) >> 1) + (size_t)(M >> 1)) * rf;
    for (int i = 0; i < rf; i += 2) g[i + 1] = g[i];
}

// the depth filter of a match: both of its points
PS_D bool match_depth_ok(float px, float py, float pz, float cx_, float cy_, float cz_)
{
    return depth_ok(px, py, pz) && depth_ok(cx_, cy_, cz_);
}

// One thread's share of the record stage of pair p.  `wanted` = false (a route's form without records) costs nothing: the
// exact bound is not computed, and the route calls neither add nor finish.
struct PairRecords {
    const PrepArgs &a;
    const RecPtrs &rec;
    const int p;
    const float fixedBound; // write_records' bound unless the mode is ADAPTIVE
    float cm = 0.0f;        // largest |coordinate| among this pair's depth-valid matches
    float um = 0.0f;        // largest |c - projection| among them (NaN offsets are skipped by fmaxf; they only ever score "out")
    int vbase = 0;          // depth-valid matches of the trips so far

    PS_D PairRecords(const PrepArgs &a_, const RecPtrs &rec_, int p_, bool wanted = true)
        : a(a_), rec(rec_), p(p_), fixedBound((wanted && a_.mode != PS_ADAPTIVE_ERROR) ? sq_bound_f32(a_.thrE) : 0.0f)
    {
    }

    // One trip of the route's loop, called by every thread: `ok` = this thread holds a depth-valid match -- number srcIdx of
    // the pair's list, (q, t), the two points --, vpos = its place among the trip's vtotal valid ones (the route's scan).
    PS_D void add(bool ok, int vpos, int vtotal, int srcIdx, int q, int t, float px, float py, float pz, float cx_, float cy_,
                  float cz_)
    {
        if (ok) {
            um = fmaxf(um, write_records(a, rec, p, vbase + vpos, srcIdx, q, t, px, py, pz, cx_, cy_, cz_, fixedBound));
            cm = fmaxf(cm, fmaxf(fmaxf(fabsf(px), fabsf(py)), fmaxf(fabsf(pz), fmaxf(fabsf(cx_), fmaxf(fabsf(cy_), fabsf(cz_))))));
        }
        vbase += vtotal;
    }

    // After the last trip, called by every thread: the pair's valid count and bounds, the `G` tail, the counters of the
    // scoring stage cleared.  block_max2 ends with a barrier: behind it every thread's records are visible to thread 0,
    // which finish_pair_records needs.  `red`: BLOCK / 64 entries of LDS.
    template <int BLOCK> PS_D void finish(float2 *red, int32_t *__restrict__ mvalid, float2 *__restrict__ cmaxOut)
    {
        block_max2<BLOCK>(cm, um, red);
        if (threadIdx.x == 0) {
            cmaxOut[p] = make_float2(cm, um);
            mvalid[p] = vbase;
            finish_pair_records(a, rec, p, vbase);
            if (a.zeroSurvA) {
                a.zeroSurvA[p] = 0;
                a.zeroSurvB[p] = 0;
            }
        }
        if (a.zeroCounts)
            for (int i = threadIdx.x; i < a.zeroH; i += BLOCK) a.zeroCounts[(size_t)p * a.zeroStride + i] = 0;
    }
};

// Pair p's records from a caller-supplied list of m matches over the point blocks prev / cur, by one work-group of kBlock threads
// in tiles of kBlock matches.  CHECKED: the list comes from device memory nobody has looked at: a match whose queryIdx lies
// outside 0 .. nprev-1 or whose trainIdx lies outside 0 .. ncur-1 is not followed and fails the filter, and `clean` receives the
// list with the trainIdx of every such match replaced by -1 (what kernel 4 reads for pointInlierRatio: a train index it skips).
// s_wsum: 2 * (kBlock / 64) ints, s_red: kBlock / 64 entries.
template <bool CHECKED>
PS_D void prep_match_list(const float *__restrict__ prev, int nprev, const float *__restrict__ cur, int ncur,
                          const PsDMatch *__restrict__ matches, int m, const PrepArgs &a, const RecPtrs &rec, int p,
                          int32_t *__restrict__ mvalid, float2 *__restrict__ cmaxOut, PsDMatch *__restrict__ clean, int *s_wsum,
                          float2 *s_red)
{
    PairRecords pr(a, rec, p);
    int trip = 0;
    for (int i0 = 0; i0 < m; i0 += kBlock, ++trip) {
        const int i = i0 + threadIdx.x;
        float px = 0, py = 0, pz = 0, cx_ = 0, cy_ = 0, cz_ = 0;
        int q = 0, t = 0;
        bool ok = false;
        if (i < m) {
            PsDMatch mt = matches[i];
            q = mt.queryIdx;
            t = mt.trainIdx;
            const bool in = !CHECKED || (q >= 0 && q < nprev && t >= 0 && t < ncur);
            if (CHECKED) {
                if (!in) mt.trainIdx = -1;
                clean[i] = mt;
            }
            if (in) {
                px = prev[3 * q]; py = prev[3 * q + 1]; pz = prev[3 * q + 2];
                cx_ = cur[3 * t]; cy_ = cur[3 * t + 1]; cz_ = cur[3 * t + 2];
                ok = match_depth_ok(px, py, pz, cx_, cy_, cz_);
            }
        }
        int vtotal;
        const int vpos = block_scan_flag<kBlock, false>(ok, vtotal, s_wsum, trip);
        pr.add(ok, vpos, vtotal, i, q, t, px, py, pz, cx_, cy_, cz_);
    }
    pr.finish<kBlock>(s_red, mvalid, cmaxOut);
}

// Depth filter + records for a caller-supplied match list (stand-alone RANSAC entry point; the host checked the indices).
__global__ __launch_bounds__(kBlock) void ps_prep_from_matches(const float *__restrict__ prev,
                                                               const float *__restrict__ cur,
                                                               const PsDMatch *__restrict__ matches, int m, PrepArgs a,
                                                               RecPtrs rec, int32_t *__restrict__ mvalid,
                                                               float2 *__restrict__ cmaxOut)
{
    __shared__ int s_wsum[2 * (kBlock / 64)];
    __shared__ float2 s_red[kBlock / 64];
    prep_match_list<false>(prev, 0, cur, 0, matches, m, a, rec, 0, mvalid, cmaxOut, nullptr, s_wsum, s_red);
}

// The point block of one set of a device-resident group of point sets (PsPointSets, include/putslam_hip.h)
struct PointSetsArgs {
    const float *pts;
    const int32_t *counts;
    int numSets, capacity;
    int strideFloats; // floats between consecutive sets' blocks
};

// The batched form: one work-group per pair over device-resident lists (ps_ransac_match_lists).  Pair p matches set
// pairs[2p] of `prev` with set pairs[2p + 1] of `cur` (pairs = null: set p of both).  numMatches[p] outside 0 .. cap, a set index
// outside its group or a set count outside 0 .. capacity: the pair's list counts as empty -- numClean[p] = 0, what kernel 4 is
// given as the pair's match count, so that it writes no mask byte.
__global__ __launch_bounds__(kBlock) void ps_prep_match_lists(PointSetsArgs prev, PointSetsArgs cur, const int32_t *__restrict__ pairs,
                                                              const PsDMatch *__restrict__ matches,
                                                              const int32_t *__restrict__ numMatches, PrepArgs a, RecPtrs rec,
                                                              int32_t *__restrict__ mvalid, float2 *__restrict__ cmaxOut,
                                                              PsDMatch *__restrict__ clean, int32_t *__restrict__ numClean)
{
    __shared__ int s_wsum[2 * (kBlock / 64)];
    __shared__ float2 s_red[kBlock / 64];
    const int p = blockIdx.x;
    const int sq = pairs ? pairs[2 * p] : p, st = pairs ? pairs[2 * p + 1] : p;
    const bool sets = sq >= 0 && sq < prev.numSets && st >= 0 && st < cur.numSets;
    const int nq = sets ? prev.counts[sq] : -1, nt = sets ? cur.counts[st] : -1;
    const int given = numMatches[p];
    const bool ok = sets && nq >= 0 && nq <= prev.capacity && nt >= 0 && nt <= cur.capacity && given >= 0 && given <= a.cap;
    const int m = ok ? given : 0;
    if (threadIdx.x == 0) numClean[p] = m;
    const size_t row = (size_t)p * (size_t)a.cap;
    prep_match_list<true>(prev.pts + (size_t)(ok ? sq : 0) * (size_t)prev.strideFloats, nq,
                          cur.pts + (size_t)(ok ? st : 0) * (size_t)cur.strideFloats, nt, matches + row, m, a, rec, p, mvalid, cmaxOut,
                          clean + row, s_wsum, s_red);
}

} // namespace psdev
