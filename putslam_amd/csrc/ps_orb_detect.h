// ps_orb_detect.h -- MatcherOpenCV::detectFeatures (reference src/Matcher/matcherOpenCV.cpp:118-180) for detector = "ORB", the
// shipped configuration (resources/putslammatcherOpenCVParameters.xml:64, matcherOpenCV.cpp:66-67): cvtColor(RGB2GRAY), the grid
// of ROIs, cv::ORB::create()->detect in every ROI, the per-ROI ordering and cut, the joined ordering and cut.
//
// The arithmetic is the project's reading of OpenCV 3.0 - 3.3's ORB_Impl::detectAndCompute (key points only), computeKeyPoints,
// HarrisResponses, ICAngles, KeyPointsFilter and scalar fastAtan2 (restated twice in
// tests/orb_detect_ref.py, which the kernels are held to byte for byte).  No OpenCV was at hand: the reading is UNPINNED.
// Integer arithmetic except where stated; float operations are single IEEE operations (the library is built with
// -ffp-contract=off); cvRound rounds half to even:
//  * grey: the WHOLE image with CV_RGB2GRAY -- section 8.10's weights, channel 0 weighs 4899 --, one channel as it is; every ROI
//    of the grid (section 8.10's geometry) is then an image of its own with ITS OWN pyramid of roiH x roiW = rows / gridRows x
//    cols / gridCols pixels: sizes, scales and the resize are section 8.11's, only the raw levels are read;
//  * constants of the reading: edgeThreshold 31, firstLevel 0, HARRIS_SCORE, patchSize 31;
//  * quotas: factor = (float)(1.0 / scaleFactor), nd = nFeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nLevels))
//    in float; for l = 0 .. nLevels-2: q_l = cvRound(nd), nd *= factor; q_last = max(nFeatures - sum, 0);
//  * per level: FAST-9/16 with suppression on the level as an image of its own (section 8.10, grid 1 x 1, response = score);
//    runByImageBorder keeps 31 <= x < cols_l - 31, 31 <= y < rows_l - 31 (rows_l or cols_l <= 62: nothing); retainBest(2 q_l) by the
//    FAST score: no more than n -> all stay, n = 0 -> none, else every key point whose response is >= the n-th largest stays --
//    TIES AT THE CUT ARE ALL KEPT;
//  * Harris at (x0, y0) of the raw level, block 7, k = 0.04f: over the 49 pixels p, Ix = (p[+1] - p[-1]) * 2 + (p[-s+1] - p[-s-1]) +
//    (p[s+1] - p[s-1]), Iy = (p[s] - p[-s]) * 2 + (p[s-1] - p[-s-1]) + (p[s+1] - p[-s+1]); int sums a = sum Ix^2, b = sum Iy^2,
//    c = sum Ix Iy; scale = 1.f / (4 * 7 * 255.f), s4 = scale * scale * scale * scale (left to right);
//    response = ((fa * fb - fc * fc) - (k * (fa + fb)) * (fa + fb)) * s4, every operation rounded on its own; then retainBest(q_l)
//    by this response, ties kept;
//  * angle: intensity centroid over the disc of half patch 15, umax = 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3; m10 = sum u I,
//    m01 = sum v I (integer sums commute: the order of OpenCV's loop is free); angle = fastAtan2((float)m01, (float)m10) degrees;
//  * fastAtan2: the fixed float sequence of orb_fast_atan2 below (OpenCV's scalar form as recollected);
//  * an ROI's list: levels ascending, raster order (y, then x) inside a level -- THE PROJECT'S DECISION, nth_element / partition
//    leave it open; pt = (x0 * scale_l, y0 * scale_l) (float products), octave = l, response = Harris;
//  * the grid loop is section 8.10's: both orderings STABLE by response > (descending floats), the cut to maxInROI =
//    maximalTrackedFeatures * 3 / (gridCols * gridRows), the ROI origin added as floats, the joined ordering, the cut to
//    maximalTrackedFeatures.
//
// Shape: slot f * R + q holds the pyramid of ROI q (loop order: columns outer, rows inner) of frame f, every level as raw | score.
// ps_orb_level0 (ps_orb.h, with the ROI window and the RGB2GRAY weights) and ps_orb_resize fill the raw levels; ps_orbdet_score,
// one launch per level over all slots, runs ps_fast.h's tile body with the level as the image; ps_orbdet_cut1, a work-group per
// (level, slot), is the counting sort over byte scores: the histogram's prefix gives the boundary score, everything at or above it
// is placed in raster order (a list holds one entry per 2 x 2 pixels of the level's interior -- two adjacent pixels cannot both be
// strict maxima --, so no tie is ever dropped); ps_orbdet_harris, a wavefront per survivor, reads the 9 x 9 and 31 x 31
// neighbourhoods where they lie and combines per-lane integer sums by a shuffle tree, lane 0 evaluates the floats;
// ps_orbdet_roi, a work-group per slot, cuts every level at q_l (kept iff fewer than q_l responses are greater: ties stay),
// compacts the kept ones with fast_stable_take and ranks them (rank = #greater + #equal and earlier); ps_orbdet_join, a
// work-group per frame, ranks the ROI lists the same way and writes the outputs.  Every position is a sum of counts.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ps_device_math.h"
#include "ps_fast.h"
#include "ps_glue.h"
#include "ps_orb.h"

namespace psdev {

constexpr int kOrbDetWaves = kOrbBlock / 64;
constexpr unsigned long long kOrbUmax = 0x3689ABCDDEEEFFFFull; // umax[v] = nibble v
constexpr int kOrbDetListShift = 28;                           // a compacted entry: level << 28 | offset inside the slot's lists

struct OrbDetLevel {
    OrbLevel lv;            // off: the raw plane, off + plane: the score plane
    unsigned listOff, listCap; // the level's survivor list inside a slot's lists; 0 entries: dead by the border rule
};
struct OrbDetQuota {
    int q[kOrbLevels];
};
PS_D int orbdet_quota(const OrbDetQuota &qs, int l)
{
    int q = 0;
#pragma unroll
    for (int k = 0; k < kOrbLevels; ++k) q = k == l ? qs.q[k] : q;
    return q;
}

// the lists of all slots: list1 / resp1 / ang1 / keep1 after the first cut, sel / selResp the compacted second cut
struct OrbDetLists {
    uint32_t *list1; // y << 16 | x, raster order
    float *resp1, *ang1;
    uint8_t *keep1;  // 1: survives retainBest(q_l)
    uint32_t *sel;
    float *selResp;
    int32_t *count1; // [slot][kOrbLevels]
    size_t listTotal;
};
struct OrbDetRoiLists {
    float2 *xy;
    float *resp, *ang;
    int32_t *oct;
    int32_t *count; // [slot]
    int cap;        // rows of a slot
};

// FAST score of one level of every slot: ps_fast.h's tile body, the level as the image
__global__ __launch_bounds__(kFastBlock) void ps_orbdet_score(uint8_t *__restrict__ planes, size_t slotBytes, OrbLevel lv, int t)
{
    __shared__ FastTileLds s;
    uint8_t *raw = planes + (size_t)blockIdx.z * slotBytes + lv.off;
    FastGeom g;
    g.rows = lv.rows;
    g.cols = lv.cols;
    g.gridRows = g.gridCols = 1;
    g.roiW = lv.cols;
    g.roiH = lv.rows;
    g.cw = lv.cols - 6;
    g.ch = lv.rows - 6;
    fast_score_tile(s, raw, (size_t)lv.cols, 1, g, t, (int)blockIdx.x * kFastTile, (int)blockIdx.y * kFastTile, nullptr, raw + lv.plane, nullptr);
}

// an emitted key point of the level's interior whose key lies at or below the boundary; all of them share key 0: raster order
struct OrbCutSrc {
    FastRoiSrc in;
    int boundary;
    PS_D bool operator()(int e, int &key, uint32_t &pay) const
    {
        int k = 0;
        if (!in(e, k, pay) || k > boundary) return false;
        key = 0;
        return true;
    }
};
struct OrbNoSink {
    PS_D void operator()(int, int, uint32_t) const {}
};

// retainBest(2 q_l) by the FAST score: one work-group per (level, slot)
__global__ __launch_bounds__(kFastSelBlock) void ps_orbdet_cut1(const uint8_t *__restrict__ planes, size_t slotBytes,
                                                                const OrbDetLevel *__restrict__ levels, OrbDetQuota qs, OrbDetLists L)
{
    __shared__ FastSortLds s;
    const int l = (int)blockIdx.x, slot = (int)blockIdx.y, tid = (int)threadIdx.x;
    const OrbDetLevel D = levels[l];
    const int n2 = 2 * orbdet_quota(qs, l);
    int kept = 0;
    if (D.listCap > 0 && n2 > 0) { // (uniform over the work-group)
        OrbCutSrc src;
        src.in.map = planes + (size_t)slot * slotBytes + D.lv.off + D.lv.plane;
        src.in.cols = D.lv.cols;
        src.in.cw = D.lv.cols - 2 * kOrbEdge;
        src.in.ox = src.in.oy = kOrbEdge;
        src.in.nms = 1;
        const int n = src.in.cw * (D.lv.rows - 2 * kOrbEdge);
        (void)fast_stable_take(s, n, 0, src.in, OrbNoSink()); // the histogram and its prefix: first[key] = key points above key's score
        const int total = s.total;
        const int below = __syncthreads_count(tid < 256 && s.first[tid & 255] < n2); // keys whose first position lies before the cut
        src.boundary = total <= n2 ? 255 : below - 1;                                 // the key that holds position n2 - 1
        FastRoiSink sink;
        sink.out = L.list1 + (size_t)slot * L.listTotal + D.listOff;
        kept = fast_stable_take(s, n, (int)D.listCap, src, sink);
    }
    if (tid == 0) L.count1[(size_t)slot * kOrbLevels + l] = kept;
}

// OpenCV's scalar fastAtan2 as recollected, degrees: one fixed float sequence
PS_D float orb_fast_atan2(float y, float x)
{
    const float k = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k, p5 = 0.1555786518463281f * k, p7 = -0.04432655554792128f * k;
    const float ax = fabsf(x), ay = fabsf(y);
    const float c = fminf(ax, ay) / (fmaxf(ax, ay) + (float)DBL_EPSILON);
    const float c2 = c * c;
    float a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    if (ax < ay) a = 90.f - a;
    if (x < 0.f) a = 180.f - a;
    if (y < 0.f) a = 360.f - a;
    return a;
}

PS_D float orb_harris_response(int a, int b, int c)
{
    const float scale = 1.f / (4 * 7 * 255.f);
    const float s4 = scale * scale * scale * scale;
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    return ((fa * fb - fc * fc) - (0.04f * (fa + fb)) * (fa + fb)) * s4;
}

// Harris response and intensity-centroid angle: one wavefront per survivor of the first cut
__global__ __launch_bounds__(kOrbBlock) void ps_orbdet_harris(const uint8_t *__restrict__ planes, size_t slotBytes,
                                                              const OrbDetLevel *__restrict__ levels, OrbDetLists L)
{
    const int slot = (int)blockIdx.y, l = (int)blockIdx.z, lane = (int)threadIdx.x & 63;
    const int wave = (int)blockIdx.x * kOrbDetWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), waves = (int)gridDim.x * kOrbDetWaves;
    const OrbDetLevel D = levels[l];
    const int n = min(L.count1[(size_t)slot * kOrbLevels + l], (int)D.listCap);
    const uint8_t *raw = planes + (size_t)slot * slotBytes + D.lv.off;
    const size_t base = (size_t)slot * L.listTotal + D.listOff;
    const int s = D.lv.cols;
    for (int j = wave; j < n; j += waves) {
        const uint32_t pay = L.list1[base + j];
        const uint8_t *c0 = raw + (size_t)(pay >> 16) * s + (pay & 0xFFFFu);
        int a = 0, b = 0, c = 0, m10 = 0, m01 = 0;
        if (lane < 49) {
            const int dy = lane / 7 - 3, dx = lane - (lane / 7) * 7 - 3;
            const uint8_t *p = c0 + dy * s + dx;
            const int ix = ((int)p[1] - (int)p[-1]) * 2 + ((int)p[-s + 1] - (int)p[-s - 1]) + ((int)p[s + 1] - (int)p[s - 1]);
            const int iy = ((int)p[s] - (int)p[-s]) * 2 + ((int)p[s - 1] - (int)p[-s - 1]) + ((int)p[s + 1] - (int)p[-s + 1]);
            a = ix * ix;
            b = iy * iy;
            c = ix * iy;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) { // the 31 x 31 square, 64 positions a step; inside the disc iff |u| <= umax[|v|]
            const int p = lane + 64 * k;
            const int row = p / 31, v = row - 15, u = p - row * 31 - 15;
            const int av = v < 0 ? -v : v, au = u < 0 ? -u : u;
            if (p < 961 && au <= (int)((kOrbUmax >> (4 * av)) & 15ull)) {
                const int I = c0[v * s + u];
                m10 += u * I;
                m01 += v * I;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
            c += __shfl_xor(c, o, 64);
            m10 += __shfl_xor(m10, o, 64);
            m01 += __shfl_xor(m01, o, 64);
        }
        if (lane == 0) {
            L.resp1[base + j] = orb_harris_response(a, b, c);
            L.ang1[base + j] = orb_fast_atan2((float)m01, (float)m10);
        }
    }
}

// entry i of a level's first list: kept by the second cut or not; all share key 0
struct OrbKeepSrc {
    const uint8_t *keep;
    uint32_t tag; // level << 28 | the list's offset
    PS_D bool operator()(int i, int &key, uint32_t &pay) const
    {
        if (!keep[i]) return false;
        key = 0;
        pay = tag + (uint32_t)i;
        return true;
    }
};
struct OrbKeepSink {
    uint32_t *sel;
    float *selResp;
    const float *resp; // the slot's resp1
    PS_D void operator()(int pos, int, uint32_t pay) const
    {
        sel[pos] = pay;
        selResp[pos] = resp[pay & ((1u << kOrbDetListShift) - 1u)];
    }
};

// retainBest(q_l) by the Harris response in every level of one slot: keep1, by the threads of one work-group
PS_D void orbdet_cut2(const OrbDetLevel *__restrict__ levels, int nLevels, const OrbDetQuota &qs, const OrbDetLists &L, int slot, int tid)
{
    const size_t sbase = (size_t)slot * L.listTotal;
    for (int l = 0; l < nLevels; ++l) {
        const OrbDetLevel D = levels[l];
        const int n = min(L.count1[(size_t)slot * kOrbLevels + l], (int)D.listCap), q = orbdet_quota(qs, l);
        const float *r = L.resp1 + sbase + D.listOff;
        for (int i = tid; i < n; i += kFastSelBlock) {
            const float ri = r[i];
            int greater = 0;
            for (int j = 0; j < n; ++j) greater += r[j] > ri;
            L.keep1[sbase + D.listOff + i] = greater < q; // at or above the q-th largest: ties stay
        }
    }
}

// The second cut alone, for a call that can emit nothing (maximalTrackedFeatures 0, or no quota on a live level): the diagnostic
// read-back of the level lists finds `kept` written by this call, not what an earlier call or the allocation left there
__global__ __launch_bounds__(kFastSelBlock) void ps_orbdet_cut2(const OrbDetLevel *__restrict__ levels, int nLevels, OrbDetQuota qs, OrbDetLists L)
{
    orbdet_cut2(levels, nLevels, qs, L, (int)blockIdx.x, (int)threadIdx.x);
}

// The second cut, then the ROI's ordering and its cut: one work-group per slot
__global__ __launch_bounds__(kFastSelBlock) void ps_orbdet_roi(const OrbDetLevel *__restrict__ levels, int nLevels, OrbDetQuota qs, OrbDetLists L,
                                                               OrbWindow win, int maxInRoi, OrbDetRoiLists R)
{
    __shared__ FastSortLds s;
    const int slot = (int)blockIdx.x, tid = (int)threadIdx.x;
    const size_t sbase = (size_t)slot * L.listTotal;
    orbdet_cut2(levels, nLevels, qs, L, slot, tid);
    __syncthreads();
    int m = 0;
    for (int l = 0; l < nLevels; ++l) {
        const OrbDetLevel D = levels[l];
        const int n = min(L.count1[(size_t)slot * kOrbLevels + l], (int)D.listCap);
        if (n == 0) continue; // (uniform)
        OrbKeepSrc src;
        src.keep = L.keep1 + sbase + D.listOff;
        src.tag = (uint32_t)l << kOrbDetListShift | D.listOff;
        OrbKeepSink sink;
        sink.sel = L.sel + sbase + m;
        sink.selResp = L.selResp + sbase + m;
        sink.resp = L.resp1 + sbase;
        m += fast_stable_take(s, n, n, src, sink);
        __syncthreads();
    }
    const int cells = win.gridRows * win.gridCols, q = slot % cells, wk = q / win.gridRows, wi = q - wk * win.gridRows;
    const float ox = (float)(wk * win.cols / win.gridCols), oy = (float)(wi * win.rows / win.gridRows);
    const int kept = min(min(m, maxInRoi), R.cap);
    const float *sr = L.selResp + sbase;
    for (int i = tid; i < m; i += kFastSelBlock) {
        const float ri = sr[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const float rj = sr[j];
            rank += (rj > ri) | ((rj == ri) & (j < i));
        }
        if (rank < kept) {
            const uint32_t e = L.sel[sbase + i], off = e & ((1u << kOrbDetListShift) - 1u);
            const int l = (int)(e >> kOrbDetListShift);
            const float scale = levels[l].lv.scale;
            const uint32_t pay = L.list1[sbase + off];
            const size_t o = (size_t)slot * R.cap + rank;
            R.xy[o] = make_float2((float)(pay & 0xFFFFu) * scale + ox, (float)(pay >> 16) * scale + oy);
            R.resp[o] = ri;
            R.ang[o] = L.ang1[sbase + off];
            R.oct[o] = l;
        }
    }
    if (tid == 0) R.count[slot] = kept;
}

// The ROI lists of a frame joined in loop order, ordered by response descending (stable), cut: one work-group per frame
__global__ __launch_bounds__(kFastSelBlock) void ps_orbdet_join(OrbDetRoiLists R, int numRois, int maxFeatures, int cap, float2 *__restrict__ xy,
                                                                float *__restrict__ response, float *__restrict__ angle,
                                                                int32_t *__restrict__ octave, int32_t *__restrict__ counts)
{
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int32_t *cnt = R.count + (size_t)f * numRois;
    int total = 0;
    for (int q = 0; q < numRois; ++q) total += min(cnt[q], R.cap);
    const int kept = min(min(total, maxFeatures), cap);
    for (int e = tid; e < numRois * R.cap; e += kFastSelBlock) {
        const int q = e / R.cap, p = e - q * R.cap;
        if (p >= min(cnt[q], R.cap)) continue;
        const size_t at = ((size_t)f * numRois + q) * R.cap + p;
        const float ri = R.resp[at];
        int rank = 0;
        for (int q2 = 0; q2 < numRois; ++q2) {
            const int c = min(cnt[q2], R.cap);
            const float *r = R.resp + ((size_t)f * numRois + q2) * R.cap;
            const bool before = q2 < q;
            for (int j = 0; j < c; ++j) {
                const float rj = r[j];
                rank += (rj > ri) | ((rj == ri) & (before | ((q2 == q) & (j < p))));
            }
        }
        if (rank < kept) {
            const size_t o = (size_t)f * cap + rank;
            xy[o] = R.xy[at];
            response[o] = ri;
            angle[o] = R.ang[at];
            octave[o] = R.oct[at];
        }
    }
    if (tid == 0) counts[f] = kept;
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the detector, the launches and the entry points
struct PsOrbDetector {
    int device = 0;
    int rows = 0, cols = 0, cn = 0, maxFrames = 0;
    int gridRows = 0, gridCols = 0, nLevels = 0, numRois = 0, slots = 0;
    float scaleFactor = 0.f;
    psdev::OrbDetLevel lv[psdev::kOrbLevels];
    size_t slotBytes = 0, listTotal = 0;
    uint8_t *planes = nullptr;  // per slot: raw | score of every level
    uint2 *table = nullptr;     // the resize coefficients of levels 1 ..
    psdev::OrbDetLevel *dLevels = nullptr;
    char *lists = nullptr;      // one block: list1 | resp1 | ang1 | sel | selResp | count1 | keep1
    psdev::OrbDetLists L;
    char *roi = nullptr;        // the ROI lists: grown to what a call needs, never shrunk
    size_t roiRows = 0;         // rows of a slot's ROI list the block holds
};

namespace {

enum { kOrbDetPassPyramid = 1, kOrbDetPassScore = 2, kOrbDetPassCut1 = 4, kOrbDetPassHarris = 8, kOrbDetPassRoi = 16, kOrbDetPassJoin = 32,
       kOrbDetPassAll = 63 };

const char *orbdet_params_error(const PsOrbDetectParams *p, bool &unsupported)
{
    unsupported = false;
    if (!p) return "null PsOrbDetectParams";
    if (p->nFeatures < 0) return "PsOrbDetectParams: nFeatures must not be negative";
    if (!(p->scaleFactor > 1.f && p->scaleFactor <= 2.f)) return "PsOrbDetectParams: scaleFactor must lie in (1, 2]";
    if (p->nLevels < 1 || p->nLevels > kOrbLevels) return "PsOrbDetectParams: nLevels must lie in 1 .. 8";
    if (p->gridRows < 1 || p->gridCols < 1) return "PsOrbDetectParams: gridRows and gridCols must be at least 1";
    if (p->maximalTrackedFeatures < 0) return "PsOrbDetectParams: maximalTrackedFeatures must not be negative";
    if (p->reserved != 0) return "PsOrbDetectParams: reserved must be 0";
    unsupported = true;
    if (p->nFeatures > PS_MAX_KPTS) return "PsOrbDetectParams: nFeatures above PS_MAX_KPTS";
    if (p->maximalTrackedFeatures > PS_MAX_KPTS) return "PsOrbDetectParams: maximalTrackedFeatures above PS_MAX_KPTS";
    unsupported = false;
    return nullptr;
}
int orbdet_params_check(PsContext *ctx, const PsOrbDetectParams *p)
{
    bool unsupported = false;
    if (const char *why = orbdet_params_error(p, unsupported)) return fail(ctx, unsupported ? PS_ERR_UNSUPPORTED : PS_ERR_BAD_ARG, why);
    return PS_OK;
}

// the per-level quotas of computeKeyPoints
OrbDetQuota orbdet_quotas(int nFeatures, float scaleFactor, int nLevels)
{
    OrbDetQuota qs;
    for (int l = 0; l < kOrbLevels; ++l) qs.q[l] = 0;
    const float factor = (float)(1.0 / (double)scaleFactor);
    float nd = (float)nFeatures * (1.f - factor) / (1.f - (float)std::pow((double)factor, (double)nLevels));
    int sum = 0;
    for (int l = 0; l < nLevels - 1; ++l) {
        qs.q[l] = (int)std::lrintf(nd);
        sum += qs.q[l];
        nd *= factor;
    }
    qs.q[nLevels - 1] = nFeatures - sum > 0 ? nFeatures - sum : 0;
    return qs;
}

// what a call does with a detector and a PsOrbDetectParams
struct OrbDetPlan {
    OrbDetQuota qs;
    int t = 0, maxFeatures = 0, maxInRoi = 0, roiCap = 0, maxQ = 0;
    long long need = 0; // rows a frame can fill
    bool any() const { return need > 0; }
};

OrbDetPlan orbdet_plan(const PsOrbDetector *det, const PsOrbDetectParams &p)
{
    OrbDetPlan pl;
    pl.qs = orbdet_quotas(p.nFeatures, p.scaleFactor, p.nLevels);
    pl.t = p.fastThreshold < 0 ? 0 : (p.fastThreshold > 255 ? 255 : p.fastThreshold);
    pl.maxFeatures = p.maximalTrackedFeatures;
    pl.maxInRoi = (int)(3ll * p.maximalTrackedFeatures / ((long long)p.gridCols * p.gridRows)); // matcherOpenCV.cpp:127-130
    long long room = 0; // what one ROI can emit: per live level its quota at least, its list at most (ties)
    for (int l = 0; l < det->nLevels; ++l) {
        if (pl.qs.q[l] > 0) room += det->lv[l].listCap;
        if (det->lv[l].listCap > 0 && pl.qs.q[l] > pl.maxQ) pl.maxQ = pl.qs.q[l];
    }
    pl.roiCap = (int)(room < pl.maxInRoi ? room : (long long)pl.maxInRoi);
    const long long all = (long long)det->numRois * pl.roiCap;
    pl.need = all < pl.maxFeatures ? all : (long long)pl.maxFeatures;
    return pl;
}

struct OrbDetRoiLayout {
    size_t oXy, oResp, oAng, oOct, oCount, total;
    OrbDetRoiLayout(size_t slots, size_t rows)
    {
        BlockLayout lay;
        oXy = lay.take<float2>(slots * rows, 16);
        oResp = lay.take<float>(slots * rows, 16);
        oAng = lay.take<float>(slots * rows, 16);
        oOct = lay.take<int32_t>(slots * rows, 16);
        oCount = lay.take<int32_t>(slots, 16);
        total = lay.total;
    }
};

// room for ROI lists of roiCap rows in every slot of the detector (synchronous when it has to grow: hipFree waits for the device)
int orbdet_reserve(PsContext *ctx, PsOrbDetector *det, const OrbDetPlan &pl)
{
    if ((size_t)pl.roiCap <= det->roiRows && det->roi) return PS_OK;
    if (det->roi) (void)hipFree(det->roi);
    det->roi = nullptr;
    det->roiRows = 0;
    const OrbDetRoiLayout lay((size_t)det->slots, (size_t)pl.roiCap);
    const hipError_t e = hipMalloc((void **)&det->roi, lay.total);
    if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_orb_detect_frames: hipMalloc", e);
    det->roiRows = (size_t)pl.roiCap;
    return PS_OK;
}

int orbdet_launch(PsContext *ctx, PsOrbDetector *det, const uint8_t *pixels, size_t rowStride, size_t frameStride, int frames,
                  const OrbDetPlan &pl, int cap, float *xy, float *response, float *angle, int32_t *octave, int32_t *counts, int passes)
{
    const int slots = frames * det->numRois;
    OrbWindow win;
    win.gridRows = det->gridRows;
    win.gridCols = det->gridCols;
    win.rows = det->rows;
    win.cols = det->cols;
    win.w0 = 4899; // CV_RGB2GRAY
    win.w2 = 1868;
    for (int l = 0; l < det->nLevels && (passes & (kOrbDetPassPyramid | kOrbDetPassScore)); ++l) {
        const OrbLevel &lv = det->lv[l].lv;
        const unsigned quads = ((unsigned)lv.rows * (unsigned)lv.cols + 3u) / 4u;
        const dim3 grid((quads + kOrbBlock - 1) / kOrbBlock, (unsigned)slots);
        if (l == 0 && (passes & kOrbDetPassPyramid)) {
            hipLaunchKernelGGL(ps_orb_level0, grid, dim3(kOrbBlock), 0, ctx->stream, pixels, rowStride, frameStride, det->cn, win, lv, det->planes,
                               det->slotBytes, 0);
            PS_HIP(hipGetLastError());
        }
        if (l > 0 && (passes & kOrbDetPassPyramid)) {
            hipLaunchKernelGGL(ps_orb_resize, grid, dim3(kOrbBlock), 0, ctx->stream, det->planes, det->slotBytes, 0, det->lv[l - 1].lv, lv,
                               (const uint2 *)det->table);
            PS_HIP(hipGetLastError());
        }
        if (passes & kOrbDetPassScore) {
            const dim3 tiles((unsigned)((lv.cols + kFastTile - 1) / kFastTile), (unsigned)((lv.rows + kFastTile - 1) / kFastTile), (unsigned)slots);
            hipLaunchKernelGGL(ps_orbdet_score, tiles, dim3(kFastBlock), 0, ctx->stream, det->planes, det->slotBytes, lv, pl.t);
            PS_HIP(hipGetLastError());
        }
    }
    if (passes & kOrbDetPassCut1) {
        hipLaunchKernelGGL(ps_orbdet_cut1, dim3((unsigned)det->nLevels, (unsigned)slots), dim3(kFastSelBlock), 0, ctx->stream,
                           (const uint8_t *)det->planes, det->slotBytes, (const OrbDetLevel *)det->dLevels, pl.qs, det->L);
        PS_HIP(hipGetLastError());
    }
    if (passes & kOrbDetPassHarris) {
        int gx = (2 * pl.maxQ + kOrbDetWaves - 1) / kOrbDetWaves; // a wave per survivor where no tie swells the list; the rest by stride
        gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
        hipLaunchKernelGGL(ps_orbdet_harris, dim3((unsigned)gx, (unsigned)slots, (unsigned)det->nLevels), dim3(kOrbBlock), 0, ctx->stream,
                           (const uint8_t *)det->planes, det->slotBytes, (const OrbDetLevel *)det->dLevels, det->L);
        PS_HIP(hipGetLastError());
    }
    if (!pl.any()) { // nothing can come out: the second cut for the read-back of the level lists, and the counts
        if (passes & kOrbDetPassRoi) {
            hipLaunchKernelGGL(ps_orbdet_cut2, dim3((unsigned)slots), dim3(kFastSelBlock), 0, ctx->stream, (const OrbDetLevel *)det->dLevels,
                               det->nLevels, pl.qs, det->L);
            PS_HIP(hipGetLastError());
        }
        if (passes & kOrbDetPassJoin) PS_HIP(hipMemsetAsync(counts, 0, (size_t)frames * sizeof(int32_t), ctx->stream));
        return PS_OK;
    }
    const OrbDetRoiLayout lay((size_t)det->slots, det->roiRows);
    OrbDetRoiLists R;
    R.xy = (float2 *)(det->roi + lay.oXy);
    R.resp = (float *)(det->roi + lay.oResp);
    R.ang = (float *)(det->roi + lay.oAng);
    R.oct = (int32_t *)(det->roi + lay.oOct);
    R.count = (int32_t *)(det->roi + lay.oCount);
    R.cap = (int)det->roiRows;
    if (passes & kOrbDetPassRoi) {
        hipLaunchKernelGGL(ps_orbdet_roi, dim3((unsigned)slots), dim3(kFastSelBlock), 0, ctx->stream, (const OrbDetLevel *)det->dLevels, det->nLevels,
                           pl.qs, det->L, win, pl.maxInRoi, R);
        PS_HIP(hipGetLastError());
    }
    if (passes & kOrbDetPassJoin) {
        hipLaunchKernelGGL(ps_orbdet_join, dim3((unsigned)frames), dim3(kFastSelBlock), 0, ctx->stream, R, det->numRois, pl.maxFeatures, cap,
                           reinterpret_cast<float2 *>(xy), response, angle, octave, counts);
        PS_HIP(hipGetLastError());
    }
    return PS_OK;
}

// ps_orb_detect_frames (every pass) and ps_debug_orb_detect_passes, each reporting under its own name
int orbdet_frames(PsContext *ctx, PsOrbDetector *det, const PsImageSet *images, const PsOrbDetectParams *params, int capacity, float *xy,
                  float *response, float *angle, int32_t *octave, int32_t *counts, int passes, const char *who)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const auto msg = [who](const char *what) { return std::string(who) + what; };
    rc = orbdet_params_check(ctx, params);
    if (rc) return rc;
    size_t row = 0, frame = 0;
    rc = check_image_set(ctx, det, &PsOrbDetector::maxFrames, images, 0, who, row, frame, false); // (the pixels: below, with the other arrays)
    if (rc) return rc;
    if (params->scaleFactor != det->scaleFactor || params->nLevels != det->nLevels || params->gridRows != det->gridRows ||
        params->gridCols != det->gridCols)
        return fail(ctx, PS_ERR_BAD_ARG, msg(": scaleFactor, nLevels, gridRows and gridCols must be the detector's").c_str());
    if (images->numFrames == 0) return PS_OK;
    const OrbDetPlan pl = orbdet_plan(det, *params);
    if (capacity > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, msg(": capacity above PS_MAX_KPTS").c_str());
    if (capacity < 0 || capacity < pl.need)
        return fail(ctx, PS_ERR_BAD_ARG, msg(": capacity below min(maximalTrackedFeatures, what the ROIs can emit)").c_str());
    if (!images->pixels || !counts || (capacity > 0 && (!xy || !response || !angle || !octave))) return fail(ctx, PS_ERR_BAD_ARG, msg(": null array").c_str());
    TimingOff toff(ctx);
    if (pl.any()) {
        rc = orbdet_reserve(ctx, det, pl);
        if (rc) return rc;
    }
    HandoffGuard handoffGuard{ctx};
    return orbdet_launch(ctx, det, images->pixels, row, frame, images->numFrames, pl, capacity, xy, response, angle, octave, counts,
                         passes & kOrbDetPassAll);
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_orb_detect_params(void) { return sizeof(PsOrbDetectParams); }

int ps_orb_detector_create(PsContext *ctx, int rows, int cols, int channels, const PsOrbDetectParams *params, int maxFrames, PsOrbDetector **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_detector_create: null out");
    *out = nullptr;
    rc = orbdet_params_check(ctx, params);
    if (rc) return rc;
    rc = image_shape_error(ctx, rows, cols, channels, "ps_orb_detector_create");
    if (rc) return rc;
    const long long cells = (long long)params->gridRows * params->gridCols;
    if (maxFrames < 1 || cells * maxFrames > kImageMaxFrames)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_detector_create: maxFrames x gridRows x gridCols must lie in 1 .. 65535");
    if (rows / params->gridRows < 1 || cols / params->gridCols < 1) return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_detector_create: an ROI of the grid is empty");
    HandleOwner<PsOrbDetector> own(new PsOrbDetector, ps_orb_detector_destroy);
    PsOrbDetector *d = own.get();
    d->device = ctx->device;
    d->rows = rows;
    d->cols = cols;
    d->cn = channels;
    d->maxFrames = maxFrames;
    d->gridRows = params->gridRows;
    d->gridCols = params->gridCols;
    d->nLevels = params->nLevels;
    d->scaleFactor = params->scaleFactor;
    d->numRois = (int)cells;
    d->slots = d->numRois * maxFrames;
    const int roiH = rows / params->gridRows, roiW = cols / params->gridCols;
    unsigned long long off = 0;
    unsigned tab = 0, listOff = 0;
    for (int l = 0; l < d->nLevels; ++l) {
        OrbLevel &lv = d->lv[l].lv;
        lv.scale = (float)std::pow((double)params->scaleFactor, (double)l);
        lv.invScale = 1.f / lv.scale;
        lv.rows = (int)std::lrintf((float)roiH / lv.scale);
        lv.cols = (int)std::lrintf((float)roiW / lv.scale);
        if (lv.rows < 1 || lv.cols < 1) return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_detector_create: a level of an ROI's pyramid is empty");
        lv.plane = ((unsigned)lv.rows * (unsigned)lv.cols + 15u) & ~15u;
        lv.off = off;
        off += 2ull * lv.plane;
        lv.xtab = tab;
        lv.ytab = tab + (l ? (unsigned)lv.cols : 0u);
        tab += l ? (unsigned)(lv.cols + lv.rows) : 0u;
        // the interior 31 .. n-32 of a live level; a strict maximum of its 3 x 3 leaves no second one in its 2 x 2 block
        const int iw = lv.cols - 2 * kOrbEdge, ih = lv.rows - 2 * kOrbEdge;
        d->lv[l].listOff = listOff;
        d->lv[l].listCap = (iw > 0 && ih > 0) ? (unsigned)((iw + 1) / 2) * (unsigned)((ih + 1) / 2) : 0u;
        listOff += d->lv[l].listCap;
    }
    d->slotBytes = (size_t)off;
    d->listTotal = listOff;
    std::vector<uint2> table(tab ? tab : 1u);
    for (int l = 1; l < d->nLevels; ++l) {
        orb_coeffs(d->lv[l - 1].lv.cols, d->lv[l].lv.cols, true, table.data() + d->lv[l].lv.xtab);
        orb_coeffs(d->lv[l - 1].lv.rows, d->lv[l].lv.rows, false, table.data() + d->lv[l].lv.ytab);
    }
    const size_t S = (size_t)d->slots, N = S * (d->listTotal ? d->listTotal : 1);
    BlockLayout lay;
    const size_t oList = lay.take<uint32_t>(N, 16), oResp = lay.take<float>(N, 16), oAng = lay.take<float>(N, 16), oSel = lay.take<uint32_t>(N, 16),
                 oSelResp = lay.take<float>(N, 16), oCount = lay.take<int32_t>(S * kOrbLevels, 16), oKeep = lay.take<uint8_t>(N, 16);
    hipError_t e = hipMalloc((void **)&d->planes, d->slotBytes * S);
    if (e == hipSuccess) e = hipMalloc((void **)&d->table, table.size() * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc((void **)&d->dLevels, sizeof(d->lv));
    if (e == hipSuccess) e = hipMalloc((void **)&d->lists, lay.total);
    if (e == hipSuccess) e = hipMemcpy(d->table, table.data(), table.size() * sizeof(uint2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d->dLevels, d->lv, sizeof(OrbDetLevel) * (size_t)d->nLevels, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d->lists + oCount, 0, S * kOrbLevels * sizeof(int32_t)); // (a debug read before any call finds empty lists)
    if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_orb_detector_create: hipMalloc", e);
    d->L.list1 = (uint32_t *)(d->lists + oList);
    d->L.resp1 = (float *)(d->lists + oResp);
    d->L.ang1 = (float *)(d->lists + oAng);
    d->L.sel = (uint32_t *)(d->lists + oSel);
    d->L.selResp = (float *)(d->lists + oSelResp);
    d->L.count1 = (int32_t *)(d->lists + oCount);
    d->L.keep1 = (uint8_t *)(d->lists + oKeep);
    d->L.listTotal = d->listTotal;
    *out = own.release();
    return PS_OK;
}

void ps_orb_detector_destroy(PsOrbDetector *det)
{
    if (!det) return;
    (void)hipSetDevice(det->device);
    if (det->planes) (void)hipFree(det->planes); // (hipFree waits for the device: queued work that reads the detector has finished)
    if (det->table) (void)hipFree(det->table);
    if (det->dLevels) (void)hipFree(det->dLevels);
    if (det->lists) (void)hipFree(det->lists);
    if (det->roi) (void)hipFree(det->roi);
    delete det;
}

int ps_orb_detector_level(const PsOrbDetector *det, int level, int32_t *dims2, float *scale)
{
    if (!det || level < 0 || level >= det->nLevels) return PS_ERR_BAD_ARG;
    if (dims2) {
        dims2[0] = det->lv[level].lv.rows;
        dims2[1] = det->lv[level].lv.cols;
    }
    if (scale) *scale = det->lv[level].lv.scale;
    return PS_OK;
}

int ps_orb_detect_quotas(const PsOrbDetectParams *params, int32_t *quotas8)
{
    bool unsupported = false;
    if (!quotas8 || orbdet_params_error(params, unsupported)) return PS_ERR_BAD_ARG;
    const OrbDetQuota qs = orbdet_quotas(params->nFeatures, params->scaleFactor, params->nLevels);
    for (int l = 0; l < kOrbLevels; ++l) quotas8[l] = qs.q[l];
    return PS_OK;
}

int ps_orb_detect_frames(PsContext *ctx, PsOrbDetector *det, const PsImageSet *images, const PsOrbDetectParams *params, int capacity, float *xy,
                         float *response, float *angle, int32_t *octave, int32_t *counts)
{
    return orbdet_frames(ctx, det, images, params, capacity, xy, response, angle, octave, counts, kOrbDetPassAll, "ps_orb_detect_frames");
}

int ps_debug_orb_detect_passes(PsContext *ctx, PsOrbDetector *det, const PsImageSet *images, const PsOrbDetectParams *params, int capacity,
                               float *xy, float *response, float *angle, int32_t *octave, int32_t *counts, int passes)
{
    return orbdet_frames(ctx, det, images, params, capacity, xy, response, angle, octave, counts, passes, "ps_debug_orb_detect_passes");
}

int ps_detect_features_orb(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsOrbDetectParams *params,
                           float *xy, float *response, float *angle, int32_t *octave, int cap, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = orbdet_params_check(ctx, params);
    if (rc) return rc;
    rc = image_shape_error(ctx, rows, cols, channels, "ps_detect_features_orb");
    if (rc) return rc;
    rowStride = image_row_stride(cols, channels, rowStride);
    if (!img || !nout || rowStride == 0 || cap < 0 || (cap > 0 && (!xy || !response || !angle || !octave)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_detect_features_orb: null array, negative cap or a row stride below a row");
    TimingOff toff(ctx);
    PsOrbDetector *det = nullptr;
    rc = ps_orb_detector_create(ctx, rows, cols, channels, params, 1, &det); // (refuses an empty ROI or level)
    if (rc) return rc;
    const HandleOwner<PsOrbDetector> own(det, ps_orb_detector_destroy);
    const OrbDetPlan pl = orbdet_plan(det, *params);
    const size_t room = (size_t)pl.need; // (at most maximalTrackedFeatures <= PS_MAX_KPTS)
    if (room == 0) {
        *nout = 0;
        return PS_OK;
    }
    rc = orbdet_reserve(ctx, det, pl);
    if (rc) return rc;
    const size_t imgBytes = image_bytes(rows, cols, channels, rowStride);
    // one block: the image | count | xy | response | angle | octave
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes);
    const size_t oCount = lay.take<int32_t>(1, 16), oXy = lay.take<float2>(room), oResp = lay.take<float>(room), oAng = lay.take<float>(room),
                 oOct = lay.take<int32_t>(room), total = lay.total;
    const DeviceBlock blk(total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    PS_HIP(hipMemcpyAsync(d, img, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (a pageable source may change)
    rc = orbdet_launch(ctx, det, (const uint8_t *)d, rowStride, 0, 1, pl, (int)room, (float *)(d + oXy), (float *)(d + oResp), (float *)(d + oAng),
                       (int32_t *)(d + oOct), (int32_t *)(d + oCount), kOrbDetPassAll);
    if (rc) return rc;
    std::vector<char> back(total - oCount);
    PS_HIP(hipMemcpyAsync(back.data(), d + oCount, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    int32_t n = 0;
    std::memcpy(&n, back.data(), 4);
    if (n < 0 || (size_t)n > room) return fail(ctx, PS_ERR_HIP, "ps_detect_features_orb: the device returned an impossible count");
    *nout = n;
    if (n > cap) return fail(ctx, PS_ERR_BAD_ARG, "ps_detect_features_orb: cap is too small (*nout = required)");
    std::memcpy(xy, back.data() + (oXy - oCount), (size_t)n * 8);
    std::memcpy(response, back.data() + (oResp - oCount), (size_t)n * 4);
    std::memcpy(angle, back.data() + (oAng - oCount), (size_t)n * 4);
    std::memcpy(octave, back.data() + (oOct - oCount), (size_t)n * 4);
    return PS_OK;
}

int ps_debug_orb_detect_level(PsContext *ctx, const PsOrbDetector *det, int slot, int level, uint8_t *raw, uint8_t *score, int32_t *numFirst,
                              uint32_t *yx, float *response, float *angle, uint8_t *kept, int cap)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!det || det->device != ctx->device || slot < 0 || slot >= det->slots || level < 0 || level >= det->nLevels || cap < 0)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_debug_orb_detect_level: null or foreign detector, no such slot or level, or a negative cap");
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const OrbDetLevel &D = det->lv[level];
    const uint8_t *at = det->planes + (size_t)slot * det->slotBytes + D.lv.off;
    const size_t bytes = (size_t)D.lv.rows * D.lv.cols;
    if (raw) PS_HIP(hipMemcpy(raw, at, bytes, hipMemcpyDeviceToHost));
    if (score) PS_HIP(hipMemcpy(score, at + D.lv.plane, bytes, hipMemcpyDeviceToHost));
    int32_t n = 0;
    PS_HIP(hipMemcpy(&n, det->L.count1 + (size_t)slot * kOrbLevels + level, 4, hipMemcpyDeviceToHost));
    if (n < 0 || (unsigned)n > D.listCap) return fail(ctx, PS_ERR_HIP, "ps_debug_orb_detect_level: the device holds an impossible count");
    if (numFirst) *numFirst = n;
    const size_t take = (size_t)(n < cap ? n : cap), base = (size_t)slot * det->listTotal + D.listOff;
    if (take > 0) {
        if (yx) PS_HIP(hipMemcpy(yx, det->L.list1 + base, take * 4, hipMemcpyDeviceToHost));
        if (response) PS_HIP(hipMemcpy(response, det->L.resp1 + base, take * 4, hipMemcpyDeviceToHost));
        if (angle) PS_HIP(hipMemcpy(angle, det->L.ang1 + base, take * 4, hipMemcpyDeviceToHost));
        if (kept) PS_HIP(hipMemcpy(kept, det->L.keep1 + base, take, hipMemcpyDeviceToHost));
    }
    return PS_OK;
}

} // extern "C"
