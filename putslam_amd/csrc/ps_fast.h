// ps_fast.h -- MatcherOpenCV::detectFeatures (reference src/Matcher/matcherOpenCV.cpp:118-180) for detector = "FAST", the first
// step of the refill chain of Matcher::trackKLT (src/Matcher/matcher.cpp:213-260): cvtColor(RGB2GRAY), the grid of ROIs, FAST-9/16
// with or without non-maximum suppression in every ROI, the per-ROI ordering and cut, the joined ordering and cut.
//
// The arithmetic is the project's reading of OpenCV 3.x's fast.cpp / fast_score.cpp (FAST_t<16>, cornerScore<16>) and of the 8-bit
// cvtColor(RGB2GRAY) (restated twice in tests/fast_ref.py, which the kernels are held to byte for byte).
// All of it is integer arithmetic:
//  * grey = (c0 * 4899 + c1 * 9617 + c2 * 1868 + 8192) >> 14: channel 0 takes the red weight whatever the host stored there;
//  * a pixel of an ROI of R x C pixels is a candidate in rows 3 .. R-4 and columns 3 .. C-4 OF THAT ROI; with d[k] = v - ring[k]
//    it is a corner iff nine cyclically consecutive d are all > t or all < -t; its score is max(t, D, B) - 1, D the largest over
//    the sixteen arcs of nine of the least d, B the same for -d; a non-corner scores 0;
//  * with suppression a corner is emitted iff its score is strictly above its eight neighbours' (all of them lie inside the ROI:
//    a candidate is three pixels from its edge), response = score; without it every corner is emitted with response 0;
//  * BOTH orderings by response are STABLE here (the reference's std::sort is not: among equal responses its order is whatever
//    its libstdc++ does): ties keep raster order inside an ROI and the order of the ROI loop -- columns outer, rows inner --
//    across ROIs.
//
// Shape: ps_fast_score, one launch over all frames, a work-group per 32 x 32 tile whose 38 x 38 grey pixels are converted into LDS,
// a thread per pixel column of the tile and four rows; ps_fast_select, a work-group per (frame, ROI), walks its ROI's score map
// twice -- a histogram of the 255 responses, then the placement -- and leaves the ROI's first maxInROI key points in order;
// ps_fast_merge, a work-group per frame, does the same over the ROI lists.  Responses are bytes, so each ordering is a counting
// sort; an element's place among its equals is counted with ballots and per-wave counts, never by the order atomics land in.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "ps_device_math.h"
#include "ps_glue.h"

namespace psdev {

constexpr int kFastTile = 32;                // pixels of a tile's side
constexpr int kFastBlock = 256;              // threads of the score pass: a column of the tile and every eighth row each
constexpr int kFastLds = kFastTile + 6;      // the tile with its three-pixel ring
constexpr int kFastSelBlock = 1024;          // threads of the selecting / merging work-group = elements of a chunk
constexpr int kFastSelWaves = kFastSelBlock / 64;

// The grid of ROIs (matcherOpenCV.cpp:133-146): ROI (k, i) starts at (k * cols / gridCols, i * rows / gridRows) and is
// cols / gridCols x rows / gridRows pixels, all integer divisions.  roiW = roiH = 0: no ROI holds a candidate.
struct FastGeom {
    int rows, cols, gridRows, gridCols;
    int roiW, roiH;
    int cw, ch; // candidate columns / rows of one ROI: roiW - 6, roiH - 6
};

// The ROI along one axis that pixel p falls into -- the last whose origin k * n / g is not beyond p -- and p's offset from that
// origin (a pixel of a remainder strip gets an offset >= roi).  largest k with k * n / g <= p  <=>  k * n <= (p + 1) * g - 1.
PS_D int fast_axis_offset(int p, int n, int g)
{
    int k = ((p + 1) * g - 1) / n;
    k = k > g - 1 ? g - 1 : k;
    return p - k * n / g;
}

// d[k] = v - ring[k] for the sixteen ring pixels around tile[cy][cx], then the corner test and the score
PS_D void fast_pixel(const uint8_t (*tile)[kFastLds + 2], int cy, int cx, int t, int &score, int &corner)
{
    const int v = tile[cy][cx];
    int d[16];
    d[0] = v - (int)tile[cy + 3][cx];
    d[1] = v - (int)tile[cy + 3][cx + 1];
    d[2] = v - (int)tile[cy + 2][cx + 2];
    d[3] = v - (int)tile[cy + 1][cx + 3];
    d[4] = v - (int)tile[cy][cx + 3];
    d[5] = v - (int)tile[cy - 1][cx + 3];
    d[6] = v - (int)tile[cy - 2][cx + 2];
    d[7] = v - (int)tile[cy - 3][cx + 1];
    d[8] = v - (int)tile[cy - 3][cx];
    d[9] = v - (int)tile[cy - 3][cx - 1];
    d[10] = v - (int)tile[cy - 2][cx - 2];
    d[11] = v - (int)tile[cy - 1][cx - 3];
    d[12] = v - (int)tile[cy][cx - 3];
    d[13] = v - (int)tile[cy + 1][cx - 3];
    d[14] = v - (int)tile[cy + 2][cx - 2];
    d[15] = v - (int)tile[cy + 3][cx - 1];
    // the two ring masks, doubled so that an arc may wrap; nine in a row by rotate-and-AND
    uint32_t up = 0, down = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        up |= (uint32_t)(d[k] > t) << k;
        down |= (uint32_t)(d[k] < -t) << k;
    }
    up |= up << 16;
    down |= down << 16;
    uint32_t a = up & (up >> 1), b = down & (down >> 1);
    a &= a >> 2;
    b &= b >> 2;
    a &= a >> 4;
    b &= b >> 4;
    a &= up >> 8;
    b &= down >> 8;
    corner = ((a | b) & 0xFFFFu) != 0;
    score = 0;
    if (corner) {
        // least / greatest d of every arc of nine: windows of 2, 4, 8, then the ninth
        int lo[16], hi[16], lo2[16], hi2[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            lo[k] = min(d[k], d[(k + 1) & 15]);
            hi[k] = max(d[k], d[(k + 1) & 15]);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            lo2[k] = min(lo[k], lo[(k + 2) & 15]);
            hi2[k] = max(hi[k], hi[(k + 2) & 15]);
        }
        int D = INT_MIN, B = INT_MAX;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            D = max(D, min(min(lo2[k], lo2[(k + 4) & 15]), d[(k + 8) & 15]));
            B = min(B, max(max(hi2[k], hi2[(k + 4) & 15]), d[(k + 8) & 15]));
        }
        score = max(t, max(D, -B)) - 1;
    }
}

// LDS of one tile of the score pass
struct FastTileLds {
    uint8_t tile[kFastLds][kFastLds + 2];
    uint8_t colOk[kFastTile], rowOk[kFastTile];
};

// The 32 x 32 tile at (tx0, ty0) of ONE image `img` (rows rowStride bytes apart, cn channels) of g.rows x g.cols pixels: its grey,
// score and corner bytes go to dense planes of g.cols bytes a row.  gray / corner may be null (ps_orb_detect.h scores a pyramid
// level, which is grey already and needs no corner plane).
PS_D void fast_score_tile(FastTileLds &s, const uint8_t *__restrict__ img, size_t rowStride, int cn, const FastGeom &g, int t, int tx0,
                          int ty0, uint8_t *__restrict__ gray, uint8_t *__restrict__ score, uint8_t *__restrict__ corner)
{
    const int tid = (int)threadIdx.x;
    for (int e = tid; e < kFastLds * kFastLds; e += kFastBlock) {
        const int ly = e / kFastLds, lx = e % kFastLds;
        const int x = tx0 + lx - 3, y = ty0 + ly - 3;
        int v = 0;
        if (x >= 0 && x < g.cols && y >= 0 && y < g.rows) {
            const uint8_t *p = img + (size_t)y * rowStride + (size_t)x * cn;
            // (CV_RGB2GRAY: channel 0 weighs 4899 here, 1868 in ps_orb.h's orb_gray -- intended)
            v = cn == 1 ? (int)p[0] : ((int)p[0] * 4899 + (int)p[1] * 9617 + (int)p[2] * 1868 + 8192) >> 14;
        }
        s.tile[ly][lx] = (uint8_t)v;
    }
    if (tid < 2 * kFastTile) { // which columns / rows of the tile are candidates of their ROI
        const bool row = tid >= kFastTile;
        const int i = tid & (kFastTile - 1), p = (row ? ty0 : tx0) + i, n = row ? g.rows : g.cols, roi = row ? g.roiH : g.roiW;
        bool ok = false;
        if (p < n && roi >= 7) {
            const int o = fast_axis_offset(p, n, row ? g.gridRows : g.gridCols);
            ok = o >= 3 && o <= roi - 4;
        }
        (row ? s.rowOk : s.colOk)[i] = ok;
    }
    __syncthreads();
    const int lx = tid & (kFastTile - 1), x = tx0 + lx;
    if (x >= g.cols) return;
    for (int ly = tid / kFastTile; ly < kFastTile; ly += kFastBlock / kFastTile) {
        const int y = ty0 + ly;
        if (y >= g.rows) break;
        int sc = 0, cr = 0;
        if (s.colOk[lx] && s.rowOk[ly]) fast_pixel(s.tile, ly + 3, lx + 3, t, sc, cr);
        const size_t o = (size_t)y * g.cols + x;
        if (gray) gray[o] = s.tile[ly + 3][lx + 3];
        score[o] = (uint8_t)sc;
        if (corner) corner[o] = (uint8_t)cr;
    }
}

// Grey, score and corner planes of every frame f of the set: one work-group per 32 x 32 tile.
__global__ __launch_bounds__(kFastBlock) void ps_fast_score(const uint8_t *__restrict__ src, size_t rowStride, size_t frameStride, int cn,
                                                            FastGeom g, int t, uint8_t *__restrict__ gray, uint8_t *__restrict__ score,
                                                            uint8_t *__restrict__ corner, size_t plane)
{
    __shared__ FastTileLds s;
    const size_t f = blockIdx.z;
    fast_score_tile(s, src + f * frameStride, rowStride, cn, g, t, (int)blockIdx.x * kFastTile, (int)blockIdx.y * kFastTile, gray + f * plane,
                    score + f * plane, corner + f * plane);
}

// LDS of the counting sort one work-group runs
struct FastSortLds {
    int first[256];   // elements of a key, then their exclusive prefix: the first output position of the key
    int placed[256];  // elements of a key that earlier chunks hold
    int wbin[kFastSelWaves][256];
    int total;
};

// the valid lanes of this wave that hold the same key (0 .. 255) as the caller
PS_D unsigned long long fast_peers(bool valid, int key)
{
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (key >> b) & 1;
        const unsigned long long bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// The first `take` of the elements 0 .. n-1 in the order (key ascending, index ascending).  src(i, key, payload) says whether
// index i is an element and gives its key (0 .. 255) and payload; the element that comes out at position p goes to
// sink(p, key, payload).  Returns how many came out.  Every thread of the 1024 calls it with the same n and take.
// An element's position is first[key] + (equal keys in earlier chunks) + (equal keys in earlier waves of its chunk) + (equal keys
// in earlier lanes of its wave): sums of counts, none of which depends on the order in which anything was added.
template <class Src, class Sink> PS_D int fast_stable_take(FastSortLds &s, int n, int take, const Src &src, const Sink &sink)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    int *wflat = &s.wbin[0][0];
    if (tid < 256) s.first[tid] = s.placed[tid] = 0;
#pragma unroll
    for (int j = 0; j < kFastSelWaves * 256 / kFastSelBlock; ++j) wflat[tid + j * kFastSelBlock] = 0;
    __syncthreads();
    for (int base = 0; base < n; base += kFastSelBlock) {
        const int i = base + tid;
        int key = 0;
        uint32_t pay = 0;
        const bool valid = i < n && src(i, key, pay);
        if (__ballot(valid) != 0ull) { // (wave-uniform)
            const unsigned long long peers = fast_peers(valid, key);
            if (valid && (peers & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&s.first[key], __popcll(peers));
        }
    }
    __syncthreads();
    if (w == 0) { // lane l owns keys 4l .. 4l + 3
        const int c0 = s.first[4 * lane], c1 = s.first[4 * lane + 1], c2 = s.first[4 * lane + 2], c3 = s.first[4 * lane + 3];
        const int sum = c0 + c1 + c2 + c3;
        int inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            inc += lane >= o ? v : 0;
        }
        const int ex = inc - sum;
        s.first[4 * lane] = ex;
        s.first[4 * lane + 1] = ex + c0;
        s.first[4 * lane + 2] = ex + c0 + c1;
        s.first[4 * lane + 3] = ex + c0 + c1 + c2;
        if (lane == 63) s.total = inc;
    }
    __syncthreads();
    const int kept = s.total < take ? s.total : take;
    if (kept <= 0) return 0;
    for (int base = 0; base < n; base += kFastSelBlock) {
        const int i = base + tid;
        int key = 0;
        uint32_t pay = 0;
        bool valid = i < n && src(i, key, pay);
        valid = valid && s.first[key] < kept; // a key whose first position lies beyond the cut places nothing
        if (!__syncthreads_or(valid)) continue;
        const unsigned long long peers = fast_peers(valid, key);
        const int inWave = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && inWave == 0) s.wbin[w][key] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int r = s.placed[key];
            for (int v = 0; v < w; ++v) r += s.wbin[v][key];
            const int pos = s.first[key] + r + inWave;
            if (pos < kept) sink(pos, key, pay);
        }
        int tot = 0;
        if (tid < 256) {
#pragma unroll
            for (int v = 0; v < kFastSelWaves; ++v) tot += s.wbin[v][tid];
        }
        __syncthreads();
        if (tid < 256) s.placed[tid] += tot;
#pragma unroll
        for (int j = 0; j < kFastSelWaves * 256 / kFastSelBlock; ++j) wflat[tid + j * kFastSelBlock] = 0;
        // (the barrier at the top of the next chunk stands between these stores and its reads)
    }
    return kept;
}

struct FastLists {
    uint32_t *list;     // [frame][ROI][slotCap]: y << 16 | x of the ROI's key points, in order
    int32_t *roiCount;  // [frame][ROI]
    int numRois, slotCap;
};

// candidate e of ROI (k, i) in raster order: emitted or not, key = 255 - response
struct FastRoiSrc {
    const uint8_t *map; // the frame's score plane (suppression) or corner plane
    int cols, cw, ox, oy, nms;
    PS_D bool operator()(int e, int &key, uint32_t &pay) const
    {
        const int ly = e / cw, x = ox + (e - ly * cw), y = oy + ly;
        const uint8_t *p = map + (size_t)y * cols + x;
        const int v = p[0];
        if (v == 0) return false;
        key = 255;
        if (nms) {
            const uint8_t *u = p - cols, *d = p + cols;
            const int m = max(max(max((int)u[-1], (int)u[0]), max((int)u[1], (int)p[-1])), max(max((int)p[1], (int)d[-1]), max((int)d[0], (int)d[1])));
            if (!(v > m)) return false;
            key = 255 - v;
        }
        pay = (uint32_t)y << 16 | (uint32_t)x;
        return true;
    }
};
struct FastRoiSink {
    uint32_t *out;
    PS_D void operator()(int pos, int, uint32_t pay) const { out[pos] = pay; }
};

// One work-group per (ROI, frame): the ROI's key points ordered by response descending, raster order among equals, the first
// maxInRoi of them.
__global__ __launch_bounds__(kFastSelBlock) void ps_fast_select(const uint8_t *__restrict__ score, const uint8_t *__restrict__ corner,
                                                                size_t plane, FastGeom g, int nms, int maxInRoi, FastLists l)
{
    __shared__ FastSortLds s;
    const int q = (int)blockIdx.x, f = (int)blockIdx.y;
    const int k = q / g.gridRows, i = q - k * g.gridRows; // columns outer, rows inner (matcherOpenCV.cpp:133-134)
    FastRoiSrc src;
    src.map = (nms ? score : corner) + (size_t)f * plane;
    src.cols = g.cols;
    src.cw = g.cw;
    src.ox = k * g.cols / g.gridCols + 3;
    src.oy = i * g.rows / g.gridRows + 3;
    src.nms = nms;
    FastRoiSink sink;
    sink.out = l.list + ((size_t)f * l.numRois + q) * l.slotCap;
    const int kept = fast_stable_take(s, g.cw * g.ch, maxInRoi < l.slotCap ? maxInRoi : l.slotCap, src, sink);
    if (threadIdx.x == 0) l.roiCount[(size_t)f * l.numRois + q] = kept;
}

// slot e of the frame's ROI lists, taken in the order of the ROI loop
struct FastMergeSrc {
    const uint8_t *score; // the frame's score plane
    const uint32_t *list;
    const int32_t *roiCount;
    int cols, slotCap, nms;
    PS_D bool operator()(int e, int &key, uint32_t &pay) const
    {
        const int q = e / slotCap;
        if (e - q * slotCap >= roiCount[q]) return false;
        pay = list[e];
        key = nms ? 255 - (int)score[(size_t)(pay >> 16) * cols + (pay & 0xFFFFu)] : 255;
        return true;
    }
};
struct FastMergeSink {
    float2 *xy;
    float *response;
    PS_D void operator()(int pos, int key, uint32_t pay) const
    {
        xy[pos] = make_float2((float)(pay & 0xFFFFu), (float)(pay >> 16));
        response[pos] = (float)(255 - key);
    }
};

// One work-group per frame: the ROI lists joined in loop order, ordered by response descending (stable), cut to maxFeatures.
__global__ __launch_bounds__(kFastSelBlock) void ps_fast_merge(const uint8_t *__restrict__ score, size_t plane, int cols, int nms,
                                                               FastLists l, int maxFeatures, int cap, float2 *__restrict__ xy,
                                                               float *__restrict__ response, int32_t *__restrict__ counts)
{
    __shared__ FastSortLds s;
    const int f = (int)blockIdx.x;
    FastMergeSrc src;
    src.score = score + (size_t)f * plane;
    src.list = l.list + (size_t)f * l.numRois * l.slotCap;
    src.roiCount = l.roiCount + (size_t)f * l.numRois;
    src.cols = cols;
    src.slotCap = l.slotCap;
    src.nms = nms;
    FastMergeSink sink;
    sink.xy = xy + (size_t)f * cap;
    sink.response = response + (size_t)f * cap;
    const int kept = fast_stable_take(s, l.numRois * l.slotCap, maxFeatures < cap ? maxFeatures : cap, src, sink);
    if (threadIdx.x == 0) counts[f] = kept;
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the detector, the launches and the entry points
struct PsFastDetector {
    int device = 0;
    int rows = 0, cols = 0, cn = 0, maxFrames = 0;
    size_t plane = 0;          // bytes of one frame's plane
    uint8_t *maps = nullptr;   // grey | score | corner, maxFrames planes each
    uint32_t *list = nullptr;  // the ROI lists and their counts: grown to what a call needs, never shrunk
    int32_t *roiCount = nullptr;
    size_t listElems = 0, roiElems = 0;
};

namespace {

// what a call does with an image shape and a PsDetectParams
struct FastPlan {
    FastGeom g;
    int t = 0, nms = 0, maxFeatures = 0, maxInRoi = 0, slotCap = 0, numRois = 0;
    long long candidates = 0; // candidate pixels of all ROIs
    long long need() const { return candidates < maxFeatures ? candidates : (long long)maxFeatures; } // rows a frame can fill
    bool any() const { return candidates > 0 && maxInRoi > 0; }
};

const char *fast_params_error(const PsDetectParams *p)
{
    if (!p) return "null PsDetectParams";
    if (p->gridRows < 1 || p->gridCols < 1) return "PsDetectParams: gridRows and gridCols must be at least 1";
    if (p->maximalTrackedFeatures < 0) return "PsDetectParams: maximalTrackedFeatures must not be negative";
    if (p->reserved != 0) return "PsDetectParams: reserved must be 0";
    return nullptr;
}

FastPlan fast_plan(int rows, int cols, const PsDetectParams &p)
{
    FastPlan pl;
    pl.t = p.threshold < 0 ? 0 : (p.threshold > 255 ? 255 : p.threshold); // FastFeatureDetector's clamp
    pl.nms = p.nonmaxSuppression != 0;
    pl.maxFeatures = p.maximalTrackedFeatures;
    const long long cells = (long long)p.gridCols * p.gridRows;
    const long long perRoi = 3ll * p.maximalTrackedFeatures / cells; // matcherOpenCV.cpp:127-130
    pl.maxInRoi = (int)perRoi;
    FastGeom &g = pl.g;
    g.rows = rows;
    g.cols = cols;
    g.roiW = cols / p.gridCols;
    g.roiH = rows / p.gridRows;
    if (g.roiW < 7 || g.roiH < 7) { // no ROI has a candidate: the kernels see one empty cell
        g.gridRows = g.gridCols = 1;
        g.roiW = g.roiH = g.cw = g.ch = 0;
        return pl;
    }
    g.gridRows = p.gridRows;
    g.gridCols = p.gridCols;
    g.cw = g.roiW - 6;
    g.ch = g.roiH - 6;
    pl.numRois = (int)cells;
    pl.candidates = cells * g.cw * g.ch;
    pl.slotCap = pl.maxInRoi < g.cw * g.ch ? pl.maxInRoi : g.cw * g.ch;
    return pl;
}

// room for the ROI lists of `frames` frames under `pl` (synchronous when it has to grow: hipFree waits for the device)
int fast_reserve(PsContext *ctx, PsFastDetector *det, const FastPlan &pl, int frames)
{
    const size_t rois = (size_t)frames * pl.numRois, elems = rois * pl.slotCap;
    if (elems > det->listElems) {
        if (det->list) (void)hipFree(det->list);
        det->list = nullptr;
        det->listElems = 0;
        const hipError_t e = hipMalloc((void **)&det->list, elems * sizeof(uint32_t));
        if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_detect_features: hipMalloc", e);
        det->listElems = elems;
    }
    if (rois > det->roiElems) {
        if (det->roiCount) (void)hipFree(det->roiCount);
        det->roiCount = nullptr;
        det->roiElems = 0;
        const hipError_t e = hipMalloc((void **)&det->roiCount, rois * sizeof(int32_t));
        if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_detect_features: hipMalloc", e);
        det->roiElems = rois;
    }
    return PS_OK;
}

int fast_detect_launch(PsContext *ctx, PsFastDetector *det, const uint8_t *pixels, size_t rowStride, size_t frameStride, int frames,
                       const FastPlan &pl, int cap, float *xy, float *response, int32_t *counts, int passes = 7)
{
    const size_t planes = (size_t)det->maxFrames * det->plane;
    uint8_t *gray = det->maps, *score = det->maps + planes, *corner = det->maps + 2 * planes;
    const dim3 tiles((unsigned)((det->cols + kFastTile - 1) / kFastTile), (unsigned)((det->rows + kFastTile - 1) / kFastTile), (unsigned)frames);
    if (passes & 1) {
        hipLaunchKernelGGL(ps_fast_score, tiles, dim3(kFastBlock), 0, ctx->stream, pixels, rowStride, frameStride, det->cn, pl.g, pl.t, gray,
                           score, corner, det->plane);
        PS_HIP(hipGetLastError());
    }
    if (!pl.any()) { // nothing can come out: the counts alone are written
        if (passes & 4) PS_HIP(hipMemsetAsync(counts, 0, (size_t)frames * sizeof(int32_t), ctx->stream));
        return PS_OK;
    }
    FastLists l;
    l.list = det->list;
    l.roiCount = det->roiCount;
    l.numRois = pl.numRois;
    l.slotCap = pl.slotCap;
    if (passes & 2) {
        hipLaunchKernelGGL(ps_fast_select, dim3((unsigned)pl.numRois, (unsigned)frames), dim3(kFastSelBlock), 0, ctx->stream,
                           (const uint8_t *)score, (const uint8_t *)corner, det->plane, pl.g, pl.nms, pl.maxInRoi, l);
        PS_HIP(hipGetLastError());
    }
    if (passes & 4) {
        hipLaunchKernelGGL(ps_fast_merge, dim3((unsigned)frames), dim3(kFastSelBlock), 0, ctx->stream, (const uint8_t *)score, det->plane,
                           det->cols, pl.nms, l, pl.maxFeatures, cap, reinterpret_cast<float2 *>(xy), response, counts);
        PS_HIP(hipGetLastError());
    }
    return PS_OK;
}

// ps_detect_features_device (passes = 7) and ps_debug_fast_passes, each reporting under its own name
int fast_detect_device(PsContext *ctx, PsFastDetector *det, const PsImageSet *images, const PsDetectParams *params, int capacity, float *xy,
                       float *response, int32_t *counts, int passes, const char *who)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const auto msg = [who](const char *what) { return std::string(who) + what; };
    if (const char *why = fast_params_error(params)) return fail(ctx, PS_ERR_BAD_ARG, why);
    if (params->maximalTrackedFeatures > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, msg(": maximalTrackedFeatures above PS_MAX_KPTS").c_str());
    size_t row = 0, frame = 0;
    rc = check_image_set(ctx, det, &PsFastDetector::maxFrames, images, 0, who, row, frame, false); // (the pixels: below, with the other arrays)
    if (rc) return rc;
    if (images->numFrames == 0) return PS_OK;
    const FastPlan pl = fast_plan(det->rows, det->cols, *params);
    if (capacity > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, msg(": capacity above PS_MAX_KPTS").c_str());
    if (capacity < 0 || capacity < pl.need())
        return fail(ctx, PS_ERR_BAD_ARG, msg(": capacity below min(maximalTrackedFeatures, candidate pixels)").c_str());
    if (!images->pixels || !counts || (capacity > 0 && (!xy || !response))) return fail(ctx, PS_ERR_BAD_ARG, msg(": null array").c_str());
    TimingOff toff(ctx);
    if (pl.any()) {
        rc = fast_reserve(ctx, det, pl, images->numFrames);
        if (rc) return rc;
    }
    HandoffGuard handoffGuard{ctx};
    return fast_detect_launch(ctx, det, images->pixels, row, frame, images->numFrames, pl, capacity, xy, response, counts, passes & 7);
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_detect_params(void) { return sizeof(PsDetectParams); }

int ps_fast_detector_create(PsContext *ctx, int rows, int cols, int channels, int maxFrames, PsFastDetector **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_fast_detector_create: null out");
    *out = nullptr;
    rc = image_shape_error(ctx, rows, cols, channels, "ps_fast_detector_create");
    if (rc) return rc;
    if (maxFrames < 1 || maxFrames > kImageMaxFrames) return fail(ctx, PS_ERR_BAD_ARG, "ps_fast_detector_create: maxFrames must lie in 1 .. 65535");
    HandleOwner<PsFastDetector> own(new PsFastDetector, ps_fast_detector_destroy);
    PsFastDetector *d = own.get();
    d->device = ctx->device;
    d->rows = rows;
    d->cols = cols;
    d->cn = channels;
    d->maxFrames = maxFrames;
    d->plane = (size_t)rows * cols;
    const hipError_t e = hipMalloc((void **)&d->maps, 3 * d->plane * (size_t)maxFrames);
    if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_fast_detector_create: hipMalloc", e);
    *out = own.release();
    return PS_OK;
}

void ps_fast_detector_destroy(PsFastDetector *det)
{
    if (!det) return;
    (void)hipSetDevice(det->device);
    if (det->maps) (void)hipFree(det->maps); // (hipFree waits for the device: queued work that reads the maps has finished)
    if (det->list) (void)hipFree(det->list);
    if (det->roiCount) (void)hipFree(det->roiCount);
    delete det;
}

int ps_detect_features_device(PsContext *ctx, PsFastDetector *det, const PsImageSet *images, const PsDetectParams *params, int capacity,
                              float *xy, float *response, int32_t *counts)
{
    return fast_detect_device(ctx, det, images, params, capacity, xy, response, counts, 7, "ps_detect_features_device");
}

int ps_debug_fast_passes(PsContext *ctx, PsFastDetector *det, const PsImageSet *images, const PsDetectParams *params, int capacity,
                         float *xy, float *response, int32_t *counts, int passes)
{
    return fast_detect_device(ctx, det, images, params, capacity, xy, response, counts, passes, "ps_debug_fast_passes");
}

int ps_detect_features(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsDetectParams *params,
                       float *xy, float *response, int cap, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (const char *why = fast_params_error(params)) return fail(ctx, PS_ERR_BAD_ARG, why);
    if (params->maximalTrackedFeatures > PS_MAX_KPTS)
        return fail(ctx, PS_ERR_UNSUPPORTED, "ps_detect_features: maximalTrackedFeatures above PS_MAX_KPTS");
    rc = image_shape_error(ctx, rows, cols, channels, "ps_detect_features");
    if (rc) return rc;
    rowStride = image_row_stride(cols, channels, rowStride);
    if (!img || !nout || rowStride == 0 || cap < 0 || (cap > 0 && (!xy || !response)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_detect_features: null array, negative cap or a row stride below a row");
    const FastPlan pl = fast_plan(rows, cols, *params);
    const int room = (int)pl.need(); // (at most maximalTrackedFeatures <= PS_MAX_KPTS)
    if (room == 0) {
        *nout = 0;
        return PS_OK;
    }
    TimingOff toff(ctx);
    PsFastDetector *det = nullptr;
    rc = ps_fast_detector_create(ctx, rows, cols, channels, 1, &det);
    if (rc) return rc;
    const HandleOwner<PsFastDetector> own(det, ps_fast_detector_destroy);
    if (pl.any()) {
        rc = fast_reserve(ctx, det, pl, 1);
        if (rc) return rc;
    }
    const size_t imgBytes = image_bytes(rows, cols, channels, rowStride);
    // one block: the image | count | xy | response
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes);
    const size_t oCount = lay.take<int32_t>(1, 16), oXy = lay.take<float2>((size_t)room), oResp = lay.take<float>((size_t)room), total = lay.total;
    const DeviceBlock blk(total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    PS_HIP(hipMemcpyAsync(d, img, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (a pageable source may change)
    rc = fast_detect_launch(ctx, det, (const uint8_t *)d, rowStride, 0, 1, pl, room, (float *)(d + oXy), (float *)(d + oResp),
                            (int32_t *)(d + oCount));
    if (rc) return rc;
    std::vector<char> back(total - oCount);
    PS_HIP(hipMemcpyAsync(back.data(), d + oCount, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    int32_t n = 0;
    std::memcpy(&n, back.data(), 4);
    if (n < 0 || n > room) return fail(ctx, PS_ERR_HIP, "ps_detect_features: the device returned an impossible count");
    *nout = n;
    if (n > cap) return fail(ctx, PS_ERR_BAD_ARG, "ps_detect_features: cap is too small (*nout = required)");
    std::memcpy(xy, back.data() + (oXy - oCount), (size_t)n * 8);
    std::memcpy(response, back.data() + (oResp - oCount), (size_t)n * 4);
    return PS_OK;
}

int ps_debug_fast_maps(PsContext *ctx, const PsFastDetector *det, int frame, uint8_t *gray, uint8_t *score, uint8_t *corner)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!det || det->device != ctx->device || frame < 0 || frame >= det->maxFrames)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_debug_fast_maps: null or foreign detector, or no such frame");
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const size_t planes = (size_t)det->maxFrames * det->plane, at = (size_t)frame * det->plane;
    if (gray) PS_HIP(hipMemcpy(gray, det->maps + at, det->plane, hipMemcpyDeviceToHost));
    if (score) PS_HIP(hipMemcpy(score, det->maps + planes + at, det->plane, hipMemcpyDeviceToHost));
    if (corner) PS_HIP(hipMemcpy(corner, det->maps + 2 * planes + at, det->plane, hipMemcpyDeviceToHost));
    return PS_OK;
}

} // extern "C"
