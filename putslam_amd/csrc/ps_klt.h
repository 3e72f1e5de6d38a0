// ps_klt.h -- MatcherOpenCV::performTracking (reference src/Matcher/matcherOpenCV.cpp:209-300), the first step of
// Matcher::trackKLT (src/Matcher/matcher.cpp:133-449): cv::calcOpticalFlowPyrLK on an image pair, the error gate, the
// too-close-by-error removal and the compaction into cv::DMatch(i, j, 0).
//
// The arithmetic is the project's reading of OpenCV 3.x's lkpyramid.cpp, scalar path, float accumulators (DESIGN.md section
// 8.9; restated sequentially in tests/klt_ref.py, which the kernels are held to byte for byte):
//  * pyramid: level l+1 = 5x5 binomial sum at (2x, 2y), (sum + 128) >> 8; Scharr derivatives as int16 pairs; integer, exact;
//  * every level is STORED with its W-wide border -- REFLECT_101 for the image, 0 for the derivative -- so the tracker's gathers
//    are the four bilinear taps and nothing else;
//  * per point and level: the I / Ix / Iy window as int16 (14-bit weights, rint half to even), the 2x2 matrix and the
//    mismatch vector as FLOAT sums taken in window order, the minEig / determinant gate, up to maxCount Gauss-Newton steps.
//
// Shape: one launch per pyramid level and pass over all frames of a set; the tracker is one wavefront per (pair, point) that
// walks the levels from the top.  The window's W x W x cn elements are spread over the 64 lanes: each lane samples its elements,
// keeps I / Ix / Iy in LDS as int16 and writes the per-element products to LDS as floats; the float sums are sequential by
// definition, so one lane per sum (three for the matrix, two for the vector, one for the error) walks its products in window
// order.  Waves never wait for one another (no work-group barrier: their trip counts differ).  The selection is one work-group
// per pair: every point decides its own mark by a sweep over all others staged through LDS, then an ordered compaction.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>
#include <vector>

#include "ps_device_math.h"
#include "ps_exclusion.h"
#include "ps_glue.h"

namespace psdev {

constexpr int kKltLevels = 8;      // level 0 and up to seven reduced ones
constexpr int kKltBlock = 256;     // threads of a pyramid-pass work-group; the tracker's at most
constexpr int kKltSelBlock = 1024; // threads of the selecting work-group = points of an LDS tile
constexpr int kKltSelWaves = kKltSelBlock / 64;

// One stored level: the image as (rows + 2W) x (cols + 2W) x cn bytes, the derivative with the same element index as packed
// int16 pairs (Ix low, Iy high).  Offsets are counted from the slot's start, in elements of either array.
struct KltLevel {
    int rows, cols;
    int estride; // elements per padded row: (cols + 2W) * cn
    int total;   // elements of the padded level
    unsigned long long off;
};

__device__ __forceinline__ int klt_reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// Level 0 of every frame f of the set: the image and its REFLECT_101 border.
__global__ __launch_bounds__(kKltBlock) void ps_klt_level0(const uint8_t *__restrict__ src, size_t rowStride, size_t frameStride,
                                                           KltLevel lv, int cn, int W, uint8_t *__restrict__ img, size_t slotElems,
                                                           int firstSlot)
{
    const int idx = (int)(blockIdx.x * kKltBlock + threadIdx.x), f = (int)blockIdx.y;
    if (idx >= lv.total) return;
    const int c = idx % cn, t = idx / cn, pcols = lv.cols + 2 * W;
    const int sx = klt_reflect(t % pcols - W, lv.cols), sy = klt_reflect(t / pcols - W, lv.rows);
    img[(size_t)(firstSlot + f) * slotElems + lv.off + idx] = src[(size_t)f * frameStride + (size_t)sy * rowStride + sx * cn + c];
}

// Level l+1 from the stored level l (whose border supplies REFLECT_101 to the 5x5 taps); border elements of the new level
// repeat the sum of the pixel they reflect.
__global__ __launch_bounds__(kKltBlock) void ps_klt_pyrdown(uint8_t *__restrict__ img, size_t slotElems, int firstSlot, KltLevel src,
                                                            KltLevel dst, int cn, int W)
{
    const int idx = (int)(blockIdx.x * kKltBlock + threadIdx.x), f = (int)blockIdx.y;
    if (idx >= dst.total) return;
    const int c = idx % cn, t = idx / cn, pcols = dst.cols + 2 * W;
    const int x = klt_reflect(t % pcols - W, dst.cols), y = klt_reflect(t / pcols - W, dst.rows);
    uint8_t *slot = img + (size_t)(firstSlot + f) * slotElems;
    const uint8_t *s = slot + src.off + (size_t)(2 * y - 2 + W) * src.estride + (2 * x - 2 + W) * cn + c;
    int sum = 0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const int ky = dy == 0 || dy == 4 ? 1 : (dy == 2 ? 6 : 4);
        const uint8_t *r = s + (size_t)dy * src.estride;
        sum += ky * ((int)r[0] + 4 * (int)r[cn] + 6 * (int)r[2 * cn] + 4 * (int)r[3 * cn] + (int)r[4 * cn]);
    }
    slot[dst.off + idx] = (uint8_t)((sum + 128) >> 8);
}

// Scharr derivatives of a stored level: [-3 0 3; -10 0 10; -3 0 3] and its transpose inside the image, 0 in the border.
__global__ __launch_bounds__(kKltBlock) void ps_klt_scharr(const uint8_t *__restrict__ img, uint32_t *__restrict__ der, size_t slotElems,
                                                           int firstSlot, KltLevel lv, int cn, int W)
{
    const int idx = (int)(blockIdx.x * kKltBlock + threadIdx.x), f = (int)blockIdx.y;
    if (idx >= lv.total) return;
    const int t = idx / cn, pcols = lv.cols + 2 * W;
    const int x = t % pcols - W, y = t / pcols - W;
    uint32_t out = 0;
    if (x >= 0 && x < lv.cols && y >= 0 && y < lv.rows) {
        const uint8_t *p = img + (size_t)(firstSlot + f) * slotElems + lv.off + idx;
        const int es = lv.estride;
        const int a00 = p[-es - cn], a01 = p[-es], a02 = p[-es + cn], a10 = p[-cn], a12 = p[cn], a20 = p[es - cn], a21 = p[es],
                  a22 = p[es + cn];
        const int ix = 3 * (a02 - a00) + 10 * (a12 - a10) + 3 * (a22 - a20);
        const int iy = 3 * (a20 - a00) + 10 * (a21 - a01) + 3 * (a22 - a02);
        out = ((uint32_t)ix & 0xFFFFu) | ((uint32_t)iy << 16);
    }
    der[(size_t)(firstSlot + f) * slotElems + lv.off + idx] = out;
}

struct KltTrackArgs {
    const uint8_t *img;
    const uint32_t *der;
    const KltLevel *levels; // device copy of the level table
    unsigned long long slotElems;
    double eps2, minEig;
    const int32_t *pairs;
    const float2 *prevPts;
    const int32_t *counts;
    float2 *nextPts;
    uint8_t *status;
    float *err;
    int L, cn, W, slots, maxCount, flags, cap;
    int wn, wn4, waveBytes; // window elements, rounded up to 4, LDS bytes of one wave
    float errScale;         // 1.f / (32 W cn W)
};

// the bounds test of lkpyramid.cpp, taken on the floats: NaN, +-inf and anything beyond the int range are outside
PS_D bool klt_inside(float fx, float fy, int W, int cols, int rows)
{
    return fx >= (float)(-W) && fx < (float)cols && fy >= (float)(-W) && fy < (float)rows;
}

struct KltWeights {
    int w00, w01, w10, w11;
};
PS_D KltWeights klt_weights(float a, float b)
{
    KltWeights k;
    k.w00 = (int)ps_rint((1.f - a) * (1.f - b) * 16384.f);
    k.w01 = (int)ps_rint(a * (1.f - b) * 16384.f);
    k.w10 = (int)ps_rint((1.f - a) * b * 16384.f);
    k.w11 = 16384 - k.w00 - k.w01 - k.w10;
    return k;
}

// LDS traffic of one wave is ordered by the hardware; this keeps the compiler from moving accesses across the hand-over
PS_D void klt_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lanes 0 .. nsum-1: the float sum of products row `lane`, one element at a time in window order (the rows are padded with
// zeros to a multiple of four; x + 0 = x, and no product is ever -0)
PS_D float klt_lane_sum(const float *prod, int wn4, int lane, int nsum)
{
    float s = 0.f;
    if (lane < nsum) {
        const float4 *q = reinterpret_cast<const float4 *>(prod + lane * wn4);
        for (int k = 0; k < wn4 / 4; ++k) {
            const float4 v = q[k];
            s += v.x;
            s += v.y;
            s += v.z;
            s += v.w;
        }
    }
    return s;
}
PS_D float klt_from_lane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// DESCALE(bilinear of four bytes, 9)
PS_D int klt_sample(const uint8_t *__restrict__ p, int es, int cn, const KltWeights &k)
{
    const int v = (int)p[0] * k.w00 + (int)p[cn] * k.w01 + (int)p[es] * k.w10 + (int)p[es + cn] * k.w11;
    return (v + 256) >> 9;
}

// One wavefront per (pair, point); work-groups of blockDim.x / 64 independent waves, dynamic LDS of waveBytes each.
__global__ __launch_bounds__(kKltBlock) void ps_klt_track(KltTrackArgs a)
{
    extern __shared__ __align__(16) unsigned char kltLds[];
    const int lane = (int)threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)blockDim.x >> 6, bpp = (a.cap + waves - 1) / waves;
    const int p = (int)blockIdx.x / bpp, i = ((int)blockIdx.x % bpp) * waves + w;
    const int n = a.counts[p];
    if (n < 0 || n > a.cap || i >= n) return;
    const size_t o = (size_t)p * a.cap + i;
    const int s0 = a.pairs[2 * p], s1 = a.pairs[2 * p + 1];
    if ((unsigned)s0 >= (unsigned)a.slots || (unsigned)s1 >= (unsigned)a.slots) { // a pair that names no slot: its points fail
        if (lane == 0) {
            a.status[o] = 0;
            a.err[o] = 0.f;
        }
        return;
    }
    const int W = a.W, cn = a.cn, wn = a.wn, wn4 = a.wn4;
    float *prod = reinterpret_cast<float *>(kltLds + (size_t)w * a.waveBytes); // [3][wn4]
    short *sI = reinterpret_cast<short *>(prod + 3 * wn4), *sIx = sI + wn4, *sIy = sIx + wn4;
    if (lane < wn4 - wn) prod[wn + lane] = prod[wn4 + wn + lane] = prod[2 * wn4 + wn + lane] = 0.f;

    const float2 pp = a.prevPts[o];
    float npx = 0.f, npy = 0.f;
    if (a.flags & PS_KLT_USE_INITIAL_FLOW) {
        const float2 q = a.nextPts[o];
        npx = q.x;
        npy = q.y;
    }
    const float half = (float)(W - 1) * 0.5f, kScale = 1.f / (float)(1 << 20);
    const int Wcn = W * cn, qstep = 64 / Wcn, rstep = 64 % Wcn, y0 = lane / Wcn, x0 = lane % Wcn;
    const uint8_t *img0 = a.img + (size_t)s0 * a.slotElems, *img1 = a.img + (size_t)s1 * a.slotElems;
    const uint32_t *der0 = a.der + (size_t)s0 * a.slotElems;
    int status = 1;
    float err = 0.f;

    for (int level = a.L; level >= 0; --level) {
        const KltLevel lv = a.levels[level];
        const int es = lv.estride;
        const float sc = 1.f / (float)(1 << level);
        float px = pp.x * sc, py = pp.y * sc, nx, ny;
        if (level == a.L) {
            if (a.flags & PS_KLT_USE_INITIAL_FLOW) {
                nx = npx * sc;
                ny = npy * sc;
            } else {
                nx = px;
                ny = py;
            }
        } else {
            nx = npx * 2.f;
            ny = npy * 2.f;
        }
        npx = nx;
        npy = ny;
        px -= half;
        py -= half;
        float fx = floorf(px), fy = floorf(py);
        if (!klt_inside(fx, fy, W, lv.cols, lv.rows)) {
            if (level == 0) {
                status = 0;
                err = 0.f;
            }
            continue;
        }
        KltWeights k = klt_weights(px - fx, py - fy);
        {
            const size_t at = lv.off + (size_t)((int)fy + W) * es + ((int)fx + W) * cn;
            const uint8_t *pim = img0 + at;
            const uint32_t *pde = der0 + at;
            for (int e = lane, y = y0, x = x0; e < wn; e += 64) {
                const int off = y * es + x;
                const int I = klt_sample(pim + off, es, cn, k);
                const uint32_t d00 = pde[off], d01 = pde[off + cn], d10 = pde[off + es], d11 = pde[off + es + cn];
                const int vx = (int)(short)(d00 & 0xFFFFu) * k.w00 + (int)(short)(d01 & 0xFFFFu) * k.w01 +
                               (int)(short)(d10 & 0xFFFFu) * k.w10 + (int)(short)(d11 & 0xFFFFu) * k.w11;
                const int vy = ((int)d00 >> 16) * k.w00 + ((int)d01 >> 16) * k.w01 + ((int)d10 >> 16) * k.w10 + ((int)d11 >> 16) * k.w11;
                const int ix = (vx + 8192) >> 14, iy = (vy + 8192) >> 14;
                sI[e] = (short)I;
                sIx[e] = (short)ix;
                sIy[e] = (short)iy;
                prod[e] = (float)(ix * ix);
                prod[wn4 + e] = (float)(ix * iy);
                prod[2 * wn4 + e] = (float)(iy * iy);
                x += rstep;
                y += qstep;
                if (x >= Wcn) {
                    x -= Wcn;
                    ++y;
                }
            }
        }
        klt_wave_sync();
        const float sA = klt_lane_sum(prod, wn4, lane, 3);
        const float A11 = klt_from_lane(sA, 0) * kScale, A12 = klt_from_lane(sA, 1) * kScale, A22 = klt_from_lane(sA, 2) * kScale;
        klt_wave_sync();
        float D = A11 * A22 - A12 * A12;
        const float dd = A11 - A22;
        const float minEig = ps_div((A22 + A11) - ps_sqrt(dd * dd + 4.f * A12 * A12), (float)(2 * W * W));
        if (a.flags & PS_KLT_GET_MIN_EIGENVALS) err = minEig;
        if ((double)minEig < a.minEig || D < FLT_EPSILON) {
            if (level == 0) status = 0;
            continue;
        }
        D = ps_div(1.f, D);
        nx -= half;
        ny -= half;
        const uint8_t *lvl1 = img1 + lv.off;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.maxCount; ++j) {
            fx = floorf(nx);
            fy = floorf(ny);
            if (!klt_inside(fx, fy, W, lv.cols, lv.rows)) {
                if (level == 0) status = 0;
                break;
            }
            k = klt_weights(nx - fx, ny - fy);
            const uint8_t *pj = lvl1 + (size_t)((int)fy + W) * es + ((int)fx + W) * cn;
            for (int e = lane, y = y0, x = x0; e < wn; e += 64) {
                const int diff = klt_sample(pj + (y * es + x), es, cn, k) - (int)sI[e];
                prod[e] = (float)(diff * (int)sIx[e]);
                prod[wn4 + e] = (float)(diff * (int)sIy[e]);
                x += rstep;
                y += qstep;
                if (x >= Wcn) {
                    x -= Wcn;
                    ++y;
                }
            }
            klt_wave_sync();
            const float sB = klt_lane_sum(prod, wn4, lane, 2);
            const float b1 = klt_from_lane(sB, 0) * kScale, b2 = klt_from_lane(sB, 1) * kScale;
            klt_wave_sync();
            const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
            nx += dx;
            ny += dy;
            npx = nx + half;
            npy = ny + half;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= a.eps2) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                npx -= dx * 0.5f;
                npy -= dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
        if (level == 0 && status && !(a.flags & PS_KLT_GET_MIN_EIGENVALS)) {
            const float qx = npx - half, qy = npy - half;
            fx = floorf(qx);
            fy = floorf(qy);
            if (!klt_inside(fx, fy, W, lv.cols, lv.rows)) {
                status = 0;
                continue;
            }
            k = klt_weights(qx - fx, qy - fy);
            const uint8_t *pj = lvl1 + (size_t)((int)fy + W) * es + ((int)fx + W) * cn;
            for (int e = lane, y = y0, x = x0; e < wn; e += 64) {
                const int diff = klt_sample(pj + (y * es + x), es, cn, k) - (int)sI[e];
                prod[e] = fabsf((float)diff);
                x += rstep;
                y += qstep;
                if (x >= Wcn) {
                    x -= Wcn;
                    ++y;
                }
            }
            klt_wave_sync();
            const float sE = klt_lane_sum(prod, wn4, lane, 1);
            err = klt_from_lane(sE, 0) * a.errScale;
            klt_wave_sync();
        }
    }
    if (lane == 0) {
        a.nextPts[o] = make_float2(npx, npy);
        a.status[o] = (uint8_t)status;
        a.err[o] = err;
    }
}

// performTracking's selection (matcherOpenCV.cpp:247-290), one work-group per pair.  The i < j sweep marks i if err[i] > err[j],
// else j, for every near pair: a union, so point k goes iff some near m has (k < m and err[k] > err[m]) or (m < k and not
// err[m] > err[k]).  near: sqrt((double)dx*dx + (double)dy*dy) < d, decided as sum < bound (ps_sqrt_bound_f64: the same
// decision for every input, a NaN is never near).  Survivors: status != 0, err not above the threshold, unmarked; index order.
__global__ __launch_bounds__(kKltSelBlock) void ps_klt_select(const float2 *__restrict__ pts, const uint8_t *__restrict__ status,
                                                              const float *__restrict__ err, const int32_t *__restrict__ counts, int cap,
                                                              double errThr, double bound, PsDMatch *__restrict__ matches,
                                                              int32_t *__restrict__ numMatches, float2 *__restrict__ keptPts,
                                                              int32_t *__restrict__ keptIdx)
{
    __shared__ float tx[kKltSelBlock], ty[kKltSelBlock], te[kKltSelBlock];
    __shared__ int wcnt[kKltSelWaves];
    const int p = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = counts[p];
    if (n < 0 || n > cap) {
        if (tid == 0) numMatches[p] = -1;
        return;
    }
    const size_t base = (size_t)p * cap;
    int kept = 0;
    for (int c0 = 0; c0 < n; c0 += kKltSelBlock) {
        const int k = c0 + tid;
        const bool valid = k < n;
        const float2 pk = pts[base + (valid ? k : 0)];
        const float ek = err[base + (valid ? k : 0)];
        bool marked = false;
        for (int t0 = 0; t0 < n; t0 += kKltSelBlock) {
            __syncthreads();
            if (t0 + tid < n) {
                const float2 q = pts[base + t0 + tid];
                tx[tid] = q.x;
                ty[tid] = q.y;
                te[tid] = err[base + t0 + tid];
            }
            __syncthreads();
            const int lim = n - t0 < kKltSelBlock ? n - t0 : kKltSelBlock;
            if (valid)
                for (int mm = 0; mm < lim; ++mm) {
                    const int m = t0 + mm;
                    const float dx = pk.x - tx[mm], dy = pk.y - ty[mm], em = te[mm];
                    const double s = (double)dx * (double)dx + (double)dy * (double)dy;
                    const bool goes = k < m ? ek > em : (m < k && !(em > ek));
                    marked = marked || (s < bound && goes);
                }
        }
        const bool keep = valid && status[base + (valid ? k : 0)] != 0 && !((double)ek > errThr) && !marked;
        const unsigned long long bk = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(bk);
        __syncthreads();
        int before = 0, total = 0;
        for (int v = 0; v < kKltSelWaves; ++v) {
            const int c = wcnt[v];
            before += v < w ? c : 0;
            total += c;
        }
        if (keep) {
            const int j = kept + before + __popcll(bk & ((1ull << lane) - 1ull));
            PsDMatch m;
            m.queryIdx = k;
            m.trainIdx = j;
            m.imgIdx = 0;
            m.distance = 0.f;
            matches[base + j] = m;
            keptPts[base + j] = pk;
            keptIdx[base + j] = k;
        }
        kept += total;
        __syncthreads();
    }
    if (tid == 0) numMatches[p] = kept;
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the pyramid set, the launches and the entry points
struct PsKltPyramids {
    int device = 0;
    int rows = 0, cols = 0, cn = 0, W = 0, L = 0, slots = 0;
    psdev::KltLevel lv[psdev::kKltLevels];
    size_t slotElems = 0; // elements of one slot: bytes of its images, packed pairs of its derivatives
    uint8_t *img = nullptr;
    uint32_t *der = nullptr;
    psdev::KltLevel *dLevels = nullptr;
};

namespace {

struct KltClamped {
    int maxCount;
    double eps2;
};
// cv::calcOpticalFlowPyrLK's own clamps: maxCount to 0 .. 100, epsilon to 0 .. 10, then squared (double)
KltClamped klt_clamp(const PsKltParams &p)
{
    KltClamped c;
    c.maxCount = p.maxCount < 0 ? 0 : (p.maxCount > 100 ? 100 : p.maxCount);
    const double e = !(p.eps > 0.0) ? 0.0 : (p.eps > 10.0 ? 10.0 : p.eps);
    c.eps2 = e * e;
    return c;
}

const char *klt_params_error(const PsKltParams *p)
{
    if (!p) return "null PsKltParams";
    if (p->winSize < 3 || p->winSize > 31) return "PsKltParams: winSize must lie in 3 .. 31";
    if (p->maxLevels < 0 || p->maxLevels > 7) return "PsKltParams: maxLevels must lie in 0 .. 7";
    if (p->flags & ~(PS_KLT_USE_INITIAL_FLOW | PS_KLT_GET_MIN_EIGENVALS)) return "PsKltParams: unknown flag";
    return nullptr;
}

int klt_shape_error(PsContext *ctx, int rows, int cols, int channels, int winSize, int maxLevels, const char *who)
{
    if (winSize < 3 || winSize > 31 || maxLevels < 0 || maxLevels > 7 || (channels != 1 && channels != 3))
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": winSize 3 .. 31, maxLevels 0 .. 7, channels 1 or 3").c_str());
    if (rows <= winSize || cols <= winSize)
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": the image must be larger than the window in both directions").c_str());
    return image_shape_error(ctx, rows, cols, channels, who); // (after the window rules: only its size limit is left to break)
}

int klt_build_launch(PsContext *ctx, PsKltPyramids *pyr, const uint8_t *pixels, size_t rowStride, size_t frameStride, int frames,
                     int firstSlot)
{
    const int W = pyr->W, cn = pyr->cn;
    const auto grid = [&](const KltLevel &l) { return dim3((unsigned)((l.total + kKltBlock - 1) / kKltBlock), (unsigned)frames); };
    hipLaunchKernelGGL(ps_klt_level0, grid(pyr->lv[0]), dim3(kKltBlock), 0, ctx->stream, pixels, rowStride, frameStride, pyr->lv[0], cn, W,
                       pyr->img, pyr->slotElems, firstSlot);
    PS_HIP(hipGetLastError());
    for (int l = 0; l <= pyr->L; ++l) {
        if (l > 0) {
            hipLaunchKernelGGL(ps_klt_pyrdown, grid(pyr->lv[l]), dim3(kKltBlock), 0, ctx->stream, pyr->img, pyr->slotElems, firstSlot,
                               pyr->lv[l - 1], pyr->lv[l], cn, W);
            PS_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(ps_klt_scharr, grid(pyr->lv[l]), dim3(kKltBlock), 0, ctx->stream, (const uint8_t *)pyr->img, pyr->der,
                           pyr->slotElems, firstSlot, pyr->lv[l], cn, W);
        PS_HIP(hipGetLastError());
    }
    return PS_OK;
}

int klt_track_launch(PsContext *ctx, const PsKltPyramids *pyr, const PsKltParams &prm, const int32_t *pairs, const float *prevPts,
                     const int32_t *counts, int P, int cap, float *nextPts, uint8_t *status, float *err)
{
    const KltClamped c = klt_clamp(prm);
    KltTrackArgs a;
    a.img = pyr->img;
    a.der = pyr->der;
    a.levels = pyr->dLevels;
    a.slotElems = pyr->slotElems;
    a.eps2 = c.eps2;
    a.minEig = prm.minEigThreshold;
    a.pairs = pairs;
    a.prevPts = reinterpret_cast<const float2 *>(prevPts);
    a.counts = counts;
    a.nextPts = reinterpret_cast<float2 *>(nextPts);
    a.status = status;
    a.err = err;
    a.L = pyr->L;
    a.cn = pyr->cn;
    a.W = pyr->W;
    a.slots = pyr->slots;
    a.maxCount = c.maxCount;
    a.flags = prm.flags;
    a.cap = cap;
    a.wn = pyr->W * pyr->W * pyr->cn;
    a.wn4 = (a.wn + 3) & ~3;
    a.waveBytes = (18 * a.wn4 + 15) & ~15; // three float rows of products, three int16 windows
    a.errScale = 1.f / (float)(32 * pyr->W * pyr->cn * pyr->W);
    // waves of a work-group share nothing: as many as 64 KiB of LDS hold, four at most
    int waves = 65536 / a.waveBytes;
    waves = waves > kKltBlock / 64 ? kKltBlock / 64 : waves;
    const long long blocks = (long long)P * ((cap + waves - 1) / waves);
    if (blocks > INT_MAX) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_klt_track_device: pairs x capacity beyond 2^31 work-groups");
    hipLaunchKernelGGL(ps_klt_track, dim3((unsigned)blocks), dim3((unsigned)waves * 64), (size_t)waves * a.waveBytes, ctx->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

int klt_select_launch(PsContext *ctx, const float *pts, const uint8_t *status, const float *err, const int32_t *counts, int P, int cap,
                      double errThr, double minDist, PsDMatch *matches, int32_t *numMatches, float *keptPts, int32_t *keptIdx)
{
    hipLaunchKernelGGL(ps_klt_select, dim3((unsigned)P), dim3(kKltSelBlock), 0, ctx->stream, reinterpret_cast<const float2 *>(pts), status,
                       err, counts, cap, errThr, sqrt_bound_f64(minDist), matches, numMatches, reinterpret_cast<float2 *>(keptPts), keptIdx);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// The host forms: one pair, uploads included, synchronous.  select = false: calcOpticalFlowPyrLK alone.
int klt_host_pair(PsContext *ctx, const char *who, const uint8_t *prevImg, const uint8_t *nextImg, int rows, int cols, int channels,
                  size_t rowStride, const float *prevPts, float *nextPts, int n, uint8_t *status, float *err, const PsKltParams *prm,
                  bool select, double errThr, double minDist, PsDMatch *matches, int *numMatches, float *keptPts, int32_t *keptIdx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (const char *why = klt_params_error(prm)) return fail(ctx, PS_ERR_BAD_ARG, why);
    rc = klt_shape_error(ctx, rows, cols, channels, prm->winSize, prm->maxLevels, who);
    if (rc) return rc;
    rowStride = image_row_stride(cols, channels, rowStride);
    if (!prevImg || !nextImg || rowStride == 0 || n < 0 || (select && !numMatches) ||
        (n > 0 && (!prevPts || !nextPts || (!select && (!status || !err)) || (select && (!matches || !keptPts || !keptIdx)))))
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null array, negative count or a row stride below a row").c_str());
    if (select && n > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, (std::string(who) + ": more than PS_MAX_KPTS points").c_str());
    if (select) *numMatches = 0;
    if (n == 0) return PS_OK;
    TimingOff toff(ctx);
    PsKltPyramids *pyr = nullptr;
    rc = ps_klt_pyramids_create(ctx, rows, cols, channels, prm->winSize, prm->maxLevels, 2, &pyr);
    if (rc) return rc;
    const HandleOwner<PsKltPyramids> own(pyr, ps_klt_pyramids_destroy);
    const size_t imgBytes = image_bytes(rows, cols, channels, rowStride), N = (size_t)n;
    // one block: two images | pairs[2], count, 0 | prevPts | nextPts | err | numMatches | matches | keptPts | keptIdx | status
    static_assert(alignof(float2) == 8 && alignof(PsDMatch) == 4, "the layout aligns every array to its element type");
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes, 16); // (the previous image, at 0)
    const size_t oImg1 = lay.take<uint8_t>(imgBytes, 16), oPairs = lay.take<int32_t>(4, 16), oCount = oPairs + 8, oPrev = lay.take<float2>(N),
                 oNext = lay.take<float2>(N), oErr = lay.take<float>(N), oNum = lay.take<int32_t>(1), oMatches = lay.take<PsDMatch>(N, 8),
                 oKeptPts = lay.take<float2>(N), oKeptIdx = lay.take<int32_t>(N), oStatus = lay.take<uint8_t>(N), total = lay.total;
    const DeviceBlock blk(total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    const int32_t head[4] = {0, 1, n, 0};
    PS_HIP(hipMemcpyAsync(d, prevImg, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oImg1, nextImg, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oPairs, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oPrev, prevPts, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (prm->flags & PS_KLT_USE_INITIAL_FLOW) PS_HIP(hipMemcpyAsync(d + oNext, nextPts, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (head[] and pageable sources leave scope / may change)
    rc = klt_build_launch(ctx, pyr, (const uint8_t *)d, rowStride, oImg1, 2, 0);
    if (rc) return rc;
    rc = klt_track_launch(ctx, pyr, *prm, (const int32_t *)(d + oPairs), (const float *)(d + oPrev), (const int32_t *)(d + oCount), 1, n,
                          (float *)(d + oNext), (uint8_t *)(d + oStatus), (float *)(d + oErr));
    if (rc) return rc;
    if (select) {
        rc = klt_select_launch(ctx, (const float *)(d + oNext), (const uint8_t *)(d + oStatus), (const float *)(d + oErr),
                               (const int32_t *)(d + oCount), 1, n, errThr, minDist, (PsDMatch *)(d + oMatches), (int32_t *)(d + oNum),
                               (float *)(d + oKeptPts), (int32_t *)(d + oKeptIdx));
        if (rc) return rc;
    }
    std::vector<char> back(total - oNext);
    PS_HIP(hipMemcpyAsync(back.data(), d + oNext, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const char *b = back.data() - oNext;
    std::memcpy(nextPts, b + oNext, (size_t)n * 8);
    if (status) std::memcpy(status, b + oStatus, (size_t)n);
    if (err) std::memcpy(err, b + oErr, (size_t)n * 4);
    if (select) {
        int32_t nk = 0;
        std::memcpy(&nk, b + oNum, 4);
        if (nk < 0 || nk > n) return fail(ctx, PS_ERR_HIP, (std::string(who) + ": the device returned an impossible count").c_str());
        std::memcpy(matches, b + oMatches, (size_t)nk * 16);
        std::memcpy(keptPts, b + oKeptPts, (size_t)nk * 8);
        std::memcpy(keptIdx, b + oKeptIdx, (size_t)nk * 4);
        *numMatches = nk;
    }
    return PS_OK;
}
} // namespace

static void klt_kernel_attributes()
{
    // the largest window (31 x 31 x 3) keeps 51 KiB a wave
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ps_klt_track), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
}

extern "C" {

size_t ps_abi_sizeof_klt_params(void) { return sizeof(PsKltParams); }
size_t ps_abi_sizeof_image_set(void) { return sizeof(PsImageSet); }

int ps_klt_pyramids_create(PsContext *ctx, int rows, int cols, int channels, int winSize, int maxLevels, int slots, PsKltPyramids **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_klt_pyramids_create: null out");
    *out = nullptr;
    rc = klt_shape_error(ctx, rows, cols, channels, winSize, maxLevels, "ps_klt_pyramids_create");
    if (rc) return rc;
    if (slots < 1 || slots > kImageMaxFrames) return fail(ctx, PS_ERR_BAD_ARG, "ps_klt_pyramids_create: slots must lie in 1 .. 65535");
    HandleOwner<PsKltPyramids> own(new PsKltPyramids, ps_klt_pyramids_destroy);
    PsKltPyramids *p = own.get();
    p->device = ctx->device;
    p->rows = rows;
    p->cols = cols;
    p->cn = channels;
    p->W = winSize;
    p->slots = slots;
    unsigned long long off = 0;
    int r = rows, c = cols;
    for (int l = 0;; ++l) {
        KltLevel &lv = p->lv[l];
        lv.rows = r;
        lv.cols = c;
        lv.estride = (c + 2 * winSize) * channels;
        lv.total = (r + 2 * winSize) * lv.estride;
        lv.off = off;
        off += ((unsigned long long)lv.total + 15ull) & ~15ull;
        p->L = l;
        r = (r + 1) / 2;
        c = (c + 1) / 2;
        if (l == maxLevels || r <= winSize || c <= winSize) break; // building stops before a level no larger than the window
    }
    p->slotElems = (size_t)off;
    hipError_t e = hipMalloc((void **)&p->img, p->slotElems * (size_t)slots);
    if (e == hipSuccess) e = hipMalloc((void **)&p->der, p->slotElems * (size_t)slots * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&p->dLevels, sizeof(p->lv));
    if (e == hipSuccess) e = hipMemcpy(p->dLevels, p->lv, sizeof(KltLevel) * (size_t)(p->L + 1), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_klt_pyramids_create: hipMalloc", e);
    *out = own.release();
    return PS_OK;
}

void ps_klt_pyramids_destroy(PsKltPyramids *pyr)
{
    if (!pyr) return;
    (void)hipSetDevice(pyr->device);
    if (pyr->img) (void)hipFree(pyr->img); // (hipFree waits for the device: queued work that reads the set has finished)
    if (pyr->der) (void)hipFree(pyr->der);
    if (pyr->dLevels) (void)hipFree(pyr->dLevels);
    delete pyr;
}

int ps_klt_pyramids_num_levels(const PsKltPyramids *pyr) { return pyr ? pyr->L + 1 : -1; }

int ps_klt_pyramids_build_device(PsContext *ctx, PsKltPyramids *pyr, const PsImageSet *images, int firstSlot)
{
    int rc = bind(ctx);
    if (rc) return rc;
    size_t row = 0, frame = 0;
    rc = check_image_set(ctx, pyr, &PsKltPyramids::slots, images, firstSlot, "ps_klt_pyramids_build_device", row, frame);
    if (rc) return rc;
    if (images->numFrames == 0) return PS_OK;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return klt_build_launch(ctx, pyr, images->pixels, row, frame, images->numFrames, firstSlot);
}

int ps_klt_track_device(PsContext *ctx, const PsKltPyramids *pyr, const PsKltParams *params, const int32_t *pairs, const float *prevPts,
                        const int32_t *counts, int P, int capacity, float *nextPts, uint8_t *status, float *err)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (const char *why = klt_params_error(params)) return fail(ctx, PS_ERR_BAD_ARG, why);
    if (!pyr || pyr->device != ctx->device || params->winSize != pyr->W || P < 0)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_klt_track_device: null or foreign pyramid set, a winSize other than the set's, or P < 0");
    if (P == 0) return PS_OK;
    if (capacity < 1 || !pairs || !prevPts || !counts || !nextPts || !status || !err)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_klt_track_device: null array or capacity < 1");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return klt_track_launch(ctx, pyr, *params, pairs, prevPts, counts, P, capacity, nextPts, status, err);
}

int ps_klt_select_device(PsContext *ctx, const float *nextPts, const uint8_t *status, const float *err, const int32_t *counts, int P,
                         int capacity, double trackingErrorThreshold, double minimalReprojDistance, PsDMatch *matches,
                         int32_t *numMatches, float *keptPts, int32_t *keptIdx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (P < 0) return fail(ctx, PS_ERR_BAD_ARG, "ps_klt_select_device: P < 0");
    if (P == 0) return PS_OK;
    if (capacity < 1 || !nextPts || !status || !err || !counts || !matches || !numMatches || !keptPts || !keptIdx)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_klt_select_device: null array or capacity < 1");
    if (capacity > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_klt_select_device: capacity above PS_MAX_KPTS");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return klt_select_launch(ctx, nextPts, status, err, counts, P, capacity, trackingErrorThreshold, minimalReprojDistance, matches,
                             numMatches, keptPts, keptIdx);
}

int ps_calc_optical_flow_pyr_lk(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, int rows, int cols, int channels,
                                size_t rowStride, const float *prevPts, float *nextPts, int n, uint8_t *status, float *err,
                                const PsKltParams *params)
{
    return klt_host_pair(ctx, "ps_calc_optical_flow_pyr_lk", prevImg, nextImg, rows, cols, channels, rowStride, prevPts, nextPts, n,
                         status, err, params, false, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr);
}

int ps_perform_tracking(PsContext *ctx, const uint8_t *prevImg, const uint8_t *nextImg, int rows, int cols, int channels, size_t rowStride,
                        const float *prevPts, float *nextPts, int n, const PsKltParams *params, double trackingErrorThreshold,
                        double minimalReprojDistance, uint8_t *status, float *err, PsDMatch *matches, int *numMatches, float *keptPts,
                        int32_t *keptIdx)
{
    return klt_host_pair(ctx, "ps_perform_tracking", prevImg, nextImg, rows, cols, channels, rowStride, prevPts, nextPts, n, status, err,
                         params, true, trackingErrorThreshold, minimalReprojDistance, matches, numMatches, keptPts, keptIdx);
}

int ps_debug_klt_level(PsContext *ctx, const PsKltPyramids *pyr, int slot, int level, int32_t *dims4, uint8_t *img, int16_t *der)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!pyr || pyr->device != ctx->device || slot < 0 || slot >= pyr->slots || level < 0 || level > pyr->L)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_debug_klt_level: null or foreign set, or no such slot / level");
    const KltLevel &lv = pyr->lv[level];
    if (dims4) {
        dims4[0] = lv.rows;
        dims4[1] = lv.cols;
        dims4[2] = lv.rows + 2 * pyr->W;
        dims4[3] = lv.cols + 2 * pyr->W;
    }
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const size_t at = (size_t)slot * pyr->slotElems + lv.off;
    if (img) PS_HIP(hipMemcpy(img, pyr->img + at, (size_t)lv.total, hipMemcpyDeviceToHost));
    if (der) PS_HIP(hipMemcpy(der, pyr->der + at, (size_t)lv.total * 4, hipMemcpyDeviceToHost));
    return PS_OK;
}

} // extern "C"
