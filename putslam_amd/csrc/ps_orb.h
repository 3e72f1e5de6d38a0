// ps_orb.h -- MatcherOpenCV::describeFeatures (reference src/Matcher/matcherOpenCV.cpp:183-195) for descriptor = "ORB":
// descriptorExtractor->compute(rgbImage, features, descriptors) with cv::ORB::create(), the last per-frame step of
// Matcher::detectInitFeatures (matcher.cpp:36), Matcher::match (:467) and Matcher::trackKLT (:338).
//
// The arithmetic is the project's reading of OpenCV 3.0 - 3.3's ORB_Impl::detectAndCompute with useProvidedKeypoints = true, of the
// 8-bit resize(INTER_LINEAR), the 8-bit separable GaussianBlur and cvtColor (restated twice in
// tests/orb_ref.py, which the kernels are held to byte for byte).  No OpenCV was at hand: the reading is UNPINNED.  The sampling
// pattern is DATA: 256 x (x0, y0, x1, y1) int8 in -15 .. 15, the host's or the documented default (ps_orb_pattern_default).
// Everything but the rotation is integer arithmetic; cvRound rounds half to even:
//  * grey: one channel as it is; three: COLOR_BGR2GRAY, (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14;
//  * levels: scale_l = (float)pow((double)scaleFactor, l), rows_l = cvRound((float)rows / scale_l), level l resized from l - 1;
//  * resize: 11-bit coefficients (orb_coeffs below), h = S[s] * a0 + S[s + 1] * a1,
//    out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
//  * blur: taps {18, 34, 49, 55, 49, 34, 18} (sum 257), rows then columns in int, min(255, (v + 32768) >> 16), REFLECT_101 of the
//    unblurred level in borderInterpolate's form;
//  * kept: 31 <= x < cols - 31, 31 <= y < rows - 31 (float compares), 0 <= octave < nLevels; grouped by octave ascending, input
//    order inside an octave;
//  * row: s = 1.f / scale, centre (cvRound(x * s), cvRound(y * s)), (a, b) = orb_rotation(angle), ix = cvRound(px * a - py * b),
//    iy = cvRound(px * b + py * a), bit p = v(point 0) < v(point 1); v reads the blurred level inside the level and the raw level
//    at the REFLECT_101 index outside it (OpenCV blurs a region of an atlas in place: the border around it stays unblurred);
//  * rotation: the project's own fixed float sequence (orb_rotation), no fused operation: the library is built with
//    -ffp-contract=off.
//
// Shape: ps_orb_level0 / ps_orb_resize, a thread per four pixels of a level over all frames; ps_orb_blur, a work-group per 32 x 32
// tile whose 38 x 38 reflected pixels (four a word) and 38 x 32 row sums lie in LDS, four pixels a thread in either direction;
// ps_orb_place, a work-group per frame, classifies the key points and orders them with ps_fast.h's fast_stable_take (key =
// octave): positions are sums of ballots and per-wave counts;
// ps_orb_describe, a wavefront per kept key point, lane n takes pairs n, 64 + n, 128 + n, 192 + n and four ballots are the row.
// The 512 samples of a row are read where they lie -- eight byte loads a lane -- not staged: staging the 45 x 45 neighbourhood
// is 32 loads a lane with the reflection and the raw / blurred choice on each.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ps_device_math.h"
#include "ps_fast.h" // fast_stable_take, its FastSortLds and kFastSelBlock: ps_orb_place orders the key points with them
#include "ps_glue.h"

namespace psdev {

constexpr int kOrbLevels = 8;    // most levels of a set
constexpr int kOrbEdge = 31;     // ORB's edgeThreshold
constexpr int kOrbBlock = 256;
constexpr int kOrbTile = 32;               // pixels of a blur tile's side
constexpr int kOrbHalo = kOrbTile + 6;     // the tile with its three-pixel ring
constexpr int kOrbTileWords = (kOrbHalo + 3) / 4; // 32-bit words of a tile row
constexpr int kOrbWavesPerBlock = kOrbBlock / 64;

struct OrbLevel {
    int rows, cols;
    unsigned plane;          // bytes reserved for one plane (rows x cols rounded up to 16)
    unsigned xtab, ytab;     // first entry of the level's column / row coefficients in the table (levels >= 1)
    unsigned long long off;  // the raw plane's offset inside a slot; the blurred plane follows it
    float scale, invScale;   // scale_l and 1.f / scale_l
};

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
PS_D int orb_reflect(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// (cos, sin) of `deg` degrees: the reduction to [-45, 45] and a quadrant is exact, the two polynomials are Taylor's with float
// coefficients, every operation rounds on its own.  tests/orb_ref.py rotation() is the same sequence.
PS_D void orb_rotation(float deg, float &a, float &b)
{
    if (!(fabsf(deg) <= 1048576.f)) deg = 0.f; // not finite, or beyond what reduces exactly: taken as 0
    const float q = rintf(deg * (float)(1.0 / 90.0));
    const float r = deg - q * 90.f;
    const int k = (int)q & 3;
    const float t = r * (float)(3.14159265358979323846 / 180.0);
    const float u = t * t;
    float s = (float)(1.0 / 362880);
    s = s * u + (float)(-1.0 / 5040);
    s = s * u + (float)(1.0 / 120);
    s = s * u + (float)(-1.0 / 6);
    s = s * (t * u) + t;
    float c = (float)(-1.0 / 3628800);
    c = c * u + (float)(1.0 / 40320);
    c = c * u + (float)(-1.0 / 720);
    c = c * u + (float)(1.0 / 24);
    c = c * u + -0.5f;
    c = c * u + 1.f;
    a = k == 0 ? c : (k == 1 ? -s : (k == 2 ? -c : s));
    b = k == 0 ? s : (k == 1 ? c : (k == 2 ? -s : -c));
}

// Where level 0 of a slot comes from: window q = slot % (gridRows * gridCols) of the grid of matcherOpenCV.cpp:133-146 over frame
// slot / (gridRows * gridCols) -- columns outer, rows inner, origin (k * cols / gridCols, i * rows / gridRows) -- and the weights
// of channels 0 and 2.  Description takes the whole image with COLOR_BGR2GRAY (channel 0 weighs 1868 here, 4899 in ps_fast.h's
// ps_fast_score -- intended); detection (ps_orb_detect.h) takes every ROI with CV_RGB2GRAY.
struct OrbWindow {
    int gridRows, gridCols, rows, cols; // the grid and the PARENT image's shape
    int w0, w2;
};
inline OrbWindow orb_whole_bgr(int rows, int cols) // (host)
{
    return OrbWindow{1, 1, rows, cols, 1868, 4899};
}

PS_D int orb_gray(const uint8_t *p, int cn, int w0, int w2)
{
    return cn == 1 ? (int)p[0] : ((int)p[0] * w0 + (int)p[1] * 9617 + (int)p[2] * w2 + 8192) >> 14;
}

// four pixels e .. e + 3 of a dense plane of n bytes: one word where all four exist (planes start 16-byte aligned)
PS_D void orb_store4(uint8_t *plane, unsigned e, unsigned n, const int v[4])
{
    if (e + 3 < n) {
        *reinterpret_cast<uint32_t *>(plane + e) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < n) plane[e + k] = (uint8_t)v[k];
    }
}

// Level 0 of slots firstSlot .. of the set: the grey image, four pixels a thread
__global__ __launch_bounds__(kOrbBlock) void ps_orb_level0(const uint8_t *__restrict__ src, size_t rowStride, size_t frameStride, int cn,
                                                           OrbWindow win, OrbLevel lv, uint8_t *__restrict__ planes, size_t slotBytes,
                                                           int firstSlot)
{
    const unsigned n = (unsigned)lv.rows * (unsigned)lv.cols, e = ((unsigned)blockIdx.x * kOrbBlock + threadIdx.x) * 4u;
    if (e >= n) return;
    const int f = (int)blockIdx.y; // the slot, counted from firstSlot
    const int cells = win.gridRows * win.gridCols, q = f % cells, wk = q / win.gridRows, wi = q - wk * win.gridRows;
    const uint8_t *img = src + (size_t)(f / cells) * frameStride + (size_t)(wi * win.rows / win.gridRows) * rowStride +
                         (size_t)(wk * win.cols / win.gridCols) * cn;
    int y = (int)(e / (unsigned)lv.cols), x = (int)(e - (unsigned)y * (unsigned)lv.cols);
    int v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e + k < n) v[k] = orb_gray(img + (size_t)y * rowStride + (size_t)x * cn, cn, win.w0, win.w2);
        if (++x == lv.cols) {
            x = 0;
            ++y;
        }
    }
    orb_store4(planes + (size_t)(firstSlot + f) * slotBytes + lv.off, e, n, v);
}

// Level d from level s = d - 1: an entry of the table holds the two source indices (low | high << 16) and their weights
__global__ __launch_bounds__(kOrbBlock) void ps_orb_resize(uint8_t *__restrict__ planes, size_t slotBytes, int firstSlot, OrbLevel s, OrbLevel d,
                                                           const uint2 *__restrict__ table)
{
    const unsigned n = (unsigned)d.rows * (unsigned)d.cols, e = ((unsigned)blockIdx.x * kOrbBlock + threadIdx.x) * 4u;
    if (e >= n) return;
    uint8_t *slot = planes + (size_t)(firstSlot + (int)blockIdx.y) * slotBytes;
    const uint8_t *S = slot + s.off;
    int y = (int)(e / (unsigned)d.cols), x = (int)(e - (unsigned)y * (unsigned)d.cols);
    int v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e + k < n) {
            const uint2 cx = table[d.xtab + x], cy = table[d.ytab + y];
            const int x0 = (int)(cx.x & 0xFFFFu), x1 = (int)(cx.x >> 16), a0 = (int)(cx.y & 0xFFFFu), a1 = (int)(cx.y >> 16);
            const int y0 = (int)(cy.x & 0xFFFFu), y1 = (int)(cy.x >> 16), b0 = (int)(cy.y & 0xFFFFu), b1 = (int)(cy.y >> 16);
            const uint8_t *r0 = S + (size_t)y0 * s.cols, *r1 = S + (size_t)y1 * s.cols;
            const int h0 = (int)r0[x0] * a0 + (int)r0[x1] * a1, h1 = (int)r1[x0] * a0 + (int)r1[x1] * a1;
            v[k] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
        if (++x == d.cols) {
            x = 0;
            ++y;
        }
    }
    orb_store4(slot + d.off, e, n, v);
}

// The blurred plane of one level: a work-group per 32 x 32 tile
__global__ __launch_bounds__(kOrbBlock) void ps_orb_blur(uint8_t *__restrict__ planes, size_t slotBytes, int firstSlot, OrbLevel lv)
{
    __shared__ uint32_t tile[kOrbHalo][kOrbTileWords];                      // the reflected bytes of a row, four a word
    __shared__ __attribute__((aligned(16))) uint32_t hsum[kOrbHalo][kOrbTile]; // the row sums, at most 257 * 255
    const int tid = (int)threadIdx.x, tx0 = (int)blockIdx.x * kOrbTile, ty0 = (int)blockIdx.y * kOrbTile;
    uint8_t *slot = planes + (size_t)(firstSlot + (int)blockIdx.z) * slotBytes;
    const uint8_t *raw = slot + lv.off;
    uint8_t *out = slot + lv.off + lv.plane;
    for (int e = tid; e < kOrbHalo * kOrbTileWords; e += kOrbBlock) {
        const int ly = e / kOrbTileWords, lw = e - ly * kOrbTileWords;
        // (a row or column beyond the level's last + 3 is never used: any index inside the level does)
        const uint8_t *row = raw + (size_t)orb_reflect(min(ty0 + ly - 3, lv.rows + 2), lv.rows) * lv.cols;
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) w |= (uint32_t)row[orb_reflect(min(tx0 + 4 * lw + k - 3, lv.cols + 2), lv.cols)] << (8 * k);
        tile[ly][lw] = w;
    }
    __syncthreads();
    for (int e = tid; e < kOrbHalo * (kOrbTile / 4); e += kOrbBlock) { // four adjacent row sums from twelve bytes
        const int ly = e / (kOrbTile / 4), q = e - ly * (kOrbTile / 4);
        const uint32_t w0 = tile[ly][q], w1 = tile[ly][q + 1], w2 = tile[ly][q + 2];
        int b[10];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = (int)((w0 >> (8 * k)) & 0xFFu);
            b[4 + k] = (int)((w1 >> (8 * k)) & 0xFFu);
        }
        b[8] = (int)(w2 & 0xFFu);
        b[9] = (int)((w2 >> 8) & 0xFFu);
        uint4 h;
        h.x = (uint32_t)(18 * (b[0] + b[6]) + 34 * (b[1] + b[5]) + 49 * (b[2] + b[4]) + 55 * b[3]);
        h.y = (uint32_t)(18 * (b[1] + b[7]) + 34 * (b[2] + b[6]) + 49 * (b[3] + b[5]) + 55 * b[4]);
        h.z = (uint32_t)(18 * (b[2] + b[8]) + 34 * (b[3] + b[7]) + 49 * (b[4] + b[6]) + 55 * b[5]);
        h.w = (uint32_t)(18 * (b[3] + b[9]) + 34 * (b[4] + b[8]) + 49 * (b[5] + b[7]) + 55 * b[6]);
        *reinterpret_cast<uint4 *>(&hsum[ly][4 * q]) = h;
    }
    __syncthreads();
    const int ly = tid >> 3, lx = (tid & 7) * 4, y = ty0 + ly, x = tx0 + lx;
    if (y >= lv.rows || x >= lv.cols) return;
    uint4 r[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) r[j] = *reinterpret_cast<const uint4 *>(&hsum[ly + j][lx]);
    int v[4];
    v[0] = (int)(18u * (r[0].x + r[6].x) + 34u * (r[1].x + r[5].x) + 49u * (r[2].x + r[4].x) + 55u * r[3].x);
    v[1] = (int)(18u * (r[0].y + r[6].y) + 34u * (r[1].y + r[5].y) + 49u * (r[2].y + r[4].y) + 55u * r[3].y);
    v[2] = (int)(18u * (r[0].z + r[6].z) + 34u * (r[1].z + r[5].z) + 49u * (r[2].z + r[4].z) + 55u * r[3].z);
    v[3] = (int)(18u * (r[0].w + r[6].w) + 34u * (r[1].w + r[5].w) + 49u * (r[2].w + r[4].w) + 55u * r[3].w);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = min(255, (v[k] + 32768) >> 16);
    const unsigned e = (unsigned)y * (unsigned)lv.cols + (unsigned)x;
    if ((e & 3u) == 0u && x + 3 < lv.cols) {
        *reinterpret_cast<uint32_t *>(out + e) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < lv.cols) out[e + k] = (uint8_t)v[k];
    }
}

// key point i of a frame: described or not, key = its octave, payload = i
struct OrbPlaceSrc {
    const float2 *xy;
    const int32_t *octave;
    float xHi, yHi; // cols - 31, rows - 31
    int nLevels;
    PS_D bool operator()(int i, int &key, uint32_t &pay) const
    {
        const float2 p = xy[i];
        const int o = octave[i];
        if (!(p.x >= (float)kOrbEdge && p.x < xHi && p.y >= (float)kOrbEdge && p.y < yHi) || o < 0 || o >= nLevels) return false;
        key = o;
        pay = (uint32_t)i;
        return true;
    }
};
struct OrbPlaceSink {
    int32_t *keptIdx;
    PS_D void operator()(int pos, int, uint32_t pay) const { keptIdx[pos] = (int32_t)pay; }
};

// One work-group per frame: which key points are described, in which order
__global__ __launch_bounds__(kFastSelBlock) void ps_orb_place(const int32_t *__restrict__ slots, int numSlots, const float2 *__restrict__ xy,
                                                              const int32_t *__restrict__ octave, const int32_t *__restrict__ counts, int cap,
                                                              int rows, int cols, int nLevels, int32_t *__restrict__ keptIdx,
                                                              int32_t *__restrict__ numKept)
{
    __shared__ FastSortLds s;
    const int f = (int)blockIdx.x, n = counts[f], slot = slots[f];
    if (n < 0 || n > cap || slot < 0 || slot >= numSlots) { // (uniform over the work-group)
        if (threadIdx.x == 0) numKept[f] = (n < 0 || n > cap) ? -1 : 0;
        return;
    }
    OrbPlaceSrc src;
    src.xy = xy + (size_t)f * cap;
    src.octave = octave + (size_t)f * cap;
    src.xHi = (float)(cols - kOrbEdge);
    src.yHi = (float)(rows - kOrbEdge);
    src.nLevels = (rows > 2 * kOrbEdge && cols > 2 * kOrbEdge) ? nLevels : 0;
    OrbPlaceSink sink;
    sink.keptIdx = keptIdx + (size_t)f * cap;
    const int kept = fast_stable_take(s, n, cap, src, sink);
    if (threadIdx.x == 0) numKept[f] = kept;
}

// the value a sample meets at (x, y) of a level: blurred inside, the raw level's reflection outside
PS_D int orb_sample(const uint8_t *raw, const OrbLevel &lv, int x, int y)
{
    if (x >= 0 && x < lv.cols && y >= 0 && y < lv.rows) return raw[(size_t)lv.plane + (size_t)y * lv.cols + x];
    return raw[(size_t)orb_reflect(y, lv.rows) * lv.cols + orb_reflect(x, lv.cols)];
}

// One wavefront per kept key point
__global__ __launch_bounds__(kOrbBlock) void ps_orb_describe(const uint8_t *__restrict__ planes, size_t slotBytes,
                                                             const OrbLevel *__restrict__ levels, const uint32_t *__restrict__ pattern,
                                                             const int32_t *__restrict__ slots, const float2 *__restrict__ xy,
                                                             const float *__restrict__ angle, const int32_t *__restrict__ octave, int cap,
                                                             const int32_t *__restrict__ keptIdx, const int32_t *__restrict__ numKept,
                                                             uint8_t *__restrict__ desc)
{
    const int f = (int)blockIdx.y, lane = (int)threadIdx.x & 63;
    const int j = (int)blockIdx.x * kOrbWavesPerBlock + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (j >= numKept[f]) return; // (-1 and 0 included: such a frame gets nothing)
    const size_t at = (size_t)f * cap + keptIdx[(size_t)f * cap + j];
    const OrbLevel lv = levels[octave[at]];
    const uint8_t *raw = planes + (size_t)slots[f] * slotBytes + lv.off;
    const float2 p = xy[at];
    const int cx = __float2int_rn(p.x * lv.invScale), cy = __float2int_rn(p.y * lv.invScale);
    float a, b;
    orb_rotation(angle[at], a, b);
    unsigned long long word[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t w = pattern[k * 64 + lane];
        const float x0 = (float)(int8_t)(w & 0xFFu), y0 = (float)(int8_t)((w >> 8) & 0xFFu);
        const float x1 = (float)(int8_t)((w >> 16) & 0xFFu), y1 = (float)(int8_t)(w >> 24);
        const int v0 = orb_sample(raw, lv, cx + __float2int_rn(x0 * a - y0 * b), cy + __float2int_rn(x0 * b + y0 * a));
        const int v1 = orb_sample(raw, lv, cx + __float2int_rn(x1 * a - y1 * b), cy + __float2int_rn(x1 * b + y1 * a));
        word[k] = __ballot(v0 < v1);
    }
    if (lane < 32) { // byte `lane` of the row: bit p lies in byte p >> 3 at p & 7
        const int k = lane >> 3;
        const unsigned long long w = k == 0 ? word[0] : (k == 1 ? word[1] : (k == 2 ? word[2] : word[3]));
        desc[((size_t)f * cap + j) * 32 + lane] = (uint8_t)(w >> (8 * (lane & 7)));
    }
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the pyramid set, the launches and the entry points
struct PsOrbPyramids {
    int device = 0;
    int rows = 0, cols = 0, cn = 0, nLevels = 0, slots = 0;
    psdev::OrbLevel lv[psdev::kOrbLevels];
    size_t slotBytes = 0;
    uint8_t *planes = nullptr;         // per slot: raw | blurred of every level
    uint2 *table = nullptr;            // the resize coefficients of levels 1 ..
    psdev::OrbLevel *dLevels = nullptr;
    uint32_t *dPattern = nullptr;      // 256 x (x0, y0, x1, y1) int8
};

namespace {

enum { kOrbPassLevel0 = 1, kOrbPassResize = 2, kOrbPassBlur = 4, kOrbPassPlace = 8, kOrbPassDescribe = 16, kOrbPassAll = 31 };

// The default pattern: SplitMix64 from state 0x5055545F4F5242, coordinate i of a draw u = two nibbles of byte i, summed, less 15;
// a draw whose two points are equal is drawn again
void orb_default_pattern(int8_t out[1024])
{
    uint64_t state = 0x5055545F4F5242ull;
    for (int n = 0; n < 256;) {
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        int c[4];
        for (int i = 0; i < 4; ++i) c[i] = (int)((z >> (8 * i)) & 15) + (int)((z >> (8 * i + 4)) & 15) - 15;
        if (c[0] == c[2] && c[1] == c[3]) continue;
        for (int i = 0; i < 4; ++i) out[4 * n + i] = (int8_t)c[i];
        ++n;
    }
}

// The 11-bit coefficients of one axis, sn source to dn destination pixels (the 8-bit resize(INTER_LINEAR)): columns zero the
// fraction where they clamp, rows clamp their two indices and keep it
void orb_coeffs(int sn, int dn, bool columns, uint2 *out)
{
    const double scale = 1.0 / ((double)dn / sn);
    for (int d = 0; d < dn; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (columns) {
            if (s < 0) s = 0, f = 0.f;
            if (s >= sn - 1) s = sn - 1, f = 0.f;
        }
        const int i0 = s < 0 ? 0 : (s > sn - 1 ? sn - 1 : s), i1 = s + 1 < 0 ? 0 : (s + 1 > sn - 1 ? sn - 1 : s + 1);
        const long a0 = std::lrintf((1.f - f) * 2048.f), a1 = std::lrintf(f * 2048.f);
        out[d] = make_uint2((uint32_t)i0 | (uint32_t)i1 << 16, (uint32_t)a0 | (uint32_t)a1 << 16);
    }
}

const char *orb_params_error(const PsOrbParams *p)
{
    if (!p) return "null PsOrbParams";
    if (!(p->scaleFactor > 1.f && p->scaleFactor <= 2.f)) return "PsOrbParams: scaleFactor must lie in (1, 2]";
    if (p->nLevels < 1 || p->nLevels > kOrbLevels) return "PsOrbParams: nLevels must lie in 1 .. 8";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "PsOrbParams: reserved must be 0";
    return nullptr;
}

bool orb_pattern_ok(const int8_t *p)
{
    for (int i = 0; i < 1024; ++i)
        if (p[i] < -15 || p[i] > 15) return false;
    return true;
}

int orb_build_launch(PsContext *ctx, PsOrbPyramids *pyr, const uint8_t *pixels, size_t rowStride, size_t frameStride, int frames, int firstSlot,
                     int passes)
{
    const auto grid = [&](const OrbLevel &l) {
        const unsigned quads = ((unsigned)l.rows * (unsigned)l.cols + 3u) / 4u;
        return dim3((quads + kOrbBlock - 1) / kOrbBlock, (unsigned)frames);
    };
    for (int l = 0; l < pyr->nLevels; ++l) {
        const OrbLevel &lv = pyr->lv[l];
        if (l == 0 && (passes & kOrbPassLevel0)) {
            hipLaunchKernelGGL(ps_orb_level0, grid(lv), dim3(kOrbBlock), 0, ctx->stream, pixels, rowStride, frameStride, pyr->cn,
                               orb_whole_bgr(pyr->rows, pyr->cols), lv, pyr->planes, pyr->slotBytes, firstSlot);
            PS_HIP(hipGetLastError());
        }
        if (l > 0 && (passes & kOrbPassResize)) {
            hipLaunchKernelGGL(ps_orb_resize, grid(lv), dim3(kOrbBlock), 0, ctx->stream, pyr->planes, pyr->slotBytes, firstSlot, pyr->lv[l - 1], lv,
                               (const uint2 *)pyr->table);
            PS_HIP(hipGetLastError());
        }
        if (passes & kOrbPassBlur) {
            const dim3 tiles((unsigned)((lv.cols + kOrbTile - 1) / kOrbTile), (unsigned)((lv.rows + kOrbTile - 1) / kOrbTile), (unsigned)frames);
            hipLaunchKernelGGL(ps_orb_blur, tiles, dim3(kOrbBlock), 0, ctx->stream, pyr->planes, pyr->slotBytes, firstSlot, lv);
            PS_HIP(hipGetLastError());
        }
    }
    return PS_OK;
}

int orb_describe_launch(PsContext *ctx, const PsOrbPyramids *pyr, const int32_t *slots, const float *xy, const float *angle, const int32_t *octave,
                        const int32_t *counts, int F, int cap, uint8_t *desc, int32_t *keptIdx, int32_t *numKept, int passes)
{
    if (passes & kOrbPassPlace) {
        hipLaunchKernelGGL(ps_orb_place, dim3((unsigned)F), dim3(kFastSelBlock), 0, ctx->stream, slots, pyr->slots,
                           reinterpret_cast<const float2 *>(xy), octave, counts, cap, pyr->rows, pyr->cols, pyr->nLevels, keptIdx, numKept);
        PS_HIP(hipGetLastError());
    }
    if (passes & kOrbPassDescribe) {
        const dim3 grid((unsigned)((cap + kOrbWavesPerBlock - 1) / kOrbWavesPerBlock), (unsigned)F);
        hipLaunchKernelGGL(ps_orb_describe, grid, dim3(kOrbBlock), 0, ctx->stream, (const uint8_t *)pyr->planes, pyr->slotBytes,
                           (const OrbLevel *)pyr->dLevels, (const uint32_t *)pyr->dPattern, slots, reinterpret_cast<const float2 *>(xy), angle,
                           octave, cap, (const int32_t *)keptIdx, (const int32_t *)numKept, desc);
        PS_HIP(hipGetLastError());
    }
    return PS_OK;
}

int orb_describe_check(PsContext *ctx, const PsOrbPyramids *pyr, const int32_t *slots, const float *xy, const float *angle, const int32_t *octave,
                       const int32_t *counts, int F, int capacity, uint8_t *desc, int32_t *keptIdx, int32_t *numKept, const char *who)
{
    if (!pyr || pyr->device != ctx->device || F < 0 || F > kImageMaxFrames)
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null or foreign pyramid set, or F outside 0 .. 65535").c_str());
    if (capacity > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, (std::string(who) + ": capacity above PS_MAX_KPTS").c_str());
    if (F > 0 && (capacity < 1 || !slots || !xy || !angle || !octave || !counts || !desc || !keptIdx || !numKept))
        return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": null array or capacity < 1").c_str());
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_orb_params(void) { return sizeof(PsOrbParams); }

int ps_orb_pattern_default(int8_t *out1024)
{
    if (!out1024) return PS_ERR_BAD_ARG;
    orb_default_pattern(out1024);
    return PS_OK;
}

int ps_orb_pyramids_create(PsContext *ctx, int rows, int cols, int channels, const PsOrbParams *params, const int8_t *pattern1024, int slots,
                           PsOrbPyramids **out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_pyramids_create: null out");
    *out = nullptr;
    if (const char *why = orb_params_error(params)) return fail(ctx, PS_ERR_BAD_ARG, why);
    rc = image_shape_error(ctx, rows, cols, channels, "ps_orb_pyramids_create");
    if (rc) return rc;
    if (slots < 1 || slots > kImageMaxFrames) return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_pyramids_create: slots must lie in 1 .. 65535");
    if (pattern1024 && !orb_pattern_ok(pattern1024))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_pyramids_create: a pattern coordinate outside -15 .. 15");
    HandleOwner<PsOrbPyramids> own(new PsOrbPyramids, ps_orb_pyramids_destroy);
    PsOrbPyramids *p = own.get();
    p->device = ctx->device;
    p->rows = rows;
    p->cols = cols;
    p->cn = channels;
    p->nLevels = params->nLevels;
    p->slots = slots;
    unsigned long long off = 0;
    unsigned tab = 0;
    for (int l = 0; l < p->nLevels; ++l) {
        OrbLevel &lv = p->lv[l];
        lv.scale = (float)std::pow((double)params->scaleFactor, (double)l);
        lv.invScale = 1.f / lv.scale;
        lv.rows = (int)std::lrintf((float)rows / lv.scale);
        lv.cols = (int)std::lrintf((float)cols / lv.scale);
        if (lv.rows < 1 || lv.cols < 1) return fail(ctx, PS_ERR_BAD_ARG, "ps_orb_pyramids_create: a level of the pyramid is empty");
        lv.plane = ((unsigned)lv.rows * (unsigned)lv.cols + 15u) & ~15u;
        lv.off = off;
        off += 2ull * lv.plane;
        lv.xtab = tab;
        lv.ytab = tab + (l ? (unsigned)lv.cols : 0u);
        tab += l ? (unsigned)(lv.cols + lv.rows) : 0u;
    }
    p->slotBytes = (size_t)off;
    std::vector<uint2> table(tab ? tab : 1u);
    for (int l = 1; l < p->nLevels; ++l) {
        orb_coeffs(p->lv[l - 1].cols, p->lv[l].cols, true, table.data() + p->lv[l].xtab);
        orb_coeffs(p->lv[l - 1].rows, p->lv[l].rows, false, table.data() + p->lv[l].ytab);
    }
    int8_t pat[1024];
    if (pattern1024)
        std::memcpy(pat, pattern1024, sizeof(pat));
    else
        orb_default_pattern(pat);
    hipError_t e = hipMalloc((void **)&p->planes, p->slotBytes * (size_t)slots);
    if (e == hipSuccess) e = hipMalloc((void **)&p->table, table.size() * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc((void **)&p->dLevels, sizeof(p->lv));
    if (e == hipSuccess) e = hipMalloc((void **)&p->dPattern, sizeof(pat));
    if (e == hipSuccess) e = hipMemcpy(p->table, table.data(), table.size() * sizeof(uint2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->dLevels, p->lv, sizeof(OrbLevel) * (size_t)p->nLevels, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->dPattern, pat, sizeof(pat), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "ps_orb_pyramids_create: hipMalloc", e);
    *out = own.release();
    return PS_OK;
}

void ps_orb_pyramids_destroy(PsOrbPyramids *pyr)
{
    if (!pyr) return;
    (void)hipSetDevice(pyr->device);
    if (pyr->planes) (void)hipFree(pyr->planes); // (hipFree waits for the device: queued work that reads the set has finished)
    if (pyr->table) (void)hipFree(pyr->table);
    if (pyr->dLevels) (void)hipFree(pyr->dLevels);
    if (pyr->dPattern) (void)hipFree(pyr->dPattern);
    delete pyr;
}

int ps_orb_pyramids_level(const PsOrbPyramids *pyr, int level, int32_t *dims2, float *scale)
{
    if (!pyr || level < 0 || level >= pyr->nLevels) return PS_ERR_BAD_ARG;
    if (dims2) {
        dims2[0] = pyr->lv[level].rows;
        dims2[1] = pyr->lv[level].cols;
    }
    if (scale) *scale = pyr->lv[level].scale;
    return PS_OK;
}

int ps_orb_pyramids_build_device(PsContext *ctx, PsOrbPyramids *pyr, const PsImageSet *images, int firstSlot)
{
    int rc = bind(ctx);
    if (rc) return rc;
    size_t row = 0, frame = 0;
    rc = check_image_set(ctx, pyr, &PsOrbPyramids::slots, images, firstSlot, "ps_orb_pyramids_build_device", row, frame);
    if (rc) return rc;
    if (images->numFrames == 0) return PS_OK;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return orb_build_launch(ctx, pyr, images->pixels, row, frame, images->numFrames, firstSlot, kOrbPassAll);
}

int ps_describe_features_device(PsContext *ctx, const PsOrbPyramids *pyr, const int32_t *slots, const float *xy, const float *angle,
                                const int32_t *octave, const int32_t *counts, int F, int capacity, uint8_t *desc, int32_t *keptIdx,
                                int32_t *numKept)
{
    int rc = bind(ctx);
    if (rc) return rc;
    rc = orb_describe_check(ctx, pyr, slots, xy, angle, octave, counts, F, capacity, desc, keptIdx, numKept, "ps_describe_features_device");
    if (rc) return rc;
    if (F == 0) return PS_OK;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return orb_describe_launch(ctx, pyr, slots, xy, angle, octave, counts, F, capacity, desc, keptIdx, numKept, kOrbPassAll);
}

int ps_debug_orb_passes(PsContext *ctx, PsOrbPyramids *pyr, const PsImageSet *images, int firstSlot, const int32_t *slots, const float *xy,
                        const float *angle, const int32_t *octave, const int32_t *counts, int F, int capacity, uint8_t *desc, int32_t *keptIdx,
                        int32_t *numKept, int passes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    size_t row = 0, frame = 0;
    const bool builds = (passes & (kOrbPassLevel0 | kOrbPassResize | kOrbPassBlur)) != 0, describes = (passes & (kOrbPassPlace | kOrbPassDescribe)) != 0;
    if (builds) {
        rc = check_image_set(ctx, pyr, &PsOrbPyramids::slots, images, firstSlot, "ps_debug_orb_passes", row, frame);
        if (rc) return rc;
    }
    if (describes) {
        rc = orb_describe_check(ctx, pyr, slots, xy, angle, octave, counts, F, capacity, desc, keptIdx, numKept, "ps_debug_orb_passes");
        if (rc) return rc;
    }
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    if (builds && images->numFrames > 0) {
        rc = orb_build_launch(ctx, pyr, images->pixels, row, frame, images->numFrames, firstSlot, passes);
        if (rc) return rc;
    }
    if (describes && F > 0) return orb_describe_launch(ctx, pyr, slots, xy, angle, octave, counts, F, capacity, desc, keptIdx, numKept, passes);
    return PS_OK;
}

int ps_describe_features(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const PsOrbParams *params,
                         const int8_t *pattern1024, const float *xy, const float *angle, const int32_t *octave, int n, uint8_t *desc,
                         int32_t *keptIdx, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (const char *why = orb_params_error(params)) return fail(ctx, PS_ERR_BAD_ARG, why);
    rc = image_shape_error(ctx, rows, cols, channels, "ps_describe_features");
    if (rc) return rc;
    if (n > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_describe_features: more than PS_MAX_KPTS key points");
    rowStride = image_row_stride(cols, channels, rowStride);
    if (!img || !nout || rowStride == 0 || n < 0 || (n > 0 && (!xy || !angle || !octave || !desc || !keptIdx)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_describe_features: null array, negative n or a row stride below a row");
    TimingOff toff(ctx);
    PsOrbPyramids *pyr = nullptr;
    rc = ps_orb_pyramids_create(ctx, rows, cols, channels, params, pattern1024, 1, &pyr); // (refuses a bad pattern or an empty level)
    if (rc) return rc;
    const HandleOwner<PsOrbPyramids> own(pyr, ps_orb_pyramids_destroy);
    if (n == 0) {
        *nout = 0;
        return PS_OK;
    }
    const size_t imgBytes = image_bytes(rows, cols, channels, rowStride), N = (size_t)n;
    // one block: the image | slot, count, numKept, 0 | xy | angle | octave | keptIdx | desc
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes);
    const size_t oHead = lay.take<int32_t>(4, 16), oXy = lay.take<float2>(N), oAngle = lay.take<float>(N), oOct = lay.take<int32_t>(N),
                 oKept = lay.take<int32_t>(N), oDesc = lay.take<uint8_t>(N * 32), total = lay.total;
    const DeviceBlock blk(total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    const int32_t head[4] = {0, n, 0, 0};
    PS_HIP(hipMemcpyAsync(d, img, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oHead, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oXy, xy, N * 8, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oAngle, angle, N * 4, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oOct, octave, N * 4, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (head[] and pageable sources leave scope / may change)
    rc = orb_build_launch(ctx, pyr, (const uint8_t *)d, rowStride, 0, 1, 0, kOrbPassAll);
    if (rc) return rc;
    int32_t *h = (int32_t *)(d + oHead);
    rc = orb_describe_launch(ctx, pyr, h, (const float *)(d + oXy), (const float *)(d + oAngle), (const int32_t *)(d + oOct), h + 1, 1, n,
                             (uint8_t *)(d + oDesc), (int32_t *)(d + oKept), h + 2, kOrbPassAll);
    if (rc) return rc;
    int32_t k = 0;
    PS_HIP(hipMemcpyAsync(&k, h + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    if (k < 0 || k > n) return fail(ctx, PS_ERR_HIP, "ps_describe_features: the device returned an impossible count");
    if (k > 0) { // keptIdx | desc lie side by side
        std::vector<char> back((oDesc - oKept) + (size_t)k * 32);
        PS_HIP(hipMemcpyAsync(back.data(), d + oKept, back.size(), hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
        std::memcpy(keptIdx, back.data(), (size_t)k * 4);
        std::memcpy(desc, back.data() + (oDesc - oKept), (size_t)k * 32);
    }
    *nout = k;
    return PS_OK;
}

int ps_debug_orb_level(PsContext *ctx, const PsOrbPyramids *pyr, int slot, int level, uint8_t *raw, uint8_t *blurred)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!pyr || pyr->device != ctx->device || slot < 0 || slot >= pyr->slots || level < 0 || level >= pyr->nLevels)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_debug_orb_level: null or foreign pyramid set, or no such slot or level");
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const OrbLevel &lv = pyr->lv[level];
    const uint8_t *at = pyr->planes + (size_t)slot * pyr->slotBytes + lv.off;
    const size_t bytes = (size_t)lv.rows * lv.cols;
    if (raw) PS_HIP(hipMemcpy(raw, at, bytes, hipMemcpyDeviceToHost));
    if (blurred) PS_HIP(hipMemcpy(blurred, at + lv.plane, bytes, hipMemcpyDeviceToHost));
    return PS_OK;
}

} // extern "C"
