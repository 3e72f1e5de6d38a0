// ORB detection restated in plain single-thread C++ (the specification of include/putslam_hip.h and DESIGN.md section 8.12, a third
// time after the two of tests/orb_detect_ref.py): tests/cpp/test_dropin_orb_detect.cpp holds the drop-in to it,
// profiles/scripts/orb_detect_host_loop.cpp is the timing control built from it.  The levels and the resize are orb_restated.h's.
// Compile with -ffp-contract=off: every float operation rounds on its own.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "orb_restated.h"

namespace orb_detect_restated {

using orb_restated::cv_round;
using orb_restated::Level;

struct Params {
    int nFeatures = 500;
    float scaleFactor = 1.2f;
    int nLevels = 8, fastThreshold = 20, gridRows = 1, gridCols = 1, maximalTrackedFeatures = 500;
};

struct Kp {
    float x = 0, y = 0, size = 0, angle = 0, response = 0;
    int octave = 0;
};

inline std::vector<int> quotas(int nFeatures, float scaleFactor, int nLevels)
{
    std::vector<int> q((size_t)nLevels, 0);
    const float factor = (float)(1.0 / (double)scaleFactor);
    float nd = (float)nFeatures * (1.f - factor) / (1.f - (float)std::pow((double)factor, (double)nLevels));
    int sum = 0;
    for (int l = 0; l < nLevels - 1; ++l) {
        q[(size_t)l] = cv_round(nd);
        sum += q[(size_t)l];
        nd *= factor;
    }
    q[(size_t)nLevels - 1] = std::max(nFeatures - sum, 0);
    return q;
}

inline float fast_atan2(float y, float x)
{
    const float k = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k, p5 = 0.1555786518463281f * k, p7 = -0.04432655554792128f * k;
    const float ax = std::fabs(x), ay = std::fabs(y);
    const float c = std::min(ax, ay) / (std::max(ax, ay) + (float)DBL_EPSILON);
    const float c2 = c * c;
    float a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    if (ax < ay) a = 90.f - a;
    if (x < 0.f) a = 180.f - a;
    if (y < 0.f) a = 360.f - a;
    return a;
}

struct Cand {
    int x, y;
    float response;
};

// FAST-9/16 with suppression on one level, by the definition (arcs of nine tried one by one), inside the border of 31
inline std::vector<Cand> fast_level(const Level &L, int t)
{
    static const int ring[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3}, {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0},
                                    {-3, 1}, {-2, 2}, {-1, 3}};
    const int w = L.cols, h = L.rows;
    std::vector<int> score((size_t)w * h, 0);
    for (int y = 3; y < h - 3; ++y)
        for (int x = 3; x < w - 3; ++x) {
            int d[16];
            const int v = L.raw[(size_t)y * w + x];
            for (int k = 0; k < 16; ++k) d[k] = v - (int)L.raw[(size_t)(y + ring[k][1]) * w + x + ring[k][0]];
            int D = -1000, B = -1000;
            for (int s = 0; s < 16; ++s) {
                int lo = 1000, hi = -1000;
                for (int j = 0; j < 9; ++j) {
                    lo = std::min(lo, d[(s + j) & 15]);
                    hi = std::max(hi, d[(s + j) & 15]);
                }
                D = std::max(D, lo);
                B = std::max(B, -hi);
            }
            if (D > t || B > t) score[(size_t)y * w + x] = std::max(t, std::max(D, B)) - 1;
        }
    std::vector<Cand> out;
    for (int y = 31; y < h - 31; ++y)
        for (int x = 31; x < w - 31; ++x) {
            const int s = score[(size_t)y * w + x];
            if (s == 0) continue; // (no corner, or a corner of score 0: never strictly above its neighbours)
            bool top = true;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if ((dx || dy) && !(s > score[(size_t)(y + dy) * w + x + dx])) top = false;
            if (top) out.push_back(Cand{x, y, (float)s});
        }
    return out;
}

// KeyPointsFilter::retainBest as a set: every key point at or above the n-th largest response, in the list's order
inline void retain_best(std::vector<Cand> &v, int n)
{
    if (n >= (int)v.size()) return;
    if (n == 0) {
        v.clear();
        return;
    }
    std::vector<float> r;
    for (const Cand &c : v) r.push_back(c.response);
    std::sort(r.begin(), r.end(), [](float a, float b) { return a > b; });
    const float boundary = r[(size_t)n - 1];
    std::vector<Cand> out;
    for (const Cand &c : v)
        if (c.response >= boundary) out.push_back(c);
    v.swap(out);
}

inline float harris(const Level &L, int x0, int y0)
{
    const int s = L.cols;
    int a = 0, b = 0, c = 0;
    for (int dy = -3; dy <= 3; ++dy)
        for (int dx = -3; dx <= 3; ++dx) {
            const uint8_t *p = L.raw.data() + (size_t)(y0 + dy) * s + x0 + dx;
            const int ix = (p[1] - p[-1]) * 2 + (p[-s + 1] - p[-s - 1]) + (p[s + 1] - p[s - 1]);
            const int iy = (p[s] - p[-s]) * 2 + (p[s - 1] - p[-s - 1]) + (p[s + 1] - p[-s + 1]);
            a += ix * ix;
            b += iy * iy;
            c += ix * iy;
        }
    const float scale = 1.f / (4 * 7 * 255.f);
    const float s4 = scale * scale * scale * scale;
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    return ((fa * fb - fc * fc) - (0.04f * (fa + fb)) * (fa + fb)) * s4;
}

inline float ic_angle(const Level &L, int x0, int y0)
{
    static const int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    const int s = L.cols;
    const uint8_t *c = L.raw.data() + (size_t)y0 * s + x0;
    int m01 = 0, m10 = 0;
    for (int u = -15; u <= 15; ++u) m10 += u * c[u];
    for (int v = 1; v <= 15; ++v) {
        int vsum = 0;
        for (int u = -umax[v]; u <= umax[v]; ++u) {
            const int plus = c[u + v * s], minus = c[u - v * s];
            vsum += plus - minus;
            m10 += u * (plus + minus);
        }
        m01 += v * vsum;
    }
    return fast_atan2((float)m01, (float)m10);
}

// the detector on one grey image of w x h pixels (an ROI is an image of its own): levels ascending, raster order inside a level
inline std::vector<Kp> detect_roi(const uint8_t *gray, size_t stride, int w, int h, const Params &p)
{
    const std::vector<int> q = quotas(p.nFeatures, p.scaleFactor, p.nLevels);
    const int t = std::min(std::max(p.fastThreshold, 0), 255);
    std::vector<Level> lv((size_t)p.nLevels);
    std::vector<Kp> out;
    for (int l = 0; l < p.nLevels; ++l) {
        Level &L = lv[(size_t)l];
        L.scale = (float)std::pow((double)p.scaleFactor, (double)l);
        L.rows = cv_round((float)h / L.scale);
        L.cols = cv_round((float)w / L.scale);
        if (l == 0) {
            L.raw.resize((size_t)w * h);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) L.raw[(size_t)y * w + x] = gray[(size_t)y * stride + x];
        } else {
            orb_restated::resize(lv[(size_t)l - 1], L);
        }
        if (L.rows <= 62 || L.cols <= 62) continue;
        std::vector<Cand> c = fast_level(L, t);
        retain_best(c, 2 * q[(size_t)l]);
        for (Cand &k : c) k.response = harris(L, k.x, k.y);
        retain_best(c, q[(size_t)l]);
        for (const Cand &k : c) {
            Kp kp;
            kp.x = (float)k.x * L.scale;
            kp.y = (float)k.y * L.scale;
            kp.size = 31.f * L.scale;
            kp.angle = ic_angle(L, k.x, k.y);
            kp.response = k.response;
            kp.octave = l;
            out.push_back(kp);
        }
    }
    return out;
}

inline bool by_response(const Kp &a, const Kp &b) { return a.response > b.response; } // compare_response, matcherOpenCV.h:84-87

// the grid loop of matcherOpenCV.cpp:118-180 with both orderings stable
inline std::vector<Kp> detect(const uint8_t *img, int rows, int cols, int cn, size_t step, const Params &p)
{
    std::vector<uint8_t> gray((size_t)rows * cols);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const uint8_t *px = img + (size_t)y * step + (size_t)x * cn;
            gray[(size_t)y * cols + x] = cn == 1 ? px[0] : (uint8_t)((px[0] * 4899 + px[1] * 9617 + px[2] * 1868 + 8192) >> 14);
        }
    const int maxInRoi = p.maximalTrackedFeatures * 3 / (p.gridCols * p.gridRows);
    std::vector<Kp> joined;
    for (int k = 0; k < p.gridCols; ++k)
        for (int i = 0; i < p.gridRows; ++i) {
            const int x0 = k * cols / p.gridCols, y0 = i * rows / p.gridRows;
            std::vector<Kp> in = detect_roi(gray.data() + (size_t)y0 * cols + x0, (size_t)cols, cols / p.gridCols, rows / p.gridRows, p);
            std::stable_sort(in.begin(), in.end(), by_response);
            for (size_t j = 0; j < in.size() && (int)j < maxInRoi; ++j) {
                in[j].x += (float)x0;
                in[j].y += (float)y0;
                joined.push_back(in[j]);
            }
        }
    std::stable_sort(joined.begin(), joined.end(), by_response);
    if ((int)joined.size() > p.maximalTrackedFeatures) joined.resize((size_t)std::max(p.maximalTrackedFeatures, 0));
    return joined;
}

} // namespace orb_detect_restated
