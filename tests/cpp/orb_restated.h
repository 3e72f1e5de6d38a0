// ORB description restated in plain single-thread C++ (the specification of include/putslam_hip.h and DESIGN.md section 8.11, a third
// time after the two of tests/orb_ref.py): tests/cpp/test_dropin_orb.cpp holds the drop-in to it, profiles/scripts/orb_host_loop.cpp
// is the timing control built from it.  Compile with -ffp-contract=off: every float operation rounds on its own.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace orb_restated {

struct Level {
    int rows = 0, cols = 0;
    float scale = 1.f;
    std::vector<uint8_t> raw, blurred;
};

inline int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

inline int cv_round(float v) { return (int)std::lrintf(v); } // (the default rounding mode: half to even)

inline void default_pattern(int8_t out[1024])
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

struct Coeff {
    int i0, i1, a0, a1;
};
inline std::vector<Coeff> coeffs(int sn, int dn, bool columns)
{
    std::vector<Coeff> out((size_t)dn);
    const double scale = 1.0 / ((double)dn / sn);
    for (int d = 0; d < dn; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (columns) {
            if (s < 0) s = 0, f = 0.f;
            if (s >= sn - 1) s = sn - 1, f = 0.f;
        }
        Coeff &c = out[(size_t)d];
        c.i0 = s < 0 ? 0 : (s > sn - 1 ? sn - 1 : s);
        c.i1 = s + 1 < 0 ? 0 : (s + 1 > sn - 1 ? sn - 1 : s + 1);
        c.a0 = cv_round((1.f - f) * 2048.f);
        c.a1 = cv_round(f * 2048.f);
    }
    return out;
}

inline void resize(const Level &s, Level &d)
{
    const std::vector<Coeff> cx = coeffs(s.cols, d.cols, true), cy = coeffs(s.rows, d.rows, false);
    d.raw.resize((size_t)d.rows * d.cols);
    for (int y = 0; y < d.rows; ++y) {
        const uint8_t *r0 = s.raw.data() + (size_t)cy[(size_t)y].i0 * s.cols, *r1 = s.raw.data() + (size_t)cy[(size_t)y].i1 * s.cols;
        const int b0 = cy[(size_t)y].a0, b1 = cy[(size_t)y].a1;
        for (int x = 0; x < d.cols; ++x) {
            const Coeff &c = cx[(size_t)x];
            const int h0 = r0[c.i0] * c.a0 + r0[c.i1] * c.a1, h1 = r1[c.i0] * c.a0 + r1[c.i1] * c.a1;
            d.raw[(size_t)y * d.cols + x] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

inline void blur(Level &l)
{
    static const int taps[7] = {18, 34, 49, 55, 49, 34, 18};
    const int R = l.rows, C = l.cols;
    std::vector<int> h((size_t)R * C);
    std::vector<int> xi((size_t)C * 7);
    for (int x = 0; x < C; ++x)
        for (int i = 0; i < 7; ++i) xi[(size_t)x * 7 + i] = reflect101(x + i - 3, C);
    for (int y = 0; y < R; ++y) {
        const uint8_t *row = l.raw.data() + (size_t)y * C;
        for (int x = 0; x < C; ++x) {
            int s = 0;
            for (int i = 0; i < 7; ++i) s += taps[i] * row[xi[(size_t)x * 7 + i]];
            h[(size_t)y * C + x] = s;
        }
    }
    l.blurred.resize((size_t)R * C);
    for (int y = 0; y < R; ++y) {
        const int *rows[7];
        for (int j = 0; j < 7; ++j) rows[j] = h.data() + (size_t)reflect101(y + j - 3, R) * C;
        for (int x = 0; x < C; ++x) {
            int v = 0;
            for (int j = 0; j < 7; ++j) v += taps[j] * rows[j][x];
            v = (v + 32768) >> 16;
            l.blurred[(size_t)y * C + x] = (uint8_t)(v > 255 ? 255 : v);
        }
    }
}

inline std::vector<Level> pyramid(const uint8_t *img, int rows, int cols, int cn, size_t step, float scaleFactor, int nLevels)
{
    std::vector<Level> lv((size_t)nLevels);
    for (int l = 0; l < nLevels; ++l) {
        Level &L = lv[(size_t)l];
        L.scale = (float)std::pow((double)scaleFactor, (double)l);
        L.rows = cv_round((float)rows / L.scale);
        L.cols = cv_round((float)cols / L.scale);
        if (l == 0) {
            L.raw.resize((size_t)rows * cols);
            for (int y = 0; y < rows; ++y)
                for (int x = 0; x < cols; ++x) {
                    const uint8_t *p = img + (size_t)y * step + (size_t)x * cn;
                    L.raw[(size_t)y * cols + x] = cn == 1 ? p[0] : (uint8_t)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14);
                }
        } else {
            resize(lv[(size_t)l - 1], L);
        }
        blur(L);
    }
    return lv;
}

inline void rotation(float deg, float &a, float &b)
{
    if (!(std::fabs(deg) <= 1048576.f)) deg = 0.f;
    const float q = std::nearbyintf(deg * (float)(1.0 / 90.0));
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

inline int sample(const Level &l, int x, int y)
{
    if (x >= 0 && x < l.cols && y >= 0 && y < l.rows) return l.blurred[(size_t)y * l.cols + x];
    return l.raw[(size_t)reflect101(y, l.rows) * l.cols + reflect101(x, l.cols)];
}

// desc: n x 32 bytes, keptIdx: n; returns the number of rows written
inline int describe(const uint8_t *img, int rows, int cols, int cn, size_t step, float scaleFactor, int nLevels, const int8_t *pattern1024,
                    const float *xy, const float *angle, const int32_t *octave, int n, uint8_t *desc, int32_t *keptIdx)
{
    int8_t pat[1024];
    if (pattern1024)
        std::memcpy(pat, pattern1024, sizeof(pat));
    else
        default_pattern(pat);
    const std::vector<Level> lv = pyramid(img, rows, cols, cn, step, scaleFactor, nLevels);
    int k = 0;
    if (rows <= 62 || cols <= 62) return 0;
    for (int l = 0; l < nLevels; ++l)
        for (int i = 0; i < n; ++i) {
            const float x = xy[2 * i], y = xy[2 * i + 1];
            if (octave[i] != l || !(x >= 31.f && x < (float)(cols - 31) && y >= 31.f && y < (float)(rows - 31))) continue;
            const Level &L = lv[(size_t)l];
            const float s = 1.f / L.scale;
            const int cx = cv_round(x * s), cy = cv_round(y * s);
            float a, b;
            rotation(angle[i], a, b);
            uint8_t *row = desc + (size_t)k * 32;
            std::memset(row, 0, 32);
            for (int p = 0; p < 256; ++p) {
                const float x0 = pat[4 * p], y0 = pat[4 * p + 1], x1 = pat[4 * p + 2], y1 = pat[4 * p + 3];
                const int v0 = sample(L, cx + cv_round(x0 * a - y0 * b), cy + cv_round(x0 * b + y0 * a));
                const int v1 = sample(L, cx + cv_round(x1 * a - y1 * b), cy + cv_round(x1 * b + y1 * a));
                if (v0 < v1) row[p >> 3] |= (uint8_t)(1u << (p & 7));
            }
            keptIdx[k++] = i;
        }
    return k;
}

} // namespace orb_restated
