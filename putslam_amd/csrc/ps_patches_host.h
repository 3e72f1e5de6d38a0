// ps_patches_host.h -- the sub-pixel matching on patches (ps_patches.h) restated sequentially in plain C++:
// MatchingOnPatches::computePatch / computeGradient / optimizeLocation / evaluatePatches (src/Matcher/MatchingOnPatches.cpp:14-246),
// one point at a time on one thread, every operation rounded separately when compiled with -ffp-contract=off on a target without
// implicit FMA.  It is what a host does WITHOUT the device calls: the control of profiles/scripts/patches_times.py and the body of
// tests/cpp/test_patches_host.cpp, which holds its bytes to tests/patches_ref.py's; the GPU tests hold the device to the same.
// Pure -- no HIP header, no runtime call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "ps_patches_rule.h"

namespace patch_host {

struct Image { // rows x cols x cn uint8, rows `step` bytes apart
    const uint8_t *p;
    size_t step;
    int rows, cols, cn;
};

// one channel as it is, three by CV_RGB2GRAY (ps_fast.h's rule)
inline int grey(const Image &im, int i, int j)
{
    const uint8_t *q = im.p + (size_t)i * im.step + (size_t)j * im.cn;
    return im.cn == 1 ? (int)q[0] : ((int)q[0] * 4899 + (int)q[1] * 9617 + (int)q[2] * 1868 + 8192) >> 14;
}

// computePatch (:14-51); the caller has applied a tap rule.  out: E doubles
inline void patch(const Image &im, double x, double y, int h, double *out)
{
    const int ix = (int)x, iy = (int)y;
    const double xs = x - (double)ix, ys = y - (double)iy;
    const double tl = (1.0 - xs) * (1.0 - ys), tr = xs * (1.0 - ys), bl = (1.0 - xs) * ys, br = xs * ys;
    int k = 0;
    for (int i = iy - h; i <= iy + h; ++i)
        for (int j = ix - h; j <= ix + h; ++j)
            out[k++] = ((tl * (double)grey(im, i, j) + tr * (double)grey(im, i, j + 1)) + bl * (double)grey(im, i + 1, j)) +
                       br * (double)grey(im, i + 1, j + 1);
}

// every NaN written is the one quiet pattern (a host's 0 x inf carries the sign bit, the device's does not)
inline float canon(float v)
{
    if (v == v) return v;
    const uint32_t bits = 0x7FC00000u;
    std::memcpy(&v, &bits, 4);
    return v;
}
inline double canon(double v)
{
    if (v == v) return v;
    const uint64_t bits = 0x7FF8000000000000ull;
    std::memcpy(&v, &bits, 8);
    return v;
}

inline float cofactor(const float (&m)[3][3], int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
}
// the float twin of ps_uncertainty_host.h's inverse(): the project's reading of Eigen 3's fixed-size inverse (unpinned)
inline void inverse(const float (&m)[3][3], float *r)
{
    const float det = (cofactor(m, 0, 0) * m[0][0] + cofactor(m, 1, 0) * m[1][0]) + cofactor(m, 2, 0) * m[2][0];
    const float invdet = 1.f / det;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[3 * i + j] = canon(cofactor(m, j, i) * invdet);
}

// computeGradient (:53-99).  gx, gy: E floats; inv: 9 floats row-major
inline void gradient(const Image &im, double x, double y, int h, float *gx, float *gy, float *inv)
{
    const int ix = (int)x, iy = (int)y;
    float H[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    int k = 0;
    for (int i = iy - h; i <= iy + h; ++i)
        for (int j = ix - h; j <= ix + h; ++j) {
            float J[3];
            J[0] = 0.5f * (float)(grey(im, i, j + 1) - grey(im, i, j - 1));
            J[1] = 0.5f * (float)(grey(im, i + 1, j) - grey(im, i - 1, j));
            J[2] = 1.f;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) H[a][b] = H[a][b] + J[a] * J[b];
            gx[k] = J[0];
            gy[k] = J[1];
            ++k;
        }
    inverse(H, inv);
}

// optimizeLocation (:101-200) on a given model; scratch: E doubles.  Returns the status, x / y / iterations as the reference
// leaves them
inline int optimize(const Image &nw, const double *oldPatch, const float *gx, const float *gy, const float *inv, int h, int maxIter,
                    double minSqrtIncrement, double &x, double &y, int &iterations, double *scratch)
{
    iterations = 0;
    if (inv[0] != inv[0]) return PS_PATCH_NAN_HESSIAN;
    const int E = (2 * h + 1) * (2 * h + 1);
    const double sx = x, sy = y, mean = 0.0;
    for (int it = 0; it < maxIter; ++it) {
        if (patch_gate_out(x, y, h, nw.rows, nw.cols)) return PS_PATCH_OUT_OF_IMAGE;
        if (!patch_new_taps_inside(x, y, h, nw.rows, nw.cols)) return PS_PATCH_NEW_TAPS_OUTSIDE;
        patch(nw, x, y, h, scratch);
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        for (int k = 0; k < E; ++k) {
            const float diff = (float)((scratch[k] - oldPatch[k]) + mean);
            t0 = t0 - diff * gx[k];
            t1 = t1 - diff * gy[k];
            t2 = t2 - diff;
        }
        const float inc0 = (inv[0] * t0 + inv[1] * t1) + inv[2] * t2, inc1 = (inv[3] * t0 + inv[4] * t1) + inv[5] * t2;
        x = canon(x + (double)inc0);
        y = canon(y + (double)inc1);
        iterations = it + 1;
        if ((double)(inc0 * inc0 + inc1 * inc1) < minSqrtIncrement) {
            if ((x - sx) * (x - sx) + (y - sy) * (y - sy) > (double)(h * h)) return PS_PATCH_MOVED_TOO_FAR;
            return PS_PATCH_CONVERGED;
        }
    }
    return PS_PATCH_MAX_ITERATIONS;
}

// The fused form for one point: the model from the old image at (ox, oy), then the alignment in the new one from (x, y).
// work: 2 E doubles and 2 E floats the caller owns (patch, scratch; gx, gy); inv 9 floats
inline int align(const Image &old, const Image &nw, double ox, double oy, const PsPatchParams &prm, double &x, double &y, int &iterations,
                 double *patchOut, double *scratch, float *gx, float *gy, float *inv)
{
    const int h = patch_half(prm.patchSize);
    iterations = 0;
    if (!patch_old_taps_inside(ox, oy, h, old.rows, old.cols)) return PS_PATCH_OLD_TAPS_OUTSIDE;
    patch(old, ox, oy, h, patchOut);
    gradient(old, ox, oy, h, gx, gy, inv);
    return optimize(nw, patchOut, gx, gy, inv, h, prm.maxIter, prm.minSqrtIncrement, x, y, iterations, scratch);
}

} // namespace patch_host
