// ps_uncertainty_host.h -- the measurement uncertainty (ps_uncertainty.h) restated sequentially in plain
// C++: RGBD::computeNormal / computeRGBGradient (src/RGBD/RGBD.cpp:100-187) and the covariance models of
// src/Grabber/depthSensorModel.cpp:27-36,55-101, one feature at a time on one thread, every operation rounded separately when
// compiled with -ffp-contract=off on a target without implicit FMA.  It is what a host does WITHOUT the device calls: the control
// of profiles/scripts/uncertainty_times.py, and the arithmetic of the drop-in's DepthSensorModel, whose reference signatures return
// covariances the C ABI does not export.  tests hold its bytes to the device's.
// Pure -- no HIP header, no runtime call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "ps_uncertainty_rule.h"

namespace unc_host {

struct Camera {
    float fx, fy, cx, cy; // K
    double scale;         // depthImageScale
};
struct DepthImage { // rows x cols uint16, rows `step` bytes apart
    const uint8_t *p;
    size_t step;
    int rows, cols;
};
struct ColourImage { // rows x cols x 3 uint8, rows `step` bytes apart
    const uint8_t *p;
    size_t step;
};

inline double canon(double x)
{
    if (x == x) return x;
    const uint64_t bits = 0x7FF8000000000000ull;
    std::memcpy(&x, &bits, 8);
    return x;
}

// RGBD::roundSize and point2Dto3D on the image as the dense one the reference holds (ps_assemble_frames' rule)
inline int round_size(double x, int size)
{
    if (x < 0)
        x = 0;
    else if (x > size - 1)
        x = size;
    return (int)std::round(x);
}
inline void point(const Camera &c, const DepthImage &d, float x, float y, float &X, float &Y, float &Z)
{
    unsigned dv = 0;
    if (x == x && y == y) {
        const size_t pix = (size_t)round_size((double)y, d.rows) * (size_t)d.cols + (size_t)round_size((double)x, d.cols);
        if (pix < (size_t)d.rows * (size_t)d.cols) {
            const uint8_t *at = d.p + (pix / (size_t)d.cols) * d.step + (pix % (size_t)d.cols) * 2;
            dv = (unsigned)at[0] | ((unsigned)at[1] << 8);
        }
    }
    Z = (float)(((double)dv) / c.scale);
    const float u = (x - c.cx) / c.fx, v = (y - c.cy) / c.fy;
    X = u * Z;
    Y = v * Z;
}

inline bool pixel_of(float u, float v, int &pu, int &pv)
{
    const float lim = 2147483520.0f;
    if (!(u >= -lim && u <= lim && v >= -lim && v <= lim)) return false;
    pu = (int)u;
    pv = (int)v;
    return true;
}

inline void normalize(double (&v)[3])
{
    const double n = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] / n;
    v[1] = v[1] / n;
    v[2] = v[2] / n;
}
inline void cross(const double (&a)[3], const double (&b)[3], double (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// RGBD::computeNormal, with its list
inline void normal(const Camera &c, const DepthImage &d, int u, int v, double (&n)[3])
{
    static const int uidx[8] = {-1, -1, -1, 0, 1, 1, 1, 0}, vidx[8] = {-1, 0, 1, 1, 1, 0, -1, -1};
    float cX, cY, cZ;
    point(c, d, (float)u, (float)v, cX, cY, cZ);
    double vecs[8][3];
    int k = 0;
    for (int i = 0; i < 8; ++i) {
        float X, Y, Z;
        point(c, d, (float)(u + uidx[i]), (float)(v + vidx[i]), X, Y, Z);
        if (Z > 0) {
            vecs[k][0] = (double)(X - cX), vecs[k][1] = (double)(Y - cY), vecs[k][2] = (double)(Z - cZ);
            ++k;
        }
    }
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < k; ++i) {
        double t[3];
        cross(vecs[i], vecs[i == k - 1 ? 0 : i + 1], t);
        s[0] += t[0], s[1] += t[1], s[2] += t[2];
    }
    n[0] = s[0] / (double)k, n[1] = s[1] / (double)k, n[2] = s[2] / (double)k;
    normalize(n);
}

// RGBD::computeRGBGradient; tie: unc_tie_table(1)
inline void gradient(const Camera &c, const DepthImage &d, const ColourImage &im, const int32_t *tie, int u, int v, double (&g)[3])
{
    if (!((u - 1 > 0) && (v - 1 > 0) && (u + 1 < d.cols) && (v + 1 < d.rows))) {
        g[0] = g[1] = g[2] = 1.0;
        return;
    }
    int w[3][3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            const uint8_t *at = im.p + (size_t)(v - 1 + r) * im.step + (size_t)(u - 1) * 3 + 2 * k;
            w[r][k] = (int)at[0] | ((int)at[1] << 8);
        }
    const int gradx = -3 * w[0][0] - 10 * w[0][1] - 3 * w[0][2] + 3 * w[2][0] + 10 * w[2][1] + 3 * w[2][2];
    const int grady = -3 * w[0][0] - 10 * w[1][0] - 3 * w[2][0] + 3 * w[0][2] + 10 * w[1][2] + 3 * w[2][2];
    const int ax = gradx < 0 ? -gradx : gradx, ay = grady < 0 ? -grady : grady;
    int c1x, c1y, c2x, c2y;
    if (ax == ay) {
        const int t = gradx == 0 ? 0 : (gradx > 0 ? (grady > 0 ? 1 : 4) : (grady > 0 ? 2 : 3));
        c1x = tie[4 * t], c1y = tie[4 * t + 1], c2x = tie[4 * t + 2], c2y = tie[4 * t + 3];
    } else {
        c1x = ax > ay ? (gradx > 0 ? 1 : -1) : 0;
        c1y = ay > ax ? (grady > 0 ? -1 : 1) : 0;
        c2x = -c1x, c2y = -c1y;
    }
    float cen[3], end[3], beg[3];
    point(c, d, (float)u, (float)v, cen[0], cen[1], cen[2]);
    point(c, d, (float)(u + c1x), (float)(v + c1y), end[0], end[1], end[2]);
    point(c, d, (float)(u + c2x), (float)(v + c2y), beg[0], beg[1], beg[2]);
    if (end[2] > 0 && beg[2] != 0.f) {
        for (int i = 0; i < 3; ++i) g[i] = (double)(end[i] - beg[i]);
    } else if (cen[2] > 0 && beg[2] != 0.f) {
        for (int i = 0; i < 3; ++i) g[i] = (double)(cen[i] - beg[i]);
    } else if (cen[2] > 0 && end[2] != 0.f) {
        for (int i = 0; i < 3; ++i) g[i] = (double)(end[i] - cen[i]);
    } else {
        g[0] = (double)c1x, g[1] = (double)c1y, g[2] = 0.0;
    }
    normalize(g);
}

// ---- 3 x 3 matrices, row-major [r][c], dense products ----
inline void mul(const double (&A)[3][3], const double (&B)[3][3], double (&C)[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}
inline double cofactor(const double (&m)[3][3], int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
}
// the project's reading of Eigen 3's fixed-size inverse (unpinned: DESIGN.md section 8.16)
inline void inverse(const double (&m)[3][3], double (&r)[3][3])
{
    const double det = (cofactor(m, 0, 0) * m[0][0] + cofactor(m, 1, 0) * m[1][0]) + cofactor(m, 2, 0) * m[2][0];
    const double invdet = 1.0 / det;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[i][j] = cofactor(m, j, i) * invdet;
}

// DepthSensorModel::computeCov(u, v, depth) for unsigned u, v
inline void compute_cov(const PsSensorModel &s, double u, double v, double z, double (&cov)[3][3])
{
    const double J[3][3] = {{z / s.fu, 0.0, (u / s.fu) - (s.cu / s.fu)}, {0.0, z / s.fv, (v / s.fv) - (s.cv / s.fv)}, {0.0, 0.0, 1.0}};
    const double R[3][3] = {{s.varU, 0.0, 0.0}, {0.0, s.varV, 0.0}, {0.0, 0.0, ((s.c3 * (z * z * z) + s.c2 * (z * z)) + s.c1 * z) + s.c0}};
    double Jt[3][3], T[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Jt[i][j] = J[j][i];
    mul(J, R, T);
    mul(T, Jt, cov);
}
// informationMatrixFromImageCoordinates(u, v, z): false (a NaN matrix) where (unsigned long)u is undefined
inline bool info_image_coordinates(const PsSensorModel &s, double u, double v, double z, double (&info)[3][3])
{
    const double two64 = 18446744073709551616.0;
    if (!(u >= 0.0 && u < two64 && v >= 0.0 && v < two64)) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) info[i][j] = canon(std::nan(""));
        return false;
    }
    double cov[3][3];
    compute_cov(s, (double)(unsigned long long)u, (double)(unsigned long long)v, z, cov);
    inverse(cov, info);
    return true;
}
// ((R S) S) R^-1 for R with columns c0, c1, c2 and S = the identity with S(d, d) = scale
inline void from_basis(const double (&c0)[3], const double (&c1)[3], const double (&c2)[3], int d, double scale, double (&cov)[3][3])
{
    double R[3][3], S[3][3], T[3][3], U[3][3], Ri[3][3];
    for (int i = 0; i < 3; ++i) {
        R[i][0] = c0[i], R[i][1] = c1[i], R[i][2] = c2[i];
        for (int j = 0; j < 3; ++j) S[i][j] = i == j ? (i == d ? scale : 1.0) : 0.0;
    }
    mul(R, S, T);
    mul(T, S, U);
    inverse(R, Ri);
    mul(U, Ri, cov);
}
inline void uncertainty_from_normal(const PsSensorModel &s, const double (&normal)[3], double (&cov)[3][3])
{
    double n[3] = {normal[0], normal[1], normal[2]}, y[3], x[3];
    const double e[3] = {1.0, 0.0, 0.0};
    cross(n, e, y);
    normalize(n);
    cross(y, n, x);
    normalize(x);
    from_basis(x, y, n, 2, s.scaleUncertaintyNormal, cov);
}
inline void uncertainty_from_rgb_gradient(const PsSensorModel &s, const double (&grad)[3], double (&cov)[3][3])
{
    double y[3], z[3];
    const double e[3] = {0.0, 0.0, 1.0};
    cross(e, grad, y);
    normalize(y);
    cross(y, grad, z);
    normalize(z);
    from_basis(grad, y, z, 1, s.scaleUncertaintyGradient, cov);
}

// One feature as FeaturesMap::addMeasurements sees it: normal, gradient (im.p may be null: not computed) and info (row-major 9),
// canonical NaNs.  What ps_uncertainty.h's unc_row writes.
inline void feature(const Camera &c, const DepthImage &d, const ColourImage &im, const PsSensorModel &s, const int32_t *tie, int model, float u,
                    float v, float z, double *normalOut, double *gradientOut, double *infoOut)
{
    int pu = 0, pv = 0;
    if (!pixel_of(u, v, pu, pv)) {
        const double q = canon(std::nan(""));
        for (int i = 0; i < 3; ++i) {
            if (normalOut) normalOut[i] = q;
            if (gradientOut) gradientOut[i] = q;
        }
        if (infoOut)
            for (int i = 0; i < 9; ++i) infoOut[i] = q;
        return;
    }
    double n[3] = {0, 0, 0}, g[3] = {0, 0, 0};
    if (normalOut || (infoOut && model == 1)) normal(c, d, pu, pv, n);
    if (im.p && (gradientOut || (infoOut && model == 2))) gradient(c, d, im, tie, pu, pv, g);
    for (int i = 0; i < 3; ++i) {
        if (normalOut) normalOut[i] = canon(n[i]);
        if (gradientOut) gradientOut[i] = canon(g[i]);
    }
    if (!infoOut) return;
    double info[3][3], cov[3][3];
    if (model == 0) {
        info_image_coordinates(s, (double)u, (double)v, (double)z, info);
    } else if (model == 1) {
        uncertainty_from_normal(s, n, cov);
        inverse(cov, info);
    } else if (model == 2) {
        uncertainty_from_rgb_gradient(s, g, cov);
        inverse(cov, info);
    } else {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) info[i][j] = i == j ? 1.0 : 0.0;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) infoOut[3 * i + j] = canon(info[i][j]);
}

} // namespace unc_host
