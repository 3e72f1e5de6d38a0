// ps_uncertainty.h -- the measurement uncertainty of the frame loop on the device (include/putslam_hip.h: "Measurement
// uncertainty"): per feature the surface normal (RGBD::computeNormal, src/RGBD/RGBD.cpp:101-144), the
// colour-gradient direction (RGBD::computeRGBGradient, :147-187) and the 3 x 3 information matrix of its Edge3D
// (FeaturesMap::addFeatures / addMeasurements, src/Map/featuresMap.cpp:110-121,261-274, over DepthSensorModel::computeCov,
// informationMatrixFromImageCoordinates, uncertinatyFromNormal, uncertinatyFromRGBGradient and normalizeVector,
// src/Grabber/depthSensorModel.cpp:27-36,55-101).  Part of the device translation unit (ps_capi.hip), after ps_frame_assembly.h,
// whose back_project_in_frame is every point2Dto3D here.
// ONE row body, unc_row, and two kernels around it:
//  * ps_uncertainty_rows: one thread per row, a grid of row blocks x row sets, no LDS (ps_feature_uncertainty and the host forms);
//  * ps_measurement_edges_rows: one work-group per pair.  The pair's inlier mask is compacted in tiles of 256 by ps_block.h's flag
//    scan -- no atomics, the order is part of the result --, the tile's inliers are listed in LDS, and lanes 0 .. total-1 take one
//    each: the waves of a tile are full or idle, not sparsely lit.
// Everything is double arithmetic with each operation rounded separately (the translation unit forbids contraction); division and
// square root are the correctly rounded operators of ps_device_math.h.  A row holds at most two 3 x 3 double matrices and one
// product at a time, every index a compile-time constant: the compiler's report shows no scratch.
// Eigen's fixed-size 3 x 3 inverse (m3_inverse) is RESTATED, not compiled against an Eigen: no Eigen was at hand, so that reading
// is unpinned.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ps_block.h"
#include "ps_device_math.h"
#include "ps_glue.h"
#include "ps_uncertainty_rule.h" // the sensor defaults, the tie table, the argument rule: pure host arithmetic

namespace psdev {

// what a row needs beside its own columns
struct UncArgs {
    PsSensorModel s;
    double scale;                          // depthImageScale
    float fx, fy, cx, cy;                  // K
    const uint8_t *depth, *img;            // frame 0 of either set; img null: no images
    size_t dRow, dFrame, iRow, iFrame;     // resolved strides
    int rows, cols, dFrames, iFrames, model;
    unsigned long long tie;                // ps_debug_gradient_tie_table(1): entry k as value + 1 in bits 2k, 2k + 1
};

// the match list a pair's rows come from
struct EdgeArgs {
    const int32_t *imageFrame, *pairs, *numMatches;
    const PsDMatch *matches;
    const uint8_t *mask;
    const float *pts;
    const float2 *xyUndist;
    size_t ptsStride;                      // floats between frames
    int numMaps, numFrames, maxKpts, maxMatches;
};

PS_D double unc_nan() { return __builtin_bit_cast(double, 0x7FF8000000000000ull); }
PS_D double unc_canon(double x) { return x != x ? unc_nan() : x; }

// (int)u, (int)v where the truncation and its two neighbours fit an int: |coordinate| < 2^31, which for a float is <= 2147483520
PS_D bool unc_pixel(float u, float v, int &pu, int &pv)
{
    const float lim = 2147483520.0f;
    if (!(u >= -lim && u <= lim && v >= -lim && v <= lim)) return false; // (a NaN fails)
    pu = (int)u;
    pv = (int)v;
    return true;
}

PS_D void unc_point(const UncArgs &a, const uint8_t *__restrict__ dframe, int pu, int pv, float &X, float &Y, float &Z)
{
    back_project_in_frame(make_float2((float)pu, (float)pv), a.fx, a.fy, a.cx, a.cy, a.scale, dframe, a.dRow, a.rows, a.cols, X, Y, Z);
}

// x / n, y / n, z / n for n = sqrt((x x + y y) + z z): Eigen's norm() of a Vector3d and normalizeVector's three divisions
PS_D void unc_normalize(double &x, double &y, double &z)
{
    const double n = ps_sqrt((x * x + y * y) + z * z);
    x = x / n;
    y = y / n;
    z = z / n;
}

// uidx / vidx of RGBD.cpp:105-106, plus one, two bits each
constexpr unsigned unc_pack8(int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7)
{
    return (unsigned)(a0 + 1) | (unsigned)(a1 + 1) << 2 | (unsigned)(a2 + 1) << 4 | (unsigned)(a3 + 1) << 6 | (unsigned)(a4 + 1) << 8 |
           (unsigned)(a5 + 1) << 10 | (unsigned)(a6 + 1) << 12 | (unsigned)(a7 + 1) << 14;
}
constexpr unsigned kUncUidx = unc_pack8(-1, -1, -1, 0, 1, 1, 1, 0), kUncVidx = unc_pack8(-1, 0, 1, 1, 1, 0, -1, -1);

// RGBD::computeNormal.  The list of kept vectors is walked once: the cross product of each with its predecessor as it arrives,
// the last with the first at the end -- the list's order and the sum's
PS_D void unc_normal(const UncArgs &a, const uint8_t *__restrict__ dframe, int u, int v, double &nx, double &ny, double &nz)
{
    float cX, cY, cZ;
    unc_point(a, dframe, u, v, cX, cY, cZ);
    double fx = 0, fy = 0, fz = 0, px = 0, py = 0, pz = 0; // the first kept vector, the previous one
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int kept = 0;
    for (int i = 0; i < 8; ++i) {
        const int du = (int)((kUncUidx >> (2 * i)) & 3u) - 1, dv = (int)((kUncVidx >> (2 * i)) & 3u) - 1;
        float X, Y, Z;
        unc_point(a, dframe, u + du, v + dv, X, Y, Z);
        if (Z > 0) {
            const double x = (double)(X - cX), y = (double)(Y - cY), z = (double)(Z - cZ);
            if (kept == 0) {
                fx = x, fy = y, fz = z;
            } else {
                sx += py * z - pz * y;
                sy += pz * x - px * z;
                sz += px * y - py * x;
            }
            px = x, py = y, pz = z;
            ++kept;
        }
    }
    if (kept > 0) {
        sx += py * fz - pz * fy;
        sy += pz * fx - px * fz;
        sz += px * fy - py * fx;
    }
    const double n = (double)kept;
    nx = sx / n;
    ny = sy / n;
    nz = sz / n;
    unc_normalize(nx, ny, nz);
}

// RGBD::computeRGBGradient.  iframe: the 3-channel frame
PS_D void unc_gradient(const UncArgs &a, const uint8_t *__restrict__ dframe, const uint8_t *__restrict__ iframe, int u, int v, double &gx,
                      double &gy, double &gz)
{
    if (!((u - 1 > 0) && (v - 1 > 0) && (u + 1 < a.cols) && (v + 1 < a.rows))) {
        gx = gy = gz = 1.0;
        return;
    }
    // at<uint16_t>(r, c) of the patch of an 8-bit 3-channel image: two bytes at (v-1+r) x rowStride + (u-1) x 3 + 2 c
    const uint8_t *p0 = iframe + (size_t)(v - 1) * a.iRow + (size_t)(u - 1) * 3, *p1 = p0 + a.iRow, *p2 = p1 + a.iRow;
#define UNC_AT(row, c) ((int)depth_pixel((row) + 2 * (c)))
    const int gradx = -3 * UNC_AT(p0, 0) - 10 * UNC_AT(p0, 1) - 3 * UNC_AT(p0, 2) + 3 * UNC_AT(p2, 0) + 10 * UNC_AT(p2, 1) + 3 * UNC_AT(p2, 2);
    const int grady = -3 * UNC_AT(p0, 0) - 10 * UNC_AT(p1, 0) - 3 * UNC_AT(p2, 0) + 3 * UNC_AT(p0, 2) + 10 * UNC_AT(p1, 2) + 3 * UNC_AT(p2, 2);
#undef UNC_AT
    const int ax = gradx < 0 ? -gradx : gradx, ay = grady < 0 ? -grady : grady;
    int c1x, c1y, c2x, c2y;
    if (ax == ay) { // a tie: the host's libm decided
        const int t = gradx == 0 ? 0 : (gradx > 0 ? (grady > 0 ? 1 : 4) : (grady > 0 ? 2 : 3));
        const unsigned w = (unsigned)(a.tie >> (8 * t));
        c1x = (int)(w & 3u) - 1, c1y = (int)((w >> 2) & 3u) - 1, c2x = (int)((w >> 4) & 3u) - 1, c2y = (int)((w >> 6) & 3u) - 1;
    } else {
        c1x = ax > ay ? (gradx > 0 ? 1 : -1) : 0;
        c1y = ay > ax ? (grady > 0 ? -1 : 1) : 0;
        c2x = -c1x, c2y = -c1y;
    }
    float cX, cY, cZ, eX, eY, eZ, bX, bY, bZ;
    unc_point(a, dframe, u, v, cX, cY, cZ);
    unc_point(a, dframe, u + c1x, v + c1y, eX, eY, eZ);
    unc_point(a, dframe, u + c2x, v + c2y, bX, bY, bZ);
    if (eZ > 0 && bZ != 0.f) {
        gx = (double)(eX - bX), gy = (double)(eY - bY), gz = (double)(eZ - bZ);
    } else if (cZ > 0 && bZ != 0.f) {
        gx = (double)(cX - bX), gy = (double)(cY - bY), gz = (double)(cZ - bZ);
    } else if (cZ > 0 && eZ != 0.f) {
        gx = (double)(eX - cX), gy = (double)(eY - cY), gz = (double)(eZ - cZ);
    } else {
        gx = (double)c1x, gy = (double)c1y, gz = 0.0;
    }
    unc_normalize(gx, gy, gz);
}

// ---- 3 x 3 double matrices, row-major, every product dense: structural zeros are multiplied (0 x NaN matters) ----
PS_D void m3_mul(const double (&A)[3][3], const double (&B)[3][3], double (&C)[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}
// C = A * B^T
PS_D void m3_mul_bt(const double (&A)[3][3], const double (&B)[3][3], double (&C)[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i][j] = (A[i][0] * B[j][0] + A[i][1] * B[j][1]) + A[i][2] * B[j][2];
}
template <int I, int J> PS_D double m3_cofactor(const double (&m)[3][3])
{
    constexpr int i1 = (I + 1) % 3, i2 = (I + 2) % 3, j1 = (J + 1) % 3, j2 = (J + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
}
// the project's reading of Eigen 3's compute_inverse_size3: result(i, j) = cof(j, i) x (1 / det)
PS_D void m3_inverse(const double (&m)[3][3], double (&r)[3][3])
{
    const double c00 = m3_cofactor<0, 0>(m), c10 = m3_cofactor<1, 0>(m), c20 = m3_cofactor<2, 0>(m);
    const double det = (c00 * m[0][0] + c10 * m[1][0]) + c20 * m[2][0];
    const double invdet = 1.0 / det;
    r[0][0] = c00 * invdet, r[0][1] = c10 * invdet, r[0][2] = c20 * invdet;
    r[1][0] = m3_cofactor<0, 1>(m) * invdet, r[1][1] = m3_cofactor<1, 1>(m) * invdet, r[1][2] = m3_cofactor<2, 1>(m) * invdet;
    r[2][0] = m3_cofactor<0, 2>(m) * invdet, r[2][1] = m3_cofactor<1, 2>(m) * invdet, r[2][2] = m3_cofactor<2, 2>(m) * invdet;
}
// (((R S) S) R^-1)^-1 for S = the identity with S(D, D) = s
template <int D> PS_D void unc_info_from_basis(const double (&R)[3][3], double s, double (&info)[3][3])
{
    double S[3][3], T[3][3], U[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = i == j ? (i == D ? s : 1.0) : 0.0;
    m3_mul(R, S, T);
    m3_mul(T, S, U);
    m3_inverse(R, S);
    m3_mul(U, S, T);
    m3_inverse(T, info);
}

// informationMatrixFromImageCoordinates(u, v, z)
PS_D void unc_info_model0(const PsSensorModel &s, float u, float v, float zf, double (&info)[3][3])
{
    const double ud0 = (double)u, vd0 = (double)v, two64 = 18446744073709551616.0;
    if (!(ud0 >= 0.0 && ud0 < two64 && vd0 >= 0.0 && vd0 < two64)) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) info[i][j] = unc_nan();
        return;
    }
    const double ud = (double)(unsigned long long)ud0, vd = (double)(unsigned long long)vd0, z = (double)zf;
    double J[3][3], R[3][3], T[3][3];
    J[0][0] = z / s.fu, J[0][1] = 0.0, J[0][2] = (ud / s.fu) - (s.cu / s.fu);
    J[1][0] = 0.0, J[1][1] = z / s.fv, J[1][2] = (vd / s.fv) - (s.cv / s.fv);
    J[2][0] = 0.0, J[2][1] = 0.0, J[2][2] = 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = 0.0;
    R[0][0] = s.varU;
    R[1][1] = s.varV;
    R[2][2] = ((s.c3 * (z * z * z) + s.c2 * (z * z)) + s.c1 * z) + s.c0; // z z and z z z: the correctly rounded powers of a float z
    m3_mul(J, R, T);
    m3_mul_bt(T, J, R);
    m3_inverse(R, info);
}

// uncertinatyFromNormal(normal).inverse(): y = normal x (1, 0, 0) is taken BEFORE the normalisation and never normalised itself
PS_D void unc_info_model1(const PsSensorModel &s, double nx, double ny, double nz, double (&info)[3][3])
{
    const double yx = ny * 0.0 - nz * 0.0, yy = nz * 1.0 - nx * 0.0, yz = nx * 0.0 - ny * 1.0;
    unc_normalize(nx, ny, nz);
    double xx = yy * nz - yz * ny, xy = yz * nx - yx * nz, xz = yx * ny - yy * nx;
    unc_normalize(xx, xy, xz);
    const double R[3][3] = {{xx, yx, nx}, {xy, yy, ny}, {xz, yz, nz}};
    unc_info_from_basis<2>(R, s.scaleUncertaintyNormal, info);
}

// uncertinatyFromRGBGradient(grad).inverse(): only S(1, 1) is set
PS_D void unc_info_model2(const PsSensorModel &s, double gx, double gy, double gz, double (&info)[3][3])
{
    double yx = 0.0 * gz - 1.0 * gy, yy = 1.0 * gx - 0.0 * gz, yz = 0.0 * gy - 0.0 * gx;
    unc_normalize(yx, yy, yz);
    double zx = yy * gz - yz * gy, zy = yz * gx - yx * gz, zz = yx * gy - yy * gx;
    unc_normalize(zx, zy, zz);
    const double R[3][3] = {{gx, yx, zx}, {gy, yy, zy}, {gz, yz, zz}};
    unc_info_from_basis<1>(R, s.scaleUncertaintyGradient, info);
}

PS_D void unc_store3(double *to, double x, double y, double z)
{
    to[0] = unc_canon(x);
    to[1] = unc_canon(y);
    to[2] = unc_canon(z);
}

// THE ROW BODY of both kernels: the row at (u, v) with depth coordinate z in image / depth frame `frame`; nOut / gOut / iOut: where
// the row's normal, gradient and information matrix go, null = not wanted
PS_D void unc_row(const UncArgs &a, int frame, float u, float v, float z, double *__restrict__ nOut, double *__restrict__ gOut,
                  double *__restrict__ iOut)
{
    int pu = 0, pv = 0;
    const bool inSets = frame >= 0 && frame < a.dFrames && (a.img == nullptr || frame < a.iFrames);
    if (!inSets || !unc_pixel(u, v, pu, pv)) {
        const double q = unc_nan();
        if (nOut) unc_store3(nOut, q, q, q);
        if (gOut) unc_store3(gOut, q, q, q);
        if (iOut)
            for (int k = 0; k < 9; ++k) iOut[k] = q;
        return;
    }
    const uint8_t *dframe = a.depth + (size_t)frame * a.dFrame;
    double nx = 0, ny = 0, nz = 0, gx = 0, gy = 0, gz = 0;
    if (nOut || (iOut && a.model == 1)) {
        unc_normal(a, dframe, pu, pv, nx, ny, nz);
        if (nOut) unc_store3(nOut, nx, ny, nz);
    }
    if (gOut || (iOut && a.model == 2)) {
        unc_gradient(a, dframe, a.img + (size_t)frame * a.iFrame, pu, pv, gx, gy, gz);
        if (gOut) unc_store3(gOut, gx, gy, gz);
    }
    if (iOut) {
        double info[3][3];
        if (a.model == 0)
            unc_info_model0(a.s, u, v, z, info);
        else if (a.model == 1)
            unc_info_model1(a.s, nx, ny, nz, info);
        else if (a.model == 2)
            unc_info_model2(a.s, gx, gy, gz, info);
        else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) info[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) iOut[3 * i + j] = unc_canon(info[i][j]);
    }
}

// Row j of set f; a count outside 0 .. cap: nothing written
__global__ __launch_bounds__(kBlock) void ps_uncertainty_rows(UncArgs a, const int32_t *__restrict__ imageFrame, const float2 *__restrict__ xy,
                                                              const float *__restrict__ pts, const int32_t *__restrict__ counts, int cap,
                                                              PsUncertaintyOut o)
{
    const int f = (int)blockIdx.y, j = (int)(blockIdx.x * kBlock + threadIdx.x);
    const int n = counts[f];
    if (n < 0 || n > cap || j >= n) return;
    const size_t to = (size_t)f * (size_t)cap + (size_t)j;
    const float2 q = xy[to];
    const float z = pts ? pts[3 * to + 2] : 0.f;
    unc_row(a, imageFrame[f], q.x, q.y, z, o.normal ? o.normal + 3 * to : nullptr, o.gradient ? o.gradient + 3 * to : nullptr,
            o.info ? o.info + 9 * to : nullptr);
}

// Pair blockIdx.x: its final inliers, in match-list order, to the first rows of every wanted array
__global__ __launch_bounds__(kBlock) void ps_measurement_edges_rows(UncArgs a, EdgeArgs e, PsMeasurementEdgesOut o)
{
    __shared__ int wsum[kBlock / 64];
    __shared__ int lst[kBlock];
    const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int m = e.numMatches[p], view = e.pairs[2 * p], fr = e.pairs[2 * p + 1];
    if (m <= 0 || m > e.maxMatches || view < 0 || view >= e.numMaps || fr < 0 || fr >= e.numFrames) { // (uniform over the work-group)
        if (tid == 0 && o.count) o.count[p] = 0;
        return;
    }
    const size_t pairBase = (size_t)p * (size_t)e.maxMatches;
    const int frame = e.imageFrame ? e.imageFrame[fr] : -1;
    int base = 0;
    for (int tile = 0; tile < m; tile += kBlock) {
        const int i = tile + tid;
        const bool flag = i < m && e.mask[pairBase + (size_t)i] != 0;
        int total = 0;
        const int pos = block_scan_flag<kBlock, true>(flag, total, wsum);
        if (flag) lst[pos] = i;
        __syncthreads();
        if (tid < total) {
            const PsDMatch mt = e.matches[pairBase + (size_t)lst[tid]];
            const size_t to = pairBase + (size_t)(base + tid);
            const bool in = mt.trainIdx >= 0 && mt.trainIdx < e.maxKpts;
            float2 q = make_float2(__builtin_nanf(""), __builtin_nanf(""));
            float X = q.x, Y = q.x, Z = q.x;
            if (in) {
                const size_t row = (size_t)fr * (size_t)e.maxKpts + (size_t)mt.trainIdx;
                const float *pt = e.pts + (size_t)fr * e.ptsStride + 3 * (size_t)mt.trainIdx;
                q = e.xyUndist[row];
                X = pt[0], Y = pt[1], Z = pt[2];
            }
            if (o.mapRow) o.mapRow[to] = mt.queryIdx;
            if (o.curRow) o.curRow[to] = mt.trainIdx;
            if (o.uv) reinterpret_cast<float2 *>(o.uv)[to] = q;
            if (o.position) unc_store3(o.position + 3 * to, (double)X, (double)Y, (double)Z);
            if (o.normal || o.gradient || o.info)
                unc_row(a, frame, q.x, q.y, Z, o.normal ? o.normal + 3 * to : nullptr, o.gradient ? o.gradient + 3 * to : nullptr,
                        o.info ? o.info + 9 * to : nullptr);
        }
        base += total;
        // (lst is written again behind the next scan's barriers, which every thread reaches after it has read its entry)
    }
    if (tid == 0 && o.count) o.count[p] = base;
}

} // namespace psdev

// Host side: the checks, the launches and the entry points
namespace {

// geometry, sensor, model and the two sets as every call takes them (ps_uncertainty_rule.h's argument rule); `a` resolved.
// needImages: the gradient or model 2 is wanted; needSensor: an information matrix is
int unc_check(PsContext *ctx, const PsFrameGeometry *g, const PsSensorModel *sensor, int model, const PsImageSet *images, const PsDepthSet *depth,
              bool needImages, bool needSensor, const char *who, UncArgs &a)
{
    UncStrides st;
    const char *why = "";
    const int rc = unc_sets_error(g, sensor, model, images, depth, needImages, needSensor, st, why);
    if (rc) return fail(ctx, rc, (std::string(who) + ": " + why).c_str());
    a.dRow = st.dRow, a.dFrame = st.dFrame, a.iRow = st.iRow, a.iFrame = st.iFrame;
    a.img = images ? images->pixels : nullptr;
    a.iFrames = images ? images->numFrames : 0;
    a.s = sensor ? *sensor : PsSensorModel{};
    a.scale = g->depthImageScale;
    a.fx = g->K[0], a.fy = g->K[4], a.cx = g->K[2], a.cy = g->K[5];
    a.depth = reinterpret_cast<const uint8_t *>(depth->pixels);
    a.rows = depth->rows, a.cols = depth->cols, a.dFrames = depth->numFrames;
    a.model = model;
    int32_t tie[20];
    unc_tie_table(1, tie);
    a.tie = unc_tie_pack(tie);
    return PS_OK;
}

int unc_rows_launch(PsContext *ctx, const UncArgs &a, const int32_t *imageFrame, const float *xy, const float *pts, const int32_t *counts, int F,
                    int cap, const PsUncertaintyOut &out)
{
    hipLaunchKernelGGL(ps_uncertainty_rows, rows_grid(F, cap), dim3(kBlock), 0, ctx->stream, a, imageFrame, reinterpret_cast<const float2 *>(xy), pts,
                       counts, cap, out);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// One frame from HOST arrays: upload, one launch, download.  Any of normal / gradient / info may be null
int unc_host(PsContext *ctx, const PsFrameGeometry *g, const PsSensorModel *sensor, int model, const uint8_t *img, int channels, size_t rowStride,
             const uint16_t *depth, int rows, int cols, size_t depthStep, const float *xy, const float *pts, int n, double *normal, double *gradient,
             double *info, const char *who)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const auto msg = [who](const char *what) { return std::string(who) + what; };
    const bool needImages = gradient || (info && model == 2), needPts = info && model == 0;
    if (n < 0 || !depth || (n > 0 && (!xy || (needPts && !pts) || !(normal || gradient || info))))
        return fail(ctx, PS_ERR_BAD_ARG, msg(": null array or n < 0").c_str());
    if (n > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, msg(": more than PS_MAX_KPTS rows").c_str());
    if (needImages && !img) return fail(ctx, PS_ERR_BAD_ARG, msg(": the gradient needs the image").c_str());
    if (!needImages) img = nullptr;
    PsDepthSet ds{};
    ds.pixels = depth; // (the host array: checked for NULL only; the device copy is named below)
    ds.rowStride = depthStep;
    ds.numFrames = 1;
    ds.rows = rows;
    ds.cols = cols;
    PsImageSet is{};
    is.pixels = img;
    is.rowStride = rowStride;
    is.numFrames = 1;
    is.rows = rows;
    is.cols = cols;
    is.channels = channels;
    UncArgs a{};
    rc = unc_check(ctx, g, sensor, model, img ? &is : nullptr, &ds, needImages, info != nullptr, who, a);
    if (rc) return rc;
    if (n == 0) return PS_OK;
    TimingOff toff(ctx);
    const size_t N = (size_t)n, view = depth_view_bytes(rows, cols, a.dRow), imgBytes = img ? image_bytes(rows, cols, 3, a.iRow) : 0;
    // one block: the depth view | the image | xy | pts | counts | imageFrame | normal | gradient | info
    BlockLayout lay;
    const size_t oDepth = lay.take<uint16_t>(view / 2, 16), oImg = lay.take<uint8_t>(imgBytes, 16), oXy = lay.take<float2>(N, 16),
                 oPts = lay.take<float>(3 * N, 16), oCnt = lay.take<int32_t>(2, 16), oOut = lay.take<double>(15 * N, 16);
    const DeviceBlock blk(lay.total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    const int32_t head[2] = {n, 0};
    PS_HIP(hipMemcpyAsync(d + oDepth, depth, view, hipMemcpyHostToDevice, ctx->stream));
    if (img) PS_HIP(hipMemcpyAsync(d + oImg, img, imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oXy, xy, N * 8, hipMemcpyHostToDevice, ctx->stream));
    if (pts) PS_HIP(hipMemcpyAsync(d + oPts, pts, N * 12, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oCnt, head, sizeof head, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (pageable sources may change)
    a.depth = (const uint8_t *)(d + oDepth);
    a.img = img ? (const uint8_t *)(d + oImg) : nullptr;
    double *base = (double *)(d + oOut);
    PsUncertaintyOut dev{};
    dev.normal = normal ? base : nullptr;
    dev.gradient = gradient ? base + 3 * N : nullptr;
    dev.info = info ? base + 6 * N : nullptr;
    rc = unc_rows_launch(ctx, a, (const int32_t *)(d + oCnt) + 1, (const float *)(d + oXy), pts ? (const float *)(d + oPts) : nullptr,
                         (const int32_t *)(d + oCnt), 1, n, dev);
    if (rc) return rc;
    if (normal) PS_HIP(hipMemcpyAsync(normal, dev.normal, N * 24, hipMemcpyDeviceToHost, ctx->stream));
    if (gradient) PS_HIP(hipMemcpyAsync(gradient, dev.gradient, N * 24, hipMemcpyDeviceToHost, ctx->stream));
    if (info) PS_HIP(hipMemcpyAsync(info, dev.info, N * 72, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_sensor_model(void) { return sizeof(PsSensorModel); }
size_t ps_abi_sizeof_uncertainty_out(void) { return sizeof(PsUncertaintyOut); }
size_t ps_abi_sizeof_measurement_edges_out(void) { return sizeof(PsMeasurementEdgesOut); }

int ps_sensor_model_default(PsSensorModel *out)
{
    if (!out) return PS_ERR_BAD_ARG;
    unc_sensor_default(*out);
    return PS_OK;
}

int ps_debug_gradient_tie_table(int k, int32_t *table20)
{
    if (!table20 || k < 1) return PS_ERR_BAD_ARG;
    unc_tie_table(k, table20);
    return PS_OK;
}

int ps_feature_uncertainty(PsContext *ctx, const PsFrameGeometry *geometry, const PsSensorModel *sensor, int model, const PsImageSet *images,
                           const PsDepthSet *depth, const int32_t *imageFrame, const float *xy, const float *pts, const int32_t *counts, int F,
                           int capacity, const PsUncertaintyOut *out)
{
    static const char *who = "ps_feature_uncertainty";
    int rc = bind(ctx);
    if (rc) return rc;
    rc = rows_grid_check(ctx, F, capacity, who);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_feature_uncertainty: null output block");
    UncArgs a{};
    rc = unc_check(ctx, geometry, sensor, model, images, depth, out->gradient || (out->info && model == 2), out->info != nullptr, who, a);
    if (rc) return rc;
    if (F == 0) return PS_OK;
    if (!imageFrame || !xy || !counts || (out->info && model == 0 && !pts) || !(out->normal || out->gradient || out->info))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_feature_uncertainty: null array, or no output wanted");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return unc_rows_launch(ctx, a, imageFrame, xy, pts, counts, F, capacity, *out);
}

int ps_measurement_edges(PsContext *ctx, const PsFrameGeometry *geometry, const PsSensorModel *sensor, int model, const PsImageSet *images,
                         const PsDepthSet *depth, const int32_t *imageFrame, const PsMapBatch *b, const PsPairResults *res, const float *xyUndist,
                         const PsMeasurementEdgesOut *out)
{
    static const char *who = "ps_measurement_edges";
    int rc = bind(ctx);
    if (rc) return rc;
    if (!b || !res || !out) return fail(ctx, PS_ERR_BAD_ARG, "ps_measurement_edges: null batch, result block or output block");
    if (b->P < 0 || b->maxMatches < 1) return fail(ctx, PS_ERR_BAD_ARG, "ps_measurement_edges: P < 0 or maxMatches < 1");
    if (b->maxMatches > (1 << 22)) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_measurement_edges: maxMatches above 1 << 22");
    if (b->frames.maxKpts > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_measurement_edges: more than PS_MAX_KPTS keypoints per frame");
    if (!b->frames.pts || b->frames.maxKpts < 1 || b->frames.numFrames < 1 || b->maps.numFrames < 1)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_measurement_edges: bad frame set (null points, maxKpts or numFrames < 1)");
    FrameStrides fs;
    rc = frame_strides(ctx, b->frames, false, true, who, fs);
    if (rc) return rc;
    const bool rows = out->normal || out->gradient || out->info;
    UncArgs a{};
    rc = unc_check(ctx, geometry, sensor, model, images, depth, out->gradient || (out->info && model == 2), out->info != nullptr, who, a);
    if (rc) return rc;
    if (b->P == 0) return PS_OK;
    if (!b->pairs || !res->matches || !res->numMatches || !res->inlierMask || !xyUndist || (rows && !imageFrame))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_measurement_edges: null array");
    EdgeArgs e{};
    e.imageFrame = imageFrame;
    e.pairs = b->pairs;
    e.numMatches = res->numMatches;
    e.matches = res->matches;
    e.mask = res->inlierMask;
    e.pts = b->frames.pts;
    e.xyUndist = reinterpret_cast<const float2 *>(xyUndist);
    e.ptsStride = (size_t)fs.ptsFloats();
    e.numMaps = b->maps.numFrames;
    e.numFrames = b->frames.numFrames;
    e.maxKpts = b->frames.maxKpts;
    e.maxMatches = b->maxMatches;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    hipLaunchKernelGGL(ps_measurement_edges_rows, dim3((unsigned)b->P), dim3(kBlock), 0, ctx->stream, a, e, *out);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

int ps_compute_normals(PsContext *ctx, const PsFrameGeometry *geometry, const uint16_t *depth, int rows, int cols, size_t depthStep, const float *xy,
                       int n, double *normal)
{
    if (ctx && n > 0 && !normal) return fail(ctx, PS_ERR_BAD_ARG, "ps_compute_normals: null output");
    return unc_host(ctx, geometry, nullptr, -1, nullptr, 3, 0, depth, rows, cols, depthStep, xy, nullptr, n, normal, nullptr, nullptr,
                    "ps_compute_normals");
}

int ps_compute_rgb_gradients(PsContext *ctx, const PsFrameGeometry *geometry, const uint8_t *img, int channels, size_t rowStride,
                             const uint16_t *depth, int rows, int cols, size_t depthStep, const float *xy, int n, double *gradient)
{
    if (ctx && (!gradient || !img)) return fail(ctx, PS_ERR_BAD_ARG, "ps_compute_rgb_gradients: null image or output");
    return unc_host(ctx, geometry, nullptr, -1, img, channels, rowStride, depth, rows, cols, depthStep, xy, nullptr, n, nullptr, gradient, nullptr,
                    "ps_compute_rgb_gradients");
}

int ps_information_matrices(PsContext *ctx, const PsFrameGeometry *geometry, const PsSensorModel *sensor, int model, const uint8_t *img, int channels,
                            size_t rowStride, const uint16_t *depth, int rows, int cols, size_t depthStep, const float *xy, const float *pts, int n,
                            double *info)
{
    if (ctx && !info) return fail(ctx, PS_ERR_BAD_ARG, "ps_information_matrices: null output");
    return unc_host(ctx, geometry, sensor, model, img, channels, rowStride, depth, rows, cols, depthStep, xy, pts, n, nullptr, nullptr, info,
                    "ps_information_matrices");
}

} // extern "C"
