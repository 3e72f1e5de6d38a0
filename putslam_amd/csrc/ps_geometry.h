// ps_geometry.h -- the stand-alone geometry of the C ABI: the float Umeyama fit of point sets (ps_umeyama_f32), KabschEst in
// double precision (ps_kabsch_f64; reference src/TransformEst/kabschEst.cpp), RGBD's back-projection, undistortion and projection
// (ps_keypoints2Dto3D, ps_remove_image_distortion, ps_points3Dto2D; reference src/RGBD/RGBD.cpp).  The depth rule, point_from_depth
// and undistort_point are shared with ps_frame_assembly.h.
#pragma once
#include "ps_block.h" // kBlock
#include "ps_device_math.h"
#include "ps_glue.h"
#include "ps_select_refit.h" // wave_umeyama, store_pose

namespace psdev {

// ------------------------------------------------------------------------------------------
// Stand-alone fits
// ------------------------------------------------------------------------------------------
// ps_umeyama_f32: one wavefront per point set.
__global__ __launch_bounds__(64) void ps_umeyama_sets(const float *__restrict__ src, const float *__restrict__ dst,
                                                      int k, int nsets, float *__restrict__ T,
                                                      int32_t *__restrict__ valid)
{
    const int s = blockIdx.x;
    if (s >= nsets) return;
    const float *sp = src + (size_t)s * k * 3;
    const float *dp = dst + (size_t)s * k * 3;
    Rigid m;
    auto get = [&](int j, float4 &u, float4 &v) {
        u = make_float4(sp[3 * j], sp[3 * j + 1], sp[3 * j + 2], dp[3 * j]);
        v = make_float4(dp[3 * j + 1], dp[3 * j + 2], 0.0f, 0.0f);
    };
    bool ok = wave_umeyama(k, 0, get, get, m);
    if ((threadIdx.x & 63) == 0) {
        store_pose(T + (size_t)s * 16, m);
        valid[s] = ok ? 1 : 0;
    }
}

PS_D double wave_tree_sum_f64(double v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}

// The handedness of the Kabsch rotation.  The reference takes sign(A.determinant()) of the covariance (kabschEst.cpp:53; 1 for
// a determinant of 0): for a covariance of full rank that is the sign of det(V) det(W), and the only rule that differs is
// meaningless -- for a planar, collinear or three-point set the determinant is rounding noise (or exactly 0) and says nothing
// about the handedness of W V^T, so the reference returns a reflection for about every second such set.  Here the sign comes
// from the factors themselves, as Eigen::umeyama takes it: det(W diag(1, 1, d) V^T) = +1 for every input.
PS_D double kabsch_handedness(const double (&V)[3][3], const double (&W)[3][3])
{
    return (det3(V) * det3(W) < 0.0) ? -1.0 : 1.0;
}

// KabschEst::computeTransformation (reference src/TransformEst/kabschEst.cpp:24-68), double precision.
// A, B: n x 3 column-major with leading dimension ld.  One wavefront.
__global__ __launch_bounds__(64) void ps_kabsch_f64_kernel(const double *__restrict__ A, const double *__restrict__ B,
                                                           int n, int ld, double *__restrict__ T)
{
    const int lane = threadIdx.x & 63;
    double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    for (int i = lane; i < n; i += 64) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sa[c] += A[(size_t)c * ld + i];
            sb[c] += B[(size_t)c * ld + i];
        }
    }
    double cA[3], cB[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cA[c] = wave_tree_sum_f64(sa[c]) / (double)n;
        cB[c] = wave_tree_sum_f64(sb[c]) / (double)n;
    }
    double acc[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[r][c] = 0.0;
    for (int i = lane; i < n; i += 64) {
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[c] = A[(size_t)c * ld + i] - cA[c];
            b[c] = B[(size_t)c * ld + i] - cB[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[r][c] += a[r] * b[c];
    }
    double Am[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Am[r][c] = wave_tree_sum_f64(acc[r][c]);
    double V[3][3], W[3][3], S[3];
    jacobi_svd3<double>(Am, V, S, W); // V = svd.matrixU(), W = svd.matrixV()  (kabschEst.cpp:48-49)
    double d = kabsch_handedness(V, W);
    double R[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = (W[i][0] * V[j][0] + W[i][1] * V[j][1]) + (W[i][2] * d) * V[j][2];
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
        if (n > 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double ti = (R[i][0] * (-cA[0]) + (R[i][1] * (-cA[1]) + R[i][2] * (-cA[2]))) + cB[i];
#pragma unroll
                for (int j = 0; j < 3; ++j) T[4 * j + i] = R[i][j];
                T[12 + i] = ti;
            }
        }
    }
}

// Large point sets: the same arithmetic spread over G wavefronts (one 64-lane work-group each, strided like the
// single-wave kernel's lanes), partial sums combined in wave order by every wave / by the finishing wave.  The
// summation tree is a function of (n, G) only: tests/kabsch_tree_ref.py restates it (lane-strided sequential partial sums,
// the shuffle tree, per-wave partials added in wave order, each product rounded before it is added) and the pose equals that
// restatement byte for byte, for this form and the single-wave one.  The oracle's sequential sums are another order: the two
// poses agree only as far as the data's conditioning lets them (1e-15 on centred clouds, 1e-8 a million units from the origin).
//   pass 1: part[g][0..5]  = column sums of A, B over the wave's points
//   pass 2: part2[g][0..8] = sum (a - cA)(b - cB)^T over the wave's points, cA / cB from all part[] in order
//   finish: one wave adds part2[] in order, SVD, pose
__global__ __launch_bounds__(64) void ps_kabsch_f64_sums(const double *__restrict__ A, const double *__restrict__ B, int n,
                                                         int ld, double *__restrict__ part)
{
    const int lane = threadIdx.x & 63, g = blockIdx.x, G = gridDim.x;
    double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    for (long long i = (long long)g * 64 + lane; i < n; i += (long long)G * 64) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sa[c] += A[(size_t)c * ld + i];
            sb[c] += B[(size_t)c * ld + i];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double va = wave_tree_sum_f64(sa[c]), vb = wave_tree_sum_f64(sb[c]);
        if (lane == 0) {
            part[(size_t)g * 6 + c] = va;
            part[(size_t)g * 6 + 3 + c] = vb;
        }
    }
}

PS_D void kabsch_means(const double *__restrict__ part, int G, int n, double (&cA)[3], double (&cB)[3])
{
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int g = 0; g < G; ++g) // every lane of every wave: the same order, the same values
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] += part[(size_t)g * 6 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cA[c] = s[c] / (double)n;
        cB[c] = s[3 + c] / (double)n;
    }
}

__global__ __launch_bounds__(64) void ps_kabsch_f64_cov(const double *__restrict__ A, const double *__restrict__ B, int n,
                                                        int ld, const double *__restrict__ part,
                                                        double *__restrict__ part2)
{
    const int lane = threadIdx.x & 63, g = blockIdx.x, G = gridDim.x;
    double cA[3], cB[3];
    kabsch_means(part, G, n, cA, cB);
    double acc[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[r][c] = 0.0;
    for (long long i = (long long)g * 64 + lane; i < n; i += (long long)G * 64) {
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[c] = A[(size_t)c * ld + i] - cA[c];
            b[c] = B[(size_t)c * ld + i] - cB[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[r][c] += a[r] * b[c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double v = wave_tree_sum_f64(acc[r][c]);
            if (lane == 0) part2[(size_t)g * 9 + 3 * r + c] = v;
        }
}

__global__ __launch_bounds__(64) void ps_kabsch_f64_finish(const double *__restrict__ part, const double *__restrict__ part2,
                                                           int G, int n, double *__restrict__ T)
{
    const int lane = threadIdx.x & 63;
    double cA[3], cB[3];
    kabsch_means(part, G, n, cA, cB);
    double Am[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            for (int g = 0; g < G; ++g) v += part2[(size_t)g * 9 + 3 * r + c];
            Am[r][c] = v;
        }
    double V[3][3], W[3][3], S[3];
    jacobi_svd3<double>(Am, V, S, W);
    double d = kabsch_handedness(V, W);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double R[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) R[j] = (W[i][0] * V[j][0] + W[i][1] * V[j][1]) + (W[i][2] * d) * V[j][2];
            double ti = (R[0] * (-cA[0]) + (R[1] * (-cA[1]) + R[2] * (-cA[2]))) + cB[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) T[4 * j + i] = R[j];
            T[12 + i] = ti;
        }
    }
}

// RGBD::keypoints2Dto3D / point2Dto3D / roundSize (reference src/RGBD/RGBD.cpp:10-16,30-65).
PS_D int round_size(double x, int size)
{
    if (x < 0)
        x = 0;
    else if (x > size - 1)
        x = size; // sic: the reference clamps to size, not size-1
    return (int)round(x);
}
// ONE statement of the depth read's rule and ONE of point2Dto3D's arithmetic, shared by ps_backproject and ps_assemble_rows
// (ps_frame_assembly.h).  depth_rule_offset: the byte offset of the rounded pixel in an image whose rows lie `step` bytes apart and
// whose addressable bytes end at `bytes`; false where there is no pixel to read (depth 0 = missing).
PS_D bool depth_rule_offset(float x, float y, int rows, int cols, size_t step, size_t bytes, size_t &off)
{
    // A NaN coordinate has no pixel (the reference's (int)round(NaN) is undefined): depth 0 (= missing).
    if (!(x == x && y == y)) return false;
    int uR = round_size((double)x, cols), vR = round_size((double)y, rows);
    off = (size_t)vR * step + (size_t)uR * 2;
    // cv::Mat::at is plain pointer arithmetic: u == cols in a row that is not the last reads what follows that row's
    // pixels (the parent image's next pixel for a region, the next row's first pixel for a dense image).  `bytes` =
    // depth_view_bytes(rows, cols, step) is where the last row's pixels end: from there on the reference reads out of
    // bounds, here that is depth 0 (= missing).
    return off + 2 <= bytes;
}
PS_D unsigned depth_pixel(const uint8_t *__restrict__ at) { return (unsigned)at[0] | ((unsigned)at[1] << 8); }
PS_D void point_from_depth(float x, float y, unsigned dv, float fx, float fy, float cx, float cy, double scale, float &X, float &Y, float &Z)
{
    Z = (float)(((double)dv) / scale);
    float u = (x - cx) / fx;
    float v = (y - cy) / fy;
    X = u * Z;
    Y = v * Z;
}
__global__ __launch_bounds__(kBlock) void ps_backproject(const float *__restrict__ xy, int n,
                                                         const uint8_t *__restrict__ depth, int rows, int cols,
                                                         size_t step, size_t bytes, float fx, float fy, float cx,
                                                         float cy, double scale, float *__restrict__ out)
{
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float x = xy[2 * i], y = xy[2 * i + 1];
    size_t off = 0;
    const unsigned dv = depth_rule_offset(x, y, rows, cols, step, bytes, off) ? depth_pixel(depth + off) : 0u;
    float X, Y, Z;
    point_from_depth(x, y, dv, fx, fy, cx, cy, scale, X, Y, Z);
    out[3 * i] = X;
    out[3 * i + 1] = Y;
    out[3 * i + 2] = Z;
}

// RGBD::removeImageDistortion (reference src/RGBD/RGBD.cpp:254-314): cv::undistortPoints with R = P = I
// (OpenCV 3.x cvUndistortPoints: 5 fixed-point iterations of the Brown model, double precision) and
// u = x_n * fx + cx in float.
struct DistArgs {
    double k[5]; // k1 k2 p1 p2 k3
    float fx, fy, cx, cy;
};
// ONE statement of the iteration, shared by ps_undistort_kernel and ps_assemble_rows (ps_frame_assembly.h)
PS_D void undistort_point(float px, float py, const DistArgs &a, float &u, float &v)
{
    const double fx = (double)a.fx, fy = (double)a.fy, cx = (double)a.cx, cy = (double)a.cy;
    const double ifx = 1. / fx, ify = 1. / fy;
    const double k0 = a.k[0], k1 = a.k[1], k2 = a.k[2], k3 = a.k[3], k4 = a.k[4];
    const double z = 0.0; // k[5..11] of OpenCV's 12-coefficient form: absent in the reference's configs
    double x = (double)px, y = (double)py;
    double x0 = x = (x - cx) * ifx;
    double y0 = y = (y - cy) * ify;
    for (int j = 0; j < 5; ++j) {
        double r2 = x * x + y * y;
        double icdist = (1 + ((z * r2 + z) * r2 + z) * r2) / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x) + z * r2 + z * r2 * r2;
        double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y + z * r2 + z * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    float xn = (float)x, yn = (float)y;
    u = xn * a.fx + a.cx;
    v = yn * a.fy + a.cy;
}
__global__ __launch_bounds__(kBlock) void ps_undistort_kernel(const float *__restrict__ xy, int n, DistArgs a,
                                                              float *__restrict__ out)
{
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float u, v;
    undistort_point(xy[2 * i], xy[2 * i + 1], a, u, v);
    out[2 * i] = u;
    out[2 * i + 1] = v;
}

__global__ __launch_bounds__(kBlock) void ps_project_kernel(const float *__restrict__ xyz, int n, float fx, float fy,
                                                            float cx, float cy, float *__restrict__ uv)
{
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float u, v;
    project(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], fx, fy, cx, cy, u, v);
    uv[2 * i] = u;
    uv[2 * i + 1] = v;
}

} // namespace psdev

extern "C" {

// ---------------------------------------------------------------------------------------------
int ps_umeyama_f32(PsContext *ctx, const float *src, const float *dst, int k, int nsets, float *T, int32_t *valid)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (k < 0 || nsets < 0 || !T || !valid || (k > 0 && nsets > 0 && (!src || !dst)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_umeyama_f32: bad argument");
    if (nsets == 0) return PS_OK;
    size_t bytes = (size_t)nsets * (k > 0 ? k : 1) * 12;
    PS_ENSURE(ctx->sMisc0, bytes);
    PS_ENSURE(ctx->sMisc1, bytes);
    PS_ENSURE(ctx->sPose, (size_t)nsets * 16 * sizeof(float));
    PS_ENSURE(ctx->sMisc2, (size_t)nsets * sizeof(int32_t));
    if (k > 0) {
        PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, src, (size_t)nsets * k * 12, hipMemcpyHostToDevice, ctx->stream));
        PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, dst, (size_t)nsets * k * 12, hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(ps_umeyama_sets, dim3((unsigned)nsets), dim3(64), 0, ctx->stream, (const float *)ctx->sMisc0.p,
                       (const float *)ctx->sMisc1.p, k, nsets, (float *)ctx->sPose.p, (int32_t *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(T, ctx->sPose.p, (size_t)nsets * 16 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipMemcpyAsync(valid, ctx->sMisc2.p, (size_t)nsets * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_kabsch_f64(PsContext *ctx, const double *A, const double *B, int n, int ld, double *T)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (T)
        for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!T || n < 0 || (n > 0 && (!A || !B || ld < n))) return fail(ctx, PS_ERR_BAD_ARG, "ps_kabsch_f64: bad argument");
    if (n == 0) return PS_OK; // kabschEst.cpp:28
    size_t bytes = (size_t)3 * ld * sizeof(double);
    PS_ENSURE(ctx->sMisc0, bytes);
    PS_ENSURE(ctx->sMisc1, bytes);
    PS_ENSURE(ctx->sMisc2, (16 + (size_t)15 * 1024) * sizeof(double)); // pose + per-wave partial sums
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, A, bytes - (size_t)(ld - n) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, B, bytes - (size_t)(ld - n) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n <= 16384) { // one wavefront: lowest latency (config 1 has 500 points)
        hipLaunchKernelGGL(ps_kabsch_f64_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double *)ctx->sMisc0.p,
                           (const double *)ctx->sMisc1.p, n, ld, (double *)ctx->sMisc2.p);
    } else { // G wavefronts, two passes over the points + a finishing wave
        int G = (n + 4095) / 4096;
        if (G > 1024) G = 1024;
        double *part = (double *)ctx->sMisc2.p + 16, *part2 = part + (size_t)6 * 1024;
        hipLaunchKernelGGL(ps_kabsch_f64_sums, dim3((unsigned)G), dim3(64), 0, ctx->stream, (const double *)ctx->sMisc0.p,
                           (const double *)ctx->sMisc1.p, n, ld, part);
        hipLaunchKernelGGL(ps_kabsch_f64_cov, dim3((unsigned)G), dim3(64), 0, ctx->stream, (const double *)ctx->sMisc0.p,
                           (const double *)ctx->sMisc1.p, n, ld, (const double *)part, part2);
        hipLaunchKernelGGL(ps_kabsch_f64_finish, dim3(1), dim3(64), 0, ctx->stream, (const double *)part,
                           (const double *)part2, G, n, (double *)ctx->sMisc2.p);
    }
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(T, ctx->sMisc2.p, 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

size_t ps_depth_view_bytes(int rows, int cols, size_t depthStep) { return depth_view_bytes(rows, cols, depthStep); }

int ps_keypoints2Dto3D(PsContext *ctx, const float *xy, int n, const uint16_t *depth, int rows, int cols,
                       size_t depthStep, const float *K, double depthImageScale, float *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n < 0 || rows <= 0 || cols <= 0 || !depth || !K || depthStep < (size_t)cols * 2 || (n > 0 && (!xy || !out)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_keypoints2Dto3D: bad argument");
    if (n == 0) return PS_OK;
    const size_t bytes = depth_view_bytes(rows, cols, depthStep); // not rows x depthStep: the last row ends after its pixels
    PS_ENSURE(ctx->sMisc0, (size_t)n * 8);
    PS_ENSURE(ctx->sMisc1, bytes);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 12);
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, depth, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ps_backproject, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, n, (const uint8_t *)ctx->sMisc1.p, rows, cols, depthStep, bytes, K[0],
                       K[4], K[2], K[5], depthImageScale, (float *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(out, ctx->sMisc2.p, (size_t)n * 12, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_remove_image_distortion(PsContext *ctx, const float *xy, int n, const float *K, const double *dist5, float *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n < 0 || !K || !dist5 || (n > 0 && (!xy || !out)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_remove_image_distortion: bad argument");
    if (n == 0) return PS_OK;
    PS_ENSURE(ctx->sMisc0, (size_t)n * 8);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 8);
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    DistArgs a;
    for (int i = 0; i < 5; ++i) a.k[i] = dist5[i];
    a.fx = K[0]; a.fy = K[4]; a.cx = K[2]; a.cy = K[5];
    hipLaunchKernelGGL(ps_undistort_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, n, a, (float *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(out, ctx->sMisc2.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_points3Dto2D(PsContext *ctx, const float *xyz, int n, const float *K, float *uv)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n < 0 || !K || (n > 0 && (!xyz || !uv))) return fail(ctx, PS_ERR_BAD_ARG, "ps_points3Dto2D: bad argument");
    if (n == 0) return PS_OK;
    PS_ENSURE(ctx->sMisc0, (size_t)n * 12);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 8);
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ps_project_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, n, K[0], K[4], K[2], K[5], (float *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(uv, ctx->sMisc2.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

} // extern "C"
