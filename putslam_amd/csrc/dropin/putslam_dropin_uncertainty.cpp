// putslam_dropin_uncertainty.cpp -- the drop-in's measurement uncertainty (putslam_dropin.h): RGBD::computeNormal
// / computeRGBGradient over the C ABI, DepthSensorModel's covariances over the sequential restatement (csrc/ps_uncertainty_host.h),
// FrameMatcherHIP::measurementEdges.  A translation unit of its own beside putslam_dropin.cpp, whose calling thread's context it
// uses: a program that links putslam_dropin.cpp alone against a stand-in of the older C ABI stays as it was.
#include "putslam_dropin.h"

#include <cmath>
#include <iostream>

#include "putslam_hip.h"
#include "../ps_uncertainty_host.h"

namespace putslam_hip {
PsContext *dropinThreadContext(int *status);
void dropinReportError(const PsContext *ctx);
} // namespace putslam_hip

namespace {
PsContext *threadContext(int *status) { return putslam_hip::dropinThreadContext(status); }
void reportError(const PsContext *ctx) { putslam_hip::dropinReportError(ctx); }
} // namespace

namespace {

putslam_hip::Vec3 nanVec3()
{
    const double q = unc_host::canon(std::nan(""));
    return putslam_hip::Vec3(q, q, q);
}

// K of a 3 x 3 CV_32F camera matrix (zeros without one), as the drop-in's other calls read it
PsFrameGeometry geometryOf(const cv::Mat &cameraMatrix, double depthImageScale)
{
    PsFrameGeometry g{};
    if (!cameraMatrix.empty() && cameraMatrix.rows >= 3 && cameraMatrix.cols >= 3)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) g.K[3 * r + c] = cameraMatrix.at<float>(r, c);
    g.depthImageScale = depthImageScale;
    return g;
}

std::vector<putslam_hip::Vec3> toVec3(const std::vector<double> &flat)
{
    std::vector<putslam_hip::Vec3> out(flat.size() / 3);
    for (size_t i = 0; i < out.size(); ++i) out[i] = putslam_hip::Vec3(flat[3 * i], flat[3 * i + 1], flat[3 * i + 2]);
    return out;
}

void toRows(const putslam_hip::Mat33 &m, double (&r)[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[i][j] = m(i, j);
}

putslam_hip::Mat33 fromRows(const double (&r)[3][3])
{
    putslam_hip::Mat33 m;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m(i, j) = r[i][j];
    return m;
}

} // namespace

#if !PUTSLAM_HAVE_CV_EIGEN
putslam_hip::Mat33 putslam_hip::Mat33::inverse() const
{
    double a[3][3], r[3][3];
    toRows(*this, a);
    unc_host::inverse(a, r);
    return fromRows(r);
}
#endif

std::vector<putslam_hip::Vec3> RGBD::normalsAt(const cv::Mat &depthImage, const std::vector<cv::Point2f> &px, const cv::Mat &cameraMatrix,
                                           double depthImageScale)
{
    std::vector<putslam_hip::Vec3> bad(px.size(), nanVec3());
    if (px.empty()) return bad;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return bad;
    const PsFrameGeometry g = geometryOf(cameraMatrix, depthImageScale);
    std::vector<double> flat(3 * px.size());
    status = ps_compute_normals(ctx, &g, reinterpret_cast<const uint16_t *>(depthImage.data), depthImage.rows, depthImage.cols, (size_t)depthImage.step,
                                reinterpret_cast<const float *>(px.data()), (int)px.size(), flat.data());
    if (status != PS_OK) {
        reportError(ctx);
        return bad;
    }
    return toVec3(flat);
}

std::vector<putslam_hip::Vec3> RGBD::gradientsAt(const cv::Mat &rgbImage, const cv::Mat &depthImage, const std::vector<cv::Point2f> &px,
                                             const cv::Mat &cameraMatrix, double depthImageScale)
{
    std::vector<putslam_hip::Vec3> bad(px.size(), nanVec3());
    if (px.empty()) return bad;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return bad;
    if (rgbImage.rows != depthImage.rows || rgbImage.cols != depthImage.cols) {
        std::cerr << "putslam_hip: computeRGBGradient: the colour image and the depth image differ in size" << std::endl;
        return bad;
    }
    const PsFrameGeometry g = geometryOf(cameraMatrix, depthImageScale);
    std::vector<double> flat(3 * px.size());
    status = ps_compute_rgb_gradients(ctx, &g, rgbImage.data, rgbImage.channels(), (size_t)rgbImage.step,
                                      reinterpret_cast<const uint16_t *>(depthImage.data), depthImage.rows, depthImage.cols, (size_t)depthImage.step,
                                      reinterpret_cast<const float *>(px.data()), (int)px.size(), flat.data());
    if (status != PS_OK) {
        reportError(ctx);
        return bad;
    }
    return toVec3(flat);
}

putslam_hip::Vec3 RGBD::computeNormal(const cv::Mat &depthImage, int u, int v, const cv::Mat &cameraMatrix, double depthImageScale)
{
    return normalsAt(depthImage, std::vector<cv::Point2f>(1, cv::Point2f((float)u, (float)v)), cameraMatrix, depthImageScale)[0];
}

putslam_hip::Vec3 RGBD::computeRGBGradient(const cv::Mat &rgbImage, const cv::Mat &depthImage, int u, int v, const cv::Mat &cameraMatrix,
                                       double depthImageScale)
{
    return gradientsAt(rgbImage, depthImage, std::vector<cv::Point2f>(1, cv::Point2f((float)u, (float)v)), cameraMatrix, depthImageScale)[0];
}

DepthSensorModel::Config::Config()
{
    PsSensorModel s;
    unc_sensor_default(s);
    focalLength[0] = s.fu, focalLength[1] = s.fv, focalAxis[0] = s.cu, focalAxis[1] = s.cv, varU = s.varU, varV = s.varV;
    distVarCoefs[0] = s.c3, distVarCoefs[1] = s.c2, distVarCoefs[2] = s.c1, distVarCoefs[3] = s.c0;
    scaleUncertaintyNormal = s.scaleUncertaintyNormal, scaleUncertaintyGradient = s.scaleUncertaintyGradient;
}

namespace {
// the C ABI's block of a Config's numbers
PsSensorModel sensorOf(const DepthSensorModel::Config &config)
{
    const PsSensorModel s = {config.focalLength[0], config.focalLength[1], config.focalAxis[0],    config.focalAxis[1],
                             config.varU,           config.varV,           config.distVarCoefs[0], config.distVarCoefs[1],
                             config.distVarCoefs[2], config.distVarCoefs[3], config.scaleUncertaintyNormal, config.scaleUncertaintyGradient};
    return s;
}
} // namespace

void DepthSensorModel::computeCov(uint_fast16_t u, uint_fast16_t v, double depth, putslam_hip::Mat33 &cov)
{
    double c[3][3];
    unc_host::compute_cov(sensorOf(config), (double)u, (double)v, depth, c);
    cov = fromRows(c);
}

putslam_hip::Mat33 DepthSensorModel::informationMatrixFromImageCoordinates(double u, double v, double z)
{
    double info[3][3];
    unc_host::info_image_coordinates(sensorOf(config), u, v, z, info); // (a u or v the reference's cast is undefined for: NaN)
    return fromRows(info);
}

putslam_hip::Mat33 DepthSensorModel::uncertinatyFromNormal(const putslam_hip::Vec3 &normal)
{
    const double n[3] = {normal.x(), normal.y(), normal.z()};
    double cov[3][3];
    unc_host::uncertainty_from_normal(sensorOf(config), n, cov);
    return fromRows(cov);
}

putslam_hip::Mat33 DepthSensorModel::uncertinatyFromRGBGradient(const putslam_hip::Vec3 &grad)
{
    const double g[3] = {grad.x(), grad.y(), grad.z()};
    double cov[3][3];
    unc_host::uncertainty_from_rgb_gradient(sensorOf(config), g, cov);
    return fromRows(cov);
}

namespace putslam_hip {

std::vector<FrameMatcherHIP::MeasurementEdge> FrameMatcherHIP::measurementEdges(const std::vector<cv::DMatch> &inlierMatches,
                                                                                const std::vector<cv::Point2f> &undistorted,
                                                                                const std::vector<Eigen::Vector3f> &features3D, cv::Mat rgbImage,
                                                                                cv::Mat depthImage, double depthImageScale, DepthSensorModel &sensor,
                                                                                int uncertaintyModel)
{
    std::vector<MeasurementEdge> out;
    const size_t n = inlierMatches.size();
    if (n == 0) return out;
    std::vector<cv::Point2f> uv(n);
    std::vector<float> pts(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const int t = inlierMatches[i].trainIdx;
        if (t < 0 || (size_t)t >= undistorted.size() || (size_t)t >= features3D.size()) {
            std::cerr << "putslam_hip: measurementEdges: a trainIdx outside the frame's rows" << std::endl;
            return out;
        }
        uv[i] = undistorted[(size_t)t];
        for (int k = 0; k < 3; ++k) pts[3 * i + (size_t)k] = features3D[(size_t)t][k];
    }
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return out;
    if (rgbImage.rows != depthImage.rows || rgbImage.cols != depthImage.cols) {
        std::cerr << "putslam_hip: measurementEdges: the colour image and the depth image differ in size" << std::endl;
        return out;
    }
    const PsFrameGeometry g = geometryOf(matcherParameters.cameraMatrixMat, depthImageScale);
    const PsSensorModel s = sensorOf(sensor.config);
    const uint16_t *depth = reinterpret_cast<const uint16_t *>(depthImage.data);
    std::vector<double> normal(3 * n), gradient(3 * n), info(9 * n);
    status = ps_compute_normals(ctx, &g, depth, depthImage.rows, depthImage.cols, (size_t)depthImage.step, reinterpret_cast<const float *>(uv.data()),
                                (int)n, normal.data());
    if (status == PS_OK)
        status = ps_compute_rgb_gradients(ctx, &g, rgbImage.data, rgbImage.channels(), (size_t)rgbImage.step, depth, depthImage.rows, depthImage.cols,
                                          (size_t)depthImage.step, reinterpret_cast<const float *>(uv.data()), (int)n, gradient.data());
    if (status == PS_OK)
        status = ps_information_matrices(ctx, &g, &s, uncertaintyModel, rgbImage.data, rgbImage.channels(), (size_t)rgbImage.step, depth,
                                         depthImage.rows, depthImage.cols, (size_t)depthImage.step, reinterpret_cast<const float *>(uv.data()),
                                         pts.data(), (int)n, info.data());
    if (status != PS_OK) {
        reportError(ctx);
        return out;
    }
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
        MeasurementEdge &e = out[i];
        e.mapRow = inlierMatches[i].queryIdx;
        e.curRow = inlierMatches[i].trainIdx;
        e.u = uv[i].x, e.v = uv[i].y;
        e.position = putslam_hip::Vec3((double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]);
        e.normal = putslam_hip::Vec3(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
        e.RGBgradient = putslam_hip::Vec3(gradient[3 * i], gradient[3 * i + 1], gradient[3 * i + 2]);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) e.info(r, c) = info[9 * i + 3 * (size_t)r + (size_t)c];
    }
    return out;
}

} // namespace putslam_hip
