// The drop-in's measurement uncertainty (putslam_dropin.h: RGBD::computeNormal / computeRGBGradient and their templates,
// DepthSensorModel, FrameMatcherHIP::measurementEdges) against the C ABI on a context of its own: the drop-in's bytes are the C
// ABI's.  A 40 x 30 RGB-D frame that is a region of larger images, 25 % holes in the depth; every pixel and some named positions.
// Built by build() next to the other drop-in tests; tests/test_gpu_dropin_uncertainty.py runs it on the GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <list>
#include <vector>

#include "putslam_dropin.h"
#include "putslam_hip.h"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

struct Feature { // "anything with u, v, normal, RGBgradient" (MapFeature's four members)
    float u, v;
    putslam_hip::Vec3 normal, RGBgradient;
};

static PsSensorModel sensorOf(const DepthSensorModel::Config &c)
{
    const PsSensorModel s = {c.focalLength[0], c.focalLength[1], c.focalAxis[0],    c.focalAxis[1],    c.varU, c.varV, c.distVarCoefs[0], c.distVarCoefs[1],
                             c.distVarCoefs[2], c.distVarCoefs[3], c.scaleUncertaintyNormal, c.scaleUncertaintyGradient};
    return s;
}
static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double canon(double x)
{
    if (x == x) return x;
    const uint64_t b = 0x7FF8000000000000ull;
    std::memcpy(&x, &b, 8);
    return x;
}
static bool sameVec(const putslam_hip::Vec3 &a, const double *b)
{
    const double v[3] = {canon(a.x()), canon(a.y()), canon(a.z())};
    return std::memcmp(v, b, 24) == 0;
}
static bool sameMat(const putslam_hip::Mat33 &m, const double *rowMajor)
{
    double v[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) v[3 * r + c] = canon(m(r, c));
    return std::memcmp(v, rowMajor, 72) == 0;
}

int main()
{
    const int rows = 30, cols = 40;
    uint32_t seed = 12345u;
    cv::Mat dparent(rows + 3, cols + 6, CV_16U), iparent(rows + 4, cols + 9, CV_8UC3);
    for (int r = 0; r < dparent.rows; ++r)
        for (int c = 0; c < dparent.cols; ++c) dparent.at<uint16_t>(r, c) = (lcg(seed) >> 8) % 4 == 0 ? 0 : (uint16_t)(2000 + (lcg(seed) >> 8) % 9000);
    for (size_t i = 0; i < (size_t)iparent.rows * iparent.step; ++i) iparent.data[i] = (unsigned char)(lcg(seed) >> 16);
    cv::Mat depth(rows, cols, CV_16U, dparent.data + 1 * dparent.step + 2 * 2, dparent.step);
    cv::Mat rgb(rows, cols, CV_8UC3, iparent.data + 2 * iparent.step + 5 * 3, iparent.step);
    cv::Mat K(3, 3, CV_32FC1);
    K.at<float>(0, 0) = 41.f, K.at<float>(1, 1) = 39.5f, K.at<float>(0, 2) = 19.5f, K.at<float>(1, 2) = 14.5f, K.at<float>(2, 2) = 1.f;
    const double scale = 5000.0;

    std::vector<cv::Point2f> px;
    for (int v = 0; v < rows; ++v)
        for (int u = 0; u < cols; ++u) px.push_back(cv::Point2f((float)u, (float)v));
    const float named[][2] = {{3.7f, 5.2f}, {-0.5f, 3.f}, {NAN, 4.f}, {3e9f, 2.f}, {(float)cols, 5.f}, {5.f, (float)rows}, {-3.f, -1.f}};
    for (const auto &p : named) px.push_back(cv::Point2f(p[0], p[1]));
    const int n = (int)px.size();
    std::vector<float> pts(3 * (size_t)n);
    for (auto &p : pts) p = (float)((lcg(seed) >> 8) % 12000) / 5000.f;

    // the C ABI on a context of its own
    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("no device\n");
        return 2;
    }
    PsFrameGeometry g{};
    g.K[0] = 41.f, g.K[4] = 39.5f, g.K[2] = 19.5f, g.K[5] = 14.5f, g.K[8] = 1.f;
    g.depthImageScale = scale;
    DepthSensorModel::Config cfg;
    PsSensorModel def;
    CHECK(ps_sensor_model_default(&def) == PS_OK);
    const PsSensorModel fromCfg = sensorOf(cfg);
    CHECK(std::memcmp(&def, &fromCfg, sizeof def) == 0); // Config()'s defaults are the C ABI's
    cfg.scaleUncertaintyNormal = 3.0, cfg.scaleUncertaintyGradient = 0.25;
    DepthSensorModel sensor(cfg);
    const PsSensorModel s = sensorOf(cfg);
    const uint16_t *dp = reinterpret_cast<const uint16_t *>(depth.data);
    std::vector<double> normal(3 * (size_t)n), grad(3 * (size_t)n), info[4];
    CHECK(ps_compute_normals(ctx, &g, dp, rows, cols, depth.step, &px[0].x, n, normal.data()) == PS_OK);
    CHECK(ps_compute_rgb_gradients(ctx, &g, rgb.data, 3, rgb.step, dp, rows, cols, depth.step, &px[0].x, n, grad.data()) == PS_OK);
    for (int model = -1; model <= 2; ++model) {
        info[model + 1].resize(9 * (size_t)n);
        CHECK(ps_information_matrices(ctx, &g, &s, model, rgb.data, 3, rgb.step, dp, rows, cols, depth.step, &px[0].x, pts.data(), n,
                                      info[model + 1].data()) == PS_OK);
    }

    // the batch forms and the templates, over a vector and over a list
    const std::vector<putslam_hip::Vec3> nAll = RGBD::normalsAt(depth, px, K, scale), gAll = RGBD::gradientsAt(rgb, depth, px, K, scale);
    int finite = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(sameVec(nAll[(size_t)i], &normal[3 * (size_t)i]) && sameVec(gAll[(size_t)i], &grad[3 * (size_t)i]));
        finite += nAll[(size_t)i].x() == nAll[(size_t)i].x();
    }
    CHECK(finite > n / 2 && finite < n);
    std::vector<Feature> fv((size_t)n);
    std::list<Feature> fl;
    for (int i = 0; i < n; ++i) {
        fv[(size_t)i].u = px[(size_t)i].x, fv[(size_t)i].v = px[(size_t)i].y;
        if (std::fabs(px[(size_t)i].x) < 1e6f) fl.push_back(fv[(size_t)i]); // (the template's (int) cast is the reference's: defined values only)
    }
    std::vector<Feature> fdef;
    for (const Feature &f : fl) fdef.push_back(f);
    RGBD::computeNormals(depth, fdef, K, scale);
    RGBD::computeRGBGradients(rgb, depth, fdef, K, scale);
    RGBD::computeNormals(depth, fl, K, scale);
    RGBD::computeRGBGradients(rgb, depth, fl, K, scale);
    size_t j = 0;
    auto it = fl.begin();
    for (int i = 0; i < n; ++i) {
        if (!(std::fabs(px[(size_t)i].x) < 1e6f)) continue;
        CHECK(sameVec(fdef[j].normal, &normal[3 * (size_t)i]) && sameVec(fdef[j].RGBgradient, &grad[3 * (size_t)i]));
        CHECK(sameVec(it->normal, &normal[3 * (size_t)i]) && sameVec(it->RGBgradient, &grad[3 * (size_t)i]));
        ++j, ++it;
    }
    // the single-feature forms, on a stride of pixels
    for (int i = 0; i < rows * cols; i += 37) {
        const int u = i % cols, v = i / cols;
        CHECK(sameVec(RGBD::computeNormal(depth, u, v, K, scale), &normal[3 * (size_t)i]));
        CHECK(sameVec(RGBD::computeRGBGradient(rgb, depth, u, v, K, scale), &grad[3 * (size_t)i]));
    }

    // DepthSensorModel: the covariances' inverses are the C ABI's information matrices
    int checked = 0;
    for (int i = 0; i < n; ++i) {
        const float u = px[(size_t)i].x, v = px[(size_t)i].y;
        if (!(std::fabs(u) < 1e6f) || !(std::fabs(v) < 1e6f)) continue; // (rows the kernels give NaN for the pixel's sake)
        CHECK(sameMat(sensor.informationMatrixFromImageCoordinates((double)u, (double)v, (double)pts[3 * (size_t)i + 2]), &info[1][9 * (size_t)i]));
        CHECK(sameMat(sensor.uncertinatyFromNormal(nAll[(size_t)i]).inverse(), &info[2][9 * (size_t)i]));
        CHECK(sameMat(sensor.uncertinatyFromRGBGradient(gAll[(size_t)i]).inverse(), &info[3][9 * (size_t)i]));
        if (u >= 0 && v >= 0) {
            putslam_hip::Mat33 cov;
            sensor.computeCov((uint_fast16_t)u, (uint_fast16_t)v, (double)pts[3 * (size_t)i + 2], cov);
            CHECK(sameMat(cov.inverse(), &info[1][9 * (size_t)i]));
        }
        ++checked;
    }
    CHECK(checked >= rows * cols);

    // measurementEdges: inlier matches in their order, rows of the frame
    putslam_hip::FrameMatcherHIP matcher;
    matcher.matcherParameters.cameraMatrixMat = K;
    std::vector<Eigen::Vector3f> f3d((size_t)n);
    for (int i = 0; i < n; ++i) f3d[(size_t)i] = Eigen::Vector3f(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
    std::vector<cv::DMatch> inl;
    for (int k = 0; k < 300; ++k) inl.push_back(cv::DMatch((int)((lcg(seed) >> 8) % 777), (int)((lcg(seed) >> 8) % (uint32_t)n), -1, 1.f));
    for (int model = -1; model <= 2; ++model) {
        const auto edges = matcher.measurementEdges(inl, px, f3d, rgb, depth, scale, sensor, model);
        CHECK(edges.size() == inl.size());
        for (size_t k = 0; k < edges.size(); ++k) {
            const size_t t = (size_t)inl[k].trainIdx;
            const auto &e = edges[k];
            CHECK(e.mapRow == inl[k].queryIdx && e.curRow == inl[k].trainIdx && std::memcmp(&e.u, &px[t].x, 4) == 0 && std::memcmp(&e.v, &px[t].y, 4) == 0);
            const double pos[3] = {(double)pts[3 * t], (double)pts[3 * t + 1], (double)pts[3 * t + 2]};
            CHECK(sameVec(e.position, pos) && sameVec(e.normal, &normal[3 * t]) && sameVec(e.RGBgradient, &grad[3 * t]));
            CHECK(sameMat(e.info, &info[model + 1][9 * t]));
        }
    }
    CHECK(matcher.measurementEdges(std::vector<cv::DMatch>(1, cv::DMatch(0, n, -1, 0.f)), px, f3d, rgb, depth, scale, sensor, 0).empty());
    ps_context_destroy(ctx);
    if (failures) return 1;
    std::printf("dropin uncertainty ok: %d rows, %d finite normals\n", n, finite);
    return 0;
}
