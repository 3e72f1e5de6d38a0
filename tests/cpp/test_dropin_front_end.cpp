// FrameMatcherHIP::frontEnd (Matcher::detectInitFeatures, matcher.cpp:19-49, as one call) on cv::Mat-shaped images -- a CV_8UC3 or
// CV_8UC1 image and a CV_16U depth image, both regions of parent Mats with their steps -- against the C ABI (ps_front_end_frame on the
// same bytes): descriptors, 3-D points, all six cv::KeyPoint fields and the undistorted positions.  Then as the frontEnd callable of
// putslam_matcher_glue.h: putslam_hip::detectInitFeatures / putslam_hip::match on two sensor frames return what
// FrameMatcher::detectInitFeatures / match return on the rows frontEnd made.  Another detector or descriptor is refused.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "putslam_dropin.h"
#include "putslam_hip.h"
#include "putslam_matcher_glue.h"

namespace {

uint64_t g_state = 0x2545F4914F6CDD1Dull;
int below(int n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((g_state >> 33) % (uint64_t)n);
}

// what Matcher::match reads of a SensorFrame (include/putslam/Defs/putslam_defs.h)
struct SensorFrame {
    cv::Mat rgbImage, depthImage;
    double depthImageScale = 5000.0;
};

// a parent image and a parent depth image with a frame inside each; dx, dy move the scene
struct Frame {
    std::vector<unsigned char> rgbParent, depthParent;
    SensorFrame s;
};

void make_frame(Frame &f, const std::vector<unsigned char> &canvas, int canvasCols, int rows, int cols, int cn, int dx, int dy)
{
    const size_t step = (size_t)cols * cn + 10, dstep = (size_t)cols * 2 + 6;
    f.rgbParent.assign(step * (size_t)(rows + 4), 0xEE);
    f.depthParent.assign(dstep * (size_t)(rows + 2), 0xEE);
    f.s.rgbImage = cv::Mat(rows, cols, cn == 3 ? CV_8UC3 : CV_8UC1, f.rgbParent.data() + 2 * step + 5, step);
    f.s.depthImage = cv::Mat(rows, cols, CV_16U, f.depthParent.data() + dstep + 2, dstep);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const size_t at = (size_t)(y + dy) * canvasCols + (size_t)(x + dx);
            for (int c = 0; c < cn; ++c) f.s.rgbImage.data[(size_t)y * step + (size_t)x * cn + c] = (unsigned char)(canvas[at] + 29 * c);
            // a tilted plane that moves with the scene; every 11th pixel has no depth
            const int xs = x + dx, ys = y + dy;
            f.s.depthImage.at<uint16_t>(y, x) = (xs * 7 + ys * 3) % 11 == 0 ? (uint16_t)0 : (uint16_t)(5000 + 20 * xs + 9 * ys);
        }
}

// rectangles of random grey on a grey ground, a little noise on top: a canvas larger than the frames cut out of it
std::vector<unsigned char> make_canvas(int rows, int cols, int rects)
{
    std::vector<unsigned char> m((size_t)rows * cols, 100);
    for (int r = 0; r < rects; ++r) {
        const int x0 = below(cols), y0 = below(rows), w = 2 + below(cols / 5), h = 2 + below(rows / 5);
        const unsigned char v = (unsigned char)below(200);
        for (int y = y0; y < y0 + h && y < rows; ++y)
            for (int x = x0; x < x0 + w && x < cols; ++x) m[(size_t)y * cols + x] = v;
    }
    for (auto &v : m) v = (unsigned char)(v + below(9));
    return m;
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

void configure(putslam_hip::FrameMatcherHIP &m, int gridCols, int maxFeatures)
{
    auto &p = m.matcherParameters;
    p.OpenCVParams.gridCols = gridCols;
    p.OpenCVParams.maximalTrackedFeatures = maxFeatures;
    p.OpenCVParams.DBScanEps = 3.0;
    const float K[9] = {210.f, 0.f, 99.5f, 0.f, 208.f, 74.5f, 0.f, 0.f, 1.f}; // a camera whose image is 200 x 150
    for (int i = 0; i < 9; ++i) p.cameraMatrixMat.at<float>(i / 3, i % 3) = K[i];
}

int run_case(const char *name, int cn, int gridCols, int maxFeatures, int minFound)
{
    const int rows = 150, cols = 200;
    const std::vector<unsigned char> canvas = make_canvas(rows + 8, cols + 8, 170);
    Frame f;
    make_frame(f, canvas, cols + 8, rows, cols, cn, 0, 0);

    putslam_hip::FrameMatcherHIP matcher;
    const auto &mp = matcher.matcherParameters;
    bool ok = mp.OpenCVParams.DBScanEps == 1.0 && mp.distortionCoeffsMat.cols == 5 && mp.distortionCoeffsMat.at<float>(0, 1) == 0.3286f; // as shipped
    configure(matcher, gridCols, maxFeatures);
    cv::Mat desc;
    std::vector<Eigen::Vector3f> pts;
    std::vector<cv::KeyPoint> kps;
    std::vector<cv::Point2f> und;
    matcher.frontEnd(f.s.rgbImage, f.s.depthImage, f.s.depthImageScale, desc, pts, &kps, &und);

    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("%s: no context\n", name);
        return 1;
    }
    PsFrontEndParams prm;
    std::memset(&prm, 0, sizeof prm);
    prm.detect = {500, 1.2f, 8, 20, 1, gridCols, maxFeatures, 0};
    prm.describe.scaleFactor = 1.2f;
    prm.describe.nLevels = 8;
    prm.DBScanEps = 3.0;
    PsFrameGeometry geo;
    const float K[9] = {210.f, 0.f, 99.5f, 0.f, 208.f, 74.5f, 0.f, 0.f, 1.f};
    std::memcpy(geo.K, K, sizeof K);
    for (int i = 0; i < 5; ++i) geo.dist5[i] = (double)mp.distortionCoeffsMat.at<float>(0, i);
    geo.depthImageScale = f.s.depthImageScale;
    const size_t room = (size_t)maxFeatures;
    std::vector<unsigned char> wdesc(room * 32);
    std::vector<float> wpts(room * 3), wxy(room * 2), wund(room * 2), wang(room), wresp(room);
    std::vector<int32_t> woct(room);
    PsFrameRowsOut out;
    std::memset(&out, 0, sizeof out);
    out.pts = wpts.data(), out.xy = wxy.data(), out.xyUndist = wund.data(), out.angle = wang.data(), out.response = wresp.data(), out.octave = woct.data();
    int n = -1;
    const int rc = ps_front_end_frame(ctx, f.s.rgbImage.data, reinterpret_cast<const uint16_t *>(f.s.depthImage.data), rows, cols, cn, f.s.rgbImage.step,
                                      f.s.depthImage.step, &prm, nullptr, &geo, wdesc.data(), &out, maxFeatures, &n);
    if (rc != PS_OK) {
        std::printf("%s: C ABI failed: %s\n", name, ps_last_error(ctx));
        ps_context_destroy(ctx);
        return 1;
    }
    ps_context_destroy(ctx);
    ok = ok && n >= minFound && (n == 0 ? desc.empty() : (desc.rows == n && desc.cols == 32)) && (int)pts.size() == n && (int)kps.size() == n &&
         (int)und.size() == n;
    int levels = 0, missing = 0;
    for (int j = 0; ok && j < n; ++j) {
        const cv::KeyPoint &kp = kps[(size_t)j];
        const size_t J = (size_t)j;
        ok = std::memcmp(desc.data + J * desc.step, wdesc.data() + J * 32, 32) == 0 && same_bits(pts[J][0], wpts[3 * J]) &&
             same_bits(pts[J][1], wpts[3 * J + 1]) && same_bits(pts[J][2], wpts[3 * J + 2]) && same_bits(kp.pt.x, wxy[2 * J]) &&
             same_bits(kp.pt.y, wxy[2 * J + 1]) && same_bits(und[J].x, wund[2 * J]) && same_bits(und[J].y, wund[2 * J + 1]) &&
             same_bits(kp.angle, wang[J]) && same_bits(kp.response, wresp[J]) && kp.octave == woct[J] && kp.class_id == -1 &&
             same_bits(kp.size, 31.f * (float)std::pow((double)1.2f, (double)woct[J]));
        levels |= 1 << kp.octave;
        missing += pts[J][2] == 0.f ? 1 : 0;
    }
    std::printf("%s: %s (%d rows, level mask %d, %d without depth)\n", name, ok ? "ok" : "MISMATCH", n, levels, missing);
    return ok ? 0 : 1;
}

// the glue's templates with frontEnd as their callable = the matcher's own calls on the rows frontEnd made
int run_glue()
{
    const int rows = 150, cols = 200;
    const std::vector<unsigned char> canvas = make_canvas(rows + 8, cols + 8, 170);
    Frame a, b;
    make_frame(a, canvas, cols + 8, rows, cols, 3, 0, 0);
    make_frame(b, canvas, cols + 8, rows, cols, 3, 3, 2);

    putslam_hip::FrameMatcherHIP viaGlue, byHand, front;
    for (putslam_hip::FrameMatcherHIP *m : {&viaGlue, &byHand, &front}) {
        configure(*m, 1, 300);
        m->setSampleSeed(77);
    }
    auto callable = [&](const SensorFrame &s, cv::Mat &d, std::vector<Eigen::Vector3f> &p) {
        viaGlue.frontEnd(s.rgbImage, s.depthImage, s.depthImageScale, d, p);
    };
    Eigen::Matrix4f T1, T2;
    std::vector<cv::DMatch> in1, in2;
    putslam_hip::detectInitFeatures(viaGlue, a.s, callable);
    const double r1 = putslam_hip::match(viaGlue, b.s, callable, T1, in1);

    cv::Mat da, db;
    std::vector<Eigen::Vector3f> pa, pb;
    front.frontEnd(a.s.rgbImage, a.s.depthImage, a.s.depthImageScale, da, pa);
    front.frontEnd(b.s.rgbImage, b.s.depthImage, b.s.depthImageScale, db, pb);
    byHand.detectInitFeatures(da, pa);
    const double r2 = byHand.match(db, pb, T2, in2);

    bool ok = r1 == r2 && r1 > 0.0 && in1.size() == in2.size() && in1.size() >= 10 && std::memcmp(T1.data(), T2.data(), 64) == 0 &&
              viaGlue.getNumberOfFeatures() == (int)pb.size();
    for (size_t i = 0; ok && i < in1.size(); ++i) ok = in1[i].queryIdx == in2[i].queryIdx && in1[i].trainIdx == in2[i].trainIdx;
    // the scene moved by (3, 2) pixels on a plane about a metre away: a translation of centimetres, no identity
    ok = ok && (T1(0, 3) != 0.f || T1(1, 3) != 0.f);
    std::printf("glue: %s (ratio %.3f, %zu inliers of %zu and %zu rows, t = %.4f %.4f %.4f)\n", ok ? "ok" : "MISMATCH", r1, in1.size(), pa.size(),
                pb.size(), T1(0, 3), T1(1, 3), T1(2, 3));
    return ok ? 0 : 1;
}

// SURF and SIFT are refused loudly with empty outputs; a depth image of another type or size too; maximalTrackedFeatures 0 is silent
int run_refusals()
{
    const int rows = 150, cols = 200;
    const std::vector<unsigned char> canvas = make_canvas(rows + 8, cols + 8, 60);
    Frame f;
    make_frame(f, canvas, cols + 8, rows, cols, 1, 0, 0);
    putslam_hip::FrameMatcherHIP m;
    configure(m, 1, 100);
    cv::Mat desc(3, 32, CV_8U);
    std::vector<Eigen::Vector3f> pts(5);
    std::vector<cv::KeyPoint> kps(5);
    std::vector<cv::Point2f> und(5);
    auto empty = [&]() { return desc.empty() && pts.empty() && kps.empty() && und.empty(); };
    auto refill = [&]() { desc = cv::Mat(3, 32, CV_8U), pts.resize(5), kps.resize(5), und.resize(5); };
    m.matcherParameters.OpenCVParams.detector = "SURF";
    m.frontEnd(f.s.rgbImage, f.s.depthImage, 5000.0, desc, pts, &kps, &und);
    bool ok = empty();
    refill();
    m.matcherParameters.OpenCVParams.detector = "ORB";
    m.matcherParameters.OpenCVParams.descriptor = "SIFT";
    m.frontEnd(f.s.rgbImage, f.s.depthImage, 5000.0, desc, pts, &kps, &und);
    ok = ok && empty();
    refill();
    m.matcherParameters.OpenCVParams.descriptor = "ORB";
    cv::Mat wrongType(rows, cols, CV_32F), wrongSize(rows - 1, cols, CV_16U);
    m.frontEnd(f.s.rgbImage, wrongType, 5000.0, desc, pts, &kps, &und);
    ok = ok && empty();
    refill();
    m.frontEnd(f.s.rgbImage, wrongSize, 5000.0, desc, pts, &kps, &und);
    ok = ok && empty();
    refill();
    m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 0; // nothing asked for: nothing said
    m.frontEnd(f.s.rgbImage, f.s.depthImage, 5000.0, desc, pts, &kps, &und);
    ok = ok && empty();
    std::printf("refusals: %s\n", ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run_case("colour regions with steps, grid 1 x 1, the shipped maximum", 3, 1, 500, 30);
    bad += run_case("grey regions with steps, grid 1 x 2", 1, 2, 120, 30);
    bad += run_case("one key point", 3, 1, 1, 1);
    bad += run_glue();
    bad += run_refusals();
    if (bad == 0) std::printf("all ok\n");
    return bad;
}
