// FrameMatcherHIP::trackStep (the first half of Matcher::trackKLT, matcher.cpp:147-211) on cv::Mat-shaped inputs: its outputs equal
// what ps_track_vo_pair returns for the same pair, and what the reference's loop :151-211 gives when it is restated over the
// drop-in's own performTracking, RGBD::removeImageDistortion, RGBD::keypoints2Dto3D and RANSAC classes -- as bytes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <iostream>
#include <vector>

#include "putslam_dropin.h"
#include "putslam_hip.h"

namespace {

// a smooth texture sampled at (x + sx, y + sy): the pair (0, 0) / (-sx, -sy) carries the flow (sx, sy)
void texture(cv::Mat &m, int cn, double sx, double sy)
{
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols; ++x)
            for (int c = 0; c < cn; ++c) {
                const double u = x + sx, v = y + sy;
                const double t = std::cos(0.31 * u + 0.17 * v + c) + std::cos(0.11 * u - 0.29 * v + 2.0 * c) + std::cos(0.23 * u + 0.05 * v * c) +
                                 std::cos(0.07 * u * 0.5 + 0.37 * v);
                m.data[(size_t)y * m.step + (size_t)x * cn + c] = (unsigned char)std::lrint(127.5 + 30.0 * t);
            }
}

// a tilted plane 2 .. 4.5 m moved with the texture, with a block of zeros and a block beyond 6 m
void plane(cv::Mat &d, double sx, double sy)
{
    for (int y = 0; y < d.rows; ++y)
        for (int x = 0; x < d.cols; ++x) {
            const double u = x + sx, v = y + sy;
            double z = 10000.0 + 90.0 * u + 70.0 * v;
            if (u >= 10 && u < 22 && v >= 10 && v < 22) z = 0.0;
            if (u >= 50 && u < 62 && v >= 30 && v < 42) z = 32000.0;
            reinterpret_cast<uint16_t *>(d.data + (size_t)y * d.step)[x] = (uint16_t)std::lrint(z);
        }
}

uint64_t g_state = 0x2545F4914F6CDD1Dull;
float uniform(float lo, float hi)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (hi - lo) * (float)((g_state >> 40) & 0xFFFF) / 65535.0f;
}

bool same_bits(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

void configure(putslam_hip::FrameMatcherHIP &m, int errorVersionVO, double errThr, double minDist)
{
    auto &p = m.matcherParameters;
    const float K[9] = {110.f, 0.f, 39.5f, 0.f, 108.f, 29.5f, 0.f, 0.f, 1.f}; // a camera whose image is 80 x 60
    for (int i = 0; i < 9; ++i) p.cameraMatrixMat.at<float>(i / 3, i % 3) = K[i];
    p.OpenCVParams.trackingErrorThreshold = errThr;
    p.OpenCVParams.minimalReprojDistanceNewTrackingFeatures = minDist;
    p.RANSACParams.errorVersion = 3;              // (not the one the step may use)
    p.RANSACParams.errorVersionVO = errorVersionVO;
    m.setSampleSeed(41);
}

int run_case(const char *name, int cn, bool padded, int errorVersionVO, double errThr, double minDist, int n, bool expectAccepted)
{
    const int rows = 60, cols = 80;
    const double sx = 1.7, sy = -0.9, scale = 5000.0;
    const size_t step = (size_t)cols * cn + (padded ? 13 : 0);
    std::vector<unsigned char> bufA(step * rows, 0xEE), bufB(step * rows, 0xEE);
    std::vector<uint16_t> bufD0((size_t)rows * cols), bufD1((size_t)rows * cols);
    const int type = cn == 3 ? CV_8UC3 : CV_8UC1;
    cv::Mat prevImg(rows, cols, type, bufA.data(), step), img(rows, cols, type, bufB.data(), step);
    cv::Mat prevDepth(rows, cols, CV_16U, bufD0.data(), (size_t)cols * 2), depth(rows, cols, CV_16U, bufD1.data(), (size_t)cols * 2);
    texture(prevImg, cn, 0.0, 0.0);
    texture(img, cn, -sx, -sy);
    plane(prevDepth, 0.0, 0.0);
    plane(depth, -sx, -sy);

    putslam_hip::FrameMatcherHIP matcher, stepwise;
    configure(matcher, errorVersionVO, errThr, minDist);
    configure(stepwise, errorVersionVO, errThr, minDist);
    const auto &mp = matcher.matcherParameters;

    // the previous frame's rows
    std::vector<cv::Point2f> prevDistorted;
    std::vector<cv::KeyPoint> prevKeyPoints;
    std::vector<double> prevDetDists;
    for (int i = 0; i < n; ++i) {
        cv::Point2f p(uniform(-2.f, cols + 2.f), uniform(-2.f, rows + 2.f));
        if (i % 7 == 3 && i > 0) p = cv::Point2f(prevDistorted[(size_t)i - 1].x + 0.4f, prevDistorted[(size_t)i - 1].y); // a close neighbour
        prevDistorted.push_back(p);
        cv::KeyPoint kp;
        kp.pt = p;
        kp.octave = i % 5;
        kp.response = (float)i;
        kp.angle = 0.5f * (float)i;
        prevKeyPoints.push_back(kp);
        prevDetDists.push_back(1.0 + 0.01 * i);
    }
    std::vector<cv::Point2f> tmp = prevDistorted;
    std::vector<cv::Point2f> prevUndistorted = n ? RGBD::removeImageDistortion(tmp, mp.cameraMatrixMat, mp.distortionCoeffsMat) : tmp;
    std::vector<Eigen::Vector3f> prev3D = n ? RGBD::keypoints2Dto3D(prevUndistorted, prevDepth, mp.cameraMatrixMat, scale) : std::vector<Eigen::Vector3f>();

    // the drop-in's one call (stale content in every output: the call replaces it)
    std::vector<cv::Point2f> distorted(3), undistorted(2);
    std::vector<Eigen::Vector3f> features3D(4);
    std::vector<cv::KeyPoint> keyPoints(3);
    std::vector<double> detDists(5, -1.0);
    std::vector<cv::DMatch> matches(2), inliers(1);
    Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
    for (int i = 0; i < 16; ++i) T.data()[i] = 0.f;
    bool ok = matcher.trackStep(prevImg, img, depth, scale, prevDistorted, prev3D, prevKeyPoints, prevDetDists, distorted, undistorted, features3D,
                                keyPoints, detDists, matches, inliers, T);
    const int k = (int)matches.size();
    ok = ok && (int)distorted.size() == k && (int)undistorted.size() == k && (int)features3D.size() == k && (int)keyPoints.size() == k &&
         (int)detDists.size() == k && (int)prevDistorted.size() == n;

    // the C ABI on the same pair
    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("%s: no context\n", name);
        return 1;
    }
    const auto &cvp = mp.OpenCVParams;
    PsKltParams klt = {cvp.eps, cvp.trackingMinEigThreshold, cvp.winSize, cvp.maxLevels, cvp.maxIter, 0};
    PsTrackVoParams tp = {errThr, minDist, 0, 0};
    PsRansacParams prm;
    std::memset(&prm, 0, sizeof prm);
    const auto &rp = mp.RANSACParams;
    prm.verbose = rp.verbose;
    prm.errorVersion = errorVersionVO;
    prm.errorVersionVO = rp.errorVersionVO;
    prm.errorVersionMap = rp.errorVersionMap;
    prm.inlierThresholdEuclidean = rp.inlierThresholdEuclidean;
    prm.inlierThresholdReprojection = rp.inlierThresholdReprojection;
    prm.inlierThresholdMahalanobis = rp.inlierThresholdMahalanobis;
    prm.minimalInlierRatioThreshold = rp.minimalInlierRatioThreshold;
    prm.minimalNumberOfMatches = rp.minimalNumberOfMatches;
    prm.usedPairs = rp.usedPairs;
    prm.iterationCount = 487; // RANSAC.cpp:30 for 0.20
    PsRansacConfig cfg = {PS_EST_RANSAC, 487, 41, nullptr};
    PsFrameGeometry geo;
    for (int i = 0; i < 9; ++i) geo.K[i] = mp.cameraMatrixMat.at<float>(i / 3, i % 3);
    for (int i = 0; i < 5; ++i) geo.dist5[i] = (double)mp.distortionCoeffsMat.at<float>(0, i);
    geo.depthImageScale = scale;
    const size_t N = (size_t)(n ? n : 1);
    std::vector<float> next(2 * N), xy(2 * N), und(2 * N), pts(3 * N), ang(N), resp(N), pang(N), presp(N);
    std::vector<int32_t> keptIdx(N), oct(N), poct(N);
    std::vector<double> dist(N);
    std::vector<uint8_t> mask(N), status(N);
    std::vector<float> err(N);
    std::vector<PsDMatch> abi(N);
    for (int i = 0; i < n; ++i) {
        pang[(size_t)i] = prevKeyPoints[(size_t)i].angle;
        presp[(size_t)i] = prevKeyPoints[(size_t)i].response;
        poct[(size_t)i] = prevKeyPoints[(size_t)i].octave;
    }
    PsTrackVoIn in;
    std::memset(&in, 0, sizeof in);
    in.prevXY = (const float *)prevDistorted.data();
    in.prevPts = (const float *)prev3D.data();
    in.prev.angle = pang.data();
    in.prev.response = presp.data();
    in.prev.octave = poct.data();
    in.prev.detDist = prevDetDists.data();
    PsTrackVoOut out;
    std::memset(&out, 0, sizeof out);
    float pose[16];
    PsRansacStats st;
    out.nextPts = next.data();
    out.status = status.data();
    out.err = err.data();
    out.matches = abi.data();
    out.keptIdx = keptIdx.data();
    out.rows.xy = xy.data();
    out.rows.xyUndist = und.data();
    out.rows.pts = pts.data();
    out.rows.angle = ang.data();
    out.rows.response = resp.data();
    out.rows.octave = oct.data();
    out.rows.detDist = dist.data();
    out.inlierMask = mask.data();
    out.pose = pose;
    out.stats = &st;
    int kAbi = -1;
    int rc = ps_track_vo_pair(ctx, prevImg.data, img.data, (const uint16_t *)depth.data, rows, cols, cn, step, (size_t)depth.step, &klt, &tp, &prm,
                              &cfg, &geo, &in, n, &out, &kAbi);
    if (rc != PS_OK) {
        std::printf("%s: C ABI failed: %s\n", name, ps_last_error(ctx));
        ps_context_destroy(ctx);
        return 1;
    }
    ps_context_destroy(ctx);
    ok = ok && kAbi == k && same_bits(distorted.data(), xy.data(), (size_t)k * 8) && same_bits(undistorted.data(), und.data(), (size_t)k * 8) &&
         same_bits(features3D.data(), pts.data(), (size_t)k * 12) && same_bits(matches.data(), abi.data(), (size_t)k * 16) &&
         same_bits(T.data(), pose, 64) && same_bits(detDists.data(), dist.data(), (size_t)k * 8);
    int nin = 0;
    for (int j = 0; ok && j < k; ++j) {
        const cv::KeyPoint &kp = keyPoints[(size_t)j];
        ok = same_bits(&kp.pt, &xy[2 * (size_t)j], 8) && kp.angle == ang[(size_t)j] && kp.response == resp[(size_t)j] && kp.octave == oct[(size_t)j] &&
             matches[(size_t)j].queryIdx == keptIdx[(size_t)j] && matches[(size_t)j].trainIdx == j;
        if (ok && mask[(size_t)j]) ok = nin < (int)inliers.size() && same_bits(&inliers[(size_t)nin++], &abi[(size_t)j], 16);
    }
    ok = ok && nin == (int)inliers.size() && nin == st.numInliers * (st.accepted ? 1 : 0) && (st.accepted != 0) == expectAccepted &&
         st.numMatchesIn == k;

    // the reference's loop, matcher.cpp:151-211, over the drop-in's separate classes
    std::vector<cv::Point2f> pd = prevDistorted, sDistorted;
    std::vector<cv::KeyPoint> pk = prevKeyPoints, sKeyPoints;
    std::vector<double> pdd = prevDetDists, sDetDists;
    std::vector<cv::DMatch> sMatches = stepwise.performTracking(prevImg, img, pd, sDistorted, pk, sKeyPoints, pdd, sDetDists);      // :151-157
    std::vector<cv::Point2f> sUndistorted = sDistorted.empty() ? sDistorted
                                                               : RGBD::removeImageDistortion(sDistorted, mp.cameraMatrixMat, mp.distortionCoeffsMat);  // :159-170
    std::vector<Eigen::Vector3f> s3D = sDistorted.empty() ? std::vector<Eigen::Vector3f>()
                                                            : RGBD::keypoints2Dto3D(sUndistorted, depth, mp.cameraMatrixMat, scale);  // :172-181
    RANSAC::parameters sp = mp.RANSACParams;
    sp.errorVersion = sp.errorVersionVO;                                                                                              // :190-191
    RANSAC ransac(sp, mp.cameraMatrixMat);
    ransac.setSampleSeed(41);
    std::vector<cv::DMatch> sInliers;
    Eigen::Matrix4f sT = ransac.estimateTransformation(prev3D, s3D, sMatches, sInliers);                                              // :193-211
    ok = ok && (int)sMatches.size() == k && same_bits(sMatches.data(), matches.data(), (size_t)k * 16) &&
         same_bits(sDistorted.data(), distorted.data(), (size_t)k * 8) && same_bits(sUndistorted.data(), undistorted.data(), (size_t)k * 8) &&
         same_bits(s3D.data(), features3D.data(), (size_t)k * 12) && same_bits(sDetDists.data(), detDists.data(), (size_t)k * 8) &&
         sInliers.size() == inliers.size() && same_bits(sInliers.data(), inliers.data(), inliers.size() * 16) && same_bits(sT.data(), T.data(), 64);
    for (int j = 0; ok && j < k; ++j)
        ok = same_bits(&sKeyPoints[(size_t)j].pt, &keyPoints[(size_t)j].pt, 8) && sKeyPoints[(size_t)j].octave == keyPoints[(size_t)j].octave &&
             sKeyPoints[(size_t)j].response == keyPoints[(size_t)j].response;
    int noDepth = 0, far = 0;
    for (int j = 0; j < k; ++j) {
        const float z = reinterpret_cast<const float *>(features3D.data())[3 * (size_t)j + 2];
        noDepth += z == 0.f;
        far += z > 6.f;
    }
    std::printf("%s: %s (%d points, %d kept, %d without depth, %d beyond 6 m, %d inliers, accepted %d)\n", name, ok ? "ok" : "MISMATCH", n, k,
                noDepth, far, nin, st.accepted);
    return ok ? 0 : 1;
}

// removeTooCloseFeatures > 0: one line on std::cerr, false, the identity, every output empty
int refusal()
{
    putslam_hip::FrameMatcherHIP matcher;
    matcher.matcherParameters.OpenCVParams.removeTooCloseFeatures = 1;
    std::vector<unsigned char> buf(60 * 80, 7);
    std::vector<uint16_t> dbuf(60 * 80, 9000);
    cv::Mat img(60, 80, CV_8UC1, buf.data(), 80), depth(60, 80, CV_16U, dbuf.data(), 160);
    std::vector<cv::Point2f> prev(3, cv::Point2f(20.f, 20.f)), distorted(2), undistorted(2);
    std::vector<Eigen::Vector3f> prev3D(3, Eigen::Vector3f(0.f, 0.f, 2.f)), f3d(2);
    std::vector<cv::KeyPoint> pk(3), kps(2);
    std::vector<double> pdd(3, 1.0), dd(2);
    std::vector<cv::DMatch> matches(2), inliers(2);
    Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
    for (int i = 0; i < 16; ++i) T.data()[i] = 0.f;
    std::ostringstream captured;
    std::streambuf *old = std::cerr.rdbuf(captured.rdbuf());
    const bool r = matcher.trackStep(img, img, depth, 5000.0, prev, prev3D, pk, pdd, distorted, undistorted, f3d, kps, dd, matches, inliers, T);
    std::cerr.rdbuf(old);
    const Eigen::Matrix4f ident = Eigen::Matrix4f::Identity();
    const bool ok = !r && captured.str().find("removeTooCloseFeatures") != std::string::npos && same_bits(T.data(), ident.data(), 64) &&
                    distorted.empty() && undistorted.empty() && f3d.empty() && kps.empty() && dd.empty() && matches.empty() && inliers.empty();
    std::printf("removeTooCloseFeatures refused: %s\n", ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run_case("grey, dense rows, E0", 1, false, 0, 25.0, 3.0, 150, true);
    bad += run_case("colour, padded rows, E1", 3, true, 1, 25.0, 3.0, 150, true);
    bad += run_case("grey, padded rows, E4, 65 points", 1, true, 4, 25.0, 1.0, 65, true);
    bad += run_case("two points", 1, false, 0, 25.0, 3.0, 2, false);
    bad += run_case("no features", 1, false, 0, 25.0, 3.0, 0, false);
    bad += refusal();
    if (bad == 0) std::printf("all ok\n");
    return bad;
}
