// test_dropin_calls.cpp -- every entry point of the C++ drop-in (putslam_dropin.cpp) except matchXYZLadder, driven over the recording
// stand-in of the C ABI (capi_recorder.cpp): one accepted call on the smallest inputs that pass the checks, each refusal, one run with
// the C ABI call failing.  The program's output -- the recorder's lines, the drop-in's own std::cerr / std::cout lines and what each
// call handed back -- is the transcript tests/test_dropin_calls_host.py compares with tests/golden/dropin_calls_parent.txt.  Every seed
// is set, so nothing in it comes from the clock; no GPU is touched.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <thread>

#include "putslam_dropin.h"
#include "putslam_hip.h"

void recorderFailNext(const char *name, int code); // capi_recorder.cpp

using namespace putslam_hip;
typedef FrameMatcher::MatcherParameters Params;

namespace {

const int ROWS = 16, COLS = 24;
const int CV_8UC2_ = 8; // CV_MAKETYPE(CV_8U, 2)

void say(const char *what) { std::printf("== %s\n", what); }

cv::Mat image(int rows, int cols, int type, int seed)
{
    cv::Mat m(rows, cols, type);
    for (size_t i = 0; i < (size_t)rows * m.step; ++i) m.data[i] = (unsigned char)(i * (size_t)seed + 3);
    return m;
}
cv::Mat binaryRows(int n, int seed) { return image(n, 32, CV_8U, seed); }
cv::Mat floatRows(int n, int dim, int seed)
{
    cv::Mat m(n, dim, CV_32F);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < dim; ++c) m.at<float>(r, c) = 0.5f * (float)(r * dim + c + seed);
    return m;
}
std::vector<Eigen::Vector3f> points3(int n, float z0)
{
    std::vector<Eigen::Vector3f> v;
    for (int i = 0; i < n; ++i) v.push_back(Eigen::Vector3f(0.1f * (float)i, -0.2f * (float)i, z0 + 0.25f * (float)i));
    return v;
}
std::vector<cv::Point2f> points2(int n, float x0)
{
    std::vector<cv::Point2f> v;
    for (int i = 0; i < n; ++i) v.push_back(cv::Point2f(x0 + 2.0f * (float)i, 3.0f + (float)i));
    return v;
}
std::vector<cv::KeyPoint> keyPoints(int n)
{
    std::vector<cv::KeyPoint> v((size_t)n);
    for (int i = 0; i < n; ++i) {
        v[(size_t)i].pt = cv::Point2f(1.0f + (float)i, 2.0f + 1.5f * (float)i);
        v[(size_t)i].size = 31.0f + (float)i;
        v[(size_t)i].angle = 10.0f * (float)i;
        v[(size_t)i].response = 0.5f * (float)i;
        v[(size_t)i].octave = i % 4;
        v[(size_t)i].class_id = 100 + i;
    }
    return v;
}
std::vector<double> dists(int n)
{
    std::vector<double> v;
    for (int i = 0; i < n; ++i) v.push_back(1.0 + 0.5 * i);
    return v;
}
std::vector<cv::DMatch> someMatches(int n, int nq, int nt)
{
    std::vector<cv::DMatch> v;
    for (int i = 0; i < n; ++i) v.push_back(cv::DMatch(i % nq, (i * 2) % nt, 0, 0.5f * (float)i));
    return v;
}

void show(const char *what, const std::vector<cv::KeyPoint> &v)
{
    std::printf("  %s: %zu key points\n", what, v.size());
    for (const cv::KeyPoint &k : v)
        std::printf("    pt=(%.9g,%.9g) size=%.9g angle=%.9g response=%.9g octave=%d class_id=%d\n", k.pt.x, k.pt.y, k.size, k.angle, k.response,
                    k.octave, k.class_id);
}
void show(const char *what, const std::vector<cv::DMatch> &v)
{
    std::printf("  %s: %zu matches", what, v.size());
    for (const cv::DMatch &m : v) std::printf(" (%d,%d,%d,%.9g)", m.queryIdx, m.trainIdx, m.imgIdx, m.distance);
    std::printf("\n");
}
void show(const char *what, const std::vector<cv::Point2f> &v)
{
    std::printf("  %s: %zu points", what, v.size());
    for (const cv::Point2f &p : v) std::printf(" (%.9g,%.9g)", p.x, p.y);
    std::printf("\n");
}
void show(const char *what, const std::vector<Eigen::Vector3f> &v)
{
    std::printf("  %s: %zu points", what, v.size());
    for (const Eigen::Vector3f &p : v) std::printf(" (%.9g,%.9g,%.9g)", p[0], p[1], p[2]);
    std::printf("\n");
}
void show(const char *what, const std::vector<double> &v)
{
    std::printf("  %s: %zu values", what, v.size());
    for (double d : v) std::printf(" %.17g", d);
    std::printf("\n");
}
void show(const char *what, const std::vector<int> &v)
{
    std::printf("  %s: %zu values", what, v.size());
    for (int d : v) std::printf(" %d", d);
    std::printf("\n");
}
void show(const char *what, const Eigen::Matrix4f &T)
{
    std::printf("  %s:", what);
    for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
    std::printf("\n");
}
void show(const char *what, const cv::Mat &m)
{
    unsigned long long h = 1469598103934665603ull;
    for (int r = 0; r < m.rows; ++r)
        for (size_t i = 0; i < (size_t)m.cols * m.elemSize(); ++i) h = (h ^ m.data[(size_t)r * m.step + i]) * 1099511628211ull;
    std::printf("  %s: Mat %d x %d type %d", what, m.rows, m.cols, m.empty() ? -1 : m.type());
    if (!m.empty()) std::printf(" bytes %llx", h);
    std::printf("\n");
}

cv::Mat distortion(int rows, int cols)
{
    cv::Mat m(rows, cols, CV_32FC1);
    for (int i = 0; i < rows * cols; ++i) m.at<float>(rows == 1 ? 0 : i, rows == 1 ? i : 0) = 0.01f * (float)(i + 1);
    return m;
}

// ---------------------------------------------------------------------------------------------
void runRansac()
{
    say("RANSAC");
    Params mp;
    const std::vector<Eigen::Vector3f> a = points3(6, 1.0f), b = points3(6, 1.5f);
    const std::vector<cv::DMatch> m = someMatches(5, 6, 6);
    const double ratios[3] = {0.2, 0.01, 1.0};
    for (double r : ratios) {
        RANSAC::parameters p = mp.RANSACParams;
        p.minimalInlierRatioThreshold = r;
        RANSAC ransac(p, mp.cameraMatrixMat);
        ransac.setSampleSeed(41);
        std::vector<cv::DMatch> inl = someMatches(2, 6, 6);
        show("pose", ransac.estimateTransformation(a, b, m, inl));
        show("inliers", inl);
        std::printf("  status %d seed %llu\n", ransac.lastStatus(), (unsigned long long)ransac.sampleSeed());
    }
    {
        say("RANSAC verbose, no camera matrix, unknown error version, no matches");
        RANSAC::parameters p = mp.RANSACParams;
        p.verbose = 1;
        p.errorVersion = 7;
        RANSAC ransac(p);
        ransac.setSampleSeed(42);
        std::vector<cv::DMatch> inl;
        show("pose", ransac.estimateTransformation(a, b, std::vector<cv::DMatch>(), inl));
        show("inliers", inl);
    }
    {
        say("RANSAC failing");
        RANSAC ransac(mp.RANSACParams, mp.cameraMatrixMat);
        ransac.setSampleSeed(43);
        std::vector<cv::DMatch> inl = someMatches(2, 6, 6);
        recorderFailNext("ps_ransac_rigid3d", PS_ERR_HIP);
        show("pose", ransac.estimateTransformation(a, b, m, inl));
        show("inliers", inl);
        std::printf("  status %d\n", ransac.lastStatus());
    }
    say("RANSAC_USAC");
    PUTSLAMEstimator::parameters up;
    up.verbose = 0;
    up.errorVersion = 1;
    up.errorVersionVO = 2;
    up.errorVersionMap = 3;
    up.inlierThresholdEuclidean = 0.03;
    up.inlierThresholdReprojection = 1.5;
    up.inlierThresholdMahalanobis = 0.0003;
    up.minimalInlierRatioThreshold = 0.3;
    up.usedPairs = 3;
    up.iterationCount = 99;
    const std::vector<Eigen::Vector3f> a9 = points3(9, 1.0f), b9 = points3(9, 1.5f);
    const int counts[2] = {3, 9};
    for (int n : counts) {
        RANSAC_USAC usac(up, mp.cameraMatrixMat);
        usac.setSampleSeed(51);
        if (n == 9) usac.setMaxHypotheses(1000);
        std::vector<cv::DMatch> inl = someMatches(2, 9, 9);
        show("pose", usac.estimateTransformation(a9, b9, someMatches(n, 9, 9), inl));
        show("inliers", inl);
        std::printf("  status %d\n", usac.lastStatus());
    }
    {
        say("RANSAC_USAC verbose, failing");
        up.verbose = 1;
        RANSAC_USAC usac(up, mp.cameraMatrixMat);
        usac.setSampleSeed(52);
        std::vector<cv::DMatch> inl = someMatches(2, 9, 9);
        show("pose", usac.estimateTransformation(a9, b9, someMatches(9, 9, 9), inl));
        show("inliers", inl);
        recorderFailNext("ps_ransac_rigid3d", PS_ERR_BAD_ARG);
        show("pose", usac.estimateTransformation(a9, b9, someMatches(9, 9, 9), inl));
        show("inliers", inl);
        std::printf("  status %d\n", usac.lastStatus());
    }
}

void runRgbd()
{
    say("RGBD");
    Params mp;
    std::printf("  roundSize %d %d %d %d\n", RGBD::roundSize(-1.5, 10), RGBD::roundSize(3.5, 10), RGBD::roundSize(9.4, 10), RGBD::roundSize(2.4, 10));
    const cv::Mat depth = image(ROWS, COLS, CV_16U, 5);
    show("3-D", RGBD::keypoints2Dto3D(points2(4, 1.0f), depth, mp.cameraMatrixMat));
    show("3-D from 2", RGBD::keypoints2Dto3D(points2(4, 1.0f), depth, mp.cameraMatrixMat, 1000.0, 2));
    show("3-D of none", RGBD::keypoints2Dto3D(points2(2, 1.0f), depth, mp.cameraMatrixMat, 5000.0, 2));
    recorderFailNext("ps_keypoints2Dto3D", PS_ERR_HIP);
    show("3-D failing", RGBD::keypoints2Dto3D(points2(4, 1.0f), depth, cv::Mat()));
    std::vector<cv::Point2f> f = points2(4, 2.0f), none;
    show("undistorted 1x5", RGBD::removeImageDistortion(f, mp.cameraMatrixMat, mp.distortionCoeffsMat));
    show("undistorted 5x1", RGBD::removeImageDistortion(f, mp.cameraMatrixMat, distortion(5, 1)));
    show("undistorted 1x4", RGBD::removeImageDistortion(f, mp.cameraMatrixMat, distortion(1, 4)));
    show("undistorted empty", RGBD::removeImageDistortion(f, mp.cameraMatrixMat, cv::Mat()));
    show("undistorted none", RGBD::removeImageDistortion(none, mp.cameraMatrixMat, mp.distortionCoeffsMat));
    recorderFailNext("ps_remove_image_distortion", PS_ERR_HIP);
    show("undistorted failing", RGBD::removeImageDistortion(f, mp.cameraMatrixMat, mp.distortionCoeffsMat));
    show("2-D", RGBD::points3Dto2D(points3(4, 1.0f), mp.cameraMatrixMat));
    show("2-D of none", RGBD::points3Dto2D(std::vector<Eigen::Vector3f>(), mp.cameraMatrixMat));
    recorderFailNext("ps_points3Dto2D", PS_ERR_HIP);
    show("2-D failing", RGBD::points3Dto2D(points3(4, 1.0f), mp.cameraMatrixMat));
}

void runDbscanKabsch()
{
    say("DBScan");
    std::vector<cv::KeyPoint> k = keyPoints(5), none;
    DBScan(2.0, 3, 2).run(k);
    show("thinned", k);
    DBScan().run(none);
    show("none", none);
    k = keyPoints(4);
    recorderFailNext("ps_dbscan_thin", PS_ERR_HIP);
    DBScan().run(k);
    show("failing", k);

    say("KabschEst");
    putslam::TransformEst *est = putslam::createKabschEstimator();
    std::printf("  name %s\n", est->getName().c_str());
    Eigen::MatrixXd A(4, 3), B(4, 3), E(0, 3);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 3; ++c) {
            A(r, c) = 0.5 * r + c;
            B(r, c) = 0.25 * r - c;
        }
    const int fails[3] = {0, 0, 1};
    for (int i = 0; i < 3; ++i) {
        if (fails[i]) recorderFailNext("ps_kabsch_f64", PS_ERR_HIP);
        putslam::Mat34 &T = i == 1 ? est->computeTransformation(E, E) : est->computeTransformation(A, B);
        std::printf("  transformation:");
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) std::printf(" %.17g", T(r, c));
        std::printf("\n");
    }
}

void runExclusion()
{
    say("chooseFeaturesToAddToMap");
    std::vector<int> accepted;
    std::printf("  returns %d\n", chooseFeaturesToAddToMap(points3(4, 1.0f), points2(4, 1.0f), 2, 10, points3(3, 2.0f), points2(3, 5.0f), 0.05f, 4.0f, accepted));
    show("accepted", accepted);
    std::printf("  sizes differ: returns %d\n",
                chooseFeaturesToAddToMap(points3(4, 1.0f), points2(3, 1.0f), 2, 10, points3(3, 2.0f), points2(3, 5.0f), 0.05f, 4.0f, accepted));
    std::printf("  full: returns %d\n", chooseFeaturesToAddToMap(points3(4, 1.0f), points2(4, 1.0f), 10, 10, points3(3, 2.0f), points2(3, 5.0f), 0.05f, 4.0f, accepted));
    std::printf("  no candidates: returns %d\n", chooseFeaturesToAddToMap(points3(0, 1.0f), points2(0, 1.0f), -5, 0x7fffffff, points3(3, 2.0f), points2(3, 5.0f), 0.05f, 4.0f, accepted));
    std::printf("  empty map: returns %d\n", chooseFeaturesToAddToMap(points3(4, 1.0f), points2(4, 1.0f), -5, 0x7fffffff, points3(0, 2.0f), points2(0, 5.0f), 0.05f, 4.0f, accepted));
    show("accepted", accepted);
    recorderFailNext("ps_exclude", PS_ERR_HIP);
    std::printf("  failing: returns %d\n", chooseFeaturesToAddToMap(points3(4, 1.0f), points2(4, 1.0f), 2, 10, points3(3, 2.0f), points2(3, 5.0f), 0.05f, 4.0f, accepted));
    show("accepted", accepted);

    for (int fail = 0; fail < 2; ++fail) {
        say(fail ? "mergeTrackedFeatures failing" : "mergeTrackedFeatures");
        FrameMatcherHIP m;
        std::vector<cv::Point2f> und = points2(3, 1.0f), dis = points2(3, 1.5f);
        std::vector<Eigen::Vector3f> p3 = points3(3, 1.0f);
        std::vector<cv::KeyPoint> kp = keyPoints(3);
        std::vector<double> dd = dists(3);
        if (fail) recorderFailNext("ps_exclude", PS_ERR_HIP);
        m.mergeTrackedFeatures(und, points2(4, 20.0f), dis, points2(4, 20.5f), p3, points3(4, 3.0f), kp, keyPoints(4), dd, dists(4));
        show("undistorted", und);
        show("distorted", dis);
        show("3-D", p3);
        show("key points", kp);
        show("detection distances", dd);
    }
    for (int mode = 0; mode < 3; ++mode) {
        say(mode == 0 ? "removeTooCloseFeatures" : mode == 1 ? "removeTooCloseFeatures failing" : "removeTooCloseFeatures sizes differ");
        FrameMatcherHIP m;
        std::vector<cv::Point2f> und = points2(mode == 2 ? 4 : 5, 1.0f), dis = points2(6, 1.5f);
        std::vector<Eigen::Vector3f> p3 = points3(5, 1.0f);
        std::vector<cv::KeyPoint> kp = keyPoints(4);
        std::vector<double> dd = dists(5);
        std::vector<cv::DMatch> mt = someMatches(6, 5, 5);
        if (mode == 1) recorderFailNext("ps_exclude", PS_ERR_HIP);
        const std::set<int> gone = m.removeTooCloseFeatures(dis, und, p3, kp, dd, mt);
        show("removed", std::vector<int>(gone.begin(), gone.end()));
        show("undistorted", und);
        show("distorted", dis);
        show("3-D", p3);
        show("key points", kp);
        show("detection distances", dd);
        show("matches", mt);
    }
}

void runMatch()
{
    say("cross-check matching");
    show("hamming", hammingCrossCheckMatch(binaryRows(3, 3), binaryRows(4, 5)));
    show("hamming of none", hammingCrossCheckMatch(cv::Mat(), binaryRows(4, 5)));
    show("hamming of floats", hammingCrossCheckMatch(floatRows(3, 8, 1), binaryRows(4, 5)));
    recorderFailNext("ps_match_hamming256", PS_ERR_HIP);
    show("hamming failing", hammingCrossCheckMatch(binaryRows(3, 3), binaryRows(4, 5)));
    show("l2", l2CrossCheckMatch(floatRows(3, 8, 1), floatRows(4, 8, 2)));
    show("l2 of none", l2CrossCheckMatch(floatRows(3, 8, 1), cv::Mat()));
    show("l2 of bytes", l2CrossCheckMatch(floatRows(3, 8, 1), binaryRows(4, 5)));
    show("l2 of two widths", l2CrossCheckMatch(floatRows(3, 8, 1), floatRows(3, 4, 1)));
    recorderFailNext("ps_match_l2_f32", PS_ERR_HIP);
    show("l2 failing", l2CrossCheckMatch(floatRows(3, 8, 1), floatRows(4, 8, 2)));

    const double ratios[3] = {0.2, 0.01, 1.0};
    for (double r : ratios) {
        std::printf("== match, minimalInlierRatioThreshold %.17g\n", r);
        FrameMatcher *fm = createFrameMatcher();
        std::printf("  name %s\n", fm->getName().c_str());
        fm->setSampleSeed(7);
        fm->matcherParameters.RANSACParams.minimalInlierRatioThreshold = r;
        fm->matcherParameters.RANSACParams.errorVersionVO = 1;
        fm->detectInitFeatures(binaryRows(3, 3), points3(3, 1.0f));
        for (int i = 0; i < 3; ++i) { // the resident frame: loaded on the first call, kept from then on
            Eigen::Matrix4f T;
            std::vector<cv::DMatch> inl;
            std::printf("  returns %.17g\n", fm->runVO(binaryRows(3 + i, 5 + i), points3(3 + i, 1.5f), T, inl));
            show("pose", T);
            show("inliers", inl);
            std::printf("  features %d\n", fm->getNumberOfFeatures());
        }
    }
    {
        say("match: the stream's push failing, then float descriptors, then no camera matrix");
        FrameMatcherHIP m("a", "b");
        std::printf("  name %s\n", m.getName().c_str());
        m.setSampleSeed(8);
        m.detectInitFeatures(binaryRows(3, 3), points3(3, 1.0f));
        Eigen::Matrix4f T;
        std::vector<cv::DMatch> inl;
        recorderFailNext("ps_vo_stream_push", PS_ERR_HIP);
        std::printf("  returns %.17g\n", m.match(binaryRows(4, 5), points3(4, 1.5f), T, inl));
        show("inliers", inl);
        recorderFailNext("ps_vo_stream_create", PS_ERR_ALLOC);
        FrameMatcherHIP m2;
        m2.setSampleSeed(9);
        m2.detectInitFeatures(binaryRows(3, 3), points3(3, 1.0f));
        std::printf("  returns %.17g\n", m2.match(binaryRows(4, 5), points3(4, 1.5f), T, inl));
        m.detectInitFeatures(floatRows(3, 8, 1), points3(3, 1.0f));
        std::printf("  returns %.17g\n", m.match(floatRows(4, 8, 2), points3(4, 1.5f), T, inl));
        show("pose", T);
        show("inliers", inl);
        m.matcherParameters.cameraMatrixMat = cv::Mat();
        m.detectInitFeatures(binaryRows(3, 3), points3(3, 1.0f));
        std::printf("  returns %.17g\n", m.match(binaryRows(4, 5), points3(4, 1.5f), T, inl));
        FrameMatcher::featureSet fs = m.getFeatures();
        show("kept descriptors", fs.descriptors);
        show("kept points", fs.feature3D);
    }
    {
        say("matchFeatureLoopClosure");
        FrameMatcher *fm = createLoopClosingFrameMatcher("a", "b");
        fm->setSampleSeed(11);
        Eigen::Matrix4f T;
        std::vector<cv::DMatch> inl;
        std::printf("  few: returns %.17g\n", fm->matchFeatureLoopClosure(binaryRows(9, 3), points3(9, 1.0f), binaryRows(10, 5), points3(10, 1.0f), T, inl));
        std::printf("  returns %.17g\n", fm->matchFeatureLoopClosure(binaryRows(10, 3), points3(10, 1.0f), binaryRows(11, 5), points3(11, 1.0f), T, inl));
        show("pose", T);
        show("inliers", inl);
        recorderFailNext("ps_match_hamming256", PS_ERR_HIP);
        std::printf("  no matches: returns %.17g\n", fm->matchFeatureLoopClosure(binaryRows(10, 3), points3(10, 1.0f), binaryRows(11, 5), points3(11, 1.0f), T, inl));
    }
}

std::vector<FrameMatcher::MapFeatureXYZ> mapFeatures(int n, bool isFloat, int dim)
{
    std::vector<FrameMatcher::MapFeatureXYZ> v((size_t)n);
    for (int j = 0; j < n; ++j) {
        FrameMatcher::MapFeatureXYZ &f = v[(size_t)j];
        f.id = 100u + (unsigned)j;
        f.position[0] = 0.1 * j;
        f.position[1] = 0.2 * j;
        f.position[2] = 1.0 + 0.3 * j;
        if (j != 1) f.descriptor = isFloat ? floatRows(1, dim, j) : binaryRows(1, 3 + j); // (feature 1 has no descriptor: its row stays zero)
        f.octave = j % 3;
        f.detDist = 1.25;
    }
    return v;
}

void runMatchXYZ()
{
    for (int isFloat = 0; isFloat < 2; ++isFloat) {
        say(isFloat ? "matchXYZ, float rows" : "matchXYZ, binary rows");
        FrameMatcherHIP m;
        m.setSampleSeed(13);
        m.matcherParameters.verbose = 1;
        m.matcherParameters.RANSACParams.errorVersionMap = 2;
        const char *fn = isFloat ? "ps_match_xyz_l2_f32" : "ps_match_xyz";
        const std::vector<FrameMatcher::MapFeatureXYZ> map = mapFeatures(5, isFloat != 0, 8);
        const cv::Mat desc = isFloat ? floatRows(3, 8, 2) : binaryRows(3, 9);
        std::vector<Eigen::Vector3f> cur = points3(3, 1.0f);
        const std::vector<int> oct = {0, 1, 2};
        const std::vector<double> dd = dists(3);
        const int tries[5] = {1, 3, 12, 1, 1};
        for (int i = 0; i < 5; ++i) {
            if (i == 3) recorderFailNext(fn, PS_ERR_HIP);
            if (i == 4) recorderFailNext(fn, PS_ERR_ALLOC); // (reports an overflow: the call is made again with room)
            Eigen::Matrix4f T;
            std::vector<cv::DMatch> inl;
            std::printf("  try %d: returns %.17g\n", tries[i], m.matchXYZ(map, desc, cur, oct, dd, T, inl, tries[i]));
            show("pose", T);
            show("inliers", inl);
        }
        Eigen::Matrix4f T;
        std::vector<cv::DMatch> inl;
        std::printf("  empty map: returns %.17g\n", m.matchXYZ(std::vector<FrameMatcher::MapFeatureXYZ>(), desc, cur, oct, dd, T, inl));
        std::printf("  mixed types: returns %.17g\n", m.matchXYZ(mapFeatures(5, isFloat == 0, 8), desc, cur, oct, dd, T, inl));
        if (isFloat) std::printf("  two widths: returns %.17g\n", m.matchXYZ(mapFeatures(5, true, 4), desc, cur, oct, dd, T, inl));
    }
}

// (the status is taken first, then the text it left: the arguments of one call are evaluated in no fixed order)
void report(const char *what, int status, const FrameMatcher &m) { std::printf("  %s: %d, %s\n", what, status, m.lastError().c_str()); }

void runPipeline()
{
    say("pipeline");
    FrameMatcherHIP m;
    m.setSampleSeed(17);
    m.matcherParameters.RANSACParams.minimalInlierRatioThreshold = 0.01;
    m.matcherParameters.RANSACParams.errorVersionVO = 1;
    m.setPipeline(2, 1);
    Eigen::Matrix4f T;
    std::vector<cv::DMatch> inl;
    double ratio = 0;
    const auto pop = [&](bool wait) {
        const int rc = m.dequeueResult(T, inl, ratio, wait);
        std::printf("  dequeueResult returns %d ratio %.17g\n", rc, ratio);
        show("pose", T);
        show("inliers", inl);
        return rc;
    };
    std::printf("  before the first frame: flush %d\n", (int)m.flushFrames());
    pop(true);
    report("bad rows", m.enqueueFrameStatus(floatRows(3, 8, 1), points3(3, 1.0f)), m);
    for (int i = 0; i < 3; ++i) std::printf("  enqueueFrame %d\n", (int)m.enqueueFrame(binaryRows(3 + i, 3 + i), points3(3 + i, 1.0f)));
    pop(false);
    std::printf("  flush %d\n", (int)m.flushFrames());
    const int big = 2049; // more key points than the pipeline was built for: busy while results are pending, rebuilt once drained
    report("large frame", m.enqueueFrameStatus(binaryRows(big, 3), points3(big, 1.0f)), m);
    int tries = 0;
    while (!m.enqueueFrame(binaryRows(big, 3), points3(big, 1.0f)) && ++tries < 4) pop(true);
    std::printf("  large frame taken after %d results\n", tries);
    recorderFailNext("ps_vo_stream_push_async", PS_ERR_BUSY);
    report("full", m.enqueueFrameStatus(binaryRows(4, 3), points3(4, 1.0f)), m);
    recorderFailNext("ps_vo_stream_push_async", PS_ERR_HIP);
    report("failing: enqueueFrame", (int)m.enqueueFrame(binaryRows(4, 3), points3(4, 1.0f)), m);
    pop(true);
    pop(true);
    recorderFailNext("ps_vo_stream_pop", PS_ERR_HIP);
    pop(true);
    std::printf("  features %d\n", m.getNumberOfFeatures());
    m.resetPipeline();
    recorderFailNext("ps_vo_stream_configure_async", PS_ERR_BAD_ARG);
    report("configure failing", m.enqueueFrameStatus(binaryRows(3, 3), points3(3, 1.0f)), m);
    recorderFailNext("ps_vo_stream_create", PS_ERR_ALLOC);
    report("create failing", m.enqueueFrameStatus(binaryRows(3, 3), points3(3, 1.0f)), m);
    std::printf("  enqueueFrame %d\n", (int)m.enqueueFrame(binaryRows(3, 3), points3(3, 1.0f)));
    std::printf("  empty frame %d\n", (int)m.enqueueFrame(cv::Mat(), points3(0, 1.0f)));
    pop(true);
    FrameMatcherHIP m2; // (the clock would seed an unseeded pipeline: every matcher here is seeded)
    m2.setSampleSeed(18);
    recorderFailNext("ps_context_create", PS_ERR_NO_DEVICE);
    report("no device", m2.enqueueFrameStatus(binaryRows(3, 3), points3(3, 1.0f)), m2);
}

// the refusals an image pair shares: called with a function that runs the entry point on (prev, img, depth)
template <class F> void imageRefusals(bool pair, bool withDepth, F call)
{
    const cv::Mat grey = image(ROWS, COLS, CV_8UC1, 3), depth = image(ROWS, COLS, CV_16U, 5);
    static std::vector<unsigned char> wide((size_t)ROWS * (COLS + 8));
    std::printf("  -- empty image\n");
    call(grey, cv::Mat(), depth);
    std::printf("  -- CV_32F image\n");
    call(image(ROWS, COLS, CV_32F, 3), image(ROWS, COLS, CV_32F, 4), depth);
    std::printf("  -- 2 channels\n");
    call(image(ROWS, COLS, CV_8UC2_, 3), image(ROWS, COLS, CV_8UC2_, 4), depth);
    if (pair) {
        std::printf("  -- empty previous image\n");
        call(cv::Mat(), grey, depth);
        std::printf("  -- second image of another type\n");
        call(grey, image(ROWS, COLS, CV_8UC3, 4), depth);
        std::printf("  -- second image of another size\n");
        call(image(ROWS, COLS + 1, CV_8UC1, 3), grey, depth);
        call(image(ROWS + 1, COLS, CV_8UC1, 3), grey, depth);
        std::printf("  -- second image of another step\n");
        call(cv::Mat(ROWS, COLS, CV_8UC1, wide.data(), (size_t)COLS + 8), grey, depth);
    }
    if (withDepth) {
        std::printf("  -- empty depth\n");
        call(grey, grey, cv::Mat());
        std::printf("  -- depth of another type\n");
        call(grey, grey, image(ROWS, COLS, CV_8U, 5));
        std::printf("  -- depth of another size\n");
        call(grey, grey, image(ROWS, COLS + 1, CV_16U, 5));
        call(grey, grey, image(ROWS - 1, COLS, CV_16U, 5));
    }
}

void runTracking()
{
    say("performTracking");
    FrameMatcherHIP m;
    std::vector<cv::Point2f> prev = points2(4, 1.0f);
    std::vector<cv::KeyPoint> prevKp = keyPoints(4);
    std::vector<double> prevDd = dists(4);
    const auto track = [&](const cv::Mat &a, const cv::Mat &b, std::vector<cv::Point2f> features) {
        std::vector<cv::KeyPoint> kp = keyPoints(1);
        std::vector<double> dd = dists(1);
        show("matches", m.performTracking(a, b, prev, features, prevKp, kp, prevDd, dd));
        show("features", features);
        show("key points", kp);
        show("detection distances", dd);
    };
    const cv::Mat grey = image(ROWS, COLS, CV_8UC1, 3), grey2 = image(ROWS, COLS, CV_8UC1, 4);
    track(grey, grey2, points2(2, 0.0f));
    m.matcherParameters.verbose = 1;
    m.matcherParameters.OpenCVParams.trackingErrorType = 1;
    m.matcherParameters.OpenCVParams.winSize = 9;
    track(image(ROWS, COLS, CV_8UC3, 3), image(ROWS, COLS, CV_8UC3, 4), points2(0, 0.0f));
    m.matcherParameters.verbose = 0;
    imageRefusals(true, false, [&](const cv::Mat &a, const cv::Mat &b, const cv::Mat &) { track(a, b, points2(0, 0.0f)); });
    std::printf("  -- useInitialFlow without a flow, then with one\n");
    m.matcherParameters.OpenCVParams.useInitialFlow = 1;
    track(grey, grey2, points2(3, 0.0f));
    track(grey, grey2, points2(4, 0.5f));
    m.matcherParameters.OpenCVParams.useInitialFlow = 0;
    std::printf("  -- failing\n");
    recorderFailNext("ps_perform_tracking", PS_ERR_HIP);
    track(grey, grey2, points2(0, 0.0f));
    std::printf("  -- count mismatches\n");
    prevKp = keyPoints(3);
    track(grey, grey2, points2(0, 0.0f));
    prevKp = keyPoints(4);
    prevDd = dists(5);
    track(grey, grey2, points2(0, 0.0f));
    std::printf("  -- no previous feature\n");
    prev.clear();
    prevKp.clear();
    prevDd.clear();
    track(grey, grey2, points2(0, 0.0f));
}

void runDetectDescribe()
{
    say("detectFeatures");
    FrameMatcherHIP m;
    const cv::Mat grey = image(ROWS, COLS, CV_8UC1, 3), rgb = image(ROWS, COLS, CV_8UC3, 3);
    show("ORB, grey", m.detectFeatures(grey));
    m.matcherParameters.verbose = 2;
    m.matcherParameters.OpenCVParams.gridRows = 2;
    m.matcherParameters.OpenCVParams.gridCols = 3;
    m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 2;
    show("ORB, 3 channels", m.detectFeatures(rgb));
    m.matcherParameters.OpenCVParams.detector = "FAST";
    show("FAST, 3 channels", m.detectFeatures(rgb));
    m.matcherParameters.verbose = 0;
    m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 500;
    show("FAST, grey", m.detectFeatures(grey));
    const char *names[3] = {"ORB", "FAST", "SURF"};
    for (const char *name : names) {
        std::printf("  -- detector %s\n", name);
        m.matcherParameters.OpenCVParams.detector = name;
        imageRefusals(false, false, [&](const cv::Mat &, const cv::Mat &b, const cv::Mat &) { show("key points", m.detectFeatures(b)); });
        std::printf("  -- maximalTrackedFeatures 0, then the call failing\n");
        m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 0;
        show("key points", m.detectFeatures(grey));
        m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 500;
        recorderFailNext(name[0] == 'O' ? "ps_detect_features_orb" : "ps_detect_features", PS_ERR_HIP);
        show("key points", m.detectFeatures(grey));
        recorderFailNext("", 0);
    }
    std::printf("  -- the free functions by name: SIFT, and detectFeaturesFAST under detector ORB\n");
    m.matcherParameters.OpenCVParams.detector = "SIFT";
    show("detectFeaturesORB", detectFeaturesORB(m.matcherParameters, grey));
    show("detectFeaturesFAST", detectFeaturesFAST(m.matcherParameters, grey));
    m.matcherParameters.OpenCVParams.detector = "ORB";
    show("detectFeaturesFAST", detectFeaturesFAST(m.matcherParameters, cv::Mat()));

    say("describeFeatures");
    const auto describe = [&](const cv::Mat &img, int n) {
        std::vector<cv::KeyPoint> kp = keyPoints(n);
        show("descriptors", m.describeFeatures(img, kp));
        show("key points", kp);
    };
    describe(grey, 5);
    describe(rgb, 4);
    describe(grey, 0);
    imageRefusals(false, false, [&](const cv::Mat &, const cv::Mat &b, const cv::Mat &) { describe(b, 4); });
    std::printf("  -- failing, then descriptor SIFT\n");
    recorderFailNext("ps_describe_features", PS_ERR_HIP);
    describe(grey, 4);
    m.matcherParameters.OpenCVParams.descriptor = "SIFT";
    describe(cv::Mat(), 4);
}

void runFrontEnd()
{
    say("frontEnd");
    FrameMatcherHIP m;
    const cv::Mat grey = image(ROWS, COLS, CV_8UC1, 3), rgb = image(ROWS, COLS, CV_8UC3, 3), depth = image(ROWS, COLS, CV_16U, 5);
    const auto front = [&](const cv::Mat &img, const cv::Mat &d, bool lists) {
        cv::Mat desc = binaryRows(1, 1);
        std::vector<Eigen::Vector3f> p3 = points3(1, 1.0f);
        std::vector<cv::KeyPoint> kp = keyPoints(1);
        std::vector<cv::Point2f> und = points2(1, 1.0f);
        m.frontEnd(img, d, 5000.0, desc, p3, lists ? &kp : nullptr, lists ? &und : nullptr);
        show("descriptors", desc);
        show("3-D", p3);
        if (lists) show("key points", kp);
        if (lists) show("undistorted", und);
    };
    front(grey, depth, true);
    front(rgb, depth, false);
    std::printf("  -- distortion coefficients 5x1, 1x4, none; no camera matrix\n");
    m.matcherParameters.distortionCoeffsMat = distortion(5, 1);
    front(grey, depth, false);
    m.matcherParameters.distortionCoeffsMat = distortion(1, 4);
    front(grey, depth, false);
    m.matcherParameters.distortionCoeffsMat = cv::Mat();
    m.matcherParameters.cameraMatrixMat = cv::Mat();
    m.matcherParameters.OpenCVParams.gridRows = 2;
    m.matcherParameters.OpenCVParams.DBScanEps = 2.5;
    m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 2;
    front(grey, depth, true);
    imageRefusals(false, true, [&](const cv::Mat &, const cv::Mat &b, const cv::Mat &d) { front(b, d, true); });
    std::printf("  -- failing\n");
    recorderFailNext("ps_front_end_frame", PS_ERR_HIP);
    front(grey, depth, true);
    std::printf("  -- maximalTrackedFeatures 0, detector SURF, descriptor SIFT\n");
    m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 0;
    front(grey, depth, true);
    m.matcherParameters.OpenCVParams.detector = "SURF";
    front(cv::Mat(), depth, true);
    m.matcherParameters.OpenCVParams.detector = "ORB";
    m.matcherParameters.OpenCVParams.descriptor = "SIFT";
    front(grey, depth, true);
}

void runTrackStep()
{
    say("trackStep");
    FrameMatcherHIP m;
    m.setSampleSeed(23);
    m.matcherParameters.RANSACParams.errorVersionVO = 1;
    const cv::Mat grey = image(ROWS, COLS, CV_8UC1, 3), grey2 = image(ROWS, COLS, CV_8UC1, 4), depth = image(ROWS, COLS, CV_16U, 5);
    int nPrev = 4, n3 = 4, nKp = 4, nDd = 4;
    const auto step = [&](const cv::Mat &a, const cv::Mat &b, const cv::Mat &d, std::vector<cv::Point2f> distorted) {
        std::vector<cv::Point2f> und = points2(1, 1.0f);
        std::vector<Eigen::Vector3f> p3 = points3(1, 1.0f);
        std::vector<cv::KeyPoint> kp = keyPoints(1);
        std::vector<double> dd = dists(1);
        std::vector<cv::DMatch> mt = someMatches(1, 1, 1), inl = someMatches(1, 1, 1);
        Eigen::Matrix4f T;
        const bool ok = m.trackStep(a, b, d, 5000.0, points2(nPrev, 1.0f), points3(n3, 1.0f), keyPoints(nKp), dists(nDd), distorted, und, p3, kp, dd, mt,
                                    inl, T);
        std::printf("  returns %d\n", (int)ok);
        show("distorted", distorted);
        show("undistorted", und);
        show("3-D", p3);
        show("key points", kp);
        show("detection distances", dd);
        show("matches", mt);
        show("inliers", inl);
        show("pose", T);
    };
    const double ratios[3] = {0.2, 0.01, 1.0};
    for (double r : ratios) {
        m.matcherParameters.RANSACParams.minimalInlierRatioThreshold = r;
        step(grey, grey2, depth, points2(2, 0.0f));
    }
    std::printf("  -- 3 channels, distortion 5x1 and 1x4 and none, the tracker's block changed\n");
    m.matcherParameters.OpenCVParams.trackingErrorType = 1;
    m.matcherParameters.OpenCVParams.maxLevels = 2;
    m.matcherParameters.OpenCVParams.trackingErrorThreshold = 12.5;
    m.matcherParameters.distortionCoeffsMat = distortion(5, 1);
    step(image(ROWS, COLS, CV_8UC3, 3), image(ROWS, COLS, CV_8UC3, 4), depth, points2(0, 0.0f));
    m.matcherParameters.distortionCoeffsMat = distortion(1, 4);
    step(grey, grey2, depth, points2(0, 0.0f));
    m.matcherParameters.distortionCoeffsMat = cv::Mat();
    step(grey, grey2, depth, points2(0, 0.0f));
    imageRefusals(true, true, [&](const cv::Mat &a, const cv::Mat &b, const cv::Mat &d) { step(a, b, d, points2(0, 0.0f)); });
    std::printf("  -- useInitialFlow without a flow, then with one\n");
    m.matcherParameters.OpenCVParams.useInitialFlow = 1;
    step(grey, grey2, depth, points2(3, 0.0f));
    step(grey, grey2, depth, points2(4, 0.5f));
    m.matcherParameters.OpenCVParams.useInitialFlow = 0;
    std::printf("  -- failing\n");
    recorderFailNext("ps_track_vo_pair", PS_ERR_HIP);
    step(grey, grey2, depth, points2(0, 0.0f));
    std::printf("  -- count mismatches\n");
    n3 = 3;
    step(grey, grey2, depth, points2(0, 0.0f));
    n3 = 4;
    nKp = 5;
    step(grey, grey2, depth, points2(0, 0.0f));
    nKp = 4;
    nDd = 2;
    step(grey, grey2, depth, points2(0, 0.0f));
    std::printf("  -- no previous feature\n");
    nPrev = n3 = nKp = nDd = 0;
    step(grey, grey2, depth, points2(0, 0.0f));
    std::printf("  -- removeTooCloseFeatures 1\n");
    m.matcherParameters.OpenCVParams.removeTooCloseFeatures = 1;
    step(cv::Mat(), grey2, depth, points2(0, 0.0f));
}

void runTrackKLT()
{
    say("trackKLT");
    FrameMatcherHIP m;
    m.setSampleSeed(29);
    m.matcherParameters.RANSACParams.errorVersionVO = 1;
    m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 3;
    const cv::Mat depth = image(ROWS, COLS, CV_16U, 5);
    const auto klt = [&](const cv::Mat &img, const cv::Mat &d) {
        Eigen::Matrix4f T;
        std::vector<cv::DMatch> inl = someMatches(1, 1, 1);
        std::printf("  returns %.17g\n", m.trackKLT(img, d, 5000.0, T, inl));
        show("pose", T);
        show("inliers", inl);
        FrameMatcher::featureSet fs = m.getFeatures();
        show("kept descriptors", fs.descriptors);
        show("kept points", fs.feature3D);
    };
    klt(image(ROWS, COLS, CV_8UC1, 3), depth);
    klt(image(ROWS, COLS, CV_8UC1, 4), depth);
    m.matcherParameters.distortionCoeffsMat = distortion(1, 4);
    klt(image(ROWS, COLS, CV_8UC1, 5), depth);
    imageRefusals(false, true, [&](const cv::Mat &, const cv::Mat &b, const cv::Mat &d) { klt(b, d); });
    std::printf("  -- the closing call failing, then the tracking call\n");
    recorderFailNext("ps_track_close_pair", PS_ERR_HIP);
    klt(image(ROWS, COLS, CV_8UC1, 6), depth);
    recorderFailNext("ps_track_vo_pair", PS_ERR_HIP);
    klt(image(ROWS, COLS, CV_8UC1, 6), depth);
    std::printf("  -- 3 channels on a matcher with no state\n");
    FrameMatcherHIP m3;
    m3.setSampleSeed(31);
    Eigen::Matrix4f T;
    std::vector<cv::DMatch> inl;
    std::printf("  returns %.17g\n", m3.trackKLT(image(ROWS, COLS, CV_8UC3, 3), depth, 1000.0, T, inl));
    std::printf("  returns %.17g\n", m3.trackKLT(image(ROWS, COLS, CV_8UC3, 4), depth, 1000.0, T, inl));
    show("pose", T);
    show("inliers", inl);
    std::printf("  -- detector SURF, descriptor SIFT, removeTooCloseFeatures 1, maximalTrackedFeatures 0\n");
    m.matcherParameters.OpenCVParams.detector = "SURF";
    klt(cv::Mat(), depth);
    m.matcherParameters.OpenCVParams.detector = "ORB";
    m.matcherParameters.OpenCVParams.descriptor = "SIFT";
    klt(cv::Mat(), depth);
    m.matcherParameters.OpenCVParams.descriptor = "ORB";
    m.matcherParameters.OpenCVParams.removeTooCloseFeatures = 1;
    klt(cv::Mat(), depth);
    m.matcherParameters.OpenCVParams.removeTooCloseFeatures = 0;
    m.matcherParameters.OpenCVParams.maximalTrackedFeatures = 0;
    klt(cv::Mat(), depth);
}

void runTrajectory()
{
    say("VOTrajectory");
    VOTrajectory t;
    Eigen::Matrix4f inc = Eigen::Matrix4f::Identity();
    inc(0, 3) = 0.05f;
    inc(0, 1) = -0.1f;
    inc(1, 0) = 0.1f;
    t.addIncrement(inc);
    t.addIncrement(inc);
    inc(2, 3) = 0.5f; // (beyond the 0.1 m gate: taken as the identity)
    t.addIncrement(inc);
    show("pose", t.VOPoseEstimate);
    std::printf("  %s\n", VOTrajectory::freiburgLine(t.VOPoseEstimate, 1305031102.175304).c_str());
}

} // namespace

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0); // one stream in one order: the recorder's lines, std::cout and std::cerr
    std::cout << std::unitbuf;
    {
        say("a thread whose context cannot be created (PUTSLAM_HIP_DEVICE=3)");
        setenv("PUTSLAM_HIP_DEVICE", "3", 1);
        std::thread t([] {
            recorderFailNext("ps_context_create", PS_ERR_NO_DEVICE);
            show("hamming", hammingCrossCheckMatch(binaryRows(3, 3), binaryRows(4, 5)));
            std::vector<cv::KeyPoint> k = keyPoints(3);
            DBScan().run(k);
            show("key points", k);
        });
        t.join();
        setenv("PUTSLAM_HIP_DEVICE", "1", 1);
    }
    runRansac();
    unsetenv("PUTSLAM_HIP_DEVICE");
    runRgbd();
    runDbscanKabsch();
    runExclusion();
    runMatch();
    runMatchXYZ();
    runPipeline();
    runTracking();
    runDetectDescribe();
    runFrontEnd();
    runTrackStep();
    runTrackKLT();
    runTrajectory();
    say("done");
    return 0;
}
