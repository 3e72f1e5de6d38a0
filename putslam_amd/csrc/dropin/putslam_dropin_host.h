// putslam_dropin_host.h -- the pure parts of putslam_dropin.cpp, its only includer: what the entry points accept, the parameter blocks
// they hand to the C ABI and the key points they hand back, each stated once.  Functions of their inputs alone: no HIP runtime call,
// no PsContext (tests/test_dropin_calls_host.py holds the calls they lead to to a recorded transcript).  Internal linkage: none of
// this is a symbol of libputslam_dropin.so.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <ctime>

#include "putslam_dropin.h"
#include "putslam_hip.h"

namespace {

typedef putslam_hip::FrameMatcher::MatcherParameters MatcherParams;
typedef putslam_hip::FrameMatcher::MapFeatureXYZ MapFeatureXYZ;

// ---- what the image entry points take (each caller keeps its own message) ----
// an 8-bit image of 1 or 3 channels
bool image8u(const cv::Mat &m) { return !m.empty() && m.depth() == CV_8U && (m.channels() == 1 || m.channels() == 3); }
// ... and a previous one of the same type, size and step
bool imagePair8u(const cv::Mat &prev, const cv::Mat &img)
{
    return image8u(prev) && !img.empty() && prev.type() == img.type() && prev.rows == img.rows && prev.cols == img.cols && prev.step == img.step;
}
// a CV_16U depth image of the image's size
bool depth16uOf(const cv::Mat &depth, const cv::Mat &img) { return !depth.empty() && depth.type() == CV_16U && depth.rows == img.rows && depth.cols == img.cols; }

// ---- parameter blocks ----
void cameraToK(const cv::Mat &cameraMatrix, float K[9], bool &have)
{
    have = !cameraMatrix.empty() && cameraMatrix.rows >= 3 && cameraMatrix.cols >= 3;
    for (int i = 0; i < 9; ++i) K[i] = 0.0f;
    if (have)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K[3 * r + c] = cameraMatrix.at<float>(r, c);
}

// (k1, k2, p1, p2, k3) of a 1 x N or N x 1 CV_32F Mat; what it does not have is 0
void distortion5(const cv::Mat &dc, double dist5[5])
{
    const int nd = dc.empty() ? 0 : dc.rows * dc.cols;
    for (int i = 0; i < 5; ++i) dist5[i] = i < nd ? (double)dc.at<float>(dc.rows == 1 ? 0 : i, dc.rows == 1 ? i : 0) : 0.0;
}

PsFrameGeometry frameGeometry(const MatcherParams &mp, double depthImageScale)
{
    PsFrameGeometry geo;
    bool haveK;
    cameraToK(mp.cameraMatrixMat, geo.K, haveK);
    distortion5(mp.distortionCoeffsMat, geo.dist5);
    geo.depthImageScale = depthImageScale;
    return geo;
}

const float orbScaleFactor = 1.2f; // cv::ORB::create()'s defaults (matcherOpenCV.cpp:67, :90)
const int orbLevels = 8;

PsOrbDetectParams orbDetectParams(const MatcherParams &mp)
{
    PsOrbDetectParams prm;
    prm.nFeatures = 500;
    prm.scaleFactor = orbScaleFactor;
    prm.nLevels = orbLevels;
    prm.fastThreshold = 20;
    prm.gridRows = mp.OpenCVParams.gridRows;
    prm.gridCols = mp.OpenCVParams.gridCols;
    prm.maximalTrackedFeatures = mp.OpenCVParams.maximalTrackedFeatures;
    prm.reserved = 0;
    return prm;
}

PsOrbParams orbDescribeParams()
{
    PsOrbParams prm;
    prm.scaleFactor = orbScaleFactor;
    prm.nLevels = orbLevels;
    prm.reserved[0] = prm.reserved[1] = 0;
    return prm;
}

PsFrontEndParams frontEndParams(const MatcherParams &mp)
{
    PsFrontEndParams prm;
    prm.detect = orbDetectParams(mp);
    prm.describe = orbDescribeParams();
    prm.DBScanEps = mp.OpenCVParams.DBScanEps;
    return prm;
}

// the tracker's block, matcherOpenCV.cpp:220-238
PsKltParams kltParams(const MatcherParams &mp)
{
    const auto &cvp = mp.OpenCVParams;
    PsKltParams prm;
    prm.eps = cvp.eps;                                 // :220-222, TermCriteria(ITER | EPS, maxIter, eps)
    prm.minEigThreshold = cvp.trackingMinEigThreshold; // :238
    prm.winSize = cvp.winSize;                         // :234-235
    prm.maxLevels = cvp.maxLevels;                     // :236
    prm.maxCount = cvp.maxIter;
    prm.flags = (cvp.useInitialFlow > 0 ? PS_KLT_USE_INITIAL_FLOW : 0) | (cvp.trackingErrorType > 0 ? PS_KLT_GET_MIN_EIGENVALS : 0); // :225-229
    return prm;
}

// ---- RANSAC ----
int ransacIterations(double inlierRatio, double successProbability = 0.98, int numberOfPairs = 3)
{
    // RANSAC::computeRANSACIteration, RANSAC.cpp:457-461 (saturating instead of UB)
    double v = std::log(1 - successProbability) / std::log(1 - std::pow(inlierRatio, numberOfPairs));
    if (!(v < 2147483647.0)) return 2147483647;
    return v < 0 ? 0 : (int)v;
}

int defaultIterationCount() { return ransacIterations(0.20); } // RANSAC.cpp:30

// enough samples for the longest schedule the reference can run: max(iters(0.2), iters(minRatio))
int hypothesisCount(double minimalInlierRatioThreshold)
{
    return std::max(1, std::min(std::max(defaultIterationCount(), ransacIterations(minimalInlierRatioThreshold)), PS_MAX_HYPOTHESES));
}

// (P: RANSAC::parameters, or PUTSLAMEstimator::parameters, which has no minimalNumberOfMatches)
template <class P> PsRansacParams toPs(const P &p, int minimalNumberOfMatches, int iterationCount)
{
    PsRansacParams q;
    std::memset(&q, 0, sizeof q); // padding bytes too: the C ABI may compare parameter blocks bytewise
    q.verbose = p.verbose;
    q.errorVersion = p.errorVersion;
    q.errorVersionVO = p.errorVersionVO;
    q.errorVersionMap = p.errorVersionMap;
    q.inlierThresholdEuclidean = p.inlierThresholdEuclidean;
    q.inlierThresholdReprojection = p.inlierThresholdReprojection;
    q.inlierThresholdMahalanobis = p.inlierThresholdMahalanobis;
    q.minimalInlierRatioThreshold = p.minimalInlierRatioThreshold;
    q.minimalNumberOfMatches = minimalNumberOfMatches;
    q.usedPairs = p.usedPairs;
    q.iterationCount = iterationCount;
    return q;
}
PsRansacParams toPs(const RANSAC::parameters &p) { return toPs(p, p.minimalNumberOfMatches, p.iterationCount); }

PsRansacConfig ransacConfig(int estimator, int numHypotheses, uint64_t seed)
{
    PsRansacConfig cfg;
    cfg.estimator = estimator;
    cfg.numHypotheses = numHypotheses;
    cfg.seed = seed;
    cfg.sampleIdx = nullptr;
    return cfg;
}

// a matcher's seed + offset once setSampleSeed was called, else the clock (the reference: srand(time(0)), RANSAC.cpp:13)
uint64_t sampleSeed(bool seeded, uint64_t seed, uint64_t offset) { return seeded ? seed + offset : (uint64_t)std::time(nullptr); }

// What a `RANSAC ransac(p, cameraMatrix)` built per call runs with (matcher.cpp:493): its constructor's iteration count, the longest
// schedule's worth of hypotheses.
struct VoRansac { PsRansacParams prm; PsRansacConfig cfg; };
VoRansac voRansac(RANSAC::parameters p, uint64_t seed)
{
    p.iterationCount = defaultIterationCount();
    return VoRansac{toPs(p), ransacConfig(PS_EST_RANSAC, hypothesisCount(p.minimalInlierRatioThreshold), seed)};
}

// ---- key points ----
// the key point detectFeaturesORB makes: size = patchSize * scale of the level, class_id -1
cv::KeyPoint orbKeyPoint(const cv::Point2f &pt, float angle, float response, int32_t octave)
{
    cv::KeyPoint kp;
    kp.pt = pt;
    kp.size = 31.f * (float)std::pow((double)orbScaleFactor, (double)octave);
    kp.angle = angle;
    kp.response = response;
    kp.octave = octave;
    kp.class_id = -1;
    return kp;
}

// matcherOpenCV.cpp:240-245 then :267-290: a survivor keeps the previous frame's key point (its pt moved) and detection distance
void carryKeyPoint(const std::vector<cv::KeyPoint> &prevKeyPoints, const std::vector<double> &prevDetDists, int32_t keptIdx, const cv::Point2f &pt,
                   std::vector<cv::KeyPoint> &keyPoints, std::vector<double> &detDists)
{
    cv::KeyPoint kp = prevKeyPoints[(size_t)keptIdx];
    kp.pt = pt;
    keyPoints.push_back(kp);
    detDists.push_back(prevDetDists[(size_t)keptIdx]);
}

// ---- guided map matching ----
// matcher.cpp:616-622 for computationNumber = k
struct MapTry { double sphereRadius, acceptRatio; };
MapTry mapTry(const MatcherParams &mp, int k)
{
    MapTry t = {mp.OpenCVParams.matchingXYZSphereRadius, mp.OpenCVParams.matchingXYZacceptRatioOfBestMatch};
    if (k > 1) {
        t.sphereRadius += 0.02 * (k - 1);
        t.acceptRatio = std::max(0.1, t.acceptRatio - 0.05 * (k - 1));
    }
    return t;
}

// matcher.cpp:681-692: the predicted level of a map feature seen from the frame's origin, and its position as the C ABI takes it
int32_t mapFeatureLevel(const MapFeatureXYZ &f)
{
    const double curDist = std::sqrt(f.position[0] * f.position[0] + f.position[1] * f.position[1] + f.position[2] * f.position[2]);
    return ps_predicted_level(f.octave, f.detDist, curDist);
}
Eigen::Vector3f mapFeaturePosition(const MapFeatureXYZ &f) { return Eigen::Vector3f((float)f.position[0], (float)f.position[1], (float)f.position[2]); }

// :639-652, a frame feature's; curDist = Eigen float norm()
int32_t frameFeatureLevel(const Eigen::Vector3f &p, int octave, double detDist)
{
    const float nrm = std::sqrt(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2]));
    return ps_predicted_level(octave, detDist, (double)nrm);
}

} // namespace
