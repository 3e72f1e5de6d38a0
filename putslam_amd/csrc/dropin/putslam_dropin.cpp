// putslam_dropin.cpp -- reference-shaped C++ classes over the C ABI (see putslam_dropin.h).
// Host code only: marshals std::vector / cv::Mat / Eigen storage into plain pointers and calls
// libputslam_hip.so.  One PsContext (HIP stream + scratch arena) per calling thread, because the
// reference constructs a fresh RANSAC object per call (matcher.cpp:493) and runs a second Matcher on
// the loop-closure thread (featuresMap.cpp:650-652): contexts are never shared between threads.
#include "putslam_dropin.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <iomanip>

#include "putslam_dropin_host.h" // the pure parts: image checks, parameter blocks, key points (and <algorithm>, <cmath>, <cstring>, <ctime>)

#include <hip/hip_runtime_api.h> // device block of matchXYZLadder (the C ABI takes device pointers there)

static_assert(sizeof(cv::DMatch) == sizeof(PsDMatch), "cv::DMatch layout");
static_assert(sizeof(Eigen::Vector3f) == 12, "Eigen::Vector3f storage");
static_assert(sizeof(cv::Point2f) == 8, "cv::Point2f storage");

namespace {

// a context on the device PUTSLAM_HIP_DEVICE names (0 without it)
int createContext(PsContext **ctx)
{
    int dev = 0;
    if (const char *e = std::getenv("PUTSLAM_HIP_DEVICE")) dev = std::atoi(e);
    return ps_context_create(dev, ctx);
}

// the text of the C ABI call that just failed on ctx, on std::cerr
void reportError(const PsContext *ctx) { std::cerr << "putslam_hip: " << ps_last_error(ctx) << std::endl; }

struct ThreadContext {
    PsContext *ctx = nullptr;
    int status = PS_OK;
    ThreadContext()
    {
        status = createContext(&ctx);
        if (status != PS_OK)
            std::cerr << "putslam_hip: no usable HIP device (status " << status << "); the GPU path has no CPU fallback"
                      << std::endl;
    }
    ~ThreadContext() { ps_context_destroy(ctx); }
};

PsContext *threadContext(int *status)
{
    static thread_local ThreadContext tc;
    if (status) *status = tc.status;
    return tc.ctx;
}

Eigen::Matrix4f runEstimator(int estimator, int H, uint64_t seed, const PsRansacParams &prm, const cv::Mat &cameraMatrix,
                             const std::vector<Eigen::Vector3f> &prev, const std::vector<Eigen::Vector3f> &cur,
                             const std::vector<cv::DMatch> &matches, std::vector<cv::DMatch> &inliers, bool clearOnFail,
                             int &status)
{
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    PsContext *ctx = threadContext(&status);
    if (!ctx) {
        if (clearOnFail) inliers.clear();
        return pose;
    }
    float K[9];
    bool haveK;
    cameraToK(cameraMatrix, K, haveK);
    const PsRansacConfig cfg = ransacConfig(estimator, H, seed);
    std::vector<cv::DMatch> out(matches.size() ? matches.size() : 1);
    int n = 0;
    PsRansacStats st;
    status = ps_ransac_rigid3d(ctx, &prm, &cfg, haveK ? K : nullptr, reinterpret_cast<const float *>(prev.data()),
                               (int)prev.size(), reinterpret_cast<const float *>(cur.data()), (int)cur.size(),
                               reinterpret_cast<const PsDMatch *>(matches.data()), (int)matches.size(), pose.data(),
                               reinterpret_cast<PsDMatch *>(out.data()), &n, nullptr, &st);
    if (status != PS_OK) {
        reportError(ctx);
        pose = Eigen::Matrix4f::Identity();
        if (clearOnFail) inliers.clear();
        return pose;
    }
    if (estimator == PS_EST_USAC && st.numMatchesValid < 8) return pose; // USAC_wrapper.cpp:120-122: inliers untouched
    out.resize((size_t)n);
    inliers.swap(out);
    if (prm.verbose > 0) {
        std::cout << "RANSAC: matches.size() = " << st.numMatchesValid << std::endl;
        std::cout << "RANSAC best model : inlierRatio = " << st.bestInlierRatio * 100.0 << "%" << std::endl;
    }
    return pose;
}

} // namespace

// ---------------------------------------------------------------------------------------------
RANSAC::RANSAC(RANSAC::parameters _RANSACParameters, cv::Mat _cameraMatrix)
{
    seed_ = (uint64_t)std::time(nullptr); // the reference: srand(time(0)), RANSAC.cpp:13
    cameraMatrix = _cameraMatrix;
    RANSACParams = _RANSACParameters;
    RANSACParams.iterationCount = defaultIterationCount();
    if (RANSACParams.verbose > 0) {
        std::cout << "RANSACParams.verbose --> " << RANSACParams.verbose << std::endl;
        std::cout << "RANSACParams.usedPairs --> " << RANSACParams.usedPairs << std::endl;
        std::cout << "RANSACParams.errorVersion --> " << RANSACParams.errorVersion << std::endl;
        std::cout << "RANSACParams.inlierThresholdEuclidean --> " << RANSACParams.inlierThresholdEuclidean << std::endl;
        std::cout << "RANSACParams.inlierThresholdReprojection --> " << RANSACParams.inlierThresholdReprojection << std::endl;
        std::cout << "RANSACParams.minimalInlierRatioThreshold --> " << RANSACParams.minimalInlierRatioThreshold << std::endl;
    }
}

Eigen::Matrix4f RANSAC::estimateTransformation(std::vector<Eigen::Vector3f> prevFeatures, std::vector<Eigen::Vector3f> features,
                                               std::vector<cv::DMatch> matches, std::vector<cv::DMatch> &bestInlierMatches)
{
    if (RANSACParams.verbose > 0) std::cout << "RANSAC: original matches.size() = " << matches.size() << std::endl;
    if (RANSACParams.errorVersion != EUCLIDEAN_ERROR && RANSACParams.errorVersion != REPROJECTION_ERROR &&
        RANSACParams.errorVersion != EUCLIDEAN_AND_REPROJECTION_ERROR && RANSACParams.errorVersion != ADAPTIVE_ERROR)
        std::cout << "RANSAC: incorrect error version" << std::endl; // RANSAC.cpp:134-135 (once per call here, not per iteration)
    return runEstimator(PS_EST_RANSAC, hypothesisCount(RANSACParams.minimalInlierRatioThreshold), seed_, toPs(RANSACParams), cameraMatrix,
                        prevFeatures, features, matches, bestInlierMatches, true, lastStatus_);
}

// ---------------------------------------------------------------------------------------------
RANSAC_USAC::RANSAC_USAC(PUTSLAMEstimator::parameters p, cv::Mat _cameraMatrix)
{
    seed_ = (uint64_t)std::time(nullptr); // USAC_wrapper.cpp:16
    cameraMatrix = _cameraMatrix;
    params_ = p;
}
RANSAC_USAC::~RANSAC_USAC() {}

Eigen::Matrix4f RANSAC_USAC::estimateTransformation(std::vector<Eigen::Vector3f> prevFeatures, std::vector<Eigen::Vector3f> features,
                                                    std::vector<cv::DMatch> matches, std::vector<cv::DMatch> &bestInlierMatches)
{
    const PsRansacParams prm = toPs(params_, 8, 0); // minimalNumberOfMatches 8: USAC_wrapper.cpp:120; no iteration count
    return runEstimator(PS_EST_USAC, maxHyp_, seed_, prm, cameraMatrix, prevFeatures, features, matches, bestInlierMatches, false,
                        lastStatus_);
}

// ---------------------------------------------------------------------------------------------
int RGBD::roundSize(double x, int size)
{
    if (x < 0)
        x = 0;
    else if (x > size - 1)
        x = size;
    return (int)std::round(x);
}

std::vector<Eigen::Vector3f> RGBD::keypoints2Dto3D(std::vector<cv::Point2f> f2d, cv::Mat depthImage, cv::Mat cameraMatrix,
                                                   double depthImageScale, int startingID)
{
    size_t n = f2d.size() > (size_t)startingID ? f2d.size() - (size_t)startingID : 0;
    std::vector<Eigen::Vector3f> out(n);
    if (n == 0) return out;
    int status;
    PsContext *ctx = threadContext(&status);
    float K[9];
    bool haveK;
    cameraToK(cameraMatrix, K, haveK);
    if (!ctx) return out;
    status = ps_keypoints2Dto3D(ctx, reinterpret_cast<const float *>(f2d.data() + startingID), (int)n,
                                reinterpret_cast<const uint16_t *>(depthImage.data), depthImage.rows, depthImage.cols,
                                (size_t)depthImage.step, K, depthImageScale, reinterpret_cast<float *>(out.data()));
    if (status != PS_OK) reportError(ctx);
    return out;
}

// ---------------------------------------------------------------------------------------------
DBScan::DBScan(double eps_, int minPts_, int featuresFromCluster_) : eps(eps_), minPts(minPts_), featuresFromCluster(featuresFromCluster_)
{
}

void DBScan::run(std::vector<cv::KeyPoint> &clusteringSet)
{
    const size_t n = clusteringSet.size();
    if (n == 0) return;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return;
    std::vector<int32_t> kept(n);
    int nkept = 0;
    status = ps_dbscan_thin(ctx, &clusteringSet[0].pt.x, sizeof(cv::KeyPoint), &clusteringSet[0].octave, sizeof(cv::KeyPoint),
                            (int)n, eps, minPts, featuresFromCluster, kept.data(), &nkept);
    if (status != PS_OK) {
        reportError(ctx);
        return;
    }
    // kept[] ascends and kept[j] >= j: compacting in place never overwrites a survivor before it is moved
    for (int j = 0; j < nkept; ++j)
        if (kept[j] != j) clusteringSet[j] = clusteringSet[kept[j]];
    clusteringSet.resize((size_t)nkept);
}

// ---------------------------------------------------------------------------------------------
// Spatial-exclusion filters (ps_exclude)
namespace {
// the accepted candidate indices under `rule`; false (and the text on stderr) if the call failed
bool excludeCall(const PsExclusionRule &rule, const std::vector<Eigen::Vector3f> *cand3, const std::vector<cv::Point2f> &cand2,
                 const std::vector<Eigen::Vector3f> *exist3, const std::vector<cv::Point2f> &exist2, std::vector<int32_t> &kept)
{
    kept.clear();
    const size_t n = cand2.size(), m = exist2.size();
    if (n == 0) return true;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return false;
    kept.resize(n);
    int nkept = 0;
    status = ps_exclude(ctx, &rule, cand3 ? reinterpret_cast<const float *>(cand3->data()) : nullptr,
                        reinterpret_cast<const float *>(cand2.data()), (int)n,
                        exist3 && m ? reinterpret_cast<const float *>(exist3->data()) : nullptr,
                        m ? reinterpret_cast<const float *>(exist2.data()) : nullptr, (int)m, kept.data(), &nkept);
    if (status != PS_OK) {
        reportError(ctx);
        kept.clear();
        return false;
    }
    kept.resize((size_t)nkept);
    return true;
}

// v keeps the entries at the ascending positions stay[] (std::remove_if with a counting predicate, matcher.cpp:922-956)
template <class T> void keepPositions(std::vector<T> &v, const std::vector<int32_t> &stay)
{
    for (size_t j = 0; j < stay.size(); ++j)
        if ((size_t)stay[j] != j) v[j] = v[(size_t)stay[j]];
    v.resize(stay.size());
}
} // namespace

namespace putslam_hip {

int chooseFeaturesToAddToMap(const std::vector<Eigen::Vector3f> &feature3D, const std::vector<cv::Point2f> &undistortedFeature2D,
                             int addedCounter, int maxOnceFeatureAdd, const std::vector<Eigen::Vector3f> &mapFeaturePositions,
                             const std::vector<cv::Point2f> &mapFeatureUV, float minEuclideanDistanceOfFeatures,
                             float minImageDistanceOfFeatures, std::vector<int> &acceptedIndices)
{
    acceptedIndices.clear();
    if (feature3D.size() != undistortedFeature2D.size() || mapFeaturePositions.size() != mapFeatureUV.size()) {
        std::cerr << "putslam_hip: chooseFeaturesToAddToMap: list sizes differ" << std::endl; // (the reference asserts, :104-109)
        return addedCounter;
    }
    if (addedCounter >= maxOnceFeatureAdd) return addedCounter; // :113
    PsExclusionRule rule;
    // (the difference is formed as long long: maxOnceFeatureAdd - addedCounter may not fit an int for a negative counter)
    const long long room = (long long)maxOnceFeatureAdd - (long long)addedCounter;
    ps_exclusion_rule_new_map_features((double)minEuclideanDistanceOfFeatures, (double)minImageDistanceOfFeatures,
                                       room > 0x7fffffffLL ? 0x7fffffff : (int)room, &rule);
    std::vector<int32_t> kept;
    if (!excludeCall(rule, &feature3D, undistortedFeature2D, &mapFeaturePositions, mapFeatureUV, kept)) return addedCounter;
    acceptedIndices.assign(kept.begin(), kept.end());
    return addedCounter + (int)kept.size();
}

void FrameMatcher::mergeTrackedFeatures(std::vector<cv::Point2f> &undistortedFeatures2D,
                                        const std::vector<cv::Point2f> &featuresSandBoxUndistorted,
                                        std::vector<cv::Point2f> &distortedFeatures2D,
                                        const std::vector<cv::Point2f> &featuresSandBoxDistorted,
                                        std::vector<Eigen::Vector3f> &features3D, const std::vector<Eigen::Vector3f> &features3DSandBox,
                                        std::vector<cv::KeyPoint> &keyPoints, const std::vector<cv::KeyPoint> &keyPointsSandBox,
                                        std::vector<double> &detDists, const std::vector<double> &detDistsSandBox)
{
    PsExclusionRule rule;
    ps_exclusion_rule_merge_tracked(matcherParameters.OpenCVParams.minimalReprojDistanceNewTrackingFeatures, &rule);
    std::vector<int32_t> kept;
    if (!excludeCall(rule, nullptr, featuresSandBoxUndistorted, nullptr, undistortedFeatures2D, kept)) return;
    for (int32_t i : kept) { // :121-127
        undistortedFeatures2D.push_back(featuresSandBoxUndistorted[(size_t)i]);
        distortedFeatures2D.push_back(featuresSandBoxDistorted[(size_t)i]);
        features3D.push_back(features3DSandBox[(size_t)i]);
        keyPoints.push_back(keyPointsSandBox[(size_t)i]);
        detDists.push_back(detDistsSandBox[(size_t)i]);
    }
}

std::set<int> FrameMatcher::removeTooCloseFeatures(std::vector<cv::Point2f> &distortedFeatures2D,
                                                   std::vector<cv::Point2f> &undistortedFeatures2D,
                                                   std::vector<Eigen::Vector3f> &features3D, std::vector<cv::KeyPoint> &keyPoints,
                                                   std::vector<double> &detDists, std::vector<cv::DMatch> &matches)
{
    std::set<int> featuresToRemove;
    if (undistortedFeatures2D.size() != features3D.size()) { // (the reference asserts, :895-898)
        std::cerr << "putslam_hip: removeTooCloseFeatures: list sizes differ" << std::endl;
        return featuresToRemove;
    }
    PsExclusionRule rule;
    ps_exclusion_rule_too_close(matcherParameters.OpenCVParams.minimalEuclidDistanceNewTrackingFeatures,
                                matcherParameters.OpenCVParams.minimalReprojDistanceNewTrackingFeatures, &rule);
    std::vector<int32_t> stay;
    const std::vector<cv::Point2f> none;
    if (!excludeCall(rule, &features3D, undistortedFeatures2D, nullptr, none, stay)) return featuresToRemove;
    const int n = (int)features3D.size();
    for (int i = 0, j = 0; i < n; ++i) {
        if (j < (int)stay.size() && stay[(size_t)j] == i)
            ++j;
        else
            featuresToRemove.insert(i);
    }
    // each list loses the positions in featuresToRemove that it has (:921-956: the counting predicate runs over the list's own length)
    auto erase = [&](auto &v) {
        std::vector<int32_t> s;
        for (int32_t i : stay)
            if ((size_t)i < v.size()) s.push_back(i);
        for (size_t i = (size_t)n; i < v.size(); ++i) s.push_back((int32_t)i);
        keepPositions(v, s);
    };
    erase(distortedFeatures2D);
    erase(undistortedFeatures2D);
    erase(features3D);
    erase(keyPoints);
    erase(detDists);
    matches.erase(std::remove_if(matches.begin(), matches.end(),
                                 [&](const cv::DMatch &o) { return featuresToRemove.find(o.trainIdx) != featuresToRemove.end(); }),
                  matches.end()); // :960-963
    return featuresToRemove;
}

} // namespace putslam_hip

std::vector<cv::Point2f> RGBD::removeImageDistortion(std::vector<cv::Point2f> &features, cv::Mat cameraMatrix, cv::Mat distCoeffs)
{
    if (features.size() == 0) return std::vector<cv::Point2f>(); // RGBD.cpp:258-259
    std::vector<cv::Point2f> out(features.size());
    int status;
    PsContext *ctx = threadContext(&status);
    float K[9];
    bool haveK;
    cameraToK(cameraMatrix, K, haveK);
    double d[5];
    distortion5(distCoeffs, d);
    if (!ctx) return out;
    status = ps_remove_image_distortion(ctx, reinterpret_cast<const float *>(features.data()), (int)features.size(), K, d,
                                        reinterpret_cast<float *>(out.data()));
    if (status != PS_OK) reportError(ctx);
    return out;
}

std::vector<cv::Point2f> RGBD::points3Dto2D(std::vector<Eigen::Vector3f> f3d, cv::Mat cameraMatrix)
{
    std::vector<cv::Point2f> out(f3d.size());
    if (f3d.empty()) return out;
    int status;
    PsContext *ctx = threadContext(&status);
    float K[9];
    bool haveK;
    cameraToK(cameraMatrix, K, haveK);
    if (!ctx) return out;
    status = ps_points3Dto2D(ctx, reinterpret_cast<const float *>(f3d.data()), (int)f3d.size(), K,
                             reinterpret_cast<float *>(out.data()));
    if (status != PS_OK) reportError(ctx);
    return out;
}

namespace putslam {

// ---------------------------------------------------------------------------------------------
KabschEst::Ptr kabsch; // "A single instance of Kabsch Estimator", kabschEst.cpp:8

KabschEst::KabschEst(void) : name("Kabsch Estimator") {}
const std::string &KabschEst::getName() const { return name; }

Mat34 &KabschEst::computeTransformation(const Eigen::MatrixXd &setA, const Eigen::MatrixXd &setB)
{
    transformation.setIdentity();
    if (setA.rows() == 0) return transformation; // kabschEst.cpp:28
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return transformation;
    double T[16];
    status = ps_kabsch_f64(ctx, setA.data(), setB.data(), (int)setA.rows(), (int)setA.rows(), T);
    if (status != PS_OK) {
        reportError(ctx);
        return transformation;
    }
#if PUTSLAM_HAVE_CV_EIGEN
    std::memcpy(transformation.matrix().data(), T, sizeof T);
#else
    std::memcpy(transformation.data(), T, sizeof T);
#endif
    return transformation;
}

TransformEst *createKabschEstimator(void)
{
    kabsch.reset(new KabschEst());
    return kabsch.get();
}

} // namespace putslam

namespace putslam_hip {

// ---------------------------------------------------------------------------------------------
FrameMatcher::MatcherParameters::MatcherParameters()
{
    // shipped defaults, resources/putslammatcherOpenCVParameters.xml:29-37
    RANSACParams.verbose = 0;
    RANSACParams.errorVersion = 0;
    RANSACParams.errorVersionVO = 0;
    RANSACParams.errorVersionMap = 0;
    RANSACParams.inlierThresholdEuclidean = 0.04;
    RANSACParams.inlierThresholdReprojection = 2.0;
    RANSACParams.inlierThresholdMahalanobis = 0.0002;
    RANSACParams.minimalInlierRatioThreshold = 0.2;
    RANSACParams.minimalNumberOfMatches = 15;
    RANSACParams.usedPairs = 3;
    RANSACParams.iterationCount = 0;
    // resources/datasetConfig/freiburg1_desk.xml:5-6 (also hard-coded at RGBD.cpp:22-23)
    cameraMatrixMat = cv::Mat(3, 3, CV_32FC1);
    const float K[9] = {517.3f, 0.0f, 318.6f, 0.0f, 516.5f, 255.3f, 0.0f, 0.0f, 1.0f};
    for (int i = 0; i < 9; ++i) cameraMatrixMat.at<float>(i / 3, i % 3) = K[i];
    distortionCoeffsMat = cv::Mat(1, 5, CV_32FC1); // :7, rgbDistortion
    const float dist[5] = {-0.0410f, 0.3286f, 0.0087f, 0.0051f, -0.5643f};
    for (int i = 0; i < 5; ++i) distortionCoeffsMat.at<float>(0, i) = dist[i];
}

void FrameMatcher::detectInitFeatures(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D)
{
    prevDescriptors = descriptors;
    prevFeatures3D.swap(features3D);
    frameCounter = 0;
    fusedSynced_ = false;
}

// Resident-frame state of one matcher instance: its own context (stream + scratch) and the two-slot frame store.
struct FrameMatcher::Fused {
    PsContext *ctx = nullptr;
    PsVoStream *stream = nullptr;
    int cap = 0;
    PsVoStream *pipe = nullptr; // the pipelined form's stream (enqueueFrame / dequeueResult)
    int pipeCap = 0;
    std::vector<cv::DMatch> pm;
    std::vector<uint8_t> pmask;
    ~Fused()
    {
        if (pipe) ps_vo_stream_destroy(pipe);
        if (stream) ps_vo_stream_destroy(stream);
        if (ctx) ps_context_destroy(ctx);
    }
};

FrameMatcher::FrameMatcher(const std::string _name) : name(_name), frameCounter(0) {}
FrameMatcher::~FrameMatcher() {}

bool FrameMatcher::fusedMatchCall(const cv::Mat &descriptors, const std::vector<Eigen::Vector3f> &features3D,
                             Eigen::Matrix4f &estimatedTransformation, std::vector<cv::DMatch> &inlierMatches,
                             double &pointInlierRatio)
{
    const int n = (int)features3D.size(), np = (int)prevFeatures3D.size();
    if (n > PS_MAX_KPTS || np > PS_MAX_KPTS) return false;
    if ((n > 0 && (descriptors.cols != PS_DESC_BYTES || descriptors.rows != n)) ||
        (np > 0 && (prevDescriptors.cols != PS_DESC_BYTES || prevDescriptors.rows != np)))
        return false; // float descriptors / inconsistent sizes: the generic sequence reports them
    if (!fused_) fused_.reset(new Fused());
    Fused &f = *fused_;
    if (!f.ctx && createContext(&f.ctx) != PS_OK) {
        f.ctx = nullptr;
        return false;
    }
    const int need = std::max(std::max(n, np), 1);
    if (!f.stream || f.cap < need) {
        if (f.stream) ps_vo_stream_destroy(f.stream);
        f.stream = nullptr;
        f.cap = std::min(PS_MAX_KPTS, std::max(2048, need + need / 4));
        if (ps_vo_stream_create(f.ctx, f.cap, &f.stream) != PS_OK) {
            f.stream = nullptr;
            return false;
        }
        fusedSynced_ = false;
    }
    const VoRansac vo = voRansac(matcherParameters.RANSACParams, sampleSeed(seeded_, seed_, (uint64_t)frameCounter));
    float K[9];
    bool haveK;
    cameraToK(matcherParameters.cameraMatrixMat, K, haveK);
    std::vector<cv::DMatch> m((size_t)f.cap);
    std::vector<uint8_t> mask((size_t)f.cap);
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    PsRansacStats st;
    int nm = 0;
    if (!fusedSynced_) { // (re)load the previous frame as the resident one
        ps_vo_stream_reset(f.stream);
        int rc = ps_vo_stream_push(f.stream, &vo.prm, &vo.cfg, haveK ? K : nullptr, prevDescriptors.data,
                                   np > 0 ? (size_t)prevDescriptors.step : (size_t)PS_DESC_BYTES,
                                   reinterpret_cast<const float *>(prevFeatures3D.data()), np,
                                   reinterpret_cast<PsDMatch *>(m.data()), &nm, mask.data(), pose.data(), &st);
        if (rc != PS_OK) return false;
    }
    int rc = ps_vo_stream_push(f.stream, &vo.prm, &vo.cfg, haveK ? K : nullptr, descriptors.data,
                               n > 0 ? (size_t)descriptors.step : (size_t)PS_DESC_BYTES,
                               reinterpret_cast<const float *>(features3D.data()), n, reinterpret_cast<PsDMatch *>(m.data()),
                               &nm, mask.data(), pose.data(), &st);
    if (rc != PS_OK || nm < 0) {
        if (rc != PS_OK) reportError(f.ctx);
        fusedSynced_ = false;
        return false;
    }
    fusedSynced_ = true; // the frame just pushed is the resident "previous" one now
    inlierMatches.clear();
    inlierMatches.reserve((size_t)st.numInliers);
    for (int i = 0; i < nm; ++i)
        if (mask[(size_t)i]) inlierMatches.push_back(m[(size_t)i]);
    estimatedTransformation = pose;
    // RANSAC::pointInlierRatio (RANSAC.h:56-66) was evaluated on the device with two bitmaps over trainIdx
    // (unique inlier train indices / unique matched train indices, 0/0 = NaN like the reference's set sizes)
    pointInlierRatio = st.pointInlierRatio;
    return true;
}

// ---- pipelined form of runVO -------------------------------------------------------------------
void FrameMatcher::setPipeline(int chunkFrames, int lanes)
{
    pipeChunk_ = chunkFrames;
    pipeLanes_ = lanes;
    resetPipeline();
}

void FrameMatcher::resetPipeline()
{
    if (fused_ && fused_->pipe) {
        ps_vo_stream_destroy(fused_->pipe); // (drains; results not dequeued are dropped)
        fused_->pipe = nullptr;
    }
    pipeFirst_ = true;
}

// (re)builds the pipelined stream with room for `cap` keypoints per frame; pair 0 of the new pipeline is pair `pairsSoFar` of
// the sequence (it draws from seed + pairsSoFar, as it would have without the rebuild)
bool FrameMatcher::buildPipeline(int cap, uint64_t pairsSoFar)
{
    Fused &f = *fused_;
    if (f.pipe) {
        ps_vo_stream_destroy(f.pipe);
        f.pipe = nullptr;
    }
    f.pipeCap = cap;
    if (ps_vo_stream_create(f.ctx, f.pipeCap, &f.pipe) != PS_OK) {
        lastError_ = std::string("ps_vo_stream_create: ") + ps_last_error(f.ctx);
        f.pipe = nullptr;
        return false;
    }
    matcherParameters.RANSACParams.errorVersion = matcherParameters.RANSACParams.errorVersionVO; // matcher.cpp:491-492
    // pair k of the pipeline draws from seed + k: runVO's seeding (seed_ + frameCounter, the counter starting at 0 with the
    // initial frame)
    if (!pipeSeeded_) {
        pipeSeed_ = sampleSeed(seeded_, seed_, 0);
        pipeSeeded_ = true;
    }
    const VoRansac vo = voRansac(matcherParameters.RANSACParams, pipeSeed_ + pairsSoFar);
    float K[9];
    bool haveK;
    cameraToK(matcherParameters.cameraMatrixMat, K, haveK);
    // what comes back per frame is what Matcher::match returns: the inlier matches in input order + the pose (matcher.cpp:452-516)
    ps_vo_stream_set_result_mode(f.pipe, PS_RESULTS_INLIERS);
    if (ps_vo_stream_configure_async(f.pipe, &vo.prm, &vo.cfg, haveK ? K : nullptr, pipeChunk_, pipeLanes_) != PS_OK) {
        lastError_ = std::string("ps_vo_stream_configure_async: ") + ps_last_error(f.ctx);
        ps_vo_stream_destroy(f.pipe);
        f.pipe = nullptr;
        return false;
    }
    f.pm.resize((size_t)f.pipeCap);
    f.pmask.resize((size_t)f.pipeCap);
    return true;
}

bool FrameMatcher::enqueueFrame(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D)
{
    const int st = enqueueFrameStatus(descriptors, std::move(features3D));
    if (st < 0) std::cerr << "putslam_hip: " << lastError_ << std::endl;
    return st == 1;
}

int FrameMatcher::enqueueFrameStatus(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D)
{
    const int n = (int)features3D.size();
    if (n > PS_MAX_KPTS || (n > 0 && (descriptors.cols != PS_DESC_BYTES || descriptors.rows != n))) {
        lastError_ = "enqueueFrame: descriptors must be n x 32 bytes with n <= PS_MAX_KPTS rows, one per 3-D feature";
        return -1;
    }
    if (!fused_) fused_.reset(new Fused());
    Fused &f = *fused_;
    if (!f.ctx && createContext(&f.ctx) != PS_OK) {
        f.ctx = nullptr;
        lastError_ = "ps_context_create failed (no usable HIP device; there is no CPU fallback)";
        return -1;
    }
    if (!f.pipe) {
        // room for a quarter more keypoints than the first frame has; a later frame with more rebuilds the pipeline (below)
        pipeSeeded_ = false;
        if (!buildPipeline(std::min(PS_MAX_KPTS, std::max(2048, n + n / 4)), 0)) return -1;
        pipeFirst_ = true;
    }
    if (n > f.pipeCap) {
        // A frame with more keypoints than the pipeline was built for (runVO's synchronous stream regrows in place; here chunks
        // are in flight).  While results are pending the caller is told "busy" -- the `while (!enqueueFrame) dequeueResult` loop
        // drains them --; with nothing pending the pipeline is rebuilt with more room, the previous frame goes in again as its
        // initial frame and pair numbering (= the hypothesis seeds) continues where it was.
        if (ps_vo_stream_pending(f.pipe) > 0) {
            lastError_ = "enqueueFrame: the frame has more keypoints than the pipeline's capacity; dequeue the pending results, the "
                         "pipeline is rebuilt then";
            return 0;
        }
        const bool hadPrev = !pipeFirst_;
        if (!buildPipeline(std::min(PS_MAX_KPTS, std::max(n + n / 4, 2 * f.pipeCap)), hadPrev ? (uint64_t)frameCounter : 0)) return -1;
        if (hadPrev) {
            const int np = (int)prevFeatures3D.size();
            int rc = ps_vo_stream_push_async(f.pipe, prevDescriptors.data, np > 0 ? (size_t)prevDescriptors.step : (size_t)PS_DESC_BYTES,
                                             reinterpret_cast<const float *>(prevFeatures3D.data()), np);
            if (rc != PS_OK) {
                lastError_ = std::string("ps_vo_stream_push_async (previous frame into the rebuilt pipeline): ") + ps_last_error(f.ctx);
                return -1;
            }
        }
    }
    int rc = ps_vo_stream_push_async(f.pipe, descriptors.data, n > 0 ? (size_t)descriptors.step : (size_t)PS_DESC_BYTES,
                                     reinterpret_cast<const float *>(features3D.data()), n);
    if (rc == PS_ERR_BUSY) {
        lastError_ = "enqueueFrame: the pipeline is full; dequeue results first";
        return 0;
    }
    if (rc != PS_OK) {
        // (the pipelined stream has dropped the chunk this frame belonged to and started a new epoch: the frames enqueued since
        // the last submitted chunk have no results; include/putslam_hip.h)
        lastError_ = std::string("ps_vo_stream_push_async: ") + ps_last_error(f.ctx);
        return -1;
    }
    if (pipeFirst_) {
        frameCounter = 0; // detectInitFeatures, matcher.cpp:17-64
        pipeFirst_ = false;
    } else {
        ++frameCounter;
    }
    features3D.swap(prevFeatures3D); // matcher.cpp:506-513: the enqueued frame is the previous one for whatever comes next
    prevDescriptors = descriptors;
    fusedSynced_ = false;
    return 1;
}

bool FrameMatcher::flushFrames()
{
    if (!fused_ || !fused_->pipe) return true;
    return ps_vo_stream_flush(fused_->pipe) == PS_OK;
}

int FrameMatcher::dequeueResult(Eigen::Matrix4f &estimatedTransformation, std::vector<cv::DMatch> &inlierMatches,
                                double &pointInlierRatio, bool wait)
{
    if (!fused_ || !fused_->pipe) return 0;
    Fused &f = *fused_;
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    PsRansacStats st;
    int nm = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        int rc = ps_vo_stream_pop(f.pipe, wait ? 1 : 0, reinterpret_cast<PsDMatch *>(f.pm.data()), &nm, f.pmask.data(), pose.data(), &st);
        if (rc != PS_OK) {
            reportError(f.ctx);
            return -1;
        }
        if (nm >= 0 || !wait) break;
        // nothing in flight: frames may still wait in a partly filled chunk
        if (ps_vo_stream_pending(f.pipe) <= 0 || ps_vo_stream_flush(f.pipe) != PS_OK) break;
    }
    if (nm < 0) return 0;
    inlierMatches.assign(f.pm.begin(), f.pm.begin() + nm); // (PS_RESULTS_INLIERS: the popped matches ARE the inliers)
    estimatedTransformation = pose;
    pointInlierRatio = st.pointInlierRatio;
    return 1;
}

double FrameMatcher::match(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D, Eigen::Matrix4f &estimatedTransformation,
                      std::vector<cv::DMatch> &inlierMatches)
{
    matcherParameters.RANSACParams.errorVersion = matcherParameters.RANSACParams.errorVersionVO; // matcher.cpp:491-492
    double ratio = 0.0;
    if (!(fusedMatch_ && fusedMatchCall(descriptors, features3D, estimatedTransformation, inlierMatches, ratio))) {
        std::vector<cv::DMatch> matches = performMatching(prevDescriptors, descriptors); // matcher.cpp:470
        RANSAC ransac(matcherParameters.RANSACParams, matcherParameters.cameraMatrixMat);
        if (seeded_) ransac.setSampleSeed(seed_ + (uint64_t)frameCounter);
        estimatedTransformation = ransac.estimateTransformation(prevFeatures3D, features3D, matches, inlierMatches);
        fusedSynced_ = false;
        ratio = RANSAC::pointInlierRatio(inlierMatches, matches); // :515
    }
    features3D.swap(prevFeatures3D); // :506-513 save computed values for the next iteration
    prevDescriptors = descriptors;
    ++frameCounter;
    return ratio;
}

double FrameMatcher::matchFeatureLoopClosure(cv::Mat desc0, std::vector<Eigen::Vector3f> pts0, cv::Mat desc1,
                                        std::vector<Eigen::Vector3f> pts1, Eigen::Matrix4f &estimatedTransformation,
                                        std::vector<cv::DMatch> &inlierMatches)
{
    if (pts0.size() < 10 || pts1.size() < 10) return 0; // matcher.cpp:830-834
    std::vector<cv::DMatch> matches = performMatching(desc0, desc1); // :835
    if (matches.size() <= 0) return -1.0;                            // :838-839
    matcherParameters.RANSACParams.errorVersion = matcherParameters.RANSACParams.errorVersionMap; // :843-844
    RANSAC ransac(matcherParameters.RANSACParams, matcherParameters.cameraMatrixMat);
    if (seeded_) ransac.setSampleSeed(seed_ + 0x9E3779B97F4A7C15ull + (uint64_t)frameCounter);
    estimatedTransformation = ransac.estimateTransformation(pts0, pts1, matches, inlierMatches);
    return RANSAC::pointInlierRatio(inlierMatches, matches);
}

namespace {
// What matchXYZ / matchXYZLadder are given: CV_32F frame descriptors take the float calls (matcher.cpp:625-628 picks NORM_L2 for
// SURF / SIFT) with rows of `dim` floats, anything else today's 32-byte path.  False -- after one line on std::cerr -- for mixed
// types or a float map row whose width differs from the frame's (a feature without a descriptor keeps its zero row).
bool mapDescriptorKind(const std::vector<FrameMatcher::MapFeatureXYZ> &mapFeatures, const cv::Mat &cur, bool &isFloat, int &dim, const char *who)
{
    isFloat = cur.type() == CV_32F;
    dim = isFloat ? cur.cols : 32;
    for (const FrameMatcher::MapFeatureXYZ &f : mapFeatures) {
        if (f.descriptor.empty()) continue;
        if ((f.descriptor.type() == CV_32F) != isFloat || (isFloat && f.descriptor.cols != dim)) {
            std::cerr << "putslam_hip: " << who << ": map and frame descriptors differ in type or width" << std::endl;
            return false;
        }
    }
    return true;
}
} // namespace

double FrameMatcher::matchXYZ(const std::vector<MapFeatureXYZ> &mapFeatures, cv::Mat currentPoseDescriptors,
                         std::vector<Eigen::Vector3f> &currentPoseFeatures3D, const std::vector<int> &currentPoseOctaves,
                         const std::vector<double> &currentPoseDetDists, Eigen::Matrix4f &estimatedTransformation,
                         std::vector<cv::DMatch> &inlierMatches, int computationNumber)
{
    bool isFloat;
    int dim;
    if (!mapDescriptorKind(mapFeatures, currentPoseDescriptors, isFloat, dim, "matchXYZ")) return -1.0;
    const size_t rowBytes = isFloat ? (size_t)dim * 4 : 32; // 1 x 32 CV_8U, or 1 x D CV_32F
    const MapTry t = mapTry(matcherParameters, computationNumber);
    const size_t nmap = mapFeatures.size(), ncur = currentPoseFeatures3D.size();
    std::vector<int32_t> curLevels(ncur), mapLevels(nmap);
    for (size_t i = 0; i < ncur; ++i) curLevels[i] = frameFeatureLevel(currentPoseFeatures3D[i], currentPoseOctaves[i], currentPoseDetDists[i]);
    std::vector<Eigen::Vector3f> mapFeaturePositions3D(nmap);
    std::vector<unsigned char> mapDesc(nmap * rowBytes);
    for (size_t j = 0; j < nmap; ++j) { // :681-692,701-702
        const MapFeatureXYZ &f = mapFeatures[j];
        mapLevels[j] = mapFeatureLevel(f);
        mapFeaturePositions3D[j] = mapFeaturePosition(f);
        if (!f.descriptor.empty()) std::memcpy(&mapDesc[j * rowBytes], f.descriptor.data, rowBytes);
    }
    std::vector<cv::DMatch> matches;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx || nmap == 0 || ncur == 0) return -1.0;
    int cap = (int)(4 * nmap + 16), n = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        matches.resize((size_t)cap);
        if (isFloat) // norm(mapDescriptor - curDescriptor, NORM_L2) on CV_32F rows (:625-628, :719-721)
            status = ps_match_xyz_l2_f32(ctx, reinterpret_cast<const float *>(mapFeaturePositions3D.data()),
                                         reinterpret_cast<const float *>(mapDesc.data()), rowBytes, mapLevels.data(), (int)nmap,
                                         reinterpret_cast<const float *>(currentPoseFeatures3D.data()),
                                         reinterpret_cast<const float *>(currentPoseDescriptors.data), (size_t)currentPoseDescriptors.step,
                                         curLevels.data(), (int)ncur, dim, t.sphereRadius, t.acceptRatio,
                                         reinterpret_cast<PsDMatch *>(matches.data()), cap, &n);
        else
            status = ps_match_xyz(ctx, reinterpret_cast<const float *>(mapFeaturePositions3D.data()), mapDesc.data(), 32,
                                  mapLevels.data(), (int)nmap, reinterpret_cast<const float *>(currentPoseFeatures3D.data()),
                                  currentPoseDescriptors.data, (size_t)currentPoseDescriptors.step, curLevels.data(), (int)ncur,
                                  t.sphereRadius, t.acceptRatio, reinterpret_cast<PsDMatch *>(matches.data()), cap, &n);
        if (status == PS_OK || n <= cap) break;
        cap = n;
    }
    if (status != PS_OK) {
        reportError(ctx);
        return -1.0;
    }
    matches.resize((size_t)n);
    if (matcherParameters.verbose > 0) std::cout << "MatchesXYZ - we found : " << matches.size() << std::endl;
    if (matches.size() <= 0) return -1.0; // :755-756
    matcherParameters.RANSACParams.errorVersion = matcherParameters.RANSACParams.errorVersionMap; // :760-761
    RANSAC ransac(matcherParameters.RANSACParams, matcherParameters.cameraMatrixMat);
    if (seeded_) ransac.setSampleSeed(seed_ + 0x51ED270B0B5ull + (uint64_t)frameCounter);
    estimatedTransformation = ransac.estimateTransformation(mapFeaturePositions3D, currentPoseFeatures3D, matches, inlierMatches);
    return RANSAC::pointInlierRatio(inlierMatches, matches);
}

namespace {
// device block of matchXYZLadder, kept per thread like the context it is used with
struct LadderBlock {
    void *p = nullptr;
    size_t cap = 0;
    ~LadderBlock()
    {
        if (p) (void)hipFree(p);
    }
    int device = -1;
    bool room(size_t bytes) // (the calling thread's current device is the context's)
    {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        if (dev != device && p) { // (the thread's context is on another device than the block)
            (void)hipFree(p);
            p = nullptr;
            cap = 0;
        }
        device = dev;
        if (bytes <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, bytes + bytes / 4) != hipSuccess) return false;
        cap = bytes + bytes / 4;
        return true;
    }
};
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
} // namespace

double FrameMatcher::matchXYZLadder(const std::vector<MapFeatureXYZ> &mapFeatures, cv::Mat currentPoseDescriptors,
                                    std::vector<Eigen::Vector3f> &currentPoseFeatures3D, const std::vector<int> &currentPoseOctaves,
                                    const std::vector<double> &currentPoseDetDists, Eigen::Matrix4f &estimatedTransformation,
                                    std::vector<cv::DMatch> &inlierMatches, int maxTries, double minRatio, int *tryUsed)
{
    if (maxTries < 1) maxTries = 1;
    if (tryUsed) *tryUsed = maxTries; // (no try reaches minRatio: the last one is returned)
    bool isFloat;
    int dim;
    if (!mapDescriptorKind(mapFeatures, currentPoseDescriptors, isFloat, dim, "matchXYZLadder")) return -1.0;
    const size_t rowBytes = isFloat ? (size_t)dim * 4 : 32; // 1 x 32 CV_8U, or 1 x D CV_32F
    const size_t nmap = mapFeatures.size(), ncur = currentPoseFeatures3D.size();
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx || nmap == 0 || ncur == 0) return -1.0; // every try of matchXYZ returns -1.0
    const int T = maxTries;
    int cap = (int)(4 * nmap + 16);
    // inputs, in one host block that mirrors the device block: descriptors | points | levels | counts | pairs | bounds | ratios
    const size_t oMapDesc = 0, oCurDesc = oMapDesc + nmap * rowBytes, oMapPts = oCurDesc + ncur * rowBytes, oCurPts = up16(oMapPts + nmap * 12),
                 oMapLvl = up16(oCurPts + ncur * 12), oCurLvl = up16(oMapLvl + nmap * 4), oCounts = up16(oCurLvl + ncur * 4),
                 oPairs = oCounts + 16, oBound = up16(oPairs + (size_t)T * 8), oRatio = up16(oBound + (size_t)T * 4),
                 inBytes = up16(oRatio + (size_t)T * 8);
    std::vector<unsigned char> in(inBytes, 0);
    for (size_t j = 0; j < nmap; ++j) { // matcher.cpp:681-692,701-702
        const MapFeatureXYZ &f = mapFeatures[j];
        const int32_t lvl = mapFeatureLevel(f);
        const Eigen::Vector3f pos = mapFeaturePosition(f);
        std::memcpy(&in[oMapLvl + j * 4], &lvl, 4);
        std::memcpy(&in[oMapPts + j * 12], &pos, 12);
        if (!f.descriptor.empty()) std::memcpy(&in[oMapDesc + j * rowBytes], f.descriptor.data, rowBytes);
    }
    for (size_t i = 0; i < ncur; ++i) {
        const int32_t lvl = frameFeatureLevel(currentPoseFeatures3D[i], currentPoseOctaves[i], currentPoseDetDists[i]);
        std::memcpy(&in[oCurLvl + i * 4], &lvl, 4);
        std::memcpy(&in[oCurDesc + i * rowBytes], currentPoseDescriptors.data + i * (size_t)currentPoseDescriptors.step, rowBytes);
    }
    std::memcpy(&in[oCurPts], currentPoseFeatures3D.data(), ncur * 12);
    const int32_t counts[2] = {(int32_t)nmap, (int32_t)ncur};
    std::memcpy(&in[oCounts], counts, 8);
    for (int k = 1; k <= T; ++k) { // the pairs all name view 0, frame 0
        const MapTry t = mapTry(matcherParameters, k);
        const float bound = ps_map_sphere_bound(t.sphereRadius);
        std::memcpy(&in[oBound + (size_t)(k - 1) * 4], &bound, 4);
        std::memcpy(&in[oRatio + (size_t)(k - 1) * 8], &t.acceptRatio, 8);
    }
    matcherParameters.RANSACParams.errorVersion = matcherParameters.RANSACParams.errorVersionMap; // :760-761
    const VoRansac vo = voRansac(matcherParameters.RANSACParams, // (the seed is try 1's; try k: + (k - 1))
                                 sampleSeed(seeded_, seed_, 0x51ED270B0B5ull + (uint64_t)frameCounter));
    float K[9];
    bool haveK;
    cameraToK(matcherParameters.cameraMatrixMat, K, haveK);

    static thread_local LadderBlock block;
    std::vector<unsigned char> out;
    size_t oMatches = 0, oNum = 0, oMask = 0, oPose = 0, oStats = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        oMatches = 0;
        oNum = oMatches + (size_t)T * cap * sizeof(PsDMatch);
        oMask = up16(oNum + (size_t)T * 4);
        oPose = up16(oMask + (size_t)T * cap);
        oStats = oPose + (size_t)T * 64;
        const size_t outBytes = up16(oStats + (size_t)T * sizeof(PsRansacStats));
        // the block lives on the context's device, and the upload is queued on the context's stream, in front of the launches
        // that read it (`in` outlives the synchronisation below)
        hipStream_t stream = static_cast<hipStream_t>(ps_context_stream(ctx));
        if (hipSetDevice(ps_context_device(ctx)) != hipSuccess || !block.room(inBytes + outBytes) ||
            hipMemcpyAsync(block.p, in.data(), inBytes, hipMemcpyHostToDevice, stream) != hipSuccess) {
            std::cerr << "putslam_hip: matchXYZLadder: no device memory" << std::endl;
            return -1.0;
        }
        unsigned char *d = static_cast<unsigned char *>(block.p), *o = d + inBytes;
        const auto fill = [&](auto &mb) { // what PsMapBatch and PsMapBatchF32 share
            std::memset(&mb, 0, sizeof mb);
            mb.maps.pts = reinterpret_cast<const float *>(d + oMapPts);
            mb.maps.nkpts = reinterpret_cast<const int32_t *>(d + oCounts);
            mb.maps.numFrames = 1;
            mb.maps.maxKpts = (int32_t)nmap;
            mb.mapLevel = reinterpret_cast<const int32_t *>(d + oMapLvl);
            mb.frames.pts = reinterpret_cast<const float *>(d + oCurPts);
            mb.frames.nkpts = reinterpret_cast<const int32_t *>(d + oCounts) + 1;
            mb.frames.numFrames = 1;
            mb.frames.maxKpts = (int32_t)ncur;
            mb.curLevel = reinterpret_cast<const int32_t *>(d + oCurLvl);
            mb.pairs = reinterpret_cast<const int32_t *>(d + oPairs);
            mb.P = T;
            mb.maxMatches = cap;
            mb.radiusBoundPerPair = reinterpret_cast<const float *>(d + oBound);
            mb.acceptRatioPerPair = reinterpret_cast<const double *>(d + oRatio);
        };
        PsPairResults res;
        res.matches = reinterpret_cast<PsDMatch *>(o + oMatches);
        res.numMatches = reinterpret_cast<int32_t *>(o + oNum);
        res.inlierMask = o + oMask;
        res.pose = reinterpret_cast<float *>(o + oPose);
        res.stats = reinterpret_cast<PsRansacStats *>(o + oStats);
        if (isFloat) {
            PsMapBatchF32 mb;
            fill(mb);
            mb.maps.desc = reinterpret_cast<const float *>(d + oMapDesc);
            mb.frames.desc = reinterpret_cast<const float *>(d + oCurDesc);
            mb.maps.dim = mb.frames.dim = dim;
            status = ps_map_pairs_l2_device(ctx, &vo.prm, &vo.cfg, haveK ? K : nullptr, &mb, &res);
        } else {
            PsMapBatch mb;
            fill(mb);
            mb.maps.desc = d + oMapDesc;
            mb.frames.desc = d + oCurDesc;
            status = ps_map_pairs_device(ctx, &vo.prm, &vo.cfg, haveK ? K : nullptr, &mb, &res);
        }
        out.resize(outBytes);
        const bool copied = status == PS_OK && hipMemcpyAsync(out.data(), o, outBytes, hipMemcpyDeviceToHost, stream) == hipSuccess;
        const int sync = ps_context_synchronize(ctx); // (also after a failed call: the upload may still be reading `in`)
        if (status == PS_OK) status = sync;
        if (status != PS_OK) {
            reportError(ctx);
            return -1.0;
        }
        if (!copied) return -1.0;
        int32_t need = 0; // a try that overflowed its rows reports -(count): once more with room for the largest
        for (int k = 0; k < T; ++k) {
            int32_t n;
            std::memcpy(&n, &out[oNum + (size_t)k * 4], 4);
            if (-n > need) need = -n;
        }
        if (need <= cap) break;
        cap = need;
    }
    // the loop of PUTSLAM.cpp:788-798: the first try whose ratio is not below minRatio, else the last
    int pick = T - 1;
    double ratioOf = -1.0;
    for (int k = 0; k < T; ++k) {
        int32_t n;
        PsRansacStats st;
        std::memcpy(&n, &out[oNum + (size_t)k * 4], 4);
        std::memcpy(&st, &out[oStats + (size_t)k * sizeof(PsRansacStats)], sizeof st);
        ratioOf = n <= 0 ? -1.0 : st.pointInlierRatio; // matcher.cpp:755-756
        if (ratioOf >= minRatio) {
            pick = k;
            break;
        }
    }
    if (tryUsed) *tryUsed = pick + 1;
    int32_t n;
    std::memcpy(&n, &out[oNum + (size_t)pick * 4], 4);
    if (matcherParameters.verbose > 0) std::cout << "MatchesXYZ - we found : " << (n > 0 ? n : 0) << std::endl;
    if (n <= 0) return -1.0;
    const PsDMatch *m = reinterpret_cast<const PsDMatch *>(&out[oMatches]) + (size_t)pick * cap;
    const unsigned char *mask = &out[oMask + (size_t)pick * cap];
    inlierMatches.clear();
    for (int i = 0; i < n; ++i)
        if (mask[i]) inlierMatches.push_back(cv::DMatch(m[i].queryIdx, m[i].trainIdx, m[i].imgIdx, m[i].distance));
    std::memcpy(estimatedTransformation.data(), &out[oPose + (size_t)pick * 64], 64);
    return ratioOf;
}

void VOTrajectory::addIncrement(Eigen::Matrix4f inc)
{
    // PUTSLAM.cpp:735-740
    double translationVO = std::sqrt(std::pow(inc(0, 3), 2) + std::pow(inc(1, 3), 2) + std::pow(inc(2, 3), 2));
    if (translationVO > 0.1) inc = Eigen::Matrix4f::Identity();
    Eigen::Matrix4f r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float p0 = VOPoseEstimate(i, 0) * inc(0, j), p1 = VOPoseEstimate(i, 1) * inc(1, j);
            float p2 = VOPoseEstimate(i, 2) * inc(2, j), p3 = VOPoseEstimate(i, 3) * inc(3, j);
            r(i, j) = (p0 + p1) + (p2 + p3);
        }
    VOPoseEstimate = r;
}

std::string VOTrajectory::freiburgLine(const Eigen::Matrix4f &T, double timestamp)
{
    // saveTrajectoryFreiburgFormat, PUTSLAM.cpp:1006-1016; Eigen::Quaternion<float>(Matrix3f)
    float m[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = T(i, j);
    float q[4]; // x y z w
    float t = (m[0][0] + m[1][1]) + m[2][2];
    if (t > 0.0f) {
        t = std::sqrt(t + 1.0f);
        q[3] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0f);
        q[i] = 0.5f * t;
        t = 0.5f / t;
        q[3] = (m[k][j] - m[j][k]) * t;
        q[j] = (m[j][i] + m[i][j]) * t;
        q[k] = (m[k][i] + m[i][k]) * t;
    }
    std::ostringstream ossTimestamp;
    ossTimestamp << std::setfill('0') << std::setprecision(17) << timestamp;
    std::ostringstream o;
    o << ossTimestamp.str() << " " << T(0, 3) << " " << T(1, 3) << " " << T(2, 3) << " " << q[0] << " " << q[1] << " " << q[2]
      << " " << q[3];
    return o.str();
}

// "A single instance of OpenCV matcher", matcherOpenCV.cpp:20 -- the same ownership rule for the hot-path matcher
FrameMatcherHIP::Ptr matcherClass, loopClosingMatcherClass;

FrameMatcher *createFrameMatcher(void)
{
    matcherClass.reset(new FrameMatcherHIP());
    return matcherClass.get();
}
FrameMatcher *createFrameMatcher(const std::string _parametersFile, const std::string _grabberParametersFile)
{
    matcherClass.reset(new FrameMatcherHIP(_parametersFile, _grabberParametersFile));
    return matcherClass.get();
}
FrameMatcher *createLoopClosingFrameMatcher(const std::string _parametersFile, const std::string _grabberParametersFile)
{
    loopClosingMatcherClass.reset(new FrameMatcherHIP(_parametersFile, _grabberParametersFile));
    return loopClosingMatcherClass.get();
}

// ---------------------------------------------------------------------------------------------
FrameMatcherHIP::FrameMatcherHIP(void) : FrameMatcher("OpenCV Matcher") { fusedMatch_ = true; }
// XML parsing (tinyXML, matcher.h:188-357) is outside the path: parameters are plain members to set.
FrameMatcherHIP::FrameMatcherHIP(const std::string, const std::string) : FrameMatcher("OpenCVMatcher") { fusedMatch_ = true; }
FrameMatcherHIP::~FrameMatcherHIP(void) {}
const std::string &FrameMatcherHIP::getName() const { return name; }

// matcherOpenCV.cpp:97-105 builds BFMatcher(NORM_L2, true) for the float descriptors (SURF / SIFT) and the Hamming matcher for the
// binary ones; :198-206 is the same call on either.  Here the Mats' type decides.
std::vector<cv::DMatch> FrameMatcherHIP::performMatching(cv::Mat prevDescriptors, cv::Mat descriptors)
{
    if (prevDescriptors.type() == CV_32F && descriptors.type() == CV_32F) return l2CrossCheckMatch(prevDescriptors, descriptors);
    return hammingCrossCheckMatch(prevDescriptors, descriptors);
}

std::vector<cv::DMatch> FrameMatcherHIP::performTracking(cv::Mat prevImg, cv::Mat img, std::vector<cv::Point2f> &prevFeatures,
                                                         std::vector<cv::Point2f> &features, std::vector<cv::KeyPoint> &prevKeyPoints,
                                                         std::vector<cv::KeyPoint> &keyPoints, std::vector<double> &prevDetDists,
                                                         std::vector<double> &detDists)
{
    return trackFeaturesLK(matcherParameters, prevImg, img, prevFeatures, features, prevKeyPoints, keyPoints, prevDetDists, detDists);
}

// MatcherOpenCV::performTracking, matcherOpenCV.cpp:209-300
std::vector<cv::DMatch> trackFeaturesLK(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat prevImg, cv::Mat img,
                                        std::vector<cv::Point2f> &prevFeatures, std::vector<cv::Point2f> &features,
                                        std::vector<cv::KeyPoint> &prevKeyPoints, std::vector<cv::KeyPoint> &keyPoints,
                                        std::vector<double> &prevDetDists, std::vector<double> &detDists)
{
    std::vector<cv::DMatch> matches;
    const auto &cvp = matcherParameters.OpenCVParams;
    const size_t n = prevFeatures.size();
    const bool initialFlow = cvp.useInitialFlow > 0 && features.size() == n; // (calcOpticalFlowPyrLK asserts the sizes agree)
    std::vector<cv::Point2f> tracked = initialFlow ? features : std::vector<cv::Point2f>(n);
    features.clear();
    keyPoints.clear();
    detDists.clear();
    if (!imagePair8u(prevImg, img) || prevKeyPoints.size() != n || prevDetDists.size() != n || (cvp.useInitialFlow > 0 && !initialFlow)) {
        std::cerr << "putslam_hip: performTracking takes two CV_8UC1 / CV_8UC3 images of one size and step, and one key point and "
                     "detection distance per previous feature" << std::endl;
        return matches;
    }
    if (n == 0) return matches;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return matches;
    const PsKltParams prm = kltParams(matcherParameters);
    matches.resize(n);
    std::vector<cv::Point2f> keptPts(n);
    std::vector<int32_t> keptIdx(n);
    int k = 0;
    status = ps_perform_tracking(ctx, prevImg.data, img.data, prevImg.rows, prevImg.cols, prevImg.channels(), prevImg.step,
                                 reinterpret_cast<const float *>(prevFeatures.data()), reinterpret_cast<float *>(tracked.data()), (int)n,
                                 &prm, cvp.trackingErrorThreshold, cvp.minimalReprojDistanceNewTrackingFeatures, nullptr, nullptr,
                                 reinterpret_cast<PsDMatch *>(matches.data()), &k, reinterpret_cast<float *>(keptPts.data()), keptIdx.data());
    if (status != PS_OK) {
        reportError(ctx);
        matches.clear();
        return matches;
    }
    matches.resize((size_t)k);
    // :240-245 then :267-290: the survivors keep the previous frame's key point (its pt moved) and detection distance
    features.assign(keptPts.begin(), keptPts.begin() + k);
    keyPoints.reserve((size_t)k);
    detDists.reserve((size_t)k);
    for (int j = 0; j < k; ++j) carryKeyPoint(prevKeyPoints, prevDetDists, keptIdx[(size_t)j], keptPts[(size_t)j], keyPoints, detDists);
    if (matcherParameters.verbose > 0)
        std::cout << "MatcherOpenCV::performTracking -- features tracked " << matches.size() << " ("
                  << (float)matches.size() * 100.0 / (float)prevFeatures.size() << "%)" << std::endl;
    return matches;
}

// the detector of matcherOpenCV.cpp:64-67 by its name: "ORB" (the shipped one) and "FAST" run on the device, anything else is refused
std::vector<cv::KeyPoint> FrameMatcherHIP::detectFeatures(cv::Mat rgbImage)
{
    const std::string &detector = matcherParameters.OpenCVParams.detector;
    if (detector == "ORB") return detectFeaturesORB(matcherParameters, rgbImage);
    if (detector == "FAST") return detectFeaturesFAST(matcherParameters, rgbImage);
    std::cerr << "putslam_hip: detectFeatures runs detector \"ORB\" and detector \"FAST\" only (asked for \"" << detector
              << "\"): no key points; SURF / SIFT detection stays with OpenCV on the host" << std::endl;
    return std::vector<cv::KeyPoint>();
}

// MatcherOpenCV::detectFeatures, matcherOpenCV.cpp:118-180, for the detector of :66-67, cv::ORB::create()
std::vector<cv::KeyPoint> detectFeaturesORB(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat rgbImage)
{
    std::vector<cv::KeyPoint> keypoints;
    const auto &cvp = matcherParameters.OpenCVParams;
    if (!image8u(rgbImage)) {
        std::cerr << "putslam_hip: detectFeatures takes a CV_8UC1 or CV_8UC3 image" << std::endl;
        return keypoints;
    }
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return keypoints;
    const PsOrbDetectParams prm = orbDetectParams(matcherParameters);
    const int cap = cvp.maximalTrackedFeatures > 0 ? cvp.maximalTrackedFeatures : 0;
    std::vector<cv::Point2f> xy((size_t)cap);
    std::vector<float> response((size_t)cap), angle((size_t)cap);
    std::vector<int32_t> octave((size_t)cap);
    int n = 0;
    status = ps_detect_features_orb(ctx, rgbImage.data, rgbImage.rows, rgbImage.cols, rgbImage.channels(), (size_t)rgbImage.step, &prm,
                                    reinterpret_cast<float *>(xy.data()), response.data(), angle.data(), octave.data(), cap, &n);
    if (status != PS_OK) {
        reportError(ctx);
        return keypoints;
    }
    keypoints.resize((size_t)n);
    for (int j = 0; j < n; ++j) keypoints[(size_t)j] = orbKeyPoint(xy[(size_t)j], angle[(size_t)j], response[(size_t)j], octave[(size_t)j]);
    if (matcherParameters.verbose > 1) std::cout << "MatcherOpenCV: After joining we have " << keypoints.size() << " keypoints" << std::endl;
    return keypoints;
}

// MatcherOpenCV::detectFeatures, matcherOpenCV.cpp:118-180, for the detector of :64-65
std::vector<cv::KeyPoint> detectFeaturesFAST(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat rgbImage)
{
    std::vector<cv::KeyPoint> keypoints;
    const auto &cvp = matcherParameters.OpenCVParams;
    if (cvp.detector != "FAST") {
        std::cerr << "putslam_hip: detectFeaturesFAST runs detector \"FAST\" only (asked for \"" << cvp.detector << "\"): no key points"
                  << std::endl;
        return keypoints;
    }
    if (!image8u(rgbImage)) {
        std::cerr << "putslam_hip: detectFeatures takes a CV_8UC1 or CV_8UC3 image" << std::endl;
        return keypoints;
    }
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return keypoints;
    PsDetectParams prm;
    prm.threshold = 10;          // cv::FastFeatureDetector::create()'s defaults (:65)
    prm.nonmaxSuppression = 1;
    prm.gridRows = cvp.gridRows;
    prm.gridCols = cvp.gridCols;
    prm.maximalTrackedFeatures = cvp.maximalTrackedFeatures;
    prm.reserved = 0;
    const int cap = cvp.maximalTrackedFeatures > 0 ? cvp.maximalTrackedFeatures : 0;
    std::vector<cv::Point2f> xy((size_t)cap);
    std::vector<float> response((size_t)cap);
    int n = 0;
    status = ps_detect_features(ctx, rgbImage.data, rgbImage.rows, rgbImage.cols, rgbImage.channels(), (size_t)rgbImage.step, &prm,
                                reinterpret_cast<float *>(xy.data()), response.data(), cap, &n);
    if (status != PS_OK) {
        reportError(ctx);
        return keypoints;
    }
    keypoints.resize((size_t)n);
    for (int j = 0; j < n; ++j) { // cv::KeyPoint(pt, 7.f, -1, score): octave 0, class_id -1
        cv::KeyPoint &kp = keypoints[(size_t)j];
        kp.pt = xy[(size_t)j];
        kp.size = 7.f;
        kp.angle = -1.f;
        kp.response = response[(size_t)j];
        kp.octave = 0;
        kp.class_id = -1;
    }
    if (matcherParameters.verbose > 1) std::cout << "MatcherOpenCV: After joining we have " << keypoints.size() << " keypoints" << std::endl;
    return keypoints;
}

cv::Mat FrameMatcherHIP::describeFeatures(cv::Mat rgbImage, std::vector<cv::KeyPoint> &features)
{
    return describeFeaturesORB(matcherParameters, rgbImage, features);
}

// MatcherOpenCV::describeFeatures, matcherOpenCV.cpp:183-195, for the extractor cv::ORB::create()
cv::Mat describeFeaturesORB(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat rgbImage, std::vector<cv::KeyPoint> &features)
{
    const std::vector<cv::KeyPoint> in = features;
    features.clear();
    const auto &cvp = matcherParameters.OpenCVParams;
    if (cvp.descriptor != "ORB") {
        std::cerr << "putslam_hip: describeFeatures runs descriptor \"ORB\" only (asked for \"" << cvp.descriptor
                  << "\"): no descriptors; SURF / SIFT description stays with OpenCV on the host" << std::endl;
        return cv::Mat();
    }
    if (!image8u(rgbImage)) {
        std::cerr << "putslam_hip: describeFeatures takes a CV_8UC1 or CV_8UC3 image" << std::endl;
        return cv::Mat();
    }
    if (in.empty()) return cv::Mat();
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return cv::Mat();
    const PsOrbParams prm = orbDescribeParams();
    const size_t n = in.size();
    std::vector<cv::Point2f> xy(n);
    std::vector<float> angle(n);
    std::vector<int32_t> octave(n), keptIdx(n);
    for (size_t i = 0; i < n; ++i) {
        xy[i] = in[i].pt;
        angle[i] = in[i].angle;
        octave[i] = in[i].octave;
    }
    std::vector<unsigned char> rows(n * 32);
    int k = 0;
    status = ps_describe_features(ctx, rgbImage.data, rgbImage.rows, rgbImage.cols, rgbImage.channels(), (size_t)rgbImage.step, &prm, nullptr,
                                  reinterpret_cast<const float *>(xy.data()), angle.data(), octave.data(), (int)n, rows.data(), keptIdx.data(),
                                  &k);
    if (status != PS_OK) {
        reportError(ctx);
        return cv::Mat();
    }
    if (k == 0) return cv::Mat();
    cv::Mat descriptors(k, 32, CV_8U);
    std::memcpy(descriptors.data, rows.data(), (size_t)k * 32);
    features.resize((size_t)k);
    for (int j = 0; j < k; ++j) features[(size_t)j] = in[(size_t)keptIdx[(size_t)j]];
    return descriptors;
}

// Matcher::detectInitFeatures, matcher.cpp:19-49 / Matcher::match, :457-482: the frame from its images to descriptors and 3-D points
void FrameMatcherHIP::frontEnd(cv::Mat rgbImage, cv::Mat depthImage, double depthImageScale, cv::Mat &descriptors,
                               std::vector<Eigen::Vector3f> &features3D, std::vector<cv::KeyPoint> *keyPoints, std::vector<cv::Point2f> *undistorted)
{
    descriptors = cv::Mat();
    features3D.clear();
    if (keyPoints) keyPoints->clear();
    if (undistorted) undistorted->clear();
    const auto &cvp = matcherParameters.OpenCVParams;
    if (cvp.detector != "ORB" || cvp.descriptor != "ORB") {
        std::cerr << "putslam_hip: frontEnd runs detector \"ORB\" with descriptor \"ORB\" only (asked for \"" << cvp.detector << "\" and \""
                  << cvp.descriptor << "\"): nothing detected; the separate calls or OpenCV on the host serve the others" << std::endl;
        return;
    }
    if (!image8u(rgbImage) || !depth16uOf(depthImage, rgbImage)) {
        std::cerr << "putslam_hip: frontEnd takes a CV_8UC1 or CV_8UC3 image and a CV_16U depth image of the same size" << std::endl;
        return;
    }
    const int cap = cvp.maximalTrackedFeatures > 0 ? cvp.maximalTrackedFeatures : 0;
    if (cap == 0) return;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return;
    const PsFrontEndParams prm = frontEndParams(matcherParameters);
    const PsFrameGeometry geo = frameGeometry(matcherParameters, depthImageScale);
    const size_t room = (size_t)cap;
    std::vector<unsigned char> rows(room * 32);
    std::vector<cv::Point2f> xy(room), und(room);
    std::vector<float> angle(room), response(room);
    std::vector<int32_t> octave(room);
    features3D.resize(room);
    PsFrameRowsOut out;
    std::memset(&out, 0, sizeof out);
    out.pts = reinterpret_cast<float *>(features3D.data());
    out.xy = reinterpret_cast<float *>(xy.data());
    out.xyUndist = reinterpret_cast<float *>(und.data());
    out.angle = angle.data();
    out.response = response.data();
    out.octave = octave.data();
    int n = 0;
    status = ps_front_end_frame(ctx, rgbImage.data, reinterpret_cast<const uint16_t *>(depthImage.data), rgbImage.rows, rgbImage.cols,
                                rgbImage.channels(), (size_t)rgbImage.step, (size_t)depthImage.step, &prm, nullptr, &geo, rows.data(), &out, cap, &n);
    if (status != PS_OK) {
        reportError(ctx);
        features3D.clear();
        return;
    }
    features3D.resize((size_t)n);
    if (n == 0) return;
    descriptors = cv::Mat(n, 32, CV_8U);
    std::memcpy(descriptors.data, rows.data(), (size_t)n * 32);
    if (undistorted) undistorted->assign(und.begin(), und.begin() + n);
    if (keyPoints) {
        keyPoints->resize((size_t)n);
        for (int j = 0; j < n; ++j) (*keyPoints)[(size_t)j] = orbKeyPoint(xy[(size_t)j], angle[(size_t)j], response[(size_t)j], octave[(size_t)j]);
    }
}

// Matcher::trackKLT, matcher.cpp:147-211
bool FrameMatcherHIP::trackStep(cv::Mat prevRgbImage, cv::Mat rgbImage, cv::Mat depthImage, double depthImageScale,
                                const std::vector<cv::Point2f> &prevFeaturesDistorted, const std::vector<Eigen::Vector3f> &prevFeatures3D,
                                const std::vector<cv::KeyPoint> &prevKeyPoints, const std::vector<double> &prevDetDists,
                                std::vector<cv::Point2f> &distorted, std::vector<cv::Point2f> &undistorted,
                                std::vector<Eigen::Vector3f> &features3D, std::vector<cv::KeyPoint> &keyPoints, std::vector<double> &detDists,
                                std::vector<cv::DMatch> &matches, std::vector<cv::DMatch> &inlierMatches,
                                Eigen::Matrix4f &estimatedTransformation)
{
    const auto &cvp = matcherParameters.OpenCVParams;
    const size_t n = prevFeaturesDistorted.size();
    const bool initialFlow = cvp.useInitialFlow > 0 && distorted.size() == n; // (calcOpticalFlowPyrLK asserts the sizes agree)
    std::vector<cv::Point2f> tracked = initialFlow ? distorted : std::vector<cv::Point2f>(n ? n : 1);
    distorted.clear();
    undistorted.clear();
    features3D.clear();
    keyPoints.clear();
    detDists.clear();
    matches.clear();
    inlierMatches.clear();
    estimatedTransformation = Eigen::Matrix4f::Identity();
    if (cvp.removeTooCloseFeatures > 0) {
        std::cerr << "putslam_hip: trackStep does not run removeTooCloseFeatures (the reference leaves the matches' trainIdx un-renumbered, "
                     "matcher.cpp:960-963): set OpenCVParams.removeTooCloseFeatures to 0 and call removeTooCloseFeatures on the result" << std::endl;
        return false;
    }
    if (!imagePair8u(prevRgbImage, rgbImage) || !depth16uOf(depthImage, rgbImage) || prevFeatures3D.size() != n || prevKeyPoints.size() != n ||
        prevDetDists.size() != n || (cvp.useInitialFlow > 0 && !initialFlow)) {
        std::cerr << "putslam_hip: trackStep takes two CV_8UC1 / CV_8UC3 images of one size and step, a CV_16U depth image of that size, and "
                     "one 3-D point, key point and detection distance per previous feature" << std::endl;
        return false;
    }
    if (n == 0) return true; // matcher.cpp:147-148
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return false;
    const PsKltParams klt = kltParams(matcherParameters);
    PsTrackVoParams tp;
    tp.trackingErrorThreshold = cvp.trackingErrorThreshold;
    tp.minimalReprojDistanceNewTrackingFeatures = cvp.minimalReprojDistanceNewTrackingFeatures;
    tp.removeTooCloseFeatures = 0;
    tp.reserved = 0;
    // RANSAC ransac(matcherParameters.RANSACParams with errorVersion = errorVersionVO, cameraMatrixMat), as Matcher::match builds it
    RANSAC::parameters rp = matcherParameters.RANSACParams;
    rp.errorVersion = rp.errorVersionVO; // matcher.cpp:190-191
    const VoRansac vo = voRansac(rp, sampleSeed(seeded_, seed_, (uint64_t)frameCounter));
    const PsFrameGeometry geo = frameGeometry(matcherParameters, depthImageScale);
    std::vector<cv::Point2f> xy(n), und(n);
    std::vector<int32_t> keptIdx(n);
    std::vector<uint8_t> mask(n);
    matches.resize(n);
    features3D.resize(n);
    PsTrackVoIn in;
    std::memset(&in, 0, sizeof in);
    in.prevXY = reinterpret_cast<const float *>(prevFeaturesDistorted.data());
    in.prevPts = reinterpret_cast<const float *>(prevFeatures3D.data());
    PsTrackVoOut out;
    std::memset(&out, 0, sizeof out);
    out.nextPts = reinterpret_cast<float *>(tracked.data());
    out.matches = reinterpret_cast<PsDMatch *>(matches.data());
    out.keptIdx = keptIdx.data();
    out.rows.xy = reinterpret_cast<float *>(xy.data());
    out.rows.xyUndist = reinterpret_cast<float *>(und.data());
    out.rows.pts = reinterpret_cast<float *>(features3D.data());
    out.inlierMask = mask.data();
    out.pose = estimatedTransformation.data();
    PsRansacStats st;
    out.stats = &st;
    int k = 0;
    status = ps_track_vo_pair(ctx, prevRgbImage.data, rgbImage.data, reinterpret_cast<const uint16_t *>(depthImage.data), rgbImage.rows,
                              rgbImage.cols, rgbImage.channels(), (size_t)rgbImage.step, (size_t)depthImage.step, &klt, &tp, &vo.prm, &vo.cfg, &geo, &in,
                              (int)n, &out, &k);
    if (status != PS_OK) {
        reportError(ctx);
        matches.clear();
        features3D.clear();
        estimatedTransformation = Eigen::Matrix4f::Identity();
        return false;
    }
    matches.resize((size_t)k);
    features3D.resize((size_t)k);
    distorted.assign(xy.begin(), xy.begin() + k);
    undistorted.assign(und.begin(), und.begin() + k);
    keyPoints.reserve((size_t)k);
    detDists.reserve((size_t)k);
    for (int j = 0; j < k; ++j) {
        carryKeyPoint(prevKeyPoints, prevDetDists, keptIdx[(size_t)j], xy[(size_t)j], keyPoints, detDists);
        if (mask[(size_t)j]) inlierMatches.push_back(matches[(size_t)j]);
    }
    ++frameCounter;
    return true;
}

// Matcher::trackKLT, matcher.cpp:133-449
double FrameMatcherHIP::trackKLT(cv::Mat rgbImage, cv::Mat depthImage, double depthImageScale, Eigen::Matrix4f &estimatedTransformation,
                                 std::vector<cv::DMatch> &inlierMatches)
{
    const auto &cvp = matcherParameters.OpenCVParams;
    estimatedTransformation = Eigen::Matrix4f::Identity();
    inlierMatches.clear();
    if (cvp.detector != "ORB" || cvp.descriptor != "ORB" || cvp.removeTooCloseFeatures > 0 || cvp.maximalTrackedFeatures < 1) {
        std::cerr << "putslam_hip: trackKLT runs detector \"ORB\" with descriptor \"ORB\", removeTooCloseFeatures 0 (trackStep) and at least one "
                     "tracked feature allowed: nothing done" << std::endl;
        return 0.0;
    }
    if (!image8u(rgbImage) || !depth16uOf(depthImage, rgbImage)) {
        std::cerr << "putslam_hip: trackKLT takes a CV_8UC1 or CV_8UC3 image and a CV_16U depth image of the same size" << std::endl;
        return 0.0;
    }
    std::vector<cv::Point2f> distorted, undistorted;
    std::vector<Eigen::Vector3f> features3D;
    std::vector<cv::KeyPoint> keyPoints;
    std::vector<double> detDists;
    std::vector<cv::DMatch> matches;
    if (!prevFeaturesUndistorted.empty() && !prevFeaturesDistorted.empty() && // :147
        !trackStep(prevRgbImage, rgbImage, depthImage, depthImageScale, prevFeaturesDistorted, prevFeatures3D, prevKeyPoints, prevDetDists, distorted,
                   undistorted, features3D, keyPoints, detDists, matches, inlierMatches, estimatedTransformation))
        return 0.0;
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return 0.0;
    // :213-381
    const PsFrontEndParams prm = frontEndParams(matcherParameters);
    PsTrackCloseParams tp;
    tp.minimalReprojDistanceNewTrackingFeatures = cvp.minimalReprojDistanceNewTrackingFeatures;
    tp.minimalTrackedFeatures = cvp.minimalTrackedFeatures;
    tp.removeTooCloseFeatures = 0;
    const PsFrameGeometry geo = frameGeometry(matcherParameters, depthImageScale);
    const size_t n = distorted.size(), base = n > 0 ? n : 1, cap = base + (size_t)cvp.maximalTrackedFeatures;
    std::vector<float> angle(base), response(base), oAngle(cap), oResponse(cap);
    std::vector<int32_t> octave(base), oOctave(cap), srcIdx(cap);
    for (size_t i = 0; i < n; ++i) {
        angle[i] = keyPoints[i].angle;
        response[i] = keyPoints[i].response;
        octave[i] = keyPoints[i].octave;
    }
    std::vector<cv::Point2f> oXy(cap), oUn(cap);
    std::vector<Eigen::Vector3f> oPts(cap);
    std::vector<double> oDist(cap);
    std::vector<unsigned char> rows(cap * 32);
    PsTrackedRows in;
    std::memset(&in, 0, sizeof in);
    in.xy = reinterpret_cast<float *>(distorted.data());
    in.xyUndist = reinterpret_cast<float *>(undistorted.data());
    in.pts = reinterpret_cast<float *>(features3D.data());
    in.angle = angle.data();
    in.response = response.data();
    in.octave = octave.data();
    in.detDist = detDists.data();
    PsTrackedRows out;
    std::memset(&out, 0, sizeof out);
    out.xy = reinterpret_cast<float *>(oXy.data());
    out.xyUndist = reinterpret_cast<float *>(oUn.data());
    out.pts = reinterpret_cast<float *>(oPts.data());
    out.angle = oAngle.data();
    out.response = oResponse.data();
    out.octave = oOctave.data();
    out.detDist = oDist.data();
    int k = 0, refill = 0;
    status = ps_track_close_pair(ctx, rgbImage.data, reinterpret_cast<const uint16_t *>(depthImage.data), rgbImage.rows, rgbImage.cols,
                                 rgbImage.channels(), (size_t)rgbImage.step, (size_t)depthImage.step, &prm, nullptr, &geo, &tp, &in, (int)n, rows.data(),
                                 &out, srcIdx.data(), (int)cap, &k, &refill);
    if (status != PS_OK) {
        reportError(ctx);
        estimatedTransformation = Eigen::Matrix4f::Identity();
        inlierMatches.clear();
        return 0.0;
    }
    std::vector<cv::KeyPoint> closed((size_t)k);
    for (int j = 0; j < k; ++j) {
        cv::KeyPoint &kp = closed[(size_t)j];
        const size_t s = (size_t)srcIdx[(size_t)j];
        if (n > 0 && s < n)
            kp = keyPoints[s]; // the tracked key point (matcherOpenCV.cpp:240-245)
        else               // a merged one
            kp = orbKeyPoint(oXy[(size_t)j], oAngle[(size_t)j], oResponse[(size_t)j], oOctave[(size_t)j]);
        kp.pt = oXy[(size_t)j];
    }
    double inlierRatio = 0.0; // :404-406
    if (matches.size() > 0) inlierRatio = RANSAC::pointInlierRatio(inlierMatches, matches);
    // :436-445
    prevFeaturesUndistorted.assign(oUn.begin(), oUn.begin() + k);
    prevFeaturesDistorted.assign(oXy.begin(), oXy.begin() + k);
    prevFeatures3D.assign(oPts.begin(), oPts.begin() + k);
    prevDescriptors = k > 0 ? cv::Mat(k, 32, CV_8U) : cv::Mat();
    if (k > 0) std::memcpy(prevDescriptors.data, rows.data(), (size_t)k * 32);
    prevKeyPoints.swap(closed);
    prevDetDists.assign(oDist.begin(), oDist.begin() + k);
    prevRgbImage = rgbImage;
    prevDepthImage = depthImage;
    fusedSynced_ = false; // (the resident frame of match() is no longer prevDescriptors / prevFeatures3D)
    return inlierRatio;
}

// MatcherOpenCV::performMatching (matcherOpenCV.cpp:198-206) with the matcher of matcherOpenCV.cpp:100-102, cv::BFMatcher(cv::NORM_L2,
// true), on CV_32F descriptor Mats of 1 .. PS_MAX_L2_DIM columns (ps_match_l2_f32).
std::vector<cv::DMatch> l2CrossCheckMatch(cv::Mat prevDescriptors, cv::Mat descriptors)
{
    std::vector<cv::DMatch> matches;
    if (prevDescriptors.empty() || descriptors.empty()) return matches;
    if (prevDescriptors.type() != CV_32F || descriptors.type() != CV_32F || prevDescriptors.cols != descriptors.cols) {
        std::cerr << "putslam_hip: l2CrossCheckMatch takes two CV_32F descriptor Mats of the same width" << std::endl;
        return matches;
    }
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return matches;
    matches.resize((size_t)prevDescriptors.rows);
    int n = 0;
    status = ps_match_l2_f32(ctx, reinterpret_cast<const float *>(prevDescriptors.data), prevDescriptors.rows, (size_t)prevDescriptors.step,
                             reinterpret_cast<const float *>(descriptors.data), descriptors.rows, (size_t)descriptors.step,
                             prevDescriptors.cols, reinterpret_cast<PsDMatch *>(matches.data()), &n);
    if (status != PS_OK) {
        reportError(ctx);
        n = 0;
    }
    matches.resize((size_t)n);
    return matches;
}

// MatcherOpenCV::performMatching (matcherOpenCV.cpp:198-206) as a free function: the body the reference's own class
// gets in a PUTSLAM build.
std::vector<cv::DMatch> hammingCrossCheckMatch(cv::Mat prevDescriptors, cv::Mat descriptors)
{
    std::vector<cv::DMatch> matches;
    if (prevDescriptors.empty() || descriptors.empty()) return matches;
    if (prevDescriptors.cols != PS_DESC_BYTES || descriptors.cols != PS_DESC_BYTES) {
        // float descriptors (SURF/SIFT, NORM_L2: matcherOpenCV.cpp:100-102) are outside the path
        std::cerr << "putslam_hip: performMatching supports 32-byte binary descriptors (ORB/LDB) only" << std::endl;
        return matches;
    }
    int status;
    PsContext *ctx = threadContext(&status);
    if (!ctx) return matches;
    matches.resize((size_t)prevDescriptors.rows);
    int n = 0;
    status = ps_match_hamming256(ctx, prevDescriptors.data, prevDescriptors.rows, (size_t)prevDescriptors.step, descriptors.data,
                                 descriptors.rows, (size_t)descriptors.step, reinterpret_cast<PsDMatch *>(matches.data()), &n);
    if (status != PS_OK) {
        reportError(ctx);
        n = 0;
    }
    matches.resize((size_t)n);
    return matches;
}

} // namespace putslam_hip

namespace putslam_hip {
// the calling thread's context and the error line, for the drop-in's other translation unit (putslam_dropin_uncertainty.cpp)
PsContext *dropinThreadContext(int *status) { return threadContext(status); }
void dropinReportError(const PsContext *ctx) { reportError(ctx); }
} // namespace putslam_hip
