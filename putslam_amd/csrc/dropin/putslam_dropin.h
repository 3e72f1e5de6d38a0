// putslam_dropin.h -- the reference's C++ surface for the hot path, implemented over the C ABI
// (include/putslam_hip.h).  Class names, namespaces, signatures, ownership and error behaviour follow
// the reference so that PUTSLAM's callers compile unchanged against this header:
//
//   ::RANSAC                       include/putslam/TransformEst/RANSAC.h:20-66, src/TransformEst/RANSAC.cpp
//   ::RANSAC_USAC                  include/putslam/USAC/USAC_wrapper.h:16-65, src/USAC/USAC_wrapper.cpp
//   putslam::TransformEst          include/putslam/TransformEst/transformEst.h:16-26
//   putslam::KabschEst + factory   include/putslam/TransformEst/kabschEst.h, src/TransformEst/kabschEst.cpp
//
// The Matcher plugin itself (putslam::Matcher / ::MatcherOpenCV, include/putslam/Matcher/matcher.h:24,100-151,405-422)
// keeps ITS OWN class in a PUTSLAM build: detection and description are image-domain OpenCV stages outside the
// path (performTracking has a body here: trackFeaturesLK below).  This library therefore defines no symbol of that name.  What it provides for the plugin is
//   putslam_hip::FrameMatcher / FrameMatcherHIP   the hot-path state machine behind Matcher::match / runVO /
//                                  matchXYZ / matchFeatureLoopClosure (matcher.cpp:452-516,606-861) on descriptors and
//                                  3-D points, which the reference's methods call after their detect / describe part;
//   putslam_matcher_glue.h         the same entry points with the reference's own argument types (SensorFrame-derived
//                                  descriptors, std::vector<MapFeature>, framesIds[2], pairedFeatures), as templates;
//   INTEGRATION.md section 2       the bodies a maintainer puts into matcher.cpp / matcherOpenCV.cpp.
//   RGBD helpers                   include/putslam/RGBD/RGBD.h:38-51, src/RGBD/RGBD.cpp:10-16,30-65,92-98
//   ::DBScan                       include/putslam/Matcher/dbscan.h:14-24, src/Matcher/dbscan.cpp (keypoint thinning)
//
// Everything computes on the GPU through libputslam_hip.so; there is no host fallback.
#pragma once

#include <cstdint>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "putslam_compat_types.h"

#define PUTSLAM_HIP_DESC_BYTES 32 // ORB / LDB rows (matcherOpenCV.cpp:90, ldb.cpp:61,657)

// ---------------------------------------------------------------------------------------------
class RANSAC {
  public:
    enum ERROR_VERSION { EUCLIDEAN_ERROR, REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR, MAHALANOBIS_ERROR, ADAPTIVE_ERROR };
    struct parameters {
        int verbose;
        int errorVersion, errorVersionVO, errorVersionMap;
        double inlierThresholdEuclidean, inlierThresholdReprojection, inlierThresholdMahalanobis;
        double minimalInlierRatioThreshold;
        int minimalNumberOfMatches;
        int usedPairs;
        int iterationCount;
    };

    RANSAC(RANSAC::parameters RANSACParameters, cv::Mat cameraMatrix = cv::Mat());

    // prevFeatures / features: 3-D points of the previous / current frame; matches: queryIdx into
    // prevFeatures, trainIdx into features.  Returns the pose mapping current-frame points into the
    // previous frame; identity + cleared inliers on failure (no exceptions, no error codes).
    Eigen::Matrix4f estimateTransformation(std::vector<Eigen::Vector3f> prevFeatures, std::vector<Eigen::Vector3f> features,
                                           std::vector<cv::DMatch> matches, std::vector<cv::DMatch> &inlierMatches);

    static double pointInlierRatio(std::vector<cv::DMatch> &inlierMatches, std::vector<cv::DMatch> &allMatches)
    {
        std::set<int> inlier, all;
        for (auto &m : allMatches) all.insert(m.trainIdx);
        for (auto &in : inlierMatches) inlier.insert(in.trainIdx);
        return double(inlier.size()) / double(all.size());
    }

    // --- additions with no reference counterpart (the reference seeds rand() from time(0), RANSAC.cpp:13) ---
    void setSampleSeed(uint64_t seed) { seed_ = seed; }
    uint64_t sampleSeed() const { return seed_; }
    int lastStatus() const { return lastStatus_; }   // PsStatus of the last call (0 = ok)

  private:
    cv::Mat cameraMatrix;
    parameters RANSACParams;
    uint64_t seed_;
    int lastStatus_ = 0;
};

// ---------------------------------------------------------------------------------------------
class PUTSLAMEstimator { // only the parameter block of the reference class is part of the surface
  public:
    struct parameters {
        int verbose;
        int errorVersion, errorVersionVO, errorVersionMap;
        double inlierThresholdEuclidean, inlierThresholdReprojection, inlierThresholdMahalanobis;
        double minimalInlierRatioThreshold;
        int usedPairs;
        int iterationCount;
    };
};

class RANSAC_USAC {
  public:
    RANSAC_USAC(PUTSLAMEstimator::parameters RANSACParameters, cv::Mat cameraMatrix = cv::Mat());
    ~RANSAC_USAC();
    Eigen::Matrix4f estimateTransformation(std::vector<Eigen::Vector3f> prevFeatures, std::vector<Eigen::Vector3f> features,
                                           std::vector<cv::DMatch> matches, std::vector<cv::DMatch> &bestInlierMatches);
    void setSampleSeed(uint64_t seed) { seed_ = seed; }
    // samples made available to the USAC loop; default = the reference's usac_max_hypotheses_ (USAC_wrapper.cpp:70): the loop
    // stops by its own criterion long before, and a long cap costs 10 us per call (rounds 1-3 defaulted to 4096, which cut
    // the schedule short below 10 % inliers)
    void setMaxHypotheses(int h) { maxHyp_ = h; }
    int lastStatus() const { return lastStatus_; }

  private:
    cv::Mat cameraMatrix;
    PUTSLAMEstimator::parameters params_;
    uint64_t seed_;
    int maxHyp_ = 850000;
    int lastStatus_ = 0;
};

// ---------------------------------------------------------------------------------------------
class RGBD {
  public:
    static int roundSize(double x, int size);
    static std::vector<Eigen::Vector3f> keypoints2Dto3D(std::vector<cv::Point2f> undistortedFeatures2D, cv::Mat depthImage,
                                                        cv::Mat cameraMatrix, double depthImageScale = 5000, int startingID = 0);
    static std::vector<cv::Point2f> points3Dto2D(std::vector<Eigen::Vector3f> features3D, cv::Mat cameraMatrix);
    // distCoeffs: 1x5 (or 5x1) CV_32F/CV_64F-like access through at<float>: (k1, k2, p1, p2, k3)
    static std::vector<cv::Point2f> removeImageDistortion(std::vector<cv::Point2f> &features, cv::Mat cameraMatrix,
                                                          cv::Mat distCoeffs);
    // RGBD::computeNormal / computeRGBGradient (RGBD.cpp:100-187) with the reference's signatures, and their templates
    // (RGBD.h:91-106) over anything with u, v, normal, RGBgradient: ps_compute_normals / ps_compute_rgb_gradients (DESIGN.md section
    // 8.16).  The templates make ONE device call for the whole list (normalsAt / gradientsAt: pixel (px[i].x, px[i].y), truncated);
    // the single-feature forms make one call a feature.  depthImage CV_16U, rgbImage CV_8UC3 of the same size, any steps.  On an
    // error: one line on std::cerr, NaN vectors.  Nothing runs on the CPU instead.
    static putslam_hip::Vec3 computeNormal(const cv::Mat &depthImage, int u, int v, const cv::Mat &cameraMatrix, double depthImageScale);
    static putslam_hip::Vec3 computeRGBGradient(const cv::Mat &rgbImage, const cv::Mat &depthImage, int u, int v, const cv::Mat &cameraMatrix,
                                            double depthImageScale);
    static std::vector<putslam_hip::Vec3> normalsAt(const cv::Mat &depthImage, const std::vector<cv::Point2f> &px, const cv::Mat &cameraMatrix,
                                                double depthImageScale);
    static std::vector<putslam_hip::Vec3> gradientsAt(const cv::Mat &rgbImage, const cv::Mat &depthImage, const std::vector<cv::Point2f> &px,
                                                  const cv::Mat &cameraMatrix, double depthImageScale);
    template <class T> static void computeNormals(const cv::Mat &depthImage, T &features, const cv::Mat &cameraMatrix, double depthImageScale)
    {
        std::vector<cv::Point2f> px;
        for (auto it = features.begin(); it != features.end(); it++) px.push_back(cv::Point2f((float)(int)it->u, (float)(int)it->v));
        const std::vector<putslam_hip::Vec3> n = normalsAt(depthImage, px, cameraMatrix, depthImageScale);
        size_t i = 0;
        for (auto it = features.begin(); it != features.end(); it++) it->normal = n[i++];
    }
    template <class T>
    static void computeRGBGradients(const cv::Mat &rgbImage, const cv::Mat &depthImage, T &features, const cv::Mat &cameraMatrix,
                                    double depthImageScale)
    {
        std::vector<cv::Point2f> px;
        for (auto it = features.begin(); it != features.end(); it++) px.push_back(cv::Point2f((float)(int)it->u, (float)(int)it->v));
        const std::vector<putslam_hip::Vec3> g = gradientsAt(rgbImage, depthImage, px, cameraMatrix, depthImageScale);
        size_t i = 0;
        for (auto it = features.begin(); it != features.end(); it++) it->RGBgradient = g[i++];
    }
};

// ---------------------------------------------------------------------------------------------
// DepthSensorModel (include/putslam/Grabber/depthSensorModel.h, src/Grabber/depthSensorModel.cpp:27-36,55-101): the four members
// the uncertainty models read, signature-identical (putslam_hip::Vec3 / ::Mat33 ARE putslam::Vec3 / ::Mat33 where Eigen is installed).  They return COVARIANCES, which the C ABI does not export (it returns the
// information matrices): these four run on the calling thread, on the sequential restatement csrc/ps_uncertainty_host.h -- 3 x 3
// arithmetic, no loop over features -- and informationMatrixFromImageCoordinates(u, v, z), uncertinatyFromNormal(n).inverse() and
// uncertinatyFromRGBGradient(g).inverse() are byte for byte ps_information_matrices' models 0, 1 and 2
// (tests/cpp/test_dropin_uncertainty.cpp).  A whole list goes through FrameMatcherHIP::measurementEdges instead.  Config carries
// the reference's members and defaults (depthSensorModel.h:53-58; the two scale factors, unset there, are 0); the XML constructor
// is the host's.
class DepthSensorModel {
  public:
    class Config {
      public:
        Config();
        double focalLength[2], focalAxis[2], varU, varV, distVarCoefs[4], scaleUncertaintyNormal, scaleUncertaintyGradient;
    };
    DepthSensorModel() {}
    explicit DepthSensorModel(const Config &c) : config(c) {}
    void computeCov(uint_fast16_t u, uint_fast16_t v, double depth, putslam_hip::Mat33 &cov);
    putslam_hip::Mat33 informationMatrixFromImageCoordinates(double u, double v, double z);
    putslam_hip::Mat33 uncertinatyFromNormal(const putslam_hip::Vec3 &normal);
    putslam_hip::Mat33 uncertinatyFromRGBGradient(const putslam_hip::Vec3 &grad);
    Config config;
};

// ---------------------------------------------------------------------------------------------
// Keypoint thinning between detection and description (matcher.cpp:24-26,221-223,459-461,561-563): run() is ps_dbscan_thin
// on the calling thread's context and keeps every field of the surviving keypoints, in their input order.  The data members
// keep the layout of the reference class, so a translation unit compiled against the reference's dbscan.h (matcher.cpp)
// constructs and destroys this one correctly; the three containers stay empty.  The class sits behind the reference header's
// own include guard: a translation unit that includes both (matcher.cpp: Matcher/dbscan.h, and this header through the glue)
// sees ONE definition, whichever comes first -- the two are token-for-token the same interface and layout.
#ifndef _DBSCAN
#define _DBSCAN
class DBScan {
  public:
    DBScan(double eps = 10, int minPts = 2, int featuresFromCluster = 1);
    void run(std::vector<cv::KeyPoint> &clusteringSet);

  private:
    double eps;
    int minPts;
    int featuresFromCluster;
    std::vector<std::vector<float>> dist;
    std::vector<bool> visited;
    std::vector<int> cluster;
};
#endif

// ---------------------------------------------------------------------------------------------
// MatchingOnPatches (include/putslam/Matcher/MatchingOnPatches.h, src/Matcher/MatchingOnPatches.cpp:14-246): the sub-pixel alignment
// of a feature's patch, with the reference's constructors, parameter block, three calls and getters, signature-identical, over
// ps_compute_patch / ps_compute_patch_gradient / ps_optimize_location on the calling thread's context (one
// device call each, uploads included), and the batch form optimizeLocations over ps_optimize_locations: one call for a whole list.
// Images CV_8UC1 or CV_8UC3 (grey by CV_RGB2GRAY, as assertGrayscale does), any step.  `verbose` and `warping` are carried and read
// nowhere; the narration to std::cout is not reproduced.  Where the reference reads outside its images this class does not:
// computePatch returns an EMPTY vector and computeGradient a NaN InvHessian with empty gradients for a position whose taps leave the
// image, so the following optimizeLocation returns false with the position untouched; a new position that passes the reference's
// gate with taps outside stops with status 6.  optimizeLocation's bool is status == PS_PATCH_CONVERGED; lastStatus() /
// lastIterations() give the calling thread's last optimizeLocation in full (static: the object keeps the reference's layout, behind
// the reference header's own include guard, as DBScan does).  On an error: one line on std::cerr, false / empty / NaN.  Nothing runs
// on the CPU instead.
#ifndef _PATCHES
#define _PATCHES
class MatchingOnPatches {
  public:
    struct parameters {
        int verbose;
        bool warping;
        int patchSize, halfPatchSize;
        int maxIter;
        double minSqrtIncrement;
    };
    // (size, step limit, stopping threshold, verbosity; the half size follows from the size, whatever a caller's block says)
    MatchingOnPatches(int size, int stepLimit = 20, double threshold = 0.04, int verbosity = 0);
    MatchingOnPatches(parameters block);
    std::vector<double> computePatch(cv::Mat img, double x, double y);
    void computeGradient(cv::Mat img, double x, double y, Eigen::Matrix3f &InvHessian, std::vector<float> &gradientX,
                         std::vector<float> &gradientY);
    bool optimizeLocation(cv::Mat oldImg, std::vector<double> oldPatch, cv::Mat newImg, double &newX, double &newY,
                          std::vector<float> gradientX, std::vector<float> gradientY, Eigen::Matrix3f &InvHessian);
    int getPatchSize() { return params.patchSize; }
    int getHalfPatchSize() { return params.halfPatchSize; }
    // The three calls fused for a list (no reference counterpart): oldXY / newXY hold x0, y0, x1, y1, ...; newXY is read as the
    // starting guesses and written as the reference leaves each position.  Returns the PS_PATCH_* status of every point (empty on
    // an error); iterations, where given, receives the steps applied.
    std::vector<int> optimizeLocations(cv::Mat oldImg, cv::Mat newImg, const std::vector<double> &oldXY, std::vector<double> &newXY,
                                       std::vector<int> *iterations = nullptr);
    static int lastStatus();
    static int lastIterations();

  private:
    parameters params;
};
#endif

namespace putslam_hip {
// MatcherParameters::PatchesParams as every shipped matcher XML sets it: <MatchingOnPatches verbose="0" warping="false"
// patchSize="13" maxIterationCount="50" minSqrtError="0.04"/> (matcher.h:295-304,362)
inline MatchingOnPatches::parameters shippedPatchesParams() { return MatchingOnPatches::parameters{0, false, 13, 6, 50, 0.04}; }
} // namespace putslam_hip

namespace putslam {

// ---------------------------------------------------------------------------------------------
class TransformEst {
  public:
    virtual const std::string &getName() const = 0;
    // setA, setB: N x 3; returns a reference to the member `transformation` (maps A onto B)
    virtual Mat34 &computeTransformation(const Eigen::MatrixXd &setA, const Eigen::MatrixXd &setB) = 0;
    virtual ~TransformEst() {}

  protected:
    Mat34 transformation;
};

class KabschEst : public TransformEst {
  public:
    typedef std::unique_ptr<KabschEst> Ptr;
    KabschEst(void);
    const std::string &getName() const;
    Mat34 &computeTransformation(const Eigen::MatrixXd &setA, const Eigen::MatrixXd &setB);
    virtual ~KabschEst() {}

  private:
    const std::string name;
};

// library-owned singleton, raw pointer returned, a second call replaces the instance (kabschEst.cpp:8,70-73)
TransformEst *createKabschEstimator(void);

} // namespace putslam

namespace putslam_hip {

// ---------------------------------------------------------------------------------------------
// Hot-path part of the Matcher plugin.  Detection / description are image-domain OpenCV
// stages outside the path: their pure virtuals are not part of this class; the
// frame enters at the point where Matcher::match has descriptors and 3-D points (matcher.cpp:467-480).
// Deliberately NOT named putslam::Matcher: the reference's class of that name stays in a PUTSLAM build and
// delegates to this one, so the two can be linked into one program.
class FrameMatcher {
  public:
    struct MatcherParameters {
        int verbose = 0;
        RANSAC::parameters RANSACParams;
        cv::Mat cameraMatrixMat; // 3x3 CV_32FC1
        cv::Mat distortionCoeffsMat; // 1x5 CV_32FC1: k1 k2 p1 p2 k3 (datasetConfig rgbDistortion; what frontEnd undistorts with)
        struct {
            double matchingXYZSphereRadius = 0.12;            // putslammatcherOpenCVParameters.xml:71
            double matchingXYZacceptRatioOfBestMatch = 0.55;  // :72
            double minimalReprojDistanceNewTrackingFeatures = 3;     // :68
            double minimalEuclidDistanceNewTrackingFeatures = 0.01;  // :69
            // the tracker's block (matcher.h:45-49,59-60; putslammatcherOpenCVParameters.xml:64,73-75)
            int useInitialFlow = 0, winSize = 7, maxLevels = 3, maxIter = 30;
            float eps = 0.01f;
            double trackingErrorThreshold = 25.0, trackingMinEigThreshold = 0.0;
            int trackingErrorType = 0;
            int removeTooCloseFeatures = 0; // putslammatcherOpenCVParameters.xml:77; trackStep below takes 0 only
            // the detector's block (matcher.h:40,43,51; putslammatcherOpenCVParameters.xml:64,67): detectFeatures below runs "ORB" and "FAST"
            std::string detector = "ORB";
            int gridRows = 1, gridCols = 1;
            int maximalTrackedFeatures = 500;
            int minimalTrackedFeatures = 150; // matcher.h:51; putslammatcherOpenCVParameters.xml:66 (trackKLT's refill)
            // the descriptor's name (matcher.h:40; putslammatcherOpenCVParameters.xml:64): describeFeatures below runs "ORB"
            std::string descriptor = "ORB";
            double DBScanEps = 1; // matcher.h:54; putslammatcherOpenCVParameters.xml:70 (frontEnd's thinning)
        } OpenCVParams;
        MatchingOnPatches::parameters PatchesParams = shippedPatchesParams(); // matcher.h:362; MatchingOnPatches(PatchesParams) takes it
        MatcherParameters();
    };

    // What Matcher::matchXYZ reads of a MapFeature (putslam_defs.h:120-216): position, the descriptor of the
    // chosen view with its octave and detection distance (ExtendedDescriptor), and the feature id.
    struct MapFeatureXYZ {
        unsigned int id = 0;
        double position[3] = {0, 0, 0};
        cv::Mat descriptor; // 1 x 32 CV_8U, or 1 x D CV_32F
        int octave = 0;
        double detDist = 1.0;
    };
    static constexpr double scaleFactor = 1.2; // matcher.h:26-27
    static constexpr int nLevels = 8;

    // Matcher::featureSet (matcher.h:31-37) restricted to what the hot path holds: the image-domain members
    // (cv::KeyPoint lists, 2-D positions, detection distances) belong to the out-of-scope detect/describe stages.
    struct featureSet {
        cv::Mat descriptors;
        std::vector<Eigen::Vector3f> feature3D;
    };

    FrameMatcher(const std::string _name);
    virtual ~FrameMatcher();
    // one resident frame store (context + stream + HBM slots) per instance: not copyable
    FrameMatcher(const FrameMatcher &) = delete;
    FrameMatcher &operator=(const FrameMatcher &) = delete;
    virtual const std::string &getName() const = 0;
    virtual std::vector<cv::DMatch> performMatching(cv::Mat prevDescriptors, cv::Mat descriptors) = 0;

    // First frame: stores descriptors + 3-D points as the "previous" state (detectInitFeatures, matcher.cpp:17-64).
    void detectInitFeatures(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D);
    // matcher.cpp:470-515 from the described frame on: performMatching(prev, cur) -> RANSAC with errorVersionVO
    // -> swap cur -> prev; returns RANSAC::pointInlierRatio(inliers, matches).
    double match(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D, Eigen::Matrix4f &estimatedTransformation,
                 std::vector<cv::DMatch> &inlierMatches);
    double runVO(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D, Eigen::Matrix4f &estimatedTransformation,
                 std::vector<cv::DMatch> &inlierMatches)
    {
        return match(descriptors, features3D, estimatedTransformation, inlierMatches);
    }
    // Loop-closure matching of two feature sets (matchFeatureLoopClosure, matcher.cpp:802-861): BF match +
    // RANSAC with errorVersionMap; returns -1 when there are no matches, 0 when either set has < 10 features.
    double matchFeatureLoopClosure(cv::Mat desc0, std::vector<Eigen::Vector3f> pts0, cv::Mat desc1,
                                   std::vector<Eigen::Vector3f> pts1, Eigen::Matrix4f &estimatedTransformation,
                                   std::vector<cv::DMatch> &inlierMatches);
    // Guided matching of map features against the current pose's keypoints + RANSAC with errorVersionMap
    // (matchXYZ, matcher.cpp:606-798): returns RANSAC::pointInlierRatio, or -1 when nothing matched.  The type of
    // currentPoseDescriptors decides the value (:625-628): CV_32F Mats (SURF / SIFT, rows of D floats) take NORM_L2
    // (ps_match_xyz_l2_f32; matchXYZLadder: ps_map_pairs_l2_device), CV_8U Mats the Hamming path.  Mixed types, or a float map
    // row whose width differs from the frame's, print one line to std::cerr and return -1.
    double matchXYZ(const std::vector<MapFeatureXYZ> &mapFeatures, cv::Mat currentPoseDescriptors,
                    std::vector<Eigen::Vector3f> &currentPoseFeatures3D, const std::vector<int> &currentPoseOctaves,
                    const std::vector<double> &currentPoseDetDists, Eigen::Matrix4f &estimatedTransformation,
                    std::vector<cv::DMatch> &inlierMatches, int computationNumber = 1);
    // The retry loop of PUTSLAM.cpp:788-798 around matchXYZ as ONE device call (ps_map_pairs_device): tries 1 .. maxTries -- radius
    // + 0.02 (k - 1), ratio max(0.1, a - 0.05 (k - 1)), matcher.cpp:617-622 -- run side by side on the view and the frame uploaded
    // once, and the first try whose inlier ratio is not below minRatio is returned, else the last (*tryUsed = its number).  Try k
    // draws from seed + 0x51ED270B0B5 + frameCounter + (k - 1): equal to matchXYZ at try 1; matchXYZ's later tries all draw from
    // the one seed, so the sample streams differ from try 2 on.  It does maxTries times the work of a first try that succeeds: for
    // hosts that care about the worst frame (ten sequential tries are ten round trips).
    double matchXYZLadder(const std::vector<MapFeatureXYZ> &mapFeatures, cv::Mat currentPoseDescriptors,
                          std::vector<Eigen::Vector3f> &currentPoseFeatures3D, const std::vector<int> &currentPoseOctaves,
                          const std::vector<double> &currentPoseDetDists, Eigen::Matrix4f &estimatedTransformation,
                          std::vector<cv::DMatch> &inlierMatches, int maxTries = 10, double minRatio = 0.1, int *tryUsed = nullptr);
    // Matcher::mergeTrackedFeatures (matcher.cpp:97-130): a sandbox feature is appended to the five lists unless an existing
    // feature, or a sandbox feature appended before it, lies closer in the undistorted image than
    // OpenCVParams.minimalReprojDistanceNewTrackingFeatures (ps_exclude with ps_exclusion_rule_merge_tracked).
    void mergeTrackedFeatures(std::vector<cv::Point2f> &undistortedFeatures2D, const std::vector<cv::Point2f> &featuresSandBoxUndistorted,
                              std::vector<cv::Point2f> &distortedFeatures2D, const std::vector<cv::Point2f> &featuresSandBoxDistorted,
                              std::vector<Eigen::Vector3f> &features3D, const std::vector<Eigen::Vector3f> &features3DSandBox,
                              std::vector<cv::KeyPoint> &keyPoints, const std::vector<cv::KeyPoint> &keyPointsSandBox,
                              std::vector<double> &detDists, const std::vector<double> &detDistsSandBox);
    // Matcher::removeTooCloseFeatures (matcher.cpp:886-974): feature j goes iff some earlier feature lies closer than
    // minimalEuclidDistanceNewTrackingFeatures in space or minimalReprojDistanceNewTrackingFeatures in the undistorted image
    // (ps_exclusion_rule_too_close).  The five lists lose those entries; `matches` loses the matches whose trainIdx was removed
    // and is NOT renumbered (:960-963).  Returns featuresToRemove.
    std::set<int> removeTooCloseFeatures(std::vector<cv::Point2f> &distortedFeatures2D, std::vector<cv::Point2f> &undistortedFeatures2D,
                                         std::vector<Eigen::Vector3f> &features3D, std::vector<cv::KeyPoint> &keyPoints,
                                         std::vector<double> &detDists, std::vector<cv::DMatch> &matches);
    // ---- pipelined form of runVO (ps_vo_stream_push_async / ps_vo_stream_pop, include/putslam_hip.h): the same call shape --
    // one frame per call, the previous frame kept as state (matcher.cpp:452-516) -- with the result returned with a LAG, so that
    // uploads, kernels and downloads of consecutive frames overlap (BASELINE configs[2]: a sequence streamed through the matcher).
    // Results are those runVO returns for the same frames in the same order (pair k draws from seed + k either way).
    //   setPipeline    frames per submitted chunk (1 = lowest latency) and chunks in flight; before the first enqueueFrame
    //   enqueueFrame   the first frame after construction / resetPipeline is the initial one (detectInitFeatures); returns false
    //                  when the frame was NOT taken.  enqueueFrameStatus tells why: 1 = taken, 0 = busy -- the pipeline is full, or
    //                  the frame has more keypoints than the pipeline was built for and results are still pending: dequeue
    //                  results and call again (the `while (!enqueueFrame(..)) dequeueResult(..)` loop does; once drained the
    //                  pipeline is rebuilt with more room and numbering continues) --, -1 = error (lastError() has the text;
    //                  enqueueFrame also prints it): retrying the same frame will not help
    //   dequeueResult  1 = the next frame's result (in frame order), 0 = none ready (wait = false) or none pending,
    //                  -1 = error; a partly filled chunk is submitted when a waiting call finds nothing in flight
    //   flushFrames    submits a partly filled chunk now
    void setPipeline(int chunkFrames, int lanes);
    bool enqueueFrame(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D);
    int enqueueFrameStatus(cv::Mat descriptors, std::vector<Eigen::Vector3f> features3D);
    const std::string &lastError() const { return lastError_; }
    int dequeueResult(Eigen::Matrix4f &estimatedTransformation, std::vector<cv::DMatch> &inlierMatches, double &pointInlierRatio,
                      bool wait = true);
    bool flushFrames();
    void resetPipeline();
    int getNumberOfFeatures() const { return (int)prevFeatures3D.size(); }
    featureSet getFeatures() // matcher.cpp:980-989
    {
        featureSet r;
        r.descriptors = prevDescriptors;
        r.feature3D = prevFeatures3D;
        return r;
    }
    void setSampleSeed(uint64_t s) { seed_ = s; seeded_ = true; }

    MatcherParameters matcherParameters;

  protected:
    const std::string name;
    cv::Mat prevDescriptors;
    std::vector<Eigen::Vector3f> prevFeatures3D;
    int frameCounter;
    uint64_t seed_ = 0;
    bool seeded_ = false;
    // MatcherOpenCV sets fusedMatch_: match() then runs performMatching + RANSAC as ONE call against the previous
    // frame kept in HBM (ps_vo_stream_push: the prevDescriptors / prevFeatures3D state of matcher.h:379-384 lives on
    // the GPU as well, one upload and one download per frame) -- same results as the two separate calls.  A class
    // that overrides performMatching leaves it false and gets the generic sequence.
    bool fusedMatch_ = false;
    struct Fused;
    std::unique_ptr<Fused> fused_;
    bool fusedSynced_ = false; // the resident frame is prevDescriptors / prevFeatures3D
    int pipeChunk_ = 32, pipeLanes_ = 0; // (lanes 0 = the library's choice by chunk size)
    bool pipeFirst_ = true;    // the next enqueued frame has no predecessor
    uint64_t pipeSeed_ = 0;    // hypothesis seed of the pipeline's pair 0 (pair k draws from pipeSeed_ + k, across rebuilds)
    bool pipeSeeded_ = false;
    std::string lastError_;
    bool buildPipeline(int cap, uint64_t pairsSoFar);
    bool fusedMatchCall(const cv::Mat &descriptors, const std::vector<Eigen::Vector3f> &features3D,
                        Eigen::Matrix4f &estimatedTransformation, std::vector<cv::DMatch> &inlierMatches,
                        double &pointInlierRatio);
};

// PUTSLAM::chooseFeaturesToAddToMap (src/PUTSLAM/PUTSLAM.cpp:98-178) on the positions it reads: feature3D / undistortedFeature2D of
// the frame's featureSet, and of every visible map feature the float casts of position and (u, v) (:58-60,66;
// putslam_matcher_glue.h makes them from std::vector<MapFeature>).  Starts from `addedCounter` and returns the new one, as the
// reference does; acceptedIndices receives the indices j it accepted, in order.  Building the RGBDFeature of each (descriptor row,
// ExtendedDescriptor, :138-170) stays with the caller.  On an error nothing is accepted (the text goes to stderr).
int chooseFeaturesToAddToMap(const std::vector<Eigen::Vector3f> &feature3D, const std::vector<cv::Point2f> &undistortedFeature2D,
                             int addedCounter, int maxOnceFeatureAdd, const std::vector<Eigen::Vector3f> &mapFeaturePositions,
                             const std::vector<cv::Point2f> &mapFeatureUV, float minEuclideanDistanceOfFeatures,
                             float minImageDistanceOfFeatures, std::vector<int> &acceptedIndices);

// MatcherOpenCV::performMatching (matcherOpenCV.cpp:198-206) as a free function over the calling thread's context.
std::vector<cv::DMatch> hammingCrossCheckMatch(cv::Mat prevDescriptors, cv::Mat descriptors);
// ... and with the float descriptors' matcher, cv::BFMatcher(cv::NORM_L2, true) (matcherOpenCV.cpp:100-102): CV_32F Mats.
std::vector<cv::DMatch> l2CrossCheckMatch(cv::Mat prevDescriptors, cv::Mat descriptors);

// MatcherOpenCV::performTracking (matcherOpenCV.cpp:209-300) as a free function over the calling thread's context
// (ps_perform_tracking): cv::calcOpticalFlowPyrLK on the image pair (CV_8UC1 or CV_8UC3 Mats of one size), keyPoints / detDists
// copied from the previous frame's with the tracked positions, the error gate, the too-close-by-error removal, and the erase of
// every feature that did not survive from features, keyPoints and detDists; returns DMatch(i, j, 0) per survivor.  On an error
// the three vectors come back empty with no matches (the text goes to stderr).
std::vector<cv::DMatch> trackFeaturesLK(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat prevImg, cv::Mat img,
                                        std::vector<cv::Point2f> &prevFeatures, std::vector<cv::Point2f> &features,
                                        std::vector<cv::KeyPoint> &prevKeyPoints, std::vector<cv::KeyPoint> &keyPoints,
                                        std::vector<double> &prevDetDists, std::vector<double> &detDists);

// MatcherOpenCV::detectFeatures (matcherOpenCV.cpp:118-180) for OpenCVParams.detector == "FAST" (cv::FastFeatureDetector::create(),
// :64-65: threshold 10, non-maximum suppression on, pattern 9/16) as a free function over the calling thread's context
// (ps_detect_features): cvtColor(RGB2GRAY) -- channel 0 takes the red weight; a CV_8UC1 Mat is taken as grey already --, the
// gridCols x gridRows ROIs, the detector in each, the per-ROI ordering by response cut to maximalTrackedFeatures * 3 / (gridCols *
// gridRows), the joined ordering cut to maximalTrackedFeatures.  rgbImage: CV_8UC1 or CV_8UC3, any step (a region of a parent).
// Each key point is (pt, size 7, angle -1, response = score, octave 0, class_id -1).
// BOTH orderings are STABLE here: the reference's std::sort (compare_response, matcherOpenCV.h:84-87) leaves the order of equal
// responses, and who survives a cut inside a tie, to its libstdc++; this library keeps raster order inside an ROI and the order
// of the ROI loop across ROIs (include/putslam_hip.h).
// Any other detector is NOT run here: one line goes to std::cerr and the list comes back empty.
std::vector<cv::KeyPoint> detectFeaturesFAST(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat rgbImage);
// MatcherOpenCV::detectFeatures for OpenCVParams.detector == "ORB" (cv::ORB::create(), :66-67), the SHIPPED detector: the same grid
// loop around ORB detection with create()'s defaults (500 features, scaleFactor 1.2f, 8 levels, fastThreshold 20) through
// ps_detect_features_orb (include/putslam_hip.h).  Every ROI has its own pyramid.  A key point is (pt in
// image coordinates, size 31 * scale of its level, angle in degrees, the Harris response, octave = level, class_id -1): what
// describeFeaturesORB below and DBScan take.  The detector's name is not looked at (FrameMatcherHIP::detectFeatures dispatches on it).
std::vector<cv::KeyPoint> detectFeaturesORB(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat rgbImage);

// MatcherOpenCV::describeFeatures (matcherOpenCV.cpp:183-195) for OpenCVParams.descriptor == "ORB" (cv::ORB::create(): scaleFactor
// 1.2f, 8 levels) as a free function over the calling thread's context (ps_describe_features): descriptorExtractor->compute(rgbImage,
// features, descriptors) in the project's reading of OpenCV 3.0 - 3.3 (include/putslam_hip.h) with the library's default sampling
// pattern -- a host that needs OpenCV's own rows calls ps_describe_features with OpenCV's table.  rgbImage: CV_8UC1 or CV_8UC3, any
// step.  Returns an n x 32 CV_8U Mat and REPLACES `features` by the described key points in the rows' order, as OpenCV does: those
// 31 pixels inside the image, grouped by octave, input order inside an octave.
// Any other descriptor (SURF, SIFT) is NOT run on the CPU instead: one line goes to std::cerr, the Mat comes back empty and
// `features` is cleared.
cv::Mat describeFeaturesORB(const FrameMatcher::MatcherParameters &matcherParameters, cv::Mat rgbImage, std::vector<cv::KeyPoint> &features);

// Library-owned singletons with the reference factories' ownership rules (raw pointer returned, a second call
// replaces the instance: matcherOpenCV.cpp:20-47): one for the VO thread, one for the loop-closure thread.
FrameMatcher *createFrameMatcher(void);
FrameMatcher *createFrameMatcher(const std::string _parametersFile, const std::string _grabberParametersFile);
FrameMatcher *createLoopClosingFrameMatcher(const std::string _parametersFile, const std::string _grabberParametersFile);

// ---------------------------------------------------------------------------------------------
// VO driver (PUTSLAM::startProcessing, src/PUTSLAM/PUTSLAM.cpp:733-740,1006-1016): pose composition with
// the 0.1 m gate and the TUM trajectory line format.
struct VOTrajectory {
    Eigen::Matrix4f VOPoseEstimate = Eigen::Matrix4f::Identity();
    void addIncrement(Eigen::Matrix4f poseIncrement);
    static std::string freiburgLine(const Eigen::Matrix4f &pose, double timestamp);
};

// The concrete matcher: performMatching = cv::BFMatcher(NORM_HAMMING, crossCheck = true).match(prev, cur) on the GPU
// (the body MatcherOpenCV::performMatching gets in a PUTSLAM build, matcherOpenCV.cpp:198-206) for CV_8U descriptor Mats and
// cv::BFMatcher(NORM_L2, true) for CV_32F ones (matcherOpenCV.cpp:100-102); match() fused with the RANSAC against the frame
// resident in HBM (binary descriptors only).
class FrameMatcherHIP : public FrameMatcher {
  public:
    typedef std::unique_ptr<FrameMatcherHIP> Ptr;
    FrameMatcherHIP(void);
    FrameMatcherHIP(const std::string _parametersFile, const std::string _grabberParametersFile);
    ~FrameMatcherHIP(void);
    virtual const std::string &getName() const;
    virtual std::vector<cv::DMatch> performMatching(cv::Mat prevDescriptors, cv::Mat descriptors);
    // MatcherOpenCV::performTracking, matcherOpenCV.cpp:209-300 (the reference's signature; trackFeaturesLK above)
    virtual std::vector<cv::DMatch> performTracking(cv::Mat prevImg, cv::Mat img, std::vector<cv::Point2f> &prevFeatures,
                                                    std::vector<cv::Point2f> &features, std::vector<cv::KeyPoint> &prevKeyPoints,
                                                    std::vector<cv::KeyPoint> &keyPoints, std::vector<double> &prevDetDists,
                                                    std::vector<double> &detDists);
    // MatcherOpenCV::detectFeatures, matcherOpenCV.cpp:118-180 (the reference's signature; detectFeaturesORB / detectFeaturesFAST above by OpenCVParams.detector)
    virtual std::vector<cv::KeyPoint> detectFeatures(cv::Mat rgbImage);
    // MatcherOpenCV::describeFeatures, matcherOpenCV.cpp:183-195 (the reference's signature; describeFeaturesORB above)
    virtual cv::Mat describeFeatures(cv::Mat rgbImage, std::vector<cv::KeyPoint> &features);
    // The whole per-frame front end of Matcher::detectInitFeatures (matcher.cpp:19-49) / Matcher::match (:457-482) for detector and
    // descriptor "ORB" as ONE call (ps_front_end_frame): detectFeatures, DBScan(OpenCVParams.DBScanEps).run, describeFeatures,
    // removeImageDistortion with cameraMatrixMat / distortionCoeffsMat and keypoints2Dto3D with depthImageScale, the last two on the
    // DESCRIBED key points in the described order.  rgbImage CV_8UC1 / CV_8UC3, depthImage CV_16U of the same size, any steps.
    // descriptors: n x 32 CV_8U; features3D: n points; keyPoints (the described ones, all six fields) and undistorted
    // (prevFeaturesUndistorted) where asked for.  With
    //     auto fe = [&](const SensorFrame &s, cv::Mat &d, std::vector<Eigen::Vector3f> &p) { m.frontEnd(s.rgbImage, s.depthImage, s.depthImageScale, d, p); };
    // it is the frontEnd callable of putslam_matcher_glue.h.  Any other detector or descriptor is NOT run on the CPU instead: one line
    // goes to std::cerr and every output comes back empty.
    void frontEnd(cv::Mat rgbImage, cv::Mat depthImage, double depthImageScale, cv::Mat &descriptors, std::vector<Eigen::Vector3f> &features3D,
                  std::vector<cv::KeyPoint> *keyPoints = nullptr, std::vector<cv::Point2f> *undistorted = nullptr);
    // The first half of Matcher::trackKLT (matcher.cpp:147-211) as ONE call (ps_track_vo_pair): performTracking on (prevRgbImage,
    // rgbImage) from prevFeaturesDistorted, removeImageDistortion of the tracked positions with cameraMatrixMat / distortionCoeffsMat,
    // keypoints2Dto3D in depthImage with depthImageScale, keyPoints / detDists carried from the previous frame's by the kept index
    // (a key point's pt is its tracked position), and RANSAC::estimateTransformation(prevFeatures3D, features3D, matches) with
    // RANSACParams.errorVersionVO.  It reads the OpenCVParams tracking members performTracking reads.  The previous frame's four
    // lists are left as they are; the five lists of this frame, `matches` (DMatch(i, j, 0)) and inlierMatches are replaced.  Under
    // useInitialFlow `distorted` is the initial flow when it has one entry per previous feature.  Returns false -- one line on
    // std::cerr, every output empty, the identity -- on an error and for OpenCVParams.removeTooCloseFeatures > 0: the reference
    // erases the removed features from features3D and leaves the matches' trainIdx un-renumbered (matcher.cpp:960-963, recorded at
    // removeTooCloseFeatures above), so its RANSAC reads stale indices; a host that wants the filter calls removeTooCloseFeatures
    // on what this call returned.  No previous feature: true, the identity, nothing tracked (:147-148).
    bool trackStep(cv::Mat prevRgbImage, cv::Mat rgbImage, cv::Mat depthImage, double depthImageScale,
                   const std::vector<cv::Point2f> &prevFeaturesDistorted, const std::vector<Eigen::Vector3f> &prevFeatures3D,
                   const std::vector<cv::KeyPoint> &prevKeyPoints, const std::vector<double> &prevDetDists,
                   std::vector<cv::Point2f> &distorted, std::vector<cv::Point2f> &undistorted, std::vector<Eigen::Vector3f> &features3D,
                   std::vector<cv::KeyPoint> &keyPoints, std::vector<double> &detDists, std::vector<cv::DMatch> &matches,
                   std::vector<cv::DMatch> &inlierMatches, Eigen::Matrix4f &estimatedTransformation);
    // Matcher::trackKLT (matcher.cpp:133-449) on what it reads of a SensorFrame (rgbImage, depthImage, depthImageScale), for detector
    // and descriptor "ORB": trackStep above from the kept prev* state (the identity when there is none, :147-148), then :213-381 as
    // ONE call (ps_track_close_pair) -- the refill when fewer than OpenCVParams.minimalTrackedFeatures rows survived (detectFeatures,
    // DBScan(DBScanEps).run, removeImageDistortion, keypoints2Dto3D, the detection distances, mergeTrackedFeatures), the predicted
    // level of every row, the reordering by level, describeFeatures at that level and the removal of the rows it dropped -- and the
    // swap of :436-445: the closed rows, their descriptors and the two images (shallow, as the reference keeps them) are the prev*
    // state of the next call.  A merged key point is the one detectFeaturesORB makes.  Returns RANSAC::pointInlierRatio(inlierMatches,
    // matches), 0 with no matches (:404-406).  On an error and for removeTooCloseFeatures > 0: one line on std::cerr, 0, the identity,
    // the state as it was.  Where the reference's position-matching walk (:359-375) would pair a dropped row's columns with its
    // neighbour's descriptor (two rows within 0.0001 px across the border: DESIGN.md section 8.15), every descriptor stays with its row.
    double trackKLT(cv::Mat rgbImage, cv::Mat depthImage, double depthImageScale, Eigen::Matrix4f &estimatedTransformation,
                    std::vector<cv::DMatch> &inlierMatches);
    // What PUTSLAM.cpp:826-837 and FeaturesMap::addMeasurements (featuresMap.cpp:255-282) make of matchXYZ's inliers, as the data of
    // Edge3D(position, info, poseId, featureId): per inlier match, in inlierMatches' order, the map row (queryIdx), the frame's row
    // (trainIdx), (u, v) = undistorted[trainIdx], position = features3D[trainIdx] widened, the normal, the colour gradient and the
    // information matrix of `uncertaintyModel` (-1: the identity, useUncertainty off; 0, 1, 2: config.uncertaintyModel) under
    // `sensor` -- ps_compute_normals, ps_compute_rgb_gradients and ps_information_matrices on the gathered rows, byte for byte
    // ps_measurement_edges' on a device-resident batch.  rgbImage CV_8UC3, depthImage CV_16U.  On an error, or a trainIdx outside
    // the two lists: one line on std::cerr and an empty result.
    struct MeasurementEdge {
        int mapRow, curRow;
        float u, v;
        putslam_hip::Vec3 position, normal, RGBgradient;
        putslam_hip::Mat33 info;
    };
    std::vector<MeasurementEdge> measurementEdges(const std::vector<cv::DMatch> &inlierMatches, const std::vector<cv::Point2f> &undistorted,
                                                  const std::vector<Eigen::Vector3f> &features3D, cv::Mat rgbImage, cv::Mat depthImage,
                                                  double depthImageScale, DepthSensorModel &sensor, int uncertaintyModel);

  protected: // Matcher's tracking state (matcher.h:379-391); prevDescriptors and prevFeatures3D are FrameMatcher's
    cv::Mat prevRgbImage, prevDepthImage;
    std::vector<cv::Point2f> prevFeaturesUndistorted, prevFeaturesDistorted;
    std::vector<cv::KeyPoint> prevKeyPoints;
    std::vector<double> prevDetDists;
};

} // namespace putslam_hip
