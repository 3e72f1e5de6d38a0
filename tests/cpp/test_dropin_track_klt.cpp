// FrameMatcherHIP::trackKLT (Matcher::trackKLT, matcher.cpp:133-449) over four frames: after every call the pose, the inlier
// matches, the returned ratio and the whole prev* state equal what the reference's loop gives when it is restated over the drop-in's
// own classes -- performTracking, RGBD::removeImageDistortion, RGBD::keypoints2Dto3D, RANSAC, detectFeatures, DBScan,
// describeFeatures, ps_predicted_level -- with the position-matching walk of :359-375 done literally, as bytes.  The first call has
// no features at all (:147-148, then the refill from nothing); the third is due and merges a sandbox into tracked rows; the second
// and the fourth are not due.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

#include "putslam_dropin.h"
#include "putslam_hip.h"

namespace {

const int kRows = 150, kCols = 200;
const double kScale = 5000.0;

uint32_t hash2(uint32_t a, uint32_t b)
{
    uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA6Bu;
    h ^= h >> 15;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 13);
}

// blocks of 6 x 6 pixels with random brightness, smoothed by a 3 x 3 box, moved by (dx, dy) whole pixels around the torus
void scene(cv::Mat &img, cv::Mat &depth, int cn, int dx, int dy)
{
    const auto block = [](int x, int y, int c) {
        x = ((x % kCols) + kCols) % kCols;
        y = ((y % kRows) + kRows) % kRows;
        return 40 + (int)(hash2((uint32_t)(x / 6) + 131u * (uint32_t)c, (uint32_t)(y / 6)) % 176u);
    };
    for (int y = 0; y < kRows; ++y)
        for (int x = 0; x < kCols; ++x) {
            for (int c = 0; c < cn; ++c) {
                int s = 0;
                for (int j = -1; j <= 1; ++j)
                    for (int i = -1; i <= 1; ++i) s += block(x - dx + i, y - dy + j, c);
                img.data[(size_t)y * img.step + (size_t)x * cn + c] = (unsigned char)((s + 4) / 9);
            }
            const int u = ((x - dx) % kCols + kCols) % kCols, v = ((y - dy) % kRows + kRows) % kRows;
            int z = 6000 + 30 * u + 20 * v;
            if (hash2((uint32_t)u, (uint32_t)v + 977u) % 10u == 0u) z = 0; // holes
            reinterpret_cast<uint16_t *>(depth.data + (size_t)y * depth.step)[x] = (uint16_t)z;
        }
}

bool same_bits(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

void configure(putslam_hip::FrameMatcherHIP &m)
{
    auto &p = m.matcherParameters;
    const float K[9] = {210.f, 0.f, 99.5f, 0.f, 208.f, 74.5f, 0.f, 0.f, 1.f}; // a camera whose image is 200 x 150
    for (int i = 0; i < 9; ++i) p.cameraMatrixMat.at<float>(i / 3, i % 3) = K[i];
    p.OpenCVParams.maximalTrackedFeatures = 120;
    p.OpenCVParams.DBScanEps = 3.0;
    p.RANSACParams.errorVersion = 3; // (not the one the step may use)
    p.RANSACParams.errorVersionVO = 0;
    m.setSampleSeed(41);
}

// the matcher under test, with its state readable
struct Probe : putslam_hip::FrameMatcherHIP {
    using FrameMatcherHIP::prevDescriptors;
    using FrameMatcherHIP::prevDetDists;
    using FrameMatcherHIP::prevFeatures3D;
    using FrameMatcherHIP::prevFeaturesDistorted;
    using FrameMatcherHIP::prevFeaturesUndistorted;
    using FrameMatcherHIP::prevKeyPoints;
};

// Matcher's tracking state and the loop of matcher.cpp:133-449 over the drop-in's separate classes
struct Restated {
    putslam_hip::FrameMatcherHIP tools;
    cv::Mat prevRgbImage, prevDescriptors;
    std::vector<cv::Point2f> prevFeaturesUndistorted, prevFeaturesDistorted;
    std::vector<Eigen::Vector3f> prevFeatures3D;
    std::vector<cv::KeyPoint> prevKeyPoints;
    std::vector<double> prevDetDists;
    int tracked = 0;    // frames RANSAC has run for: the drop-in draws from seed + that many
    int lastMerged = 0; // candidates the last call's refill appended

    static double norm(const cv::Point2f &a, const cv::Point2f &b) // cv::norm(a - b)
    {
        const float dx = a.x - b.x, dy = a.y - b.y;
        return std::sqrt((double)dx * dx + (double)dy * dy);
    }

    double trackKLT(cv::Mat rgbImage, cv::Mat depthImage, Eigen::Matrix4f &T, std::vector<cv::DMatch> &inlierMatches)
    {
        const auto &mp = tools.matcherParameters;
        const auto &cvp = mp.OpenCVParams;
        std::vector<cv::Point2f> undistorted, distorted;
        std::vector<cv::KeyPoint> keyPoints;
        std::vector<double> detDists;
        std::vector<Eigen::Vector3f> features3D;
        std::vector<cv::DMatch> matches;
        inlierMatches.clear();
        lastMerged = 0;
        if (prevFeaturesUndistorted.size() == 0 || prevFeaturesDistorted.size() == 0) { // :147-148
            T = Eigen::Matrix4f::Identity();
        } else {
            std::vector<cv::Point2f> pd = prevFeaturesDistorted;
            std::vector<cv::KeyPoint> pk = prevKeyPoints;
            std::vector<double> pdd = prevDetDists;
            matches = tools.performTracking(prevRgbImage, rgbImage, pd, distorted, pk, keyPoints, pdd, detDists);                         // :151-156
            if (!distorted.empty()) {
                undistorted = RGBD::removeImageDistortion(distorted, mp.cameraMatrixMat, mp.distortionCoeffsMat);       // :159-161
                features3D = RGBD::keypoints2Dto3D(undistorted, depthImage, mp.cameraMatrixMat, kScale);                // :184-186
            }
            RANSAC::parameters rp = mp.RANSACParams;
            rp.errorVersion = rp.errorVersionVO;                                                                        // :203-204
            RANSAC ransac(rp, mp.cameraMatrixMat);
            ransac.setSampleSeed(41 + (uint64_t)tracked++);
            T = ransac.estimateTransformation(prevFeatures3D, features3D, matches, inlierMatches);                      // :209-210
        }
        if ((int)undistorted.size() < cvp.minimalTrackedFeatures) {                                                     // :214-215
            std::vector<cv::KeyPoint> sandbox = tools.detectFeatures(rgbImage);                                         // :218-219
            DBScan dbscan(cvp.DBScanEps);
            dbscan.run(sandbox);                                                                                        // :222-223
            std::vector<cv::Point2f> sbDistorted;
            for (const auto &kp : sandbox) sbDistorted.push_back(kp.pt);                                                // :227
            std::vector<cv::Point2f> sbUndistorted, tmp = sbDistorted;
            std::vector<Eigen::Vector3f> sb3D;
            if (!sandbox.empty()) {
                sbUndistorted = RGBD::removeImageDistortion(tmp, mp.cameraMatrixMat, mp.distortionCoeffsMat);           // :230-233
                sb3D = RGBD::keypoints2Dto3D(sbUndistorted, depthImage, mp.cameraMatrixMat, kScale);                    // :235-237
            }
            std::vector<double> sbDetDists;
            for (const auto &f : sb3D) sbDetDists.push_back(std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]));        // :240-245
            for (size_t i = 0; i < sbUndistorted.size(); ++i) {                                                         // :111-128
                bool add = true;
                for (size_t j = 0; j < undistorted.size(); ++j)
                    if (norm(sbUndistorted[i], undistorted[j]) < cvp.minimalReprojDistanceNewTrackingFeatures) {
                        add = false;
                        break;
                    }
                if (add) {
                    undistorted.push_back(sbUndistorted[i]);
                    distorted.push_back(sbDistorted[i]);
                    features3D.push_back(sb3D[i]);
                    keyPoints.push_back(sandbox[i]);
                    detDists.push_back(sbDetDists[i]);
                    ++lastMerged;
                }
            }
        }
        std::vector<cv::KeyPoint> descKeyPoints = keyPoints;                                                            // :281
        for (size_t i = 0; i < descKeyPoints.size(); ++i) {                                                             // :283-301
            const double curDist = std::sqrt(features3D[i][0] * features3D[i][0] + features3D[i][1] * features3D[i][1] + features3D[i][2] * features3D[i][2]);
            descKeyPoints[i].octave = ps_predicted_level(descKeyPoints[i].octave, detDists[i], curDist);
        }
        {                                                                                                               // :302-331
            std::vector<std::vector<size_t>> byLevel(8);
            for (size_t i = 0; i < keyPoints.size(); ++i) byLevel[(size_t)descKeyPoints[i].octave].push_back(i);
            std::vector<cv::Point2f> d, u;
            std::vector<Eigen::Vector3f> p;
            std::vector<cv::KeyPoint> k;
            std::vector<double> dd;
            for (const auto &level : byLevel)
                for (size_t i : level) {
                    d.push_back(distorted[i]);
                    u.push_back(undistorted[i]);
                    p.push_back(features3D[i]);
                    k.push_back(keyPoints[i]);
                    dd.push_back(detDists[i]);
                }
            d.swap(distorted), u.swap(undistorted), p.swap(features3D), k.swap(keyPoints), dd.swap(detDists);
        }
        cv::Mat descriptors = tools.describeFeatures(rgbImage, descKeyPoints);                                          // :338
        if (descKeyPoints.size() != keyPoints.size()) {                                                                 // :343-381
            std::vector<cv::Point2f> d, u;
            std::vector<Eigen::Vector3f> p;
            std::vector<cv::KeyPoint> k;
            std::vector<double> dd;
            for (size_t i = 0, j = 0; i < keyPoints.size(); i++) {
                if (j == descKeyPoints.size()) break;
                if (norm(keyPoints[i].pt, descKeyPoints[j].pt) < 0.0001) {
                    d.push_back(distorted[i]);
                    u.push_back(undistorted[i]);
                    p.push_back(features3D[i]);
                    k.push_back(keyPoints[i]);
                    dd.push_back(detDists[i]);
                    j++;
                }
            }
            d.swap(distorted), u.swap(undistorted), p.swap(features3D), k.swap(keyPoints), dd.swap(detDists);
        }
        double inlierRatio = 0.0;                                                                                       // :404-406
        if (matches.size() > 0) inlierRatio = RANSAC::pointInlierRatio(inlierMatches, matches);
        undistorted.swap(prevFeaturesUndistorted);                                                                      // :436-445
        distorted.swap(prevFeaturesDistorted);
        features3D.swap(prevFeatures3D);
        prevDescriptors = descriptors;
        keyPoints.swap(prevKeyPoints);
        detDists.swap(prevDetDists);
        prevRgbImage = rgbImage;
        return inlierRatio;
    }
};

int run_sequence(const char *name, int cn)
{
    const int type = cn == 3 ? CV_8UC3 : CV_8UC1;
    const int shift[4][2] = {{0, 0}, {2, 3}, {3, 1}, {5, 4}};
    const int minimal[4] = {150, 0, 10000, 0}; // due (nothing to track), not due, due (a merge), not due
    std::vector<cv::Mat> imgs, depths;
    for (int f = 0; f < 4; ++f) {
        imgs.push_back(cv::Mat(kRows, kCols, type));
        depths.push_back(cv::Mat(kRows, kCols, CV_16U));
        scene(imgs.back(), depths.back(), cn, shift[f][0], shift[f][1]);
    }
    Probe matcher;
    Restated ref;
    configure(matcher);
    configure(ref.tools);
    int bad = 0;
    size_t before = 0;
    for (int f = 0; f < 4; ++f) {
        matcher.matcherParameters.OpenCVParams.minimalTrackedFeatures = minimal[f];
        ref.tools.matcherParameters.OpenCVParams.minimalTrackedFeatures = minimal[f];
        Eigen::Matrix4f T, rT;
        std::vector<cv::DMatch> inliers(3), rInliers;
        const double ratio = matcher.trackKLT(imgs[(size_t)f], depths[(size_t)f], kScale, T, inliers);
        const double rRatio = ref.trackKLT(imgs[(size_t)f], depths[(size_t)f], rT, rInliers);
        const size_t k = ref.prevKeyPoints.size();
        bool ok = same_bits(T.data(), rT.data(), 64) && inliers.size() == rInliers.size() && same_bits(inliers.data(), rInliers.data(), inliers.size() * 16) &&
                  same_bits(&ratio, &rRatio, 8) && matcher.prevKeyPoints.size() == k && matcher.prevFeaturesDistorted.size() == k &&
                  matcher.prevFeaturesUndistorted.size() == k && matcher.prevFeatures3D.size() == k && matcher.prevDetDists.size() == k &&
                  ref.prevFeatures3D.size() == k && (size_t)ref.prevDescriptors.rows == k && (size_t)matcher.prevDescriptors.rows == k;
        ok = ok && same_bits(matcher.prevFeaturesDistorted.data(), ref.prevFeaturesDistorted.data(), k * 8) &&
             same_bits(matcher.prevFeaturesUndistorted.data(), ref.prevFeaturesUndistorted.data(), k * 8) &&
             same_bits(matcher.prevFeatures3D.data(), ref.prevFeatures3D.data(), k * 12) &&
             same_bits(matcher.prevDetDists.data(), ref.prevDetDists.data(), k * 8) &&
             (k == 0 || same_bits(matcher.prevDescriptors.data, ref.prevDescriptors.data, k * 32));
        for (size_t j = 0; ok && j < k; ++j) {
            const cv::KeyPoint &a = matcher.prevKeyPoints[j], &b = ref.prevKeyPoints[j];
            ok = same_bits(&a.pt, &b.pt, 8) && same_bits(&a.size, &b.size, 4) && same_bits(&a.angle, &b.angle, 4) &&
                 same_bits(&a.response, &b.response, 4) && a.octave == b.octave && a.class_id == b.class_id;
        }
        const bool accepted = !same_bits(rT.data(), Eigen::Matrix4f::Identity().data(), 64);
        // what the frames were chosen for: nothing to track and a refill from nothing, then tracked and accepted; frame 2 merges
        ok = ok && (f == 0 ? (before == 0 && k > 10 && !accepted && ratio == 0.0) : (accepted && !rInliers.empty() && ratio > 0.0)) &&
             (f == 0 || f == 2 ? ref.lastMerged > 0 : ref.lastMerged == 0);
        std::printf("%s frame %d: %s (%zu rows before, %d merged, %zu after, %zu inliers, ratio %.3f)\n", name, f, ok ? "ok" : "MISMATCH", before,
                    ref.lastMerged, k, rInliers.size(), rRatio);
        bad += ok ? 0 : 1;
        before = k;
    }
    return bad;
}

// removeTooCloseFeatures > 0: one line on std::cerr, 0, the identity, no state
int refusal()
{
    Probe matcher;
    configure(matcher);
    matcher.matcherParameters.OpenCVParams.removeTooCloseFeatures = 1;
    cv::Mat img(kRows, kCols, CV_8UC1), depth(kRows, kCols, CV_16U);
    scene(img, depth, 1, 0, 0);
    Eigen::Matrix4f T;
    std::vector<cv::DMatch> inliers(2);
    std::ostringstream captured;
    std::streambuf *old = std::cerr.rdbuf(captured.rdbuf());
    const double r = matcher.trackKLT(img, depth, kScale, T, inliers);
    std::cerr.rdbuf(old);
    const Eigen::Matrix4f ident = Eigen::Matrix4f::Identity();
    const bool ok = r == 0.0 && captured.str().find("removeTooCloseFeatures") != std::string::npos && same_bits(T.data(), ident.data(), 64) &&
                    inliers.empty() && matcher.prevKeyPoints.empty() && matcher.prevFeatures3D.empty();
    std::printf("removeTooCloseFeatures refused: %s\n", ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run_sequence("grey", 1);
    bad += run_sequence("colour", 3);
    bad += refusal();
    if (bad == 0) std::printf("all ok\n");
    return bad;
}
