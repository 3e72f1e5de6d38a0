// FrameMatcherHIP::performTracking (MatcherOpenCV::performTracking, matcherOpenCV.cpp:209-300) on cv::Mat-shaped inputs against the
// C ABI: its matches and the erased features / keyPoints / detDists equal what ps_perform_tracking returns for the same pair,
// and what ps_calc_optical_flow_pyr_lk + the reference's own selection loop, restated here, give.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
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

uint64_t g_state = 0x2545F4914F6CDD1Dull;
float uniform(float lo, float hi)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (hi - lo) * (float)((g_state >> 40) & 0xFFFF) / 65535.0f;
}

bool same_bits(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

int run_case(const char *name, int cn, bool padded, int initialFlow, int errorType, double errThr, double minDist, int n)
{
    const int rows = 60, cols = 80;
    const size_t step = (size_t)cols * cn + (padded ? 13 : 0);
    std::vector<unsigned char> bufA(step * rows, 0xEE), bufB(step * rows, 0xEE);
    cv::Mat prevImg(rows, cols, cn == 3 ? CV_8UC3 : CV_8UC1, bufA.data(), step), img(rows, cols, cn == 3 ? CV_8UC3 : CV_8UC1, bufB.data(), step);
    texture(prevImg, cn, 0.0, 0.0);
    texture(img, cn, -1.7, 0.9);

    putslam_hip::FrameMatcherHIP matcher;
    auto &cvp = matcher.matcherParameters.OpenCVParams;
    cvp.useInitialFlow = initialFlow;
    cvp.trackingErrorType = errorType;
    cvp.trackingErrorThreshold = errThr;
    cvp.minimalReprojDistanceNewTrackingFeatures = minDist;

    std::vector<cv::Point2f> prevFeatures, features;
    std::vector<cv::KeyPoint> prevKeyPoints, keyPoints(3); // (stale content: performTracking replaces it)
    std::vector<double> prevDetDists, detDists(5, -1.0);
    for (int i = 0; i < n; ++i) {
        cv::Point2f p(uniform(-2.f, cols + 2.f), uniform(-2.f, rows + 2.f));
        if (i % 7 == 3 && i > 0) p = cv::Point2f(prevFeatures[(size_t)i - 1].x + 0.4f, prevFeatures[(size_t)i - 1].y); // a close neighbour
        prevFeatures.push_back(p);
        cv::KeyPoint kp;
        kp.pt = p;
        kp.octave = i % 5;
        kp.response = (float)i;
        prevKeyPoints.push_back(kp);
        prevDetDists.push_back(1.0 + 0.01 * i);
        if (initialFlow) features.push_back(cv::Point2f(p.x + uniform(-2.f, 2.f), p.y + uniform(-2.f, 2.f)));
    }
    const std::vector<cv::Point2f> initial = features;

    // the C ABI on the same pair
    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("%s: no context\n", name);
        return 1;
    }
    PsKltParams prm;
    prm.eps = cvp.eps;
    prm.minEigThreshold = cvp.trackingMinEigThreshold;
    prm.winSize = cvp.winSize;
    prm.maxLevels = cvp.maxLevels;
    prm.maxCount = cvp.maxIter;
    prm.flags = (initialFlow ? PS_KLT_USE_INITIAL_FLOW : 0) | (errorType ? PS_KLT_GET_MIN_EIGENVALS : 0);
    std::vector<cv::Point2f> next = initial.empty() ? std::vector<cv::Point2f>((size_t)n) : initial, next2 = next, keptPts((size_t)n);
    std::vector<uint8_t> status((size_t)n), status2((size_t)n);
    std::vector<float> err((size_t)n), err2((size_t)n);
    std::vector<PsDMatch> abi((size_t)n);
    std::vector<int32_t> keptIdx((size_t)n);
    int k = -1;
    int rc = ps_perform_tracking(ctx, prevImg.data, img.data, rows, cols, cn, step, (const float *)prevFeatures.data(), (float *)next.data(), n,
                                 &prm, errThr, minDist, status.data(), err.data(), abi.data(), &k, (float *)keptPts.data(), keptIdx.data());
    int rc2 = ps_calc_optical_flow_pyr_lk(ctx, prevImg.data, img.data, rows, cols, cn, step, (const float *)prevFeatures.data(),
                                          (float *)next2.data(), n, status2.data(), err2.data(), &prm);
    if (rc != PS_OK || rc2 != PS_OK) {
        std::printf("%s: C ABI failed: %s\n", name, ps_last_error(ctx));
        ps_context_destroy(ctx);
        return 1;
    }
    ps_context_destroy(ctx);
    bool ok = same_bits(next.data(), next2.data(), (size_t)n * 8) && status == status2 && same_bits(err.data(), err2.data(), (size_t)n * 4);

    // the reference's selection, as written (matcherOpenCV.cpp:247-290)
    std::vector<uint8_t> st = status2;
    for (int i = 0; i < n; ++i)
        if (err2[(size_t)i] > errThr) st[(size_t)i] = 0;
    std::set<int> featuresToRemove;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const float dx = next2[(size_t)i].x - next2[(size_t)j].x, dy = next2[(size_t)i].y - next2[(size_t)j].y;
            if (std::sqrt((double)dx * dx + (double)dy * dy) < minDist) featuresToRemove.insert(err2[(size_t)i] > err2[(size_t)j] ? i : j);
        }
    std::vector<int> want;
    for (int i = 0; i < n; ++i)
        if (st[(size_t)i] != 0 && featuresToRemove.find(i) == featuresToRemove.end()) want.push_back(i);
    ok = ok && k == (int)want.size();
    for (int j = 0; ok && j < k; ++j) ok = keptIdx[(size_t)j] == want[(size_t)j];

    // the drop-in
    std::vector<cv::DMatch> matches = matcher.performTracking(prevImg, img, prevFeatures, features, prevKeyPoints, keyPoints, prevDetDists, detDists);
    ok = ok && (int)matches.size() == k && (int)features.size() == k && (int)keyPoints.size() == k && (int)detDists.size() == k &&
         (int)prevFeatures.size() == n;
    for (int j = 0; ok && j < k; ++j) {
        const int i = keptIdx[(size_t)j];
        const cv::DMatch &m = matches[(size_t)j];
        ok = m.queryIdx == i && m.trainIdx == j && m.imgIdx == abi[(size_t)j].imgIdx && m.imgIdx == 0 && m.distance == 0.f &&
             abi[(size_t)j].queryIdx == i && abi[(size_t)j].trainIdx == j &&
             same_bits(&features[(size_t)j], &next[(size_t)i], 8) && same_bits(&features[(size_t)j], &keptPts[(size_t)j], 8) &&
             same_bits(&keyPoints[(size_t)j].pt, &next[(size_t)i], 8) && keyPoints[(size_t)j].octave == i % 5 &&
             keyPoints[(size_t)j].response == (float)i && detDists[(size_t)j] == prevDetDists[(size_t)i];
    }
    int tracked = 0;
    for (int i = 0; i < n; ++i) tracked += status[(size_t)i];
    std::printf("%s: %s (%d points, %d tracked, %d kept)\n", name, ok ? "ok" : "MISMATCH", n, tracked, k);
    return ok ? 0 : 1;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run_case("grey, dense rows", 1, false, 0, 0, 25.0, 3.0, 150);
    bad += run_case("colour, padded rows", 3, true, 0, 0, 4.0, 3.0, 150);
    bad += run_case("grey, padded rows, initial flow", 1, true, 1, 0, 25.0, 1.0, 65);
    bad += run_case("colour, minimal eigenvalue as the error", 3, false, 0, 1, 0.5, 3.0, 64);
    bad += run_case("no features", 1, false, 0, 0, 25.0, 3.0, 0);
    if (bad == 0) std::printf("all ok\n");
    return bad;
}
