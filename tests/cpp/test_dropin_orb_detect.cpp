// FrameMatcherHIP::detectFeatures (MatcherOpenCV::detectFeatures, matcherOpenCV.cpp:118-180) with the SHIPPED detector "ORB" on
// cv::Mat-shaped images -- CV_8UC3 and CV_8UC1, a region of a parent Mat with its step included -- against the C ABI
// (ps_detect_features_orb on the same bytes) and against the specification restated in C++ (orb_detect_restated.h).  All six
// cv::KeyPoint fields are checked.  Another detector than "ORB" and "FAST" is refused, not run on the CPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orb_detect_restated.h"
#include "putslam_dropin.h"
#include "putslam_hip.h"

namespace {

uint64_t g_state = 0x2545F4914F6CDD1Dull;
int below(int n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((g_state >> 33) % (uint64_t)n);
}

// rectangles of random colour on a grey ground, a little noise on top
void scene(cv::Mat &m, int cn, int rects)
{
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols * cn; ++x) m.data[(size_t)y * m.step + x] = 100;
    for (int r = 0; r < rects; ++r) {
        const int x0 = below(m.cols), y0 = below(m.rows), w = 2 + below(m.cols / 5), h = 2 + below(m.rows / 5);
        unsigned char col[3] = {(unsigned char)below(256), (unsigned char)below(256), (unsigned char)below(256)};
        for (int y = y0; y < y0 + h && y < m.rows; ++y)
            for (int x = x0; x < x0 + w && x < m.cols; ++x)
                for (int c = 0; c < cn; ++c) m.data[(size_t)y * m.step + (size_t)x * cn + c] = col[c];
    }
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols * cn; ++x) {
            unsigned char &v = m.data[(size_t)y * m.step + x];
            const int n = (int)v + below(9) - 4;
            v = (unsigned char)(n < 0 ? 0 : (n > 255 ? 255 : n));
        }
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int run_case(const char *name, int rows, int cols, int cn, int padX, int padY, int gridRows, int gridCols, int maxFeatures, int minFound)
{
    // the image is a region of a parent: padX bytes left of every row and after it, padY rows above
    const size_t step = (size_t)cols * cn + 2 * (size_t)padX;
    std::vector<unsigned char> parent(step * (size_t)(rows + 2 * padY), 0xEE);
    cv::Mat img(rows, cols, cn == 3 ? CV_8UC3 : CV_8UC1, parent.data() + (size_t)padY * step + padX, step);
    scene(img, cn, 160);

    putslam_hip::FrameMatcherHIP matcher;
    auto &cvp = matcher.matcherParameters.OpenCVParams;
    bool ok = cvp.detector == "ORB" && cvp.gridRows == 1 && cvp.gridCols == 1 && cvp.maximalTrackedFeatures == 500; // the shipped values
    cvp.gridRows = gridRows;
    cvp.gridCols = gridCols;
    cvp.maximalTrackedFeatures = maxFeatures;
    const std::vector<cv::KeyPoint> got = matcher.detectFeatures(img);
    const std::vector<cv::KeyPoint> free_ = putslam_hip::detectFeaturesORB(matcher.matcherParameters, img);

    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("%s: no context\n", name);
        return 1;
    }
    PsOrbDetectParams prm = {500, 1.2f, 8, 20, gridRows, gridCols, maxFeatures, 0};
    const size_t room = (size_t)maxFeatures + 1;
    std::vector<float> xy(room * 2), resp(room), ang(room);
    std::vector<int32_t> oct(room);
    int n = -1;
    const int rc = ps_detect_features_orb(ctx, img.data, rows, cols, cn, step, &prm, xy.data(), resp.data(), ang.data(), oct.data(), maxFeatures, &n);
    if (rc != PS_OK) {
        std::printf("%s: C ABI failed: %s\n", name, ps_last_error(ctx));
        ps_context_destroy(ctx);
        return 1;
    }
    ps_context_destroy(ctx);
    orb_detect_restated::Params rp;
    rp.gridRows = gridRows;
    rp.gridCols = gridCols;
    rp.maximalTrackedFeatures = maxFeatures;
    const std::vector<orb_detect_restated::Kp> want = orb_detect_restated::detect(img.data, rows, cols, cn, step, rp);
    ok = ok && (int)got.size() == n && (int)want.size() == n && free_.size() == got.size() && n >= minFound;
    int levels = 0;
    for (int j = 0; ok && j < n; ++j) {
        const cv::KeyPoint &kp = got[(size_t)j], &fr = free_[(size_t)j];
        const orb_detect_restated::Kp &w = want[(size_t)j];
        ok = same_bits(kp.pt.x, xy[(size_t)2 * j]) && same_bits(kp.pt.y, xy[(size_t)2 * j + 1]) && same_bits(kp.response, resp[(size_t)j]) &&
             same_bits(kp.angle, ang[(size_t)j]) && kp.octave == oct[(size_t)j] && same_bits(kp.pt.x, w.x) && same_bits(kp.pt.y, w.y) &&
             same_bits(kp.size, w.size) && same_bits(kp.angle, w.angle) && same_bits(kp.response, w.response) && kp.octave == w.octave &&
             kp.class_id == -1 && same_bits(fr.pt.x, kp.pt.x) && same_bits(fr.pt.y, kp.pt.y) && same_bits(fr.size, kp.size) &&
             same_bits(fr.angle, kp.angle) && same_bits(fr.response, kp.response) && fr.octave == kp.octave && fr.class_id == -1;
        levels |= 1 << kp.octave;
    }
    std::printf("%s: %s (%d key points, level mask %d)\n", name, ok ? "ok" : "MISMATCH", n, levels);
    return ok ? 0 : 1;
}

// the shipped detector on an image too small for its border gives nothing and says nothing; SURF is refused loudly
int run_other_detector()
{
    cv::Mat img(40, 40, CV_8UC3);
    scene(img, 3, 10);
    putslam_hip::FrameMatcherHIP matcher;
    const bool shipped = matcher.detectFeatures(img).empty(); // "ORB" as shipped: every level is dead by the border rule
    matcher.matcherParameters.OpenCVParams.detector = "SURF";
    const bool surf = matcher.detectFeatures(img).empty();
    cv::Mat wrong(200, 200, CV_32F);
    matcher.matcherParameters.OpenCVParams.detector = "ORB";
    const bool type = matcher.detectFeatures(wrong).empty();
    std::printf("other detectors and types: %s\n", shipped && surf && type ? "ok" : "MISMATCH");
    return shipped && surf && type ? 0 : 1;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run_case("colour region with a step, grid 1 x 1, the shipped defaults", 150, 200, 3, 7, 2, 1, 1, 500, 40);
    bad += run_case("grey region with a step, grid 2 x 2", 200, 260, 1, 3, 3, 2, 2, 500, 40);
    bad += run_case("colour, dense rows, grid 2 x 2, cut in every ROI and in the join", 200, 260, 3, 0, 0, 2, 2, 12, 12);
    bad += run_case("grey, dense rows, one key point", 150, 200, 1, 0, 0, 1, 1, 1, 1);
    bad += run_case("maximalTrackedFeatures 0", 150, 200, 3, 0, 0, 1, 1, 0, 0);
    bad += run_other_detector();
    if (bad == 0) std::printf("all ok\n");
    return bad;
}
