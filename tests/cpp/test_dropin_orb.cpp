// FrameMatcherHIP::describeFeatures (MatcherOpenCV::describeFeatures, matcherOpenCV.cpp:183-195, descriptor "ORB") on cv::Mat-shaped
// images -- CV_8UC3 and CV_8UC1, a region of a parent Mat with its step included -- against the C ABI (ps_describe_features on the
// same bytes) and against the specification restated in C++ (orb_restated.h): the rows, and the key points that replace the caller's
// list, all six fields of each.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orb_restated.h"
#include "putslam_dropin.h"
#include "putslam_hip.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
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
        const int x0 = below(m.cols), y0 = below(m.rows), w = 2 + below(m.cols / 4), h = 2 + below(m.rows / 4);
        unsigned char col[3] = {(unsigned char)below(256), (unsigned char)below(256), (unsigned char)below(256)};
        for (int y = y0; y < y0 + h && y < m.rows; ++y)
            for (int x = x0; x < x0 + w && x < m.cols; ++x)
                for (int c = 0; c < cn; ++c) m.data[(size_t)y * m.step + (size_t)x * cn + c] = col[c];
    }
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols * cn; ++x) {
            unsigned char &v = m.data[(size_t)y * m.step + x];
            const int n = (int)v + below(17) - 8;
            v = (unsigned char)(n < 0 ? 0 : (n > 255 ? 255 : n));
        }
}

bool same_keypoint(const cv::KeyPoint &a, const cv::KeyPoint &b)
{
    return std::memcmp(&a.pt, &b.pt, 8) == 0 && a.size == b.size && std::memcmp(&a.angle, &b.angle, 4) == 0 && a.response == b.response &&
           a.octave == b.octave && a.class_id == b.class_id;
}

int run_case(const char *name, int cn, int padX, int padY, int n, bool unsorted)
{
    const int rows = 90, cols = 125;
    const size_t step = (size_t)cols * cn + 2 * (size_t)padX;
    std::vector<unsigned char> parent(step * (size_t)(rows + 2 * padY), 0xEE);
    cv::Mat img(rows, cols, cn == 3 ? CV_8UC3 : CV_8UC1, parent.data() + (size_t)padY * step + padX, step);
    scene(img, cn, 70);

    // key points over the whole image (some inside the 31-pixel border: dropped), every octave, two out of range
    std::vector<cv::KeyPoint> in((size_t)n);
    for (int i = 0; i < n; ++i) {
        cv::KeyPoint &kp = in[(size_t)i];
        kp.pt = cv::Point2f((float)below(cols * 4) / 4.f, (float)below(rows * 4) / 4.f);
        kp.size = 7.f + (float)i;
        kp.angle = i % 7 == 0 ? -1.f : (float)below(360 * 8) / 8.f;
        kp.response = (float)below(200);
        kp.octave = unsorted ? below(10) - 1 : 0;
        kp.class_id = i;
    }
    putslam_hip::FrameMatcherHIP matcher;
    bool ok = matcher.matcherParameters.OpenCVParams.descriptor == "ORB"; // the shipped value
    std::vector<cv::KeyPoint> got = in, free_ = in;
    const cv::Mat d1 = matcher.describeFeatures(img, got);
    const cv::Mat d2 = putslam_hip::describeFeaturesORB(matcher.matcherParameters, img, free_);

    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("%s: no context\n", name);
        return 1;
    }
    std::vector<float> xy((size_t)n * 2 + 2), angle((size_t)n + 1);
    std::vector<int32_t> octave((size_t)n + 1), kept((size_t)n + 1), wkept((size_t)n + 1);
    for (int i = 0; i < n; ++i) {
        xy[(size_t)2 * i] = in[(size_t)i].pt.x;
        xy[(size_t)2 * i + 1] = in[(size_t)i].pt.y;
        angle[(size_t)i] = in[(size_t)i].angle;
        octave[(size_t)i] = in[(size_t)i].octave;
    }
    std::vector<uint8_t> desc((size_t)n * 32 + 32), want((size_t)n * 32 + 32);
    const PsOrbParams prm = {1.2f, 8, {0, 0}};
    int k = -1;
    const int rc = ps_describe_features(ctx, img.data, rows, cols, cn, step, &prm, nullptr, xy.data(), angle.data(), octave.data(), n, desc.data(),
                                        kept.data(), &k);
    if (rc != PS_OK) {
        std::printf("%s: C ABI failed: %s\n", name, ps_last_error(ctx));
        ps_context_destroy(ctx);
        return 1;
    }
    ps_context_destroy(ctx);
    const int wk = orb_restated::describe(img.data, rows, cols, cn, step, 1.2f, 8, nullptr, xy.data(), angle.data(), octave.data(), n, want.data(),
                                          wkept.data());
    ok = ok && k == wk && (int)got.size() == k && (int)free_.size() == k && (k == 0 ? d1.empty() && d2.empty() : d1.rows == k && d1.cols == 32 &&
         d1.type() == CV_8U && d2.rows == k && d2.cols == 32);
    for (int j = 0; ok && j < k; ++j) {
        ok = kept[(size_t)j] == wkept[(size_t)j] && std::memcmp(&desc[(size_t)j * 32], &want[(size_t)j * 32], 32) == 0 &&
             std::memcmp(d1.data + (size_t)j * d1.step, &want[(size_t)j * 32], 32) == 0 &&
             std::memcmp(d2.data + (size_t)j * d2.step, &want[(size_t)j * 32], 32) == 0 && same_keypoint(got[(size_t)j], in[(size_t)kept[(size_t)j]]) &&
             same_keypoint(free_[(size_t)j], got[(size_t)j]);
    }
    std::printf("%s: %s (%d of %d key points described)\n", name, ok ? "ok" : "MISMATCH", k, n);
    return ok ? 0 : 1;
}

// a descriptor other than ORB is refused loudly: no rows, the list cleared, no CPU fallback
int run_other_descriptor()
{
    cv::Mat img(90, 125, CV_8UC3);
    scene(img, 3, 10);
    putslam_hip::FrameMatcherHIP matcher;
    std::vector<cv::KeyPoint> kps(3);
    for (auto &kp : kps) kp.pt = cv::Point2f(50.f, 45.f);
    std::vector<cv::KeyPoint> a = kps, b = kps, c = kps, none;
    const bool shipped = matcher.describeFeatures(img, a).rows == 3 && a.size() == 3; // "ORB" as shipped
    matcher.matcherParameters.OpenCVParams.descriptor = "SURF";
    const bool surf = matcher.describeFeatures(img, b).empty() && b.empty();
    matcher.matcherParameters.OpenCVParams.descriptor = "ORB";
    cv::Mat wrong(90, 125, CV_32F);
    const bool type = matcher.describeFeatures(wrong, c).empty() && c.empty() && matcher.describeFeatures(img, none).empty();
    std::printf("other descriptors and types: %s\n", shipped && surf && type ? "ok" : "MISMATCH");
    return shipped && surf && type ? 0 : 1;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run_case("colour region with a step, octave 0", 3, 7, 2, 300, false);
    bad += run_case("colour region with a step, unsorted octaves -1 .. 8", 3, 5, 1, 257, true);
    bad += run_case("grey, dense rows, unsorted octaves", 1, 0, 0, 64, true);
    bad += run_case("grey region with a step, one key point", 1, 3, 3, 1, false);
    bad += run_other_descriptor();
    if (bad == 0) std::printf("all ok\n");
    return bad;
}
