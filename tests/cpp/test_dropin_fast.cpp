// FrameMatcherHIP::detectFeatures (MatcherOpenCV::detectFeatures, matcherOpenCV.cpp:118-180, detector "FAST") on cv::Mat-shaped
// images -- CV_8UC3 and CV_8UC1, a region of a parent Mat with its step included -- against the C ABI (ps_detect_features on the same
// bytes) and against the grid loop restated here: grey conversion, FAST-9/16 by its definition in every ROI, suppression,
// std::stable_sort by response in the ROI and over the joined list, the two cuts.  All six cv::KeyPoint fields are checked.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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
            const int n = (int)v + below(9) - 4;
            v = (unsigned char)(n < 0 ? 0 : (n > 255 ? 255 : n));
        }
}

struct Kp {
    float x, y, response;
};

const int kRing[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3}, {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

// FAST-9/16 with suppression on one ROI of the grey image, by the definition: arcs of nine tried one by one
std::vector<Kp> fast_roi(const std::vector<uint8_t> &gray, int stride, int x0, int y0, int w, int h, int t)
{
    std::vector<int> score((size_t)w * h, 0);
    std::vector<uint8_t> corner((size_t)w * h, 0);
    for (int y = 3; y < h - 3; ++y)
        for (int x = 3; x < w - 3; ++x) {
            int d[16];
            const int v = gray[(size_t)(y0 + y) * stride + x0 + x];
            for (int k = 0; k < 16; ++k) d[k] = v - (int)gray[(size_t)(y0 + y + kRing[k][1]) * stride + x0 + x + kRing[k][0]];
            int D = -1000, B = -1000;
            for (int s = 0; s < 16; ++s) {
                int lo = 1000, hi = -1000;
                for (int j = 0; j < 9; ++j) {
                    lo = std::min(lo, d[(s + j) & 15]);
                    hi = std::max(hi, d[(s + j) & 15]);
                }
                D = std::max(D, lo);
                B = std::max(B, -hi);
            }
            if (D > t || B > t) {
                corner[(size_t)y * w + x] = 1;
                score[(size_t)y * w + x] = std::max(t, std::max(D, B)) - 1;
            }
        }
    std::vector<Kp> out;
    for (int y = 3; y < h - 3; ++y)
        for (int x = 3; x < w - 3; ++x) {
            if (!corner[(size_t)y * w + x]) continue;
            const int s = score[(size_t)y * w + x];
            bool top = true;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if ((dx || dy) && !(s > score[(size_t)(y + dy) * w + x + dx])) top = false;
            if (top) out.push_back(Kp{(float)x, (float)y, (float)s});
        }
    return out;
}

bool by_response(const Kp &a, const Kp &b) { return a.response > b.response; } // compare_response, matcherOpenCV.h:84-87

// the grid loop of matcherOpenCV.cpp:118-180 with both orderings stable
std::vector<Kp> detect_restated(const cv::Mat &img, int gridRows, int gridCols, int maxFeatures)
{
    const int W = img.cols, H = img.rows, cn = img.channels();
    std::vector<uint8_t> gray((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const unsigned char *p = img.data + (size_t)y * img.step + (size_t)x * cn;
            gray[(size_t)y * W + x] = cn == 1 ? p[0] : (uint8_t)((p[0] * 4899 + p[1] * 9617 + p[2] * 1868 + 8192) >> 14);
        }
    const int maxInRoi = maxFeatures * 3 / (gridCols * gridRows);
    std::vector<Kp> raw;
    for (int k = 0; k < gridCols; ++k)
        for (int i = 0; i < gridRows; ++i) {
            const int x0 = k * W / gridCols, y0 = i * H / gridRows;
            std::vector<Kp> in = fast_roi(gray, W, x0, y0, W / gridCols, H / gridRows, 10);
            std::stable_sort(in.begin(), in.end(), by_response);
            for (size_t j = 0; j < in.size() && (int)j < maxInRoi; ++j) {
                in[j].x += (float)x0;
                in[j].y += (float)y0;
                raw.push_back(in[j]);
            }
        }
    std::stable_sort(raw.begin(), raw.end(), by_response);
    if ((int)raw.size() > maxFeatures) raw.resize((size_t)maxFeatures);
    return raw;
}

int run_case(const char *name, int cn, int padX, int padY, int gridRows, int gridCols, int maxFeatures, int minFound)
{
    const int rows = 90, cols = 125;
    // the image is a region of a parent: padX bytes left of every row and after it, padY rows above
    const size_t step = (size_t)cols * cn + 2 * (size_t)padX;
    std::vector<unsigned char> parent(step * (size_t)(rows + 2 * padY), 0xEE);
    cv::Mat img(rows, cols, cn == 3 ? CV_8UC3 : CV_8UC1, parent.data() + (size_t)padY * step + padX, step);
    scene(img, cn, 70);

    putslam_hip::FrameMatcherHIP matcher;
    auto &cvp = matcher.matcherParameters.OpenCVParams;
    bool ok = cvp.detector == "ORB" && cvp.gridRows == 1 && cvp.gridCols == 1 && cvp.maximalTrackedFeatures == 500; // the shipped values
    cvp.detector = "FAST";
    cvp.gridRows = gridRows;
    cvp.gridCols = gridCols;
    cvp.maximalTrackedFeatures = maxFeatures;
    const std::vector<cv::KeyPoint> got = matcher.detectFeatures(img);
    const std::vector<cv::KeyPoint> free_ = putslam_hip::detectFeaturesFAST(matcher.matcherParameters, img);

    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("%s: no context\n", name);
        return 1;
    }
    PsDetectParams prm = {10, 1, gridRows, gridCols, maxFeatures, 0};
    std::vector<float> xy((size_t)maxFeatures * 2 + 2), resp((size_t)maxFeatures + 1);
    int n = -1;
    const int rc = ps_detect_features(ctx, img.data, rows, cols, cn, step, &prm, xy.data(), resp.data(), maxFeatures, &n);
    if (rc != PS_OK) {
        std::printf("%s: C ABI failed: %s\n", name, ps_last_error(ctx));
        ps_context_destroy(ctx);
        return 1;
    }
    ps_context_destroy(ctx);
    const std::vector<Kp> want = detect_restated(img, gridRows, gridCols, maxFeatures);
    ok = ok && (int)got.size() == n && (int)want.size() == n && free_.size() == got.size() && n >= minFound;
    for (int j = 0; ok && j < n; ++j) {
        const cv::KeyPoint &kp = got[(size_t)j];
        ok = std::memcmp(&kp.pt, &xy[(size_t)2 * j], 8) == 0 && std::memcmp(&kp.response, &resp[(size_t)j], 4) == 0 && kp.pt.x == want[(size_t)j].x &&
             kp.pt.y == want[(size_t)j].y && kp.response == want[(size_t)j].response && kp.size == 7.f && kp.angle == -1.f && kp.octave == 0 &&
             kp.class_id == -1 && std::memcmp(&free_[(size_t)j].pt, &kp.pt, 8) == 0 && free_[(size_t)j].response == kp.response &&
             free_[(size_t)j].size == 7.f && free_[(size_t)j].angle == -1.f && free_[(size_t)j].octave == 0 && free_[(size_t)j].class_id == -1;
    }
    int ties = 0;
    for (int j = 1; j < n; ++j) ties += got[(size_t)j].response == got[(size_t)j - 1].response;
    std::printf("%s: %s (%d key points, %d next to an equal response)\n", name, ok ? "ok" : "MISMATCH", n, ties);
    return ok ? 0 : 1;
}

// a detector other than FAST is refused loudly: no key points, no CPU fallback
int run_other_detector()
{
    cv::Mat img(40, 40, CV_8UC3);
    scene(img, 3, 10);
    putslam_hip::FrameMatcherHIP matcher;
    const bool shipped = matcher.detectFeatures(img).empty(); // "ORB" as shipped
    matcher.matcherParameters.OpenCVParams.detector = "SURF";
    const bool surf = matcher.detectFeatures(img).empty();
    cv::Mat wrong(40, 40, CV_32F);
    matcher.matcherParameters.OpenCVParams.detector = "FAST";
    const bool type = matcher.detectFeatures(wrong).empty() && !matcher.detectFeatures(img).empty();
    std::printf("other detectors and types: %s\n", shipped && surf && type ? "ok" : "MISMATCH");
    return shipped && surf && type ? 0 : 1;
}

} // namespace

int main()
{
    int bad = 0;
    bad += run_case("colour region with a step, grid 1 x 1", 3, 7, 2, 1, 1, 500, 60);
    bad += run_case("colour region with a step, grid 3 x 2, cut in every ROI", 3, 5, 1, 2, 3, 40, 40);
    bad += run_case("grey, dense rows, grid 4 x 4", 1, 0, 0, 4, 4, 500, 30);
    bad += run_case("grey region with a step, one key point", 1, 3, 3, 1, 1, 1, 1);
    bad += run_case("maximalTrackedFeatures 0", 3, 0, 0, 1, 1, 0, 0);
    bad += run_other_detector();
    if (bad == 0) std::printf("all ok\n");
    return bad;
}
