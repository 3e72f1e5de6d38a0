// FrameMatcher::matchXYZLadder of the drop-in (putslam_dropin.h) against the loop it replaces (PUTSLAM.cpp:788-798): ten
// sequential ps_match_xyz + ps_ransac_rigid3d calls of the C ABI, try k with the radius / ratio of matcher.cpp:617-622 and the
// seed S + 0x51ED270B0B5 + frameCounter + (k - 1).  Scenes are made here (a small generator of its own): map features near the
// frame's keypoints, displaced by 0.15 m (a later try is taken), undisplaced (the first), 40 m away (no try reaches 0.1: the
// tenth).  Try 1 also equals FrameMatcher::matchXYZ.  Prints "ALL OK"; exit status 0 = every check passed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "putslam_dropin.h"
#include "putslam_hip.h"

static int fails = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);   \
            ++fails;                                                   \
        }                                                              \
    } while (0)

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rngState >> 33);
}
static double uni() { return (rnd() & 0xFFFFFF) / 16777216.0; }
static double gauss() { return (uni() + uni() + uni() + uni() - 2.0) * 1.7320508; } // (variance 1)

struct Scene {
    std::vector<putslam_hip::FrameMatcher::MapFeatureXYZ> mapF;
    std::vector<uint8_t> mapD, curD;
    std::vector<Eigen::Vector3f> curF;
    std::vector<int> oct;
    std::vector<double> det;
};

static void makeScene(Scene &s, int nmap, int ncur, double shift, double sigma)
{
    s.curD.resize((size_t)ncur * 32);
    s.mapD.resize((size_t)nmap * 32);
    for (int i = 0; i < ncur; ++i) {
        // (a sparse scene: a try whose sphere misses the true keypoints finds fewer chance candidates than RANSAC accepts)
        s.curF.push_back(Eigen::Vector3f((float)(uni() * 9 - 4.5), (float)(uni() * 9 - 4.5), (float)(uni() * 3 + 1.0)));
        for (int b = 0; b < 32; ++b) s.curD[(size_t)i * 32 + b] = (uint8_t)rnd();
        s.oct.push_back((int)(rnd() % 8));
        {
            const Eigen::Vector3f &q = s.curF.back();
            s.det.push_back(std::sqrt((double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2]) * (0.8 + 0.45 * uni()));
        }
    }
    for (int j = 0; j < nmap; ++j) {
        const int src = (int)(rnd() % (uint32_t)ncur);
        putslam_hip::FrameMatcher::MapFeatureXYZ f;
        f.id = (unsigned)j;
        f.position[0] = s.curF[(size_t)src].x() + sigma * gauss() + shift;
        f.position[1] = s.curF[(size_t)src].y() + sigma * gauss();
        f.position[2] = s.curF[(size_t)src].z() + sigma * gauss();
        for (int b = 0; b < 32; ++b) {
            uint8_t flip = 0;
            for (int k = 0; k < 8; ++k)
                if (uni() < 0.05) flip |= (uint8_t)(1u << k);
            s.mapD[(size_t)j * 32 + b] = s.curD[(size_t)src * 32 + b] ^ flip;
        }
        f.octave = std::min(7, std::max(0, s.oct[(size_t)src] + (int)(rnd() % 3) - 1));
        f.detDist = s.det[(size_t)src];
        s.mapF.push_back(f);
    }
    for (int j = 0; j < nmap; ++j) s.mapF[(size_t)j].descriptor = cv::Mat(1, 32, CV_8U, s.mapD.data() + (size_t)j * 32);
}

struct Try {
    double ratio = -1.0;
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    std::vector<cv::DMatch> inliers;
};

// the ten tries through the host-pointer C ABI, as the reference-side retry loop would run them
static std::vector<Try> sequential(PsContext *ctx, putslam_hip::FrameMatcher &m, Scene &s, uint64_t seed, int tries)
{
    const int nmap = (int)s.mapF.size(), ncur = (int)s.curF.size();
    std::vector<float> mapPos((size_t)nmap * 3);
    std::vector<int32_t> mapLvl((size_t)nmap), curLvl((size_t)ncur);
    for (int j = 0; j < nmap; ++j) {
        const double *p = s.mapF[(size_t)j].position;
        for (int c = 0; c < 3; ++c) mapPos[(size_t)j * 3 + c] = (float)p[c];
        mapLvl[(size_t)j] = ps_predicted_level(s.mapF[(size_t)j].octave, s.mapF[(size_t)j].detDist, std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
    }
    for (int i = 0; i < ncur; ++i) {
        const Eigen::Vector3f &p = s.curF[(size_t)i];
        const float nrm = std::sqrt(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2]));
        curLvl[(size_t)i] = ps_predicted_level(s.oct[(size_t)i], s.det[(size_t)i], (double)nrm);
    }
    RANSAC::parameters rp = m.matcherParameters.RANSACParams;
    rp.errorVersion = rp.errorVersionMap;
    std::vector<Try> out;
    for (int k = 1; k <= tries; ++k) {
        double radius = m.matcherParameters.OpenCVParams.matchingXYZSphereRadius;
        double ratio = m.matcherParameters.OpenCVParams.matchingXYZacceptRatioOfBestMatch;
        if (k > 1) {
            radius += 0.02 * (k - 1);
            ratio = std::max(0.1, ratio - 0.05 * (k - 1));
        }
        std::vector<cv::DMatch> matches((size_t)nmap * (size_t)ncur + 16);
        int n = 0;
        int rc = ps_match_xyz(ctx, mapPos.data(), s.mapD.data(), 32, mapLvl.data(), nmap, reinterpret_cast<const float *>(s.curF.data()),
                              s.curD.data(), 32, curLvl.data(), ncur, radius, ratio, reinterpret_cast<PsDMatch *>(matches.data()),
                              (int)matches.size(), &n);
        CHECK(rc == PS_OK);
        matches.resize((size_t)n);
        Try t;
        if (n > 0) {
            RANSAC ransac(rp, m.matcherParameters.cameraMatrixMat);
            ransac.setSampleSeed(seed + (uint64_t)(k - 1));
            std::vector<Eigen::Vector3f> prev((size_t)nmap);
            std::memcpy((void *)prev.data(), mapPos.data(), (size_t)nmap * 12);
            t.pose = ransac.estimateTransformation(prev, s.curF, matches, t.inliers);
            t.ratio = RANSAC::pointInlierRatio(t.inliers, matches);
        }
        out.push_back(t);
    }
    return out;
}

static bool sameMatches(const std::vector<cv::DMatch> &a, const std::vector<cv::DMatch> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(cv::DMatch)) == 0);
}

int main()
{
    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("no device\n");
        return 2;
    }
    putslam_hip::FrameMatcher *matcher = putslam_hip::createFrameMatcher();
    const uint64_t S = 20261016;
    matcher->setSampleSeed(S);
    matcher->matcherParameters.RANSACParams.errorVersionMap = 0;
    const uint64_t mapSeed = S + 0x51ED270B0B5ull; // (frameCounter is 0: no frame has been matched)
    const struct {
        double shift, sigma;
        int expect; // 1: a later try, 0: the first, -1: none reaches 0.1
    } cases[] = {{0.15, 0.005, 1}, {0.0, 0.02, 0}, {40.0, 0.02, -1}};
    for (const auto &c : cases) {
        Scene s;
        makeScene(s, 800, 900, c.shift, c.sigma);
        cv::Mat curDesc(900, 32, CV_8U, s.curD.data());
        std::vector<Try> seq = sequential(ctx, *matcher, s, mapSeed, 10);
        int pick = 9;
        for (int k = 0; k < 10; ++k)
            if (seq[(size_t)k].ratio >= 0.1) {
                pick = k;
                break;
            }
        if (c.expect == 1) CHECK(pick > 0);
        if (c.expect == 0) CHECK(pick == 0);
        if (c.expect == -1) CHECK(pick == 9 && seq[9].ratio < 0.1);
        Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inl;
        int used = 0;
        const double r = matcher->matchXYZLadder(s.mapF, curDesc, s.curF, s.oct, s.det, T, inl, 10, 0.1, &used);
        std::printf("shift %.2f: sequential picks try %d (ratio %.4f), ladder try %d (ratio %.4f, %zu inliers)\n", c.shift, pick + 1,
                    seq[(size_t)pick].ratio, used, r, inl.size());
        CHECK(used == pick + 1);
        CHECK(r == seq[(size_t)pick].ratio);
        if (seq[(size_t)pick].ratio >= 0.0) {
            CHECK(std::memcmp(T.data(), seq[(size_t)pick].pose.data(), 64) == 0);
            CHECK(sameMatches(inl, seq[(size_t)pick].inliers));
        }
        // fewer tries: the ladder of three ends where the loop of three would
        int pick3 = 2;
        for (int k = 0; k < 3; ++k)
            if (seq[(size_t)k].ratio >= 0.1) {
                pick3 = k;
                break;
            }
        Eigen::Matrix4f T3 = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inl3;
        const double r3 = matcher->matchXYZLadder(s.mapF, curDesc, s.curF, s.oct, s.det, T3, inl3, 3, 0.1, &used);
        CHECK(used == pick3 + 1 && r3 == seq[(size_t)pick3].ratio);
        // try 1 is FrameMatcher::matchXYZ
        Eigen::Matrix4f T1 = Eigen::Matrix4f::Identity(), Tx = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inl1, inlx;
        const double r1 = matcher->matchXYZLadder(s.mapF, curDesc, s.curF, s.oct, s.det, T1, inl1, 1, 0.1, &used);
        const double rx = matcher->matchXYZ(s.mapF, curDesc, s.curF, s.oct, s.det, Tx, inlx, 1);
        CHECK(used == 1 && r1 == rx && std::memcmp(T1.data(), Tx.data(), 64) == 0 && sameMatches(inl1, inlx));
    }
    // a crowded scene: every keypoint is a candidate of every feature with equal descriptors, 20 x 300 matches a try -- far more than
    // the rows the ladder starts with (4 x features + 16): it runs again with the reported capacity and still equals the loop
    {
        Scene s;
        makeScene(s, 20, 300, 0.0, 0.01);
        for (size_t i = 0; i < s.curF.size(); ++i) {
            s.curF[i] = Eigen::Vector3f((float)(0.02 * uni()), (float)(0.02 * uni()), (float)(2.0 + 0.02 * uni()));
            s.oct[i] = 3;
            s.det[i] = 2.0;
        }
        std::fill(s.curD.begin(), s.curD.end(), (uint8_t)0x3C);
        std::fill(s.mapD.begin(), s.mapD.end(), (uint8_t)0x3C);
        for (size_t j = 0; j < s.mapF.size(); ++j) {
            const Eigen::Vector3f &q = s.curF[j];
            s.mapF[j].position[0] = q[0] + 0.001;
            s.mapF[j].position[1] = q[1];
            s.mapF[j].position[2] = q[2];
            s.mapF[j].octave = 3;
            s.mapF[j].detDist = 2.0;
        }
        cv::Mat curDesc(300, 32, CV_8U, s.curD.data());
        std::vector<Try> seq = sequential(ctx, *matcher, s, mapSeed, 4);
        int pick = 3;
        for (int k = 0; k < 4; ++k)
            if (seq[(size_t)k].ratio >= 0.1) {
                pick = k;
                break;
            }
        Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inl;
        int used = 0;
        const double r = matcher->matchXYZLadder(s.mapF, curDesc, s.curF, s.oct, s.det, T, inl, 4, 0.1, &used);
        std::printf("crowded: sequential picks try %d (ratio %.4f, %zu inliers), ladder try %d (ratio %.4f, %zu inliers)\n", pick + 1,
                    seq[(size_t)pick].ratio, seq[(size_t)pick].inliers.size(), used, r, inl.size());
        CHECK(seq[0].ratio >= 0.0); // (there were matches: 6000 of them)
        CHECK(used == pick + 1 && r == seq[(size_t)pick].ratio);
        CHECK(std::memcmp(T.data(), seq[(size_t)pick].pose.data(), 64) == 0 && sameMatches(inl, seq[(size_t)pick].inliers));
    }
    // nothing to match: -1, the last try's number
    {
        Scene s;
        makeScene(s, 10, 20, 0.0, 0.01);
        cv::Mat curDesc(20, 32, CV_8U, s.curD.data());
        std::vector<putslam_hip::FrameMatcher::MapFeatureXYZ> none;
        Eigen::Matrix4f T;
        std::vector<cv::DMatch> inl;
        int used = 0;
        CHECK(matcher->matchXYZLadder(none, curDesc, s.curF, s.oct, s.det, T, inl, 10, 0.1, &used) == -1.0 && used == 10);
    }
    ps_context_destroy(ctx);
    if (fails == 0) std::printf("ALL OK\n");
    return fails ? 1 : 0;
}
