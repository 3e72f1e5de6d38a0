// FrameMatcher::matchXYZ / matchXYZLadder of the drop-in (putslam_dropin.h) on CV_32F descriptor Mats -- the NORM_L2 value of
// matcher.cpp:625-628 -- against the loop they replace through the C ABI: ps_match_xyz_l2_f32 + the drop-in's RANSAC per try, with
// the radius / ratio of matcher.cpp:617-622 and the seed S + 0x51ED270B0B5 + frameCounter + (k - 1).  A CV_8U call before and after
// the float calls is unchanged; mixed types and a map row of another width return -1.0.  With a path as argument the scene and
// the inliers are written there (tests/test_gpu_dropin_map_l2.py holds them to the Python restatement).
// Prints one "<name>: ok" line per part and "all ok"; exit status 0 = every check passed.
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

typedef putslam_hip::FrameMatcher::MapFeatureXYZ MapFeature;

struct Scene {
    int D = 0;
    std::vector<MapFeature> mapF;
    std::vector<float> mapD, curD; // float rows (D wide)
    std::vector<uint8_t> mapB, curB; // binary rows of the same scene (32 bytes)
    std::vector<Eigen::Vector3f> curF;
    std::vector<int> oct;
    std::vector<double> det;
};

static void unitRow(float *row, int D, const float *src, double noise)
{
    std::vector<double> x((size_t)D);
    double n2 = 0.0;
    for (int k = 0; k < D; ++k) {
        x[(size_t)k] = (src ? (double)src[k] : 0.0) + noise * gauss();
        n2 += x[(size_t)k] * x[(size_t)k];
    }
    const double inv = 1.0 / std::sqrt(n2);
    for (int k = 0; k < D; ++k) row[k] = (float)(x[(size_t)k] * inv);
}

static void makeScene(Scene &s, int D, int nmap, int ncur, double shift, double sigma)
{
    s.D = D;
    s.curD.resize((size_t)ncur * D);
    s.mapD.resize((size_t)nmap * D);
    s.curB.resize((size_t)ncur * 32);
    s.mapB.resize((size_t)nmap * 32);
    for (int i = 0; i < ncur; ++i) {
        s.curF.push_back(Eigen::Vector3f((float)(uni() * 9 - 4.5), (float)(uni() * 9 - 4.5), (float)(uni() * 3 + 1.0)));
        unitRow(&s.curD[(size_t)i * D], D, nullptr, 1.0);
        for (int b = 0; b < 32; ++b) s.curB[(size_t)i * 32 + b] = (uint8_t)rnd();
        s.oct.push_back((int)(rnd() % 8));
        const Eigen::Vector3f &q = s.curF.back();
        s.det.push_back(std::sqrt((double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2]) * (0.8 + 0.45 * uni()));
    }
    for (int j = 0; j < nmap; ++j) {
        const int src = (int)(rnd() % (uint32_t)ncur);
        MapFeature f;
        f.id = (unsigned)j;
        f.position[0] = s.curF[(size_t)src].x() + sigma * gauss() + shift;
        f.position[1] = s.curF[(size_t)src].y() + sigma * gauss();
        f.position[2] = s.curF[(size_t)src].z() + sigma * gauss();
        unitRow(&s.mapD[(size_t)j * D], D, &s.curD[(size_t)src * D], 0.08);
        for (int b = 0; b < 32; ++b) s.mapB[(size_t)j * 32 + b] = s.curB[(size_t)src * 32 + b] ^ (uint8_t)(uni() < 0.3 ? 1u << (rnd() % 8) : 0u);
        f.octave = std::min(7, std::max(0, s.oct[(size_t)src] + (int)(rnd() % 3) - 1));
        f.detDist = s.det[(size_t)src];
        s.mapF.push_back(f);
    }
}

static void useFloatRows(Scene &s)
{
    for (size_t j = 0; j < s.mapF.size(); ++j) s.mapF[j].descriptor = cv::Mat(1, s.D, CV_32F, s.mapD.data() + j * (size_t)s.D);
}
static void useBinaryRows(Scene &s)
{
    for (size_t j = 0; j < s.mapF.size(); ++j) s.mapF[j].descriptor = cv::Mat(1, 32, CV_8U, s.mapB.data() + j * 32);
}

struct Try {
    double ratio = -1.0, radius = 0.0, accept = 0.0;
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    std::vector<cv::DMatch> inliers;
};

struct Levels {
    std::vector<float> mapPos;
    std::vector<int32_t> mapLvl, curLvl;
};

static Levels levelsOf(const Scene &s)
{
    Levels l;
    const int nmap = (int)s.mapF.size(), ncur = (int)s.curF.size();
    l.mapPos.resize((size_t)nmap * 3);
    l.mapLvl.resize((size_t)nmap);
    l.curLvl.resize((size_t)ncur);
    for (int j = 0; j < nmap; ++j) {
        const double *p = s.mapF[(size_t)j].position;
        for (int c = 0; c < 3; ++c) l.mapPos[(size_t)j * 3 + c] = (float)p[c];
        l.mapLvl[(size_t)j] = ps_predicted_level(s.mapF[(size_t)j].octave, s.mapF[(size_t)j].detDist, std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
    }
    for (int i = 0; i < ncur; ++i) {
        const Eigen::Vector3f &p = s.curF[(size_t)i];
        const float nrm = std::sqrt(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2]));
        l.curLvl[(size_t)i] = ps_predicted_level(s.oct[(size_t)i], s.det[(size_t)i], (double)nrm);
    }
    return l;
}

// the tries through the host-pointer C ABI, as the reference-side retry loop would run them
static std::vector<Try> sequential(PsContext *ctx, putslam_hip::FrameMatcher &m, Scene &s, const Levels &l, uint64_t seed, int tries)
{
    const int nmap = (int)s.mapF.size(), ncur = (int)s.curF.size();
    RANSAC::parameters rp = m.matcherParameters.RANSACParams;
    rp.errorVersion = rp.errorVersionMap;
    std::vector<Try> out;
    for (int k = 1; k <= tries; ++k) {
        Try t;
        t.radius = m.matcherParameters.OpenCVParams.matchingXYZSphereRadius;
        t.accept = m.matcherParameters.OpenCVParams.matchingXYZacceptRatioOfBestMatch;
        if (k > 1) {
            t.radius += 0.02 * (k - 1);
            t.accept = std::max(0.1, t.accept - 0.05 * (k - 1));
        }
        std::vector<cv::DMatch> matches((size_t)16 * nmap + 16);
        int n = 0;
        const int rc = ps_match_xyz_l2_f32(ctx, l.mapPos.data(), s.mapD.data(), (size_t)s.D * 4, l.mapLvl.data(), nmap,
                                           reinterpret_cast<const float *>(s.curF.data()), s.curD.data(), (size_t)s.D * 4, l.curLvl.data(), ncur,
                                           s.D, t.radius, t.accept, reinterpret_cast<PsDMatch *>(matches.data()), (int)matches.size(), &n);
        CHECK(rc == PS_OK);
        matches.resize((size_t)n);
        if (n > 0) {
            RANSAC ransac(rp, m.matcherParameters.cameraMatrixMat);
            ransac.setSampleSeed(seed + (uint64_t)(k - 1));
            std::vector<Eigen::Vector3f> prev((size_t)nmap);
            std::memcpy((void *)prev.data(), l.mapPos.data(), (size_t)nmap * 12);
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

template <class T> static void put(std::FILE *f, const T *p, size_t n) { std::fwrite(p, sizeof(T), n, f); }

static void dumpTry(std::FILE *f, const Try &t)
{
    const int32_t n = (int32_t)t.inliers.size();
    put(f, &t.radius, 1);
    put(f, &t.accept, 1);
    put(f, &n, 1);
    put(f, t.inliers.data(), t.inliers.size());
}

int main(int argc, char **argv)
{
    PsContext *ctx = nullptr;
    if (ps_context_create(0, &ctx) != PS_OK) {
        std::printf("no device\n");
        return 2;
    }
    putslam_hip::FrameMatcher *matcher = putslam_hip::createFrameMatcher();
    const uint64_t S = 20261019;
    matcher->setSampleSeed(S);
    matcher->matcherParameters.RANSACParams.errorVersionMap = 0;
    const uint64_t mapSeed = S + 0x51ED270B0B5ull; // (frameCounter is 0: no frame has been matched)
    std::FILE *dump = argc > 1 ? std::fopen(argv[1], "wb") : nullptr;
    const struct {
        int D;
        double shift, sigma;
        int expect; // 1: a later try, 0: the first
    } cases[] = {{64, 0.15, 0.005, 1}, {128, 0.0, 0.02, 0}, {20, 0.0, 0.02, 0}};
    for (const auto &c : cases) {
        const int before = fails;
        Scene s;
        makeScene(s, c.D, 800, 900, c.shift, c.sigma);
        const Levels l = levelsOf(s);
        cv::Mat curF32(900, c.D, CV_32F, s.curD.data()), curU8(900, 32, CV_8U, s.curB.data());
        // a CV_8U call before ...
        useBinaryRows(s);
        Eigen::Matrix4f Tb = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inlb;
        int usedb = 0;
        const double rb = matcher->matchXYZ(s.mapF, curU8, s.curF, s.oct, s.det, Tb, inlb, 1);
        const double rbl = matcher->matchXYZLadder(s.mapF, curU8, s.curF, s.oct, s.det, Tb, inlb, 10, 0.1, &usedb);
        // ... the float calls against the loop
        useFloatRows(s);
        std::vector<Try> seq = sequential(ctx, *matcher, s, l, mapSeed, 10);
        int pick = 9;
        for (int k = 0; k < 10; ++k)
            if (seq[(size_t)k].ratio >= 0.1) {
                pick = k;
                break;
            }
        if (c.expect == 1) CHECK(pick > 0);
        if (c.expect == 0) CHECK(pick == 0);
        Eigen::Matrix4f T = Eigen::Matrix4f::Identity(), T1 = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inl, inl1;
        int used = 0;
        const double r = matcher->matchXYZLadder(s.mapF, curF32, s.curF, s.oct, s.det, T, inl, 10, 0.1, &used);
        std::printf("D %d shift %.2f: sequential picks try %d (ratio %.4f), ladder try %d (ratio %.4f, %zu inliers)\n", c.D, c.shift, pick + 1,
                    seq[(size_t)pick].ratio, used, r, inl.size());
        CHECK(used == pick + 1);
        CHECK(r == seq[(size_t)pick].ratio);
        CHECK(std::memcmp(T.data(), seq[(size_t)pick].pose.data(), 64) == 0);
        CHECK(sameMatches(inl, seq[(size_t)pick].inliers) && !inl.empty());
        const double r1 = matcher->matchXYZ(s.mapF, curF32, s.curF, s.oct, s.det, T1, inl1, 1);
        CHECK(r1 == seq[0].ratio && sameMatches(inl1, seq[0].inliers));
        if (seq[0].ratio >= 0.0) CHECK(std::memcmp(T1.data(), seq[0].pose.data(), 64) == 0);
        // a later computationNumber has the radius / ratio of that try (and matchXYZ's one seed)
        Eigen::Matrix4f T4 = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inl4;
        matcher->matchXYZ(s.mapF, curF32, s.curF, s.oct, s.det, T4, inl4, 4);
        for (const cv::DMatch &m : inl4) CHECK(m.imgIdx == -1 && m.queryIdx >= 0 && m.queryIdx < 800 && m.trainIdx >= 0 && m.trainIdx < 900);
        // ... and the CV_8U call afterwards is what it was
        useBinaryRows(s);
        Eigen::Matrix4f Ta = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inla;
        int useda = 0;
        const double ra = matcher->matchXYZ(s.mapF, curU8, s.curF, s.oct, s.det, Ta, inla, 1);
        const double ral = matcher->matchXYZLadder(s.mapF, curU8, s.curF, s.oct, s.det, Ta, inla, 10, 0.1, &useda);
        CHECK(ra == rb && ral == rbl && useda == usedb && sameMatches(inla, inlb) && std::memcmp(Ta.data(), Tb.data(), 64) == 0);
        CHECK(rbl >= 0.1 || c.shift > 0.0);
        // mixed types, another width
        Eigen::Matrix4f Tm = Eigen::Matrix4f::Identity();
        std::vector<cv::DMatch> inlm;
        CHECK(matcher->matchXYZ(s.mapF, curF32, s.curF, s.oct, s.det, Tm, inlm, 1) == -1.0);       // CV_8U map rows, CV_32F frame
        CHECK(matcher->matchXYZLadder(s.mapF, curF32, s.curF, s.oct, s.det, Tm, inlm) == -1.0);
        useFloatRows(s);
        CHECK(matcher->matchXYZ(s.mapF, curU8, s.curF, s.oct, s.det, Tm, inlm, 1) == -1.0);        // CV_32F map rows, CV_8U frame
        CHECK(matcher->matchXYZLadder(s.mapF, curU8, s.curF, s.oct, s.det, Tm, inlm) == -1.0);
        s.mapF[17].descriptor = cv::Mat(1, c.D - 4, CV_32F, s.mapD.data() + 17 * (size_t)c.D);     // one row of another width
        CHECK(matcher->matchXYZ(s.mapF, curF32, s.curF, s.oct, s.det, Tm, inlm, 1) == -1.0);
        CHECK(matcher->matchXYZLadder(s.mapF, curF32, s.curF, s.oct, s.det, Tm, inlm) == -1.0);
        CHECK(inlm.empty());
        if (dump) {
            const int32_t head[4] = {c.D, 800, 900, used};
            put(dump, head, 4);
            put(dump, l.mapPos.data(), l.mapPos.size());
            put(dump, s.mapD.data(), s.mapD.size());
            put(dump, l.mapLvl.data(), l.mapLvl.size());
            put(dump, reinterpret_cast<const float *>(s.curF.data()), (size_t)900 * 3);
            put(dump, s.curD.data(), s.curD.size());
            put(dump, l.curLvl.data(), l.curLvl.size());
            Try first = seq[0], taken = seq[(size_t)pick];
            first.inliers = inl1;
            taken.inliers = inl;
            dumpTry(dump, first);
            dumpTry(dump, taken);
        }
        std::printf("float map matching, D = %d: %s\n", c.D, fails == before ? "ok" : "FAILED");
    }
    if (dump) std::fclose(dump);
    ps_context_destroy(ctx);
    if (fails == 0) std::printf("all ok\n");
    return fails == 0 ? 0 : 1;
}
