// The drop-in's three spatial-exclusion entry points (putslam_dropin.h / putslam_matcher_glue.h) on the cases of a binary file,
// called the way the reference calls its own (PUTSLAM.cpp:871, matcher.cpp:97-130,886-974).  Input: int32 cases, then per case
// int32 kind and
//   kind 1 (chooseFeaturesToAddToMap): int32 n, m, addedCounter, maxOnceFeatureAdd; float minEuclid, minImage; n x 3 float
//           feature3D; n x 2 float undistortedFeature2D; m x 5 double (position x, y, z, u, v) of the map features
//           -> int32 addedCounter returned, int32 k, k accepted indices
//   kind 2 (mergeTrackedFeatures): int32 n, s; double minReproj; n x 2 float undistorted; s x 2 float sandbox undistorted
//           -> int32 size afterwards, then the origin of every entry (existing i: i, sandbox i: 1000000 + i)
//   kind 3 (removeTooCloseFeatures): int32 n, nm; double minEuclid, minReproj; n x 3 float; n x 2 float; nm x 2 int32 (queryIdx,
//           trainIdx) -> int32 r, r removed indices (the returned set); int32 k, k origins of what stays; int32 nm', nm' x 2 int32
// Exit status 1 if the five lists of kinds 2 / 3 do not stay consistent with one another.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "putslam_matcher_glue.h"

namespace {
struct Position {
    double p[3];
    double x() const { return p[0]; }
    double y() const { return p[1]; }
    double z() const { return p[2]; }
};
struct MapFeature { // the members of putslam::MapFeature that chooseFeaturesToAddToMap reads (putslam_defs.h)
    Position position;
    double u, v;
};
struct FeatureSet { // Matcher::featureSet (matcher.h:31-37), the members read
    std::vector<Eigen::Vector3f> feature3D;
    std::vector<cv::Point2f> undistortedFeature2D;
};

template <class T> bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
void wr(FILE *f, int32_t v) { std::fwrite(&v, 4, 1, f); }

cv::KeyPoint kp(int origin)
{
    cv::KeyPoint k;
    k.class_id = origin;
    k.size = (float)(origin % 977);
    return k;
}
// the five lists carry the same origin in every entry
int consistent(const std::vector<cv::Point2f> &dist, const std::vector<cv::Point2f> &und, const std::vector<Eigen::Vector3f> &f3,
               const std::vector<cv::KeyPoint> &kps, const std::vector<double> &dd, const std::vector<cv::Point2f> &und0,
               const std::vector<cv::Point2f> &sb0)
{
    const size_t n = und.size();
    if (dist.size() != n || f3.size() != n || kps.size() != n || dd.size() != n) return 1;
    int bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const int o = kps[i].class_id;
        const cv::Point2f &src = o >= 1000000 ? sb0[(size_t)(o - 1000000)] : und0[(size_t)o];
        if (dd[i] != 0.25 * o || dist[i].x != (float)o || !(und[i].x == src.x || (und[i].x != und[i].x && src.x != src.x)) ||
            kps[i].size != (float)(o % 977))
            ++bad;
    }
    return bad;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t cases = 0;
    if (!rd(in, &cases, 1)) return 3;
    putslam_hip::FrameMatcherHIP matcher;
    int bad = 0;
    for (int c = 0; c < cases; ++c) {
        int32_t kind = 0;
        if (!rd(in, &kind, 1)) return 3;
        if (kind == 1) {
            int32_t h[4];
            float thr[2];
            if (!rd(in, h, 4) || !rd(in, thr, 2)) return 3;
            const int n = h[0], m = h[1];
            FeatureSet fs;
            fs.feature3D.resize((size_t)n);
            fs.undistortedFeature2D.resize((size_t)n);
            std::vector<double> mp((size_t)m * 5);
            if (!rd(in, reinterpret_cast<float *>(fs.feature3D.data()), (size_t)n * 3) ||
                !rd(in, reinterpret_cast<float *>(fs.undistortedFeature2D.data()), (size_t)n * 2) || !rd(in, mp.data(), mp.size()))
                return 3;
            std::vector<MapFeature> mapFeatures((size_t)m);
            for (int k = 0; k < m; ++k) {
                for (int a = 0; a < 3; ++a) mapFeatures[(size_t)k].position.p[a] = mp[(size_t)k * 5 + a];
                mapFeatures[(size_t)k].u = mp[(size_t)k * 5 + 3];
                mapFeatures[(size_t)k].v = mp[(size_t)k * 5 + 4];
            }
            std::vector<int> accepted;
            const int counter = putslam_hip::chooseFeaturesToAddToMap(fs, h[2], h[3], mapFeatures, thr[0], thr[1], accepted);
            wr(out, counter);
            wr(out, (int32_t)accepted.size());
            for (int j : accepted) wr(out, j);
        } else if (kind == 2 || kind == 3) {
            int32_t h[2];
            double thr[2] = {0, 0};
            if (!rd(in, h, 2) || !rd(in, thr, kind == 2 ? 1 : 2)) return 3;
            const int n = h[0];
            std::vector<cv::Point2f> und((size_t)n), dist((size_t)n), sb, sbDist;
            std::vector<Eigen::Vector3f> f3((size_t)n), sb3;
            std::vector<cv::KeyPoint> kps, sbK;
            std::vector<double> dd, sbD;
            std::vector<cv::DMatch> matches;
            if (kind == 3 && !rd(in, reinterpret_cast<float *>(f3.data()), (size_t)n * 3)) return 3;
            if (!rd(in, reinterpret_cast<float *>(und.data()), (size_t)n * 2)) return 3;
            for (int i = 0; i < n; ++i) {
                dist[(size_t)i] = cv::Point2f((float)i, 0.f);
                kps.push_back(kp(i));
                dd.push_back(0.25 * i);
            }
            const std::vector<cv::Point2f> und0 = und;
            if (kind == 2) {
                const int s = h[1];
                sb.resize((size_t)s);
                if (!rd(in, reinterpret_cast<float *>(sb.data()), (size_t)s * 2)) return 3;
                for (int i = 0; i < s; ++i) {
                    sbDist.push_back(cv::Point2f((float)(1000000 + i), 0.f));
                    sb3.push_back(Eigen::Vector3f((float)i, 1.f, 2.f));
                    sbK.push_back(kp(1000000 + i));
                    sbD.push_back(0.25 * (1000000 + i));
                }
                matcher.matcherParameters.OpenCVParams.minimalReprojDistanceNewTrackingFeatures = thr[0];
                matcher.mergeTrackedFeatures(und, sb, dist, sbDist, f3, sb3, kps, sbK, dd, sbD);
            } else {
                const int nm = h[1];
                std::vector<int32_t> qt((size_t)nm * 2);
                if (!rd(in, qt.data(), qt.size())) return 3;
                for (int i = 0; i < nm; ++i) matches.push_back(cv::DMatch(qt[(size_t)2 * i], qt[(size_t)2 * i + 1], (float)i));
                matcher.matcherParameters.OpenCVParams.minimalEuclidDistanceNewTrackingFeatures = thr[0];
                matcher.matcherParameters.OpenCVParams.minimalReprojDistanceNewTrackingFeatures = thr[1];
                const std::set<int> removed = matcher.removeTooCloseFeatures(dist, und, f3, kps, dd, matches);
                wr(out, (int32_t)removed.size());
                for (int r : removed) wr(out, r);
            }
            bad += consistent(dist, und, f3, kps, dd, und0, sb);
            wr(out, (int32_t)kps.size());
            for (const cv::KeyPoint &k : kps) wr(out, k.class_id);
            if (kind == 3) {
                wr(out, (int32_t)matches.size());
                for (const cv::DMatch &mt : matches) {
                    wr(out, mt.queryIdx);
                    wr(out, mt.trainIdx);
                }
            }
        } else {
            return 3;
        }
    }
    std::fclose(out);
    if (bad) std::fprintf(stderr, "%d entries whose lists disagree\n", bad);
    return bad ? 1 : 0;
}
