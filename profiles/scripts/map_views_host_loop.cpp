// map_views_host_loop.cpp -- what a host does per frame and per visible map feature before matchXYZ, as ONE single-threaded loop
// over the store layout of PsMapStore (include/putslam_hip.h): observation choice by viewing angle, angle filter, move into the
// camera frame, projection, predicted level with the host's pow / log / ceil, copy of the chosen descriptor.  Written for the
// timing comparison of profiles/scripts/map_views_times.py and tests/test_gpu_map_view.py (the side ps_map_views_device is
// measured against); built there with  g++ -O2 -shared -fPIC.  A restatement of the five steps, not reference text.
#include <cmath>
#include <cstdint>
#include <cstring>

extern "C" int host_build_views(const double *pos, const int32_t *obsStart, const int32_t *obsPose, const uint8_t *obsDesc,
                                const int32_t *obsOctave, const double *obsDetDist, int numFeatures, const double *camInv,
                                const double *poseAngle, int numPoses, const int32_t *cand, const int32_t *candCounts,
                                int candCapacity, int V, double maxAngle, double fx, double fy, double cx, double cy, double imageW,
                                double imageH, int requireVisible, int maxKpts, uint8_t *desc, float *pts, int32_t *nkpts,
                                int32_t *mapLevel)
{
    const double logScale = std::log(1.2);
    for (int v = 0; v < V; ++v) {
        const double *M = camInv + (size_t)v * 16;
        const double *ang = poseAngle + (size_t)v * numPoses;
        const int n = cand ? candCounts[v] : numFeatures;
        uint8_t *d = desc + (size_t)v * maxKpts * 32;
        float *p3 = pts + (size_t)v * maxKpts * 3;
        int32_t *lv = mapLevel + (size_t)v * maxKpts;
        int rows = 0;
        for (int i = 0; i < n; ++i) {
            const int f = cand ? cand[(size_t)v * candCapacity + i] : i;
            double best = 10.0;
            int chosen = -1;
            for (int o = obsStart[f]; o < obsStart[f + 1]; ++o) {
                const double a = ang[obsPose[o]];
                if (a < best) {
                    best = a;
                    chosen = o;
                }
            }
            if (chosen < 0 || best > maxAngle) continue;
            const double x = pos[3 * (size_t)f], y = pos[3 * (size_t)f + 1], z = pos[3 * (size_t)f + 2];
            const double p0 = ((M[0] * x + M[4] * y) + M[8] * z) + M[12];
            const double p1 = ((M[1] * x + M[5] * y) + M[9] * z) + M[13];
            const double p2 = ((M[2] * x + M[6] * y) + M[10] * z) + M[14];
            double u = ((fx * p0) / p2) + cx, w = ((fy * p1) / p2) + cy;
            if (u < 0 || u > imageW || w < 0 || w > imageH || p2 < 0.8 || p2 > 6.0) u = w = -1.0;
            if (requireVisible && u == -1.0) continue;
            if (rows >= maxKpts) return -1;
            const double curDist = std::sqrt((p0 * p0 + p1 * p1) + p2 * p2);
            const double scale = std::pow(1.2, obsOctave[chosen]) * obsDetDist[chosen] / curDist;
            int level = (int)std::ceil(std::log(scale) / logScale);
            level = level < 0 ? 0 : (level > 7 ? 7 : level);
            std::memcpy(d + (size_t)rows * 32, obsDesc + (size_t)chosen * 32, 32);
            p3[3 * rows] = (float)p0;
            p3[3 * rows + 1] = (float)p1;
            p3[3 * rows + 2] = (float)p2;
            lv[rows] = level;
            ++rows;
        }
        nkpts[v] = rows;
    }
    return 0;
}
