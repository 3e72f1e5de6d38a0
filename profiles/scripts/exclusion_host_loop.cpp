// Single-thread restatement of PUTSLAM::chooseFeaturesToAddToMap + removeCloseFeatures (src/PUTSLAM/PUTSLAM.cpp:53-178) on plain
// arrays, the host loop profiles/scripts/exclusion_times.py times ps_exclude against (g++ -O2, no -march: no FMA contraction).
// A restatement, not the reference compiled: the loop structure and the roundings are the reference's, the containers are not.
#include <cmath>
#include <vector>

namespace {
inline bool closeTo(const float *e3, const float *e2, const float *f3, const float *f2, double minEuclid, double minImage)
{
    const float d0 = e3[0] - f3[0], d1 = e3[1] - f3[1], d2 = e3[2] - f3[2];
    const float norm = std::sqrt(d0 * d0 + (d1 * d1 + d2 * d2)); // (tmp - feature3D).norm(), :61
    if (norm < minEuclid) return true;
    const float du = e2[0] - f2[0], dv = e2[1] - f2[1];
    const float imageNorm = (float)std::sqrt((double)du * du + (double)dv * dv); // (float)cv::norm(point - feature2D), :67
    return imageNorm < minImage;
}
} // namespace

extern "C" int excl_c1_host(const float *f3, const float *f2, int n, const float *m3, const float *m2, int m, float minEuclid,
                            float minImage, int maxOnceFeatureAdd, int *out)
{
    std::vector<float> a3, a2; // mapFeaturesToAdd
    int addedCounter = 0;
    for (int j = 0; j < n && addedCounter < maxOnceFeatureAdd; ++j) {
        if (!(f3[3 * j + 2] > 0.8 && f3[3 * j + 2] < 6.0)) continue;
        bool ok = true;
        for (int k = 0; k < m && ok; ++k) ok = !closeTo(m3 + 3 * k, m2 + 2 * k, f3 + 3 * j, f2 + 2 * j, minEuclid, minImage);
        for (int k = 0; k < addedCounter && ok; ++k)
            ok = !closeTo(a3.data() + 3 * k, a2.data() + 2 * k, f3 + 3 * j, f2 + 2 * j, minEuclid, minImage);
        if (!ok) continue;
        a3.insert(a3.end(), f3 + 3 * j, f3 + 3 * j + 3);
        a2.insert(a2.end(), f2 + 2 * j, f2 + 2 * j + 2);
        out[addedCounter++] = j;
    }
    return addedCounter;
}
