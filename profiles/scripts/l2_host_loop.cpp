// Single-thread restatement of cv::BFMatcher(cv::NORM_L2, true).match(query, train) (reference call site
// src/Matcher/matcherOpenCV.cpp:100-102,198-206) on plain arrays: the host loop profiles/scripts/l2_match_times.py times
// ps_match_l2_f32 against (g++ -O2 -ffp-contract=off, no -march: scalar SSE2, no FMA).  A restatement, not OpenCV compiled: the
// order of the sums is DESIGN.md section 8.6's, the containers are not OpenCV's.
#include <cfloat>
#include <cmath>
#include <vector>

namespace {
inline float l2sqr(const float *a, const float *b, int D)
{
    int j = 0;
    float d = 0.0f;
    if (D >= 8) {
        float acc0[4] = {0, 0, 0, 0}, acc1[4] = {0, 0, 0, 0};
        for (; j <= D - 8; j += 8)
            for (int i = 0; i < 4; ++i) {
                const float t0 = a[j + i] - b[j + i], t1 = a[j + 4 + i] - b[j + 4 + i];
                acc0[i] = acc0[i] + t0 * t0;
                acc1[i] = acc1[i] + t1 * t1;
            }
        d = (((acc0[0] + acc1[0]) + (acc0[1] + acc1[1])) + (acc0[2] + acc1[2])) + (acc0[3] + acc1[3]);
    }
    for (; j <= D - 4; j += 4) {
        const float t0 = a[j] - b[j], t1 = a[j + 1] - b[j + 1], t2 = a[j + 2] - b[j + 2], t3 = a[j + 3] - b[j + 3];
        d = d + (((t0 * t0 + t1 * t1) + t2 * t2) + t3 * t3);
    }
    for (; j < D; ++j) {
        const float t = a[j] - b[j];
        d = d + t * t;
    }
    return d;
}
} // namespace

// out: nq x (queryIdx, trainIdx) ints and dist: nq floats; returns the number of matches
extern "C" int l2_match_host(const float *query, int nq, const float *train, int nt, int D, int *out, float *dist)
{
    std::vector<float> qd((size_t)nq, FLT_MAX);
    std::vector<int> qi((size_t)nq, -1);
    for (int t = 0; t < nt; ++t) {
        float best = FLT_MAX;
        int nn = -1;
        for (int q = 0; q < nq; ++q) {
            const float v = std::sqrt(l2sqr(train + (size_t)t * D, query + (size_t)q * D, D));
            if (v < best) {
                best = v;
                nn = q;
            }
        }
        if (nn >= 0 && best < qd[(size_t)nn]) {
            qd[(size_t)nn] = best;
            qi[(size_t)nn] = t;
        }
    }
    int n = 0;
    for (int q = 0; q < nq; ++q)
        if (qi[(size_t)q] >= 0) {
            out[2 * n] = q;
            out[2 * n + 1] = qi[(size_t)q];
            dist[n++] = qd[(size_t)q];
        }
    return n;
}
