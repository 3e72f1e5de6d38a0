// FrameMatcherHIP::performMatching on CV_32F descriptor Mats (cv::BFMatcher(cv::NORM_L2, true), matcherOpenCV.cpp:100-102,198-206)
// against a sequential restatement of the semantics, and on CV_8U Mats against ps_match_hamming256.
// Compiled with -ffp-contract=off: every operation of the restatement rounds separately.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "putslam_dropin.h"
#include "putslam_hip.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
float unit() { return (float)((int)(rnd() % 2001) - 1000) / 1000.0f; }

float l2sqr(const float *a, const float *b, int D)
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
        const float s0 = acc0[0] + acc1[0], s1 = acc0[1] + acc1[1], s2 = acc0[2] + acc1[2], s3 = acc0[3] + acc1[3];
        d = ((s0 + s1) + s2) + s3;
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

std::vector<cv::DMatch> restated(const cv::Mat &q, const cv::Mat &t)
{
    const int nq = q.rows, nt = t.rows, D = q.cols;
    std::vector<float> qd((size_t)nq, FLT_MAX);
    std::vector<int> qi((size_t)nq, -1);
    for (int tt = 0; tt < nt; ++tt) {
        float best = FLT_MAX;
        int nn = -1;
        for (int qq = 0; qq < nq; ++qq) {
            const float dist = std::sqrt(l2sqr(&t.at<float>(tt, 0), &q.at<float>(qq, 0), D));
            if (dist < best) {
                best = dist;
                nn = qq;
            }
        }
        if (nn >= 0 && best < qd[(size_t)nn]) {
            qd[(size_t)nn] = best;
            qi[(size_t)nn] = tt;
        }
    }
    std::vector<cv::DMatch> out;
    for (int qq = 0; qq < nq; ++qq)
        if (qi[(size_t)qq] >= 0) {
            cv::DMatch m;
            m.queryIdx = qq;
            m.trainIdx = qi[(size_t)qq];
            m.imgIdx = 0;
            m.distance = qd[(size_t)qq];
            out.push_back(m);
        }
    return out;
}

bool same(const std::vector<cv::DMatch> &a, const std::vector<cv::DMatch> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(cv::DMatch)) == 0);
}

} // namespace

int main()
{
    static_assert(sizeof(cv::DMatch) == sizeof(PsDMatch), "DMatch layout");
    putslam_hip::FrameMatcherHIP matcher;
    int failures = 0;
    const int dims[] = {64, 128, 13};
    for (int D : dims) {
        const int nq = 301, nt = 287;
        std::vector<float> qbuf((size_t)nq * (D + 3), NAN); // a pitched Mat over NaN padding
        cv::Mat q(nq, D, CV_32F, qbuf.data(), (size_t)(D + 3) * 4), t(nt, D, CV_32F);
        for (int r = 0; r < nq; ++r)
            for (int c = 0; c < D; ++c) q.at<float>(r, c) = unit();
        for (int r = 0; r < nt; ++r) {
            const int src = (int)(rnd() % (uint32_t)nq);
            const bool fresh = rnd() % 10 < 3;
            for (int c = 0; c < D; ++c) t.at<float>(r, c) = fresh ? unit() : q.at<float>(src, c) + 0.05f * unit();
        }
        for (int c = 0; c < D; ++c) t.at<float>(5, c) = q.at<float>(7, c); // an exact copy: distance 0
        t.at<float>(9, 0) = NAN;                                           // chooses nobody
        const std::vector<cv::DMatch> got = matcher.performMatching(q, t), want = restated(q, t);
        const bool ok = same(got, want) && want.size() > 100;
        std::printf("CV_32F D=%d: %zu matches, restated %zu: %s\n", D, got.size(), want.size(), ok ? "ok" : "MISMATCH");
        failures += !ok;
        const bool free_ok = same(putslam_hip::l2CrossCheckMatch(q, t), want);
        failures += !free_ok;
    }
    {
        const int n = 400;
        cv::Mat a(n, 32, CV_8U), b(n, 32, CV_8U);
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < 32; ++c) {
                a.at<uint8_t>(r, c) = (uint8_t)rnd();
                b.at<uint8_t>(r, c) = (uint8_t)(rnd() % 4 ? a.at<uint8_t>((r * 7 + 3) % n, c) : rnd());
            }
        const std::vector<cv::DMatch> got = matcher.performMatching(a, b);
        int m = 0;
        PsContext *ctx = nullptr;
        std::vector<cv::DMatch> want((size_t)n);
        if (ps_context_create(0, &ctx) != PS_OK || ps_match_hamming256(ctx, a.data, n, a.step, b.data, n, b.step, reinterpret_cast<PsDMatch *>(want.data()), &m) != PS_OK) {
            std::printf("CV_8U: no context / ps_match_hamming256 failed\n");
            return 2;
        }
        ps_context_destroy(ctx);
        want.resize((size_t)m);
        const bool ok = same(got, want) && m > 100;
        std::printf("CV_8U: %zu matches, ps_match_hamming256 %d: %s\n", got.size(), m, ok ? "ok" : "MISMATCH");
        failures += !ok;
    }
    std::printf(failures ? "FAILED (%d)\n" : "all ok\n", failures);
    return failures ? 1 : 0;
}
