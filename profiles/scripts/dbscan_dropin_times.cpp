// ::DBScan::run of the drop-in (putslam_dropin.h), call -> return (the call is synchronous), on the frames of
// dbscan_times.py: keypoints uniform in 640 x 480, about 25 % of them 0.5 px from their predecessor; eps = 1, minPts = 2,
// featuresFromCluster = 1.  Median of 50 calls per size; the vector is refilled outside the timed region.  Built and run by
// dbscan_times.py.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "putslam_dropin.h"

int main()
{
    std::mt19937_64 rng(2026);
    std::uniform_real_distribution<float> ux(0.f, 640.f), uy(0.f, 480.f), u01(0.f, 1.f);
    for (int n : {500, 2000, 5000}) {
        std::vector<cv::KeyPoint> frame((size_t)n);
        for (int i = 0; i < n; ++i) {
            frame[i].pt = cv::Point2f(ux(rng), uy(rng));
            if (i > 0 && u01(rng) < 0.25f) {
                const float a = 6.2831853f * u01(rng);
                frame[i].pt = cv::Point2f(frame[i - 1].pt.x + 0.5f * std::cos(a), frame[i - 1].pt.y + 0.5f * std::sin(a));
            }
            frame[i].octave = i % 8;
        }
        std::vector<double> us;
        size_t kept = 0;
        for (int r = 0; r < 51; ++r) {
            std::vector<cv::KeyPoint> kps = frame;
            const auto t0 = std::chrono::steady_clock::now();
            DBScan dbscan(1.0);
            dbscan.run(kps);
            const auto t1 = std::chrono::steady_clock::now();
            if (r > 0) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
            kept = kps.size();
        }
        std::sort(us.begin(), us.end());
        std::printf("::DBScan::run N=%d eps=1 minPts=2 ffc=1: %.1f us call->return (median of 50), %zu kept\n", n, us[us.size() / 2],
                    kept);
    }
    return 0;
}
