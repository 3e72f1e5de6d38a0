// Runs the reference's DBScan (compiled from its own dbscan.cpp) on the cases of a binary file and writes the surviving
// keypoints' input indices.  Input: int32 cases, then per case int32 n, double eps, int32 minPts, int32 featuresFromCluster,
// n x (float x, float y), n x int32 octave.  Output: per case int32 count, then the indices (class_id carries them).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "putslam/Matcher/dbscan.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t cases = 0;
    if (std::fread(&cases, 4, 1, in) != 1) return 3;
    for (int c = 0; c < cases; ++c) {
        int32_t n, minPts, ffc;
        double eps;
        if (std::fread(&n, 4, 1, in) != 1 || std::fread(&eps, 8, 1, in) != 1 || std::fread(&minPts, 4, 1, in) != 1 ||
            std::fread(&ffc, 4, 1, in) != 1)
            return 3;
        std::vector<float> xy((size_t)n * 2);
        std::vector<int32_t> oct((size_t)n);
        if (n > 0 && (std::fread(xy.data(), 8, (size_t)n, in) != (size_t)n || std::fread(oct.data(), 4, (size_t)n, in) != (size_t)n))
            return 3;
        std::vector<cv::KeyPoint> kps((size_t)n);
        for (int i = 0; i < n; ++i) {
            kps[i].pt = cv::Point2f(xy[2 * i], xy[2 * i + 1]);
            kps[i].octave = oct[i];
            kps[i].class_id = i;
        }
        DBScan dbscan(eps, minPts, ffc);
        dbscan.run(kps);
        const int32_t k = (int32_t)kps.size();
        std::fwrite(&k, 4, 1, out);
        for (const cv::KeyPoint &kp : kps) std::fwrite(&kp.class_id, 4, 1, out);
    }
    std::fclose(out);
    return 0;
}
