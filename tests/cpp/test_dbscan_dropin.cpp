// ::DBScan of the drop-in (putslam_dropin.h) on the cases of a binary file, shaped like the reference's own call sites
// (matcher.cpp:459-461: DBScan dbscan(eps); dbscan.run(keyPoints)).  Input: int32 cases, then per case int32 n, double eps,
// int32 minPts, int32 featuresFromCluster, n x (float x, float y), n x int32 octave.  Output: per case int32 count, then the
// survivors' input indices.  Exit status 1 if a survivor's fields were not carried through intact.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "putslam_dropin.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t cases = 0;
    if (std::fread(&cases, 4, 1, in) != 1) return 3;
    int bad = 0;
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
            kps[i].size = 0.5f * (float)i;
            kps[i].angle = (float)(i % 360);
            kps[i].response = -(float)i;
            kps[i].octave = oct[i];
            kps[i].class_id = i;
        }
        DBScan dbscan(eps, minPts, ffc);
        dbscan.run(kps);
        const int32_t k = (int32_t)kps.size();
        std::fwrite(&k, 4, 1, out);
        for (const cv::KeyPoint &kp : kps) {
            const int i = kp.class_id;
            std::fwrite(&i, 4, 1, out);
            if (i < 0 || i >= n || kp.size != 0.5f * (float)i || kp.angle != (float)(i % 360) || kp.response != -(float)i ||
                kp.octave != oct[i] || std::memcmp(&kp.pt.x, &xy[2 * i], 4) != 0 || std::memcmp(&kp.pt.y, &xy[2 * i + 1], 4) != 0)
                ++bad;
        }
    }
    std::fclose(out);
    if (bad) std::fprintf(stderr, "%d survivors with altered fields\n", bad);
    return bad ? 1 : 0;
}
