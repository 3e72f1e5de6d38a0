// THE CONTROL of profiles/scripts/uncertainty_times.py, and what tests/test_uncertainty_host_loop.py holds to the restatement: the
// loop a host runs today between Matcher::matchXYZ's inliers and the graph -- matcher.cpp:769-794 (the inliers in match-list order),
// PUTSLAM.cpp:826-837 (computeNormals, computeRGBGradients) and FeaturesMap::addMeasurements' information matrix
// (featuresMap.cpp:261-274) -- on ONE thread, on host arrays, over putslam_amd/csrc/ps_uncertainty_host.h.
// g++ -O2 -ffp-contract=off -shared -fPIC.  Layouts are ps_measurement_edges': P x maxMatches rows per output, dense sets.
#include "ps_uncertainty_host.h"

extern "C" int unc_host_edges(const PsFrameGeometry *g, const PsSensorModel *s, int model, const uint8_t *images, size_t iRow, size_t iFrame,
                              int iFrames, const uint8_t *depth, size_t dRow, size_t dFrame, int dFrames, int rows, int cols,
                              const int32_t *imageFrame, const int32_t *pairs, int P, int numMaps, int numFrames, int maxKpts, int maxMatches,
                              const PsDMatch *matches, const int32_t *numMatches, const uint8_t *mask, const float *pts, const float *xyUndist,
                              int32_t *count, int32_t *mapRow, int32_t *curRow, float *uv, double *position, double *normal, double *gradient,
                              double *info)
{
    int32_t tie[20];
    unc_tie_table(1, tie);
    const unc_host::Camera cam = {g->K[0], g->K[4], g->K[2], g->K[5], g->depthImageScale};
    for (int p = 0; p < P; ++p) {
        const int m = numMatches[p], view = pairs[2 * p], fr = pairs[2 * p + 1];
        count[p] = 0;
        if (m <= 0 || m > maxMatches || view < 0 || view >= numMaps || fr < 0 || fr >= numFrames) continue;
        const int frame = imageFrame[fr];
        const bool inSets = frame >= 0 && frame < dFrames && (!images || frame < iFrames);
        const size_t base = (size_t)p * (size_t)maxMatches;
        int n = 0;
        for (int i = 0; i < m; ++i) {
            if (!mask[base + i]) continue;
            const PsDMatch mt = matches[base + i];
            const size_t to = base + (size_t)n++;
            const size_t row = (size_t)fr * (size_t)maxKpts + (size_t)mt.trainIdx;
            const float u = xyUndist[2 * row], v = xyUndist[2 * row + 1], *pt = pts + 3 * row;
            if (mapRow) mapRow[to] = mt.queryIdx;
            if (curRow) curRow[to] = mt.trainIdx;
            if (uv) uv[2 * to] = u, uv[2 * to + 1] = v;
            if (position)
                for (int k = 0; k < 3; ++k) position[3 * to + k] = unc_host::canon((double)pt[k]);
            double *no = normal ? normal + 3 * to : nullptr, *go = gradient ? gradient + 3 * to : nullptr, *io = info ? info + 9 * to : nullptr;
            if (!inSets) {
                const double q = unc_host::canon(std::nan(""));
                for (int k = 0; k < 3; ++k) {
                    if (no) no[k] = q;
                    if (go) go[k] = q;
                }
                for (int k = 0; io && k < 9; ++k) io[k] = q;
                continue;
            }
            const unc_host::DepthImage d = {depth + (size_t)frame * dFrame, dRow, rows, cols};
            const unc_host::ColourImage im = {images ? images + (size_t)frame * iFrame : nullptr, iRow};
            unc_host::feature(cam, d, im, *s, tie, model, u, v, pt[2], no, go, io);
        }
        count[p] = n;
    }
    return 0;
}
