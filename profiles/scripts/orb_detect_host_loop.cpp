// The timing control of profiles/scripts/orb_detect_times.py: ORB detection of one image on one host thread, the specification
// restated in plain C++ (tests/cpp/orb_detect_restated.h) -- grey conversion, pyramid, FAST, both cuts, Harris, angle and the grid
// loop per call, as cv::ORB::detect inside MatcherOpenCV::detectFeatures does.  g++ -O2 -ffp-contract=off -shared.  It returns the
// same bytes as ps_detect_features_orb.
#include "../../tests/cpp/orb_detect_restated.h"

extern "C" int orb_detect_host(const uint8_t *img, int rows, int cols, int cn, size_t step, int nFeatures, float scaleFactor, int nLevels,
                               int fastThreshold, int gridRows, int gridCols, int maxFeatures, float *xy, float *response, float *angle,
                               int32_t *octave)
{
    orb_detect_restated::Params p;
    p.nFeatures = nFeatures;
    p.scaleFactor = scaleFactor;
    p.nLevels = nLevels;
    p.fastThreshold = fastThreshold;
    p.gridRows = gridRows;
    p.gridCols = gridCols;
    p.maximalTrackedFeatures = maxFeatures;
    const std::vector<orb_detect_restated::Kp> k = orb_detect_restated::detect(img, rows, cols, cn, step, p);
    for (size_t j = 0; j < k.size(); ++j) {
        xy[2 * j] = k[j].x;
        xy[2 * j + 1] = k[j].y;
        response[j] = k[j].response;
        angle[j] = k[j].angle;
        octave[j] = k[j].octave;
    }
    return (int)k.size();
}
