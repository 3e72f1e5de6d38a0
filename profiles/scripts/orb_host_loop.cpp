// The timing control of profiles/scripts/orb_times.py: ORB description of one image on one host thread, the specification restated in
// plain C++ (tests/cpp/orb_restated.h) -- pyramid, blur and rows per call, as cv::ORB::compute does.  g++ -O2 -ffp-contract=off
// -shared.  It returns the same bytes as ps_describe_features.
#include "../../tests/cpp/orb_restated.h"

extern "C" int orb_describe_host(const uint8_t *img, int rows, int cols, int cn, size_t step, float scaleFactor, int nLevels, const float *xy,
                                 const float *angle, const int32_t *octave, int n, uint8_t *desc, int32_t *keptIdx)
{
    return orb_restated::describe(img, rows, cols, cn, step, scaleFactor, nLevels, nullptr, xy, angle, octave, n, desc, keptIdx);
}
