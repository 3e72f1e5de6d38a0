// ps_uncertainty_rule.h -- the host arithmetic of the measurement uncertainty (ps_uncertainty.h), each rule once: the sensor
// model's defaults, the table of the colour gradient's ties and its packed form, and what the calls require of geometry, sensor
// model, model number and the two image sets.
// Pure -- no HIP header, no runtime call: tests/cpp/test_uncertainty_rule.cpp includes it into a plain C++ program that runs
// under the address and undefined-behaviour sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "ps_image_rule.h"

// DepthSensorModel::Config() (depthSensorModel.h:53-58).  The two scale factors are not set there: 0 here
inline void unc_sensor_default(PsSensorModel &s)
{
    const PsSensorModel d = {582.64, 586.97, 320.17, 260.0, 1.1046, 0.64160, -8.9997e-06, 3.069e-003, 3.6512e-006, -0.0017512e-3, 0.0, 0.0};
    s = d;
}

// coord1 / coord2 of RGBD.cpp:164-166 for (gradx, grady) = k x (0,0), (1,1), (-1,1), (-1,-1), (1,-1), by the literal expression
// with this host's libm (the operands pass through a volatile: evaluated when run, not when compiled).  t: 5 x 4
inline void unc_tie_table(int k, int32_t *t)
{
    static const int sx[5] = {0, 1, -1, -1, 1}, sy[5] = {0, 1, 1, -1, -1};
    for (int c = 0; c < 5; ++c) {
        volatile double gradx = (double)sx[c] * (double)k, grady = (double)sy[c] * (double)k;
        volatile double angle = atan2(grady, gradx) + (M_PI / 2.0);
        t[4 * c + 0] = int(sqrt(2) * sin(angle));
        t[4 * c + 1] = int(sqrt(2) * cos(angle));
        t[4 * c + 2] = int(sqrt(2) * sin(angle + M_PI));
        t[4 * c + 3] = int(sqrt(2) * cos(angle + M_PI));
    }
}

// The table as the kernels take it: entry k as value + 1 in bits 2k, 2k + 1 (|sqrt 2 sin| < 2: every entry is -1, 0 or 1)
inline unsigned long long unc_tie_pack(const int32_t *t)
{
    unsigned long long w = 0;
    for (int k = 0; k < 20; ++k) w |= (unsigned long long)(unsigned)(t[k] + 1) << (2 * k);
    return w;
}
inline int unc_tie_entry(unsigned long long w, int k) { return (int)((w >> (2 * k)) & 3u) - 1; }

struct UncStrides {
    size_t dRow = 0, dFrame = 0, iRow = 0, iFrame = 0; // resolved; the images' are 0 without images
};

// THE ARGUMENT RULE of every uncertainty call: geometry and the depth set are there; the sensor model where an information
// matrix is wanted (needSensor); model in -1 .. 2; the images where the gradient or model 2 is wanted (needImages), 3-channel,
// of the depth's shape; both sets' strides resolve, frame counts are not negative and a set with frames has pixels.  Returns
// PS_OK with the strides, or the code with `why`.
inline int unc_sets_error(const PsFrameGeometry *g, const PsSensorModel *sensor, int model, const PsImageSet *images, const PsDepthSet *depth,
                          bool needImages, bool needSensor, UncStrides &out, const char *&why)
{
    out = UncStrides{};
    if (!g || !depth || (needSensor && !sensor)) return why = "null geometry, sensor model or depth set", PS_ERR_BAD_ARG;
    if (model < -1 || model > 2) return why = "model outside -1 .. 2", PS_ERR_BAD_ARG;
    if (needImages && !images) return why = "the gradient needs the images", PS_ERR_BAD_ARG;
    if (images && images->channels != 3) return why = "the gradient is defined for 3-channel images only", PS_ERR_UNSUPPORTED;
    size_t view = 0;
    if (!depth_set_strides(*depth, out.dRow, out.dFrame, view) || depth->numFrames < 0 || (depth->numFrames > 0 && !depth->pixels))
        return why = "depth set: rows and cols in 1 .. 8192, even strides, rowStride at least a row, frameStride at least a view, pixels", PS_ERR_BAD_ARG;
    if (images && (!image_set_strides(*images, out.iRow, out.iFrame) || images->rows != depth->rows || images->cols != depth->cols ||
                   images->numFrames < 0 || (images->numFrames > 0 && !images->pixels)))
        return why = "image set: the depth's rows and cols, strides at least a row / a frame, pixels", PS_ERR_BAD_ARG;
    return PS_OK;
}
