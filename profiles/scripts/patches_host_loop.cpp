// THE CONTROL of profiles/scripts/patches_times.py: what a host does without ps_patch_align -- MatchingOnPatches' three calls
// (MatchingOnPatches.cpp:14-246) point after point, pair after pair, on ONE thread, on host arrays, over
// putslam_amd/csrc/ps_patches_host.h.  g++ -O2 -ffp-contract=off -shared -fPIC.  Layouts are ps_patch_align's: P x capacity points.
#include <vector>

#include "putslam_hip.h"
#include "ps_patches_host.h"

extern "C" int patches_host_align(const uint8_t *images, size_t rowStride, size_t frameStride, int frames, int rows, int cols, int channels,
                                  const int32_t *pairs, const double *oldPts, double *newPts, const int32_t *counts, int P, int capacity,
                                  const PsPatchParams *prm, uint8_t *status, int32_t *iterations)
{
    if (patch_params_error(prm)) return PS_ERR_BAD_ARG;
    const size_t E = (size_t)patch_elems(prm->patchSize);
    std::vector<double> patch(E), scratch(E);
    std::vector<float> gx(E), gy(E);
    float inv[9];
    for (int p = 0; p < P; ++p) {
        const int n = counts[p], s0 = pairs[2 * p], s1 = pairs[2 * p + 1];
        if (n < 0 || n > capacity) continue;
        const bool slots = s0 >= 0 && s0 < frames && s1 >= 0 && s1 < frames;
        for (int k = 0; k < n; ++k) {
            const size_t o = (size_t)p * capacity + k;
            if (!slots) {
                status[o] = PS_PATCH_OLD_TAPS_OUTSIDE;
                iterations[o] = 0;
                continue;
            }
            const patch_host::Image io{images + (size_t)s0 * frameStride, rowStride, rows, cols, channels},
                in{images + (size_t)s1 * frameStride, rowStride, rows, cols, channels};
            double x = newPts[2 * o], y = newPts[2 * o + 1];
            int it = 0;
            status[o] = (uint8_t)patch_host::align(io, in, oldPts[2 * o], oldPts[2 * o + 1], *prm, x, y, it, patch.data(), scratch.data(), gx.data(),
                                                   gy.data(), inv);
            iterations[o] = it;
            if (it > 0) newPts[2 * o] = x, newPts[2 * o + 1] = y;
        }
    }
    return PS_OK;
}
