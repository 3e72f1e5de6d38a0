// ps_patches_rule.h -- the host arithmetic of the sub-pixel matching on patches (ps_patches.h), each rule
// once: what PsPatchParams may carry, the element count and the LDS bytes of one wave, the two tap rules that decide where this
// build diverges from the reference (MatchingOnPatches.cpp has no bounds test for the old image and a gate for the new one that
// admits taps past the bottom and right edges), and the reference's gate itself.
// Pure -- no HIP header, no runtime call: tests/cpp/test_patches_rule.cpp includes it into a plain C++ program that runs
// under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ps_image_rule.h"

constexpr int kPatchMinSize = 3, kPatchMaxSize = 31, kPatchMaxIter = 1000;

// THE PARAMETER RULE: patchSize odd, 3 .. 31 (an even size lets the reference's loops visit (2h + 1)^2 elements while its sums
// run over patchSize^2, past the end of its vectors); maxIter 0 .. 1000; no unknown flag; reserved 0.  nullptr when fine.
inline const char *patch_params_error(const PsPatchParams *p)
{
    if (!p) return "null PsPatchParams";
    if (p->patchSize < kPatchMinSize || p->patchSize > kPatchMaxSize || (p->patchSize & 1) == 0)
        return "PsPatchParams: patchSize must be odd and lie in 3 .. 31";
    if (p->maxIter < 0 || p->maxIter > kPatchMaxIter) return "PsPatchParams: maxIter must lie in 0 .. 1000";
    if (p->flags & ~PS_PATCH_GIVEN_MODEL) return "PsPatchParams: unknown flag";
    if (p->reserved != 0) return "PsPatchParams: reserved must be 0";
    return nullptr;
}

inline int patch_half(int patchSize) { return (patchSize - 1) / 2; }       // MatchingOnPatches::init (:212)
inline int patch_elems(int patchSize) { return patchSize * patchSize; }    // E
inline int patch_elems4(int patchSize) { return (patch_elems(patchSize) + 3) & ~3; } // a float row of the wave's slice

// THE LDS BYTES of one wave: the patch as E4 doubles, then five float rows of E4 (three rows of products, gx, gy).  A multiple of 16.
// 31 x 31: 26 992 bytes.
inline size_t patch_wave_bytes(int patchSize) { return (size_t)patch_elems4(patchSize) * 28; }
// Waves of a work-group (they share nothing): as many as 64 KiB of LDS hold, four at most
inline int patch_block_waves(int patchSize)
{
    const size_t w = 65536 / patch_wave_bytes(patchSize);
    return w > 4 ? 4 : (int)w;
}

// THE OLD IMAGE'S TAP RULE (the reference has none): the position is finite and every tap of the patch (columns int(x) - h ..
// int(x) + h + 1) and of the gradient (int(x) - h - 1 .. int(x) + h + 1) lies inside: int(x) - h - 1 >= 0 and int(x) + h + 1 <=
// cols - 1, the same for y.  Decided on the doubles -- int(x) >= h + 1 iff x >= h + 1, int(x) <= cols - h - 2 iff x < cols - h - 1
// -- so that nothing is truncated that does not fit an int; NaN and the infinities fail.
inline bool patch_old_taps_inside(double x, double y, int h, int rows, int cols)
{
    return x >= (double)(h + 1) && x < (double)(cols - h - 1) && y >= (double)(h + 1) && y < (double)(rows - h - 1);
}

// THE REFERENCE'S GATE (:139-143, mean is never NaN): true = "Out of image"
inline bool patch_gate_out(double x, double y, int h, int rows, int cols)
{
    return x != x || y != y || x < (double)h || x > (double)(cols - h) || y < (double)h || y > (double)(rows - h);
}

// THE NEW IMAGE'S TAP RULE for a position that passed the gate (so int(x) - h >= 0 and int(x) fits): the bilinear taps reach
// column int(x) + h + 1 and row int(y) + h + 1, which the gate lets lie up to two past the edge.
inline bool patch_new_taps_inside(double x, double y, int h, int rows, int cols)
{
    return (int)x + h + 1 <= cols - 1 && (int)y + h + 1 <= rows - 1;
}

// What a model or alignment call requires of its image set: the strides resolve, 1 or 3 channels, rows and cols within 8192,
// frames not negative, pixels where there are frames.  nullptr when fine
inline const char *patch_images_error(const PsImageSet *s, size_t &row, size_t &frame)
{
    row = frame = 0;
    if (!s) return "null image set";
    if (s->channels != 1 && s->channels != 3) return "channels must be 1 or 3";
    if (s->rows > kImageMaxDim || s->cols > kImageMaxDim) return "image above 8192 rows or columns";
    if (!image_set_strides(*s, row, frame) || s->numFrames < 0 || (s->numFrames > 0 && !s->pixels))
        return "image set: rows and cols at least 1, strides at least a row / a frame, pixels";
    return nullptr;
}
