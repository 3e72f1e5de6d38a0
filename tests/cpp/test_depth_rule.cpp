// The stride rule of a PsDepthSet (putslam_amd/csrc/ps_image_rule.h: depth_set_strides, depth_view_bytes) in a plain C++ program:
// what resolves, to what, and what is rejected -- a frame stride below one view among it.  Prints what fails and returns 1;
// tests/test_frame_assembly_host.py builds and runs it.
#include <cstdint>
#include <cstdio>

#include "ps_image_rule.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s\n", __LINE__, #cond);              \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static PsDepthSet set_of(int frames, int rows, int cols, size_t rowStride, size_t frameStride)
{
    PsDepthSet s;
    s.pixels = nullptr;
    s.rowStride = rowStride;
    s.frameStride = frameStride;
    s.numFrames = frames;
    s.rows = rows;
    s.cols = cols;
    return s;
}

static bool resolves(const PsDepthSet &s, size_t wantRow, size_t wantFrame, size_t wantView)
{
    size_t row = 0, frame = 0, view = 0;
    return depth_set_strides(s, row, frame, view) && row == wantRow && frame == wantFrame && view == wantView;
}

static bool rejected(const PsDepthSet &s)
{
    size_t row = 1, frame = 1, view = 1;
    return !depth_set_strides(s, row, frame, view);
}

int main()
{
    // the view: the last row ends after its pixels
    CHECK(depth_view_bytes(150, 200, 400) == 150 * 400 && depth_view_bytes(150, 200, 410) == 149 * 410 + 400);
    CHECK(depth_view_bytes(1, 1, 2) == 2 && depth_view_bytes(1, 7, 4096) == 14);
    CHECK(depth_view_bytes(0, 200, 400) == 0 && depth_view_bytes(150, 0, 400) == 0 && depth_view_bytes(150, 200, 399) == 0);
    // strides of 0 resolve to dense; a dense frame stride follows the row stride
    CHECK(resolves(set_of(3, 150, 200, 0, 0), 400, 150 * 400, 150 * 400));
    CHECK(resolves(set_of(3, 150, 200, 410, 0), 410, 150 * 410, 149 * 410 + 400));
    // a row stride of a dense row passes, below it is rejected; so is an odd one: the pixels are 16 bits wide
    CHECK(resolves(set_of(3, 150, 200, 400, 0), 400, 150 * 400, 150 * 400));
    CHECK(rejected(set_of(3, 150, 200, 398, 0)) && rejected(set_of(3, 150, 200, 399, 0)) && rejected(set_of(3, 150, 200, 401, 0)));
    // a frame stride of exactly one view passes, below one view it is rejected -- the next frame would begin inside this one
    CHECK(resolves(set_of(3, 150, 200, 410, 149 * 410 + 400), 410, 149 * 410 + 400, 149 * 410 + 400));
    CHECK(rejected(set_of(3, 150, 200, 410, 149 * 410 + 398)));
    CHECK(rejected(set_of(3, 150, 200, 0, 150 * 400 - 2)) && rejected(set_of(3, 150, 200, 0, 2)));
    CHECK(rejected(set_of(3, 150, 200, 0, 150 * 400 + 1)));                       // odd
    CHECK(resolves(set_of(3, 150, 200, 410, 160 * 410 + 6), 410, 160 * 410 + 6, 149 * 410 + 400)); // padding rows and bytes
    // ... for a single frame and for none too
    CHECK(rejected(set_of(1, 150, 200, 0, 150 * 400 - 2)) && rejected(set_of(0, 150, 200, 0, 150 * 400 - 2)));
    // rows or cols below 1 or above the limit
    CHECK(rejected(set_of(3, 0, 200, 0, 0)) && rejected(set_of(3, -1, 200, 0, 0)) && rejected(set_of(3, 150, 0, 0, 0)) &&
          rejected(set_of(3, 150, -4, 0, 0)));
    CHECK(rejected(set_of(3, kImageMaxDim + 1, 200, 0, 0)) && rejected(set_of(3, 150, kImageMaxDim + 1, 0, 0)));
    // the largest image with rows 2^31 bytes apart: nothing wraps
    const size_t big = (size_t)1 << 31;
    CHECK(resolves(set_of(2, kImageMaxDim, kImageMaxDim, big, 0), big, (size_t)kImageMaxDim * big, 8191 * big + 2 * 8192));
    CHECK(rejected(set_of(2, kImageMaxDim, kImageMaxDim, big, 8191 * big + 2 * 8192 - 2)));
    // a rejected set leaves nothing half resolved
    size_t row = 7, frame = 7, view = 7;
    CHECK(!depth_set_strides(set_of(3, 150, 200, 398, 0), row, frame, view) && view == 0);
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("depth rule ok\n");
    return failures ? 1 : 0;
}
