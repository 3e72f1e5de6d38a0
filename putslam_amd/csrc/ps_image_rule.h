// ps_image_rule.h -- the arithmetic of the image front end's host side (ps_klt.h, ps_fast.h, ps_orb.h), each rule once: the limits,
// the row stride and the addressable bytes of a host image, the strides of a PsImageSet and of a PsDepthSet (ps_frame_assembly.h), the
// layout of a host form's device block.
// Pure -- no HIP header, no runtime call: tests/cpp/test_image_rule.cpp includes it into a plain C++ program.
#pragma once
#include <cstddef>
#include <cstdint>

#include "putslam_hip.h"

// rows / cols: a packed (y << 16 | x) holds both; a plane's index and a padded KLT level's element count stay far inside an int
constexpr int kImageMaxDim = 8192;
constexpr int kImageMaxFrames = 65535; // frames of a call, slots of a set: a grid dimension of the launches over them

// THE ROW STRIDE of a host image (rows `rowStride` bytes apart, a row itself dense), resolved: 0 means dense.  Returns 0 for what
// the calls reject: cols or channels < 1, a stride below a dense row.
inline size_t image_row_stride(int cols, int channels, size_t rowStride)
{
    if (cols < 1 || channels < 1) return 0;
    const size_t dense = (size_t)cols * channels;
    if (rowStride == 0) return dense;
    return rowStride < dense ? 0 : rowStride;
}

// THE ADDRESSABLE BYTES of one host image (depth_view_bytes below for 8-bit channels): the last row ends after its pixels,
// not after a whole stride.  The uploads copy this many bytes and the kernels read no further.  0 for a shape the calls reject.
inline size_t image_bytes(int rows, int cols, int channels, size_t rowStride)
{
    const size_t row = image_row_stride(cols, channels, rowStride);
    if (rows < 1 || row == 0) return 0;
    return (size_t)(rows - 1) * row + (size_t)cols * channels;
}

// THE STRIDE RULE of a PsImageSet (include/putslam_hip.h), resolved: a rowStride of 0 is a dense row, a frameStride of 0 is rows x
// rowStride; rowStride is at least a dense row and frameStride at least the addressable bytes of a frame -- of a single frame
// too.  false for a set the calls reject.
inline bool image_set_strides(const PsImageSet &s, size_t &row, size_t &frame)
{
    row = image_row_stride(s.cols, s.channels, s.rowStride);
    if (s.rows < 1 || row == 0) return false;
    frame = s.frameStride ? s.frameStride : (size_t)s.rows * row;
    return frame >= image_bytes(s.rows, s.cols, s.channels, row);
}

// THE ADDRESSABLE BYTES of a rows x cols image of 16-bit pixels whose rows lie `step` bytes apart (a cv::Mat, possibly a
// region of a larger one): the last row ends after its cols pixels, not after a whole pitch -- what follows them belongs to
// the parent image or to nobody.  The upload of ps_keypoints2Dto3D copies this many bytes and its kernel reads no further.
// 0 for a shape the call rejects (rows or cols < 1, step below a row).
inline size_t depth_view_bytes(int rows, int cols, size_t step)
{
    if (rows < 1 || cols < 1 || step < (size_t)cols * 2) return 0;
    return (size_t)(rows - 1) * step + (size_t)cols * 2;
}

// THE STRIDE RULE of a PsDepthSet (image_set_strides for 16-bit pixels), resolved: a rowStride of 0 is a dense row, a frameStride
// of 0 is rows x rowStride; both even (the pixels are uint16), rowStride at least a dense row, frameStride at least one view --
// depth_view_bytes, `view` -- of a single frame too.  false for a set the calls reject.
inline bool depth_set_strides(const PsDepthSet &s, size_t &row, size_t &frame, size_t &view)
{
    row = frame = view = 0;
    if (s.rows < 1 || s.cols < 1 || s.rows > kImageMaxDim || s.cols > kImageMaxDim) return false;
    row = s.rowStride ? s.rowStride : (size_t)s.cols * 2;
    view = depth_view_bytes(s.rows, s.cols, row);
    if (view == 0 || (row & 1) != 0) return false;
    frame = s.frameStride ? s.frameStride : (size_t)s.rows * row;
    return (frame & 1) == 0 && frame >= view;
}

// Consecutive regions of ONE allocation: take<T>(count) is the offset of `count` elements of T, aligned to what T needs (or to
// `align`, a power of two, where the caller wants more); `total` covers everything handed out so far.
struct BlockLayout {
    size_t total = 0;
    template <class T> size_t take(size_t count, size_t align = alignof(T))
    {
        const size_t at = (total + align - 1) & ~(align - 1);
        total = at + count * sizeof(T);
        return at;
    }
};
