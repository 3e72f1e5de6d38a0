// The pure host rules of the image front end (putslam_amd/csrc/ps_image_rule.h) in a plain C++ program: the strides of a
// PsImageSet, the row stride and the addressable bytes of a host image, the limits, and the block layout with the element
// sizes of ps_klt.h's host block.  Prints what fails and returns 1; tests/test_image_rule_host.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ps_image_rule.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s\n", __LINE__, #cond);              \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static PsImageSet set_of(int frames, int rows, int cols, int cn, size_t rowStride, size_t frameStride)
{
    PsImageSet s;
    s.pixels = nullptr;
    s.rowStride = rowStride;
    s.frameStride = frameStride;
    s.numFrames = frames;
    s.rows = rows;
    s.cols = cols;
    s.channels = cn;
    return s;
}

static bool resolves(const PsImageSet &s, size_t wantRow, size_t wantFrame)
{
    size_t row = 0, frame = 0;
    return image_set_strides(s, row, frame) && row == wantRow && frame == wantFrame;
}

static bool rejected(const PsImageSet &s)
{
    size_t row = 0, frame = 0;
    return !image_set_strides(s, row, frame);
}

static void stride_rule()
{
    // strides of 0 resolve to dense
    CHECK(resolves(set_of(2, 48, 64, 1, 0, 0), 64, 48 * 64));
    CHECK(resolves(set_of(2, 48, 64, 3, 0, 0), 192, 48 * 192));
    CHECK(resolves(set_of(2, 48, 64, 3, 200, 0), 200, 48 * 200)); // a dense frame stride follows the row stride
    // a row stride equal to a dense row passes, one byte less is rejected
    CHECK(resolves(set_of(2, 48, 64, 1, 64, 0), 64, 48 * 64));
    CHECK(rejected(set_of(2, 48, 64, 1, 63, 0)));
    CHECK(resolves(set_of(2, 48, 64, 3, 192, 0), 192, 48 * 192));
    CHECK(rejected(set_of(2, 48, 64, 3, 191, 0)));
    // a frame stride equal to (rows - 1) * row + dense passes, one byte less is rejected
    CHECK(resolves(set_of(2, 48, 64, 1, 0, 48 * 64), 64, 48 * 64));
    CHECK(rejected(set_of(2, 48, 64, 1, 0, 48 * 64 - 1)));
    CHECK(resolves(set_of(2, 48, 64, 3, 200, 47 * 200 + 192), 200, 47 * 200 + 192));
    CHECK(rejected(set_of(2, 48, 64, 3, 200, 47 * 200 + 191)));
    // ... even for a single frame, and for none
    CHECK(rejected(set_of(1, 48, 64, 1, 0, 48 * 64 - 1)));
    CHECK(rejected(set_of(1, 48, 64, 1, 0, 1)));
    CHECK(rejected(set_of(0, 48, 64, 1, 0, 48 * 64 - 1)));
    // rows, cols or channels below 1
    CHECK(rejected(set_of(2, 0, 64, 1, 0, 0)) && rejected(set_of(2, -1, 64, 1, 0, 0)));
    CHECK(rejected(set_of(2, 48, 0, 1, 0, 0)) && rejected(set_of(2, 48, -5, 1, 0, 0)));
    CHECK(rejected(set_of(2, 48, 64, 0, 0, 0)) && rejected(set_of(2, 48, 64, -3, 0, 0)));
    CHECK(rejected(set_of(2, 0, 0, 0, 1 << 20, 1 << 30)));
    // the largest image with rows 2^31 bytes apart: nothing wraps
    const size_t big = (size_t)1 << 31, dense = (size_t)kImageMaxDim * 3;
    CHECK(resolves(set_of(2, kImageMaxDim, kImageMaxDim, 3, big, 0), big, (size_t)kImageMaxDim * big));
    CHECK((size_t)kImageMaxDim * big == (size_t)1 << 44);
    CHECK(resolves(set_of(2, kImageMaxDim, kImageMaxDim, 3, big, 8191 * big + dense), big, 8191 * big + dense));
    CHECK(rejected(set_of(2, kImageMaxDim, kImageMaxDim, 3, big, 8191 * big + dense - 1)));
}

static void host_image()
{
    CHECK(kImageMaxDim == 8192 && kImageMaxFrames == 65535);
    // the row stride: 0 means dense, a stride below a dense row is rejected
    CHECK(image_row_stride(64, 1, 0) == 64 && image_row_stride(64, 3, 0) == 192);
    CHECK(image_row_stride(64, 3, 192) == 192 && image_row_stride(64, 3, 1000) == 1000 && image_row_stride(64, 3, 191) == 0);
    CHECK(image_row_stride(0, 1, 0) == 0 && image_row_stride(64, 0, 0) == 0 && image_row_stride(-1, 1, 64) == 0);
    // the bytes: (rows - 1) * rowStride + cols * channels, 0 for what the rule rejects
    const int shapes[][4] = {{48, 64, 1, 0}, {48, 64, 3, 0}, {48, 64, 1, 73}, {48, 64, 3, 219}, {1, 1, 1, 0}, {1, 40, 3, 4096}, {40, 1, 1, 1280}};
    for (const auto &s : shapes) {
        const size_t dense = (size_t)s[1] * s[2], row = s[3] ? (size_t)s[3] : dense;
        CHECK(image_bytes(s[0], s[1], s[2], (size_t)s[3]) == (size_t)(s[0] - 1) * row + dense);
    }
    CHECK(image_bytes(48, 64, 1, 64) == 48 * 64 && image_bytes(48, 64, 1, 73) == 47 * 73 + 64);
    CHECK(image_bytes(0, 64, 1, 0) == 0 && image_bytes(48, 0, 1, 0) == 0 && image_bytes(48, 64, 0, 0) == 0 && image_bytes(-2, 64, 1, 0) == 0);
    CHECK(image_bytes(48, 64, 1, 63) == 0 && image_bytes(48, 64, 3, 191) == 0);
    const size_t big = (size_t)1 << 31;
    CHECK(image_bytes(kImageMaxDim, kImageMaxDim, 3, big) == 8191 * big + 3 * 8192);
    // a set and a host image agree: a frame stride of exactly the image's bytes is the least that passes
    CHECK(resolves(set_of(3, 37, 53, 3, 170, image_bytes(37, 53, 3, 170)), 170, image_bytes(37, 53, 3, 170)));
}

// stand-ins with the size and alignment of what ps_klt.h lays out: float2 and PsDMatch
struct alignas(8) Float2 {
    float x, y;
};
struct Match {
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;
};
struct Region {
    size_t at, bytes, align;
};

static void block_layout()
{
    static_assert(sizeof(Float2) == 8 && alignof(Float2) == 8 && sizeof(Match) == 16 && alignof(Match) == 4, "stand-ins");
    for (const size_t n : {(size_t)1, (size_t)2, (size_t)7}) {
        for (const size_t imgBytes : {(size_t)(47 * 73 + 64), (size_t)(48 * 64), (size_t)1}) {
            // ps_klt.h's block: two images | pairs[2], count, 0 | prevPts | nextPts | err | numMatches | matches | keptPts | keptIdx | status
            BlockLayout lay;
            std::vector<Region> r;
            r.push_back({lay.take<uint8_t>(imgBytes, 16), imgBytes, 16});
            r.push_back({lay.take<uint8_t>(imgBytes, 16), imgBytes, 16});
            r.push_back({lay.take<int32_t>(4, 16), 16, 16});
            r.push_back({lay.take<Float2>(n), n * 8, 8});
            r.push_back({lay.take<Float2>(n), n * 8, 8});
            r.push_back({lay.take<float>(n), n * 4, 4});
            r.push_back({lay.take<int32_t>(1), 4, 4});
            r.push_back({lay.take<Match>(n, 8), n * 16, 8});
            r.push_back({lay.take<Float2>(n), n * 8, 8});
            r.push_back({lay.take<int32_t>(n), n * 4, 4});
            r.push_back({lay.take<uint8_t>(n), n, 1});
            CHECK(r[0].at == 0);
            for (size_t i = 0; i < r.size(); ++i) {
                CHECK(r[i].at % r[i].align == 0);                                  // aligned as asked
                if (i > 0) CHECK(r[i].at >= r[i - 1].at + r[i - 1].bytes);         // no overlap with the region before
                if (i > 0) CHECK(r[i].at < r[i - 1].at + r[i - 1].bytes + r[i].align); // and no more padding than the alignment needs
            }
            CHECK(lay.total == r.back().at + r.back().bytes); // the total covers the last region
        }
    }
    BlockLayout empty;
    CHECK(empty.total == 0 && empty.take<int32_t>(0) == 0 && empty.total == 0);
    BlockLayout odd;
    CHECK(odd.take<uint8_t>(3) == 0 && odd.take<double>(1) == 8 && odd.total == 16 && odd.take<uint8_t>(1) == 16 && odd.take<int16_t>(2) == 18);
}

int main()
{
    stride_rule();
    host_image();
    block_layout();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("image rule ok\n");
    return failures ? 1 : 0;
}
