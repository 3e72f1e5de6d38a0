// The pure-host rules of the matching on patches (putslam_amd/csrc/ps_patches_rule.h) in a plain C++ program: the parameter rule,
// the element count and the LDS bytes of a wave, the two tap rules and the reference's gate at their edges, and the image-set
// rule; with a file of positions, the decisions of the three position rules for a test to compare with tests/patches_ref.py.  tests/test_patches_abi_host.py builds it with -fsanitize=address,undefined and runs it on the CPU: no GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "ps_patches_rule.h"

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                             \
        }                                                           \
    } while (0)

// `test_patches_rule <file>`: records of five doubles (x, y, h, rows, cols) -> per record the header's decisions as three digits:
// old taps inside, the gate says out, new taps inside (0 where the gate says out: the rule is defined behind the gate only)
static int decide(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return std::perror(path), 2;
    double r[5];
    while (std::fread(r, 8, 5, f) == 5) {
        const int h = (int)r[2], rows = (int)r[3], cols = (int)r[4];
        const bool out = patch_gate_out(r[0], r[1], h, rows, cols);
        std::printf("%d%d%d\n", (int)patch_old_taps_inside(r[0], r[1], h, rows, cols), (int)out,
                    (int)(!out && patch_new_taps_inside(r[0], r[1], h, rows, cols)));
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2) return decide(argv[1]);
    CHECK(sizeof(PsPatchParams) == 24 && sizeof(PsPatchModel) == 32);

    // the parameter rule
    PsPatchParams p{0.04, 13, 50, 0, 0};
    CHECK(patch_params_error(&p) == nullptr);
    CHECK(patch_params_error(nullptr) != nullptr);
    for (int ps = -3; ps <= 40; ++ps) {
        PsPatchParams q = p;
        q.patchSize = ps;
        CHECK((patch_params_error(&q) == nullptr) == (ps >= 3 && ps <= 31 && (ps & 1)));
    }
    for (int it : {-1, 0, 1, 1000, 1001}) {
        PsPatchParams q = p;
        q.maxIter = it;
        CHECK((patch_params_error(&q) == nullptr) == (it >= 0 && it <= 1000));
    }
    {
        PsPatchParams q = p;
        q.flags = PS_PATCH_GIVEN_MODEL;
        CHECK(patch_params_error(&q) == nullptr);
        q.flags = 2;
        CHECK(patch_params_error(&q) != nullptr);
        q.flags = 0;
        q.reserved = 1;
        CHECK(patch_params_error(&q) != nullptr);
        q.reserved = 0;
        q.minSqrtIncrement = std::nan(""); // (any double: a NaN never stops a point)
        CHECK(patch_params_error(&q) == nullptr);
    }

    // sizes: E, the rows of four, a wave's bytes; every size fits a work-group's 64 KiB at least twice
    CHECK(patch_half(13) == 6 && patch_elems(13) == 169 && patch_elems4(13) == 172);
    CHECK(patch_half(31) == 15 && patch_elems(31) == 961 && patch_elems4(31) == 964 && patch_wave_bytes(31) == 26992);
    for (int ps = 3; ps <= 31; ps += 2) {
        const int w = patch_block_waves(ps);
        CHECK(w >= 2 && w <= 4 && (size_t)w * patch_wave_bytes(ps) <= 65536 && patch_wave_bytes(ps) % 16 == 0);
        CHECK(patch_elems4(ps) >= patch_elems(ps) && patch_elems4(ps) - patch_elems(ps) < 4);
    }
    CHECK(patch_block_waves(3) == 4 && patch_block_waves(21) == 4 && patch_block_waves(31) == 2);

    // the old image's tap rule: 64 x 48, h = 6: x in [7, 57), y in [7, 41)
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const int rows = 48, cols = 64, h = 6;
    CHECK(patch_old_taps_inside(7.0, 7.0, h, rows, cols) && patch_old_taps_inside(56.999, 40.999, h, rows, cols));
    CHECK(!patch_old_taps_inside(std::nextafter(7.0, 0.0), 7.0, h, rows, cols) && !patch_old_taps_inside(7.0, std::nextafter(7.0, 0.0), h, rows, cols));
    CHECK(!patch_old_taps_inside(57.0, 7.0, h, rows, cols) && !patch_old_taps_inside(7.0, 41.0, h, rows, cols));
    CHECK(patch_old_taps_inside(std::nextafter(57.0, 0.0), std::nextafter(41.0, 0.0), h, rows, cols));
    for (double bad : {nan, inf, -inf, 1e300, -1e300, 3e9, -3e9}) {
        CHECK(!patch_old_taps_inside(bad, 20.0, h, rows, cols));
        CHECK(!patch_old_taps_inside(20.0, bad, h, rows, cols));
    }
    // ... every accepted position has its taps inside (the kernel's index rule), every rejected integer one has not
    for (int ps = 3; ps <= 31; ps += 2)
        for (int x = -2; x < cols + 2; ++x) {
            const int hh = patch_half(ps);
            const bool in = x - hh - 1 >= 0 && x + hh + 1 <= cols - 1;
            CHECK(patch_old_taps_inside((double)x, 24.0, hh, 49 + 2 * hh, cols) == in);
            CHECK(patch_old_taps_inside((double)x + 0.75, 24.0, hh, 49 + 2 * hh, cols) == (in && x >= 0));
        }

    // the reference's gate: [h, cols - h] x [h, rows - h], both ends included
    CHECK(!patch_gate_out(6.0, 6.0, h, rows, cols) && !patch_gate_out(58.0, 42.0, h, rows, cols));
    CHECK(patch_gate_out(std::nextafter(6.0, 0.0), 6.0, h, rows, cols) && patch_gate_out(6.0, std::nextafter(6.0, 0.0), h, rows, cols));
    CHECK(patch_gate_out(std::nextafter(58.0, 99.0), 6.0, h, rows, cols) && patch_gate_out(6.0, std::nextafter(42.0, 99.0), h, rows, cols));
    for (double bad : {nan, inf, -inf, 1e300, -1e300}) {
        CHECK(patch_gate_out(bad, 20.0, h, rows, cols));
        CHECK(patch_gate_out(20.0, bad, h, rows, cols));
    }
    // the new image's tap rule inside the gate: int(x) + h + 1 <= cols - 1 iff x < cols - h - 1 = 57
    CHECK(patch_new_taps_inside(6.0, 6.0, h, rows, cols) && patch_new_taps_inside(56.99, 40.99, h, rows, cols));
    CHECK(!patch_new_taps_inside(57.0, 6.0, h, rows, cols) && !patch_new_taps_inside(58.0, 6.0, h, rows, cols));
    CHECK(!patch_new_taps_inside(6.0, 41.0, h, rows, cols) && !patch_new_taps_inside(6.0, 42.0, h, rows, cols));

    // the image-set rule
    size_t row = 0, frame = 0;
    static const uint8_t px[1] = {0};
    PsImageSet s{};
    s.pixels = px;
    s.numFrames = 2;
    s.rows = 48, s.cols = 64, s.channels = 3;
    CHECK(patch_images_error(&s, row, frame) == nullptr && row == 192 && frame == 48 * 192);
    s.rowStride = 200;
    s.frameStride = 47 * 200 + 192;
    CHECK(patch_images_error(&s, row, frame) == nullptr && row == 200 && frame == 47 * 200 + 192);
    s.frameStride -= 1;
    CHECK(patch_images_error(&s, row, frame) != nullptr);
    s.frameStride = 0;
    s.rowStride = 191;
    CHECK(patch_images_error(&s, row, frame) != nullptr);
    s.rowStride = 0;
    for (int cn : {0, 2, 4}) {
        s.channels = cn;
        CHECK(patch_images_error(&s, row, frame) != nullptr);
    }
    s.channels = 1;
    CHECK(patch_images_error(&s, row, frame) == nullptr);
    s.cols = 8193;
    CHECK(patch_images_error(&s, row, frame) != nullptr);
    s.cols = 64;
    s.rows = 8193;
    CHECK(patch_images_error(&s, row, frame) != nullptr);
    s.rows = 0;
    CHECK(patch_images_error(&s, row, frame) != nullptr);
    s.rows = 48;
    s.numFrames = -1;
    CHECK(patch_images_error(&s, row, frame) != nullptr);
    s.numFrames = 1;
    s.pixels = nullptr;
    CHECK(patch_images_error(&s, row, frame) != nullptr);
    s.numFrames = 0;
    CHECK(patch_images_error(&s, row, frame) == nullptr);
    CHECK(patch_images_error(nullptr, row, frame) != nullptr);

    if (failures) return std::printf("%d failure(s)\n", failures), 1;
    std::printf("patches rule ok\n");
    return 0;
}
