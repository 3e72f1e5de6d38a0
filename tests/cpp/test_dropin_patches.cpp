// test_dropin_patches.cpp -- the drop-in's MatchingOnPatches (putslam_dropin.h) against vectors tests/patches_ref.py wrote: the
// reference's three-call protocol (computePatch, computeGradient, optimizeLocation) point by point and the batch form
// optimizeLocations, on cv::Mat-shaped images that are regions of larger ones, byte for byte.  tests/test_gpu_dropin_patches.py
// writes the files and runs it.
//
//   test_dropin_patches --defaults                  the compiled-in PatchesParams as one JSON line; touches no GPU
//   test_dropin_patches <cases.bin> <expected.bin>
// cases.bin:    int32 rows, cols, channels, step, patchSize, maxIter, n, 0; double minSqrtIncrement; old image (rows x step bytes);
//               new image; n x (oldX, oldY, newX, newY) doubles
// expected.bin: per point int32 status, iterations; double x, y; E doubles patch; E floats gx; E floats gy; 9 floats inverse Hessian,
//               row-major (zeros for a point without a model)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "putslam_dropin.h"
#include "putslam_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++failures <= 20) std::printf("FAILED %s:%d: %s (point %d)\n", __FILE__, __LINE__, #cond, point); \
        }                                                                             \
    } while (0)

static bool read_all(FILE *f, void *to, size_t bytes) { return bytes == 0 || fread(to, 1, bytes, f) == bytes; }
static bool same(const void *a, const void *b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

int main(int argc, char **argv)
{
    int point = -1;
    if (argc == 2 && std::strcmp(argv[1], "--defaults") == 0) {
        putslam_hip::FrameMatcher::MatcherParameters p;
        MatchingOnPatches m(p.PatchesParams), d(9);
        std::printf("{\"verbose\": %d, \"warping\": %d, \"patchSize\": %d, \"halfPatchSize\": %d, \"maxIter\": %d, \"minSqrtIncrement\": %.17g, "
                    "\"getPatchSize\": %d, \"getHalfPatchSize\": %d, \"ctorPatchSize\": %d, \"ctorHalfPatchSize\": %d}\n",
                    p.PatchesParams.verbose, (int)p.PatchesParams.warping, p.PatchesParams.patchSize, p.PatchesParams.halfPatchSize,
                    p.PatchesParams.maxIter, p.PatchesParams.minSqrtIncrement, m.getPatchSize(), m.getHalfPatchSize(), d.getPatchSize(),
                    d.getHalfPatchSize());
        return 0;
    }
    if (argc != 3) return std::fprintf(stderr, "usage: test_dropin_patches cases.bin expected.bin | --defaults\n"), 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return std::perror(argv[1]), 2;
    int32_t head[8];
    double minInc = 0.0;
    if (!read_all(f, head, sizeof head) || !read_all(f, &minInc, 8)) return std::fprintf(stderr, "short header\n"), 2;
    const int rows = head[0], cols = head[1], cn = head[2], step = head[3], ps = head[4], maxIter = head[5], n = head[6];
    if (rows < 1 || cols < 1 || (cn != 1 && cn != 3) || step < cols * cn || ps < 1 || ps > 31 || n < 0) return std::fprintf(stderr, "bad shape\n"), 2;
    std::vector<unsigned char> oldBuf((size_t)rows * step), newBuf((size_t)rows * step);
    std::vector<double> pts((size_t)n * 4);
    if (!read_all(f, oldBuf.data(), oldBuf.size()) || !read_all(f, newBuf.data(), newBuf.size()) || !read_all(f, pts.data(), pts.size() * 8))
        return std::fprintf(stderr, "short file\n"), 2;
    std::fclose(f);
    const size_t E = (size_t)ps * ps, rec = 8 + 16 + E * 16 + 36;
    std::vector<unsigned char> want((size_t)n * rec);
    f = std::fopen(argv[2], "rb");
    if (!f || !read_all(f, want.data(), want.size())) return std::fprintf(stderr, "short expectation\n"), 2;
    std::fclose(f);

    const int type = cn == 1 ? CV_8UC1 : CV_8UC3;
    cv::Mat oldImg(rows, cols, type, oldBuf.data(), (size_t)step), newImg(rows, cols, type, newBuf.data(), (size_t)step);
    MatchingOnPatches::parameters prm{0, true, ps, (ps - 1) / 2, maxIter, minInc}; // (warping is carried and read nowhere)
    MatchingOnPatches mop(prm);
    CHECK(mop.getPatchSize() == ps && mop.getHalfPatchSize() == (ps - 1) / 2);

    // the three-call protocol of demos/demoPatches.cpp, point by point
    int converged = 0, noModel = 0;
    for (point = 0; point < n; ++point) {
        const unsigned char *w = want.data() + (size_t)point * rec;
        int32_t st, it;
        std::memcpy(&st, w, 4);
        std::memcpy(&it, w + 4, 4);
        const unsigned char *wxy = w + 8, *wPatch = w + 24, *wGx = wPatch + 8 * E, *wGy = wGx + 4 * E, *wInv = wGy + 4 * E;
        const double ox = pts[4 * point], oy = pts[4 * point + 1];
        double x = pts[4 * point + 2], y = pts[4 * point + 3];
        const double sx = x, sy = y;
        std::vector<double> patch = mop.computePatch(oldImg, ox, oy);
        std::vector<float> gx, gy;
        Eigen::Matrix3f inv = Eigen::Matrix3f::Zero();
        mop.computeGradient(oldImg, ox, oy, inv, gx, gy);
        const bool ok = mop.optimizeLocation(oldImg, patch, newImg, x, y, gx, gy, inv);
        if (st == PS_PATCH_OLD_TAPS_OUTSIDE) { // this build's own outcome: no model, false, the position untouched
            ++noModel;
            CHECK(patch.empty() && gx.empty() && gy.empty() && std::isnan(inv(0, 0)) && !ok);
            CHECK(same(&x, &sx, 8) && same(&y, &sy, 8) && MatchingOnPatches::lastIterations() == 0);
            continue;
        }
        CHECK(patch.size() == E && gx.size() == E && gy.size() == E);
        if (patch.size() != E || gx.size() != E || gy.size() != E) continue;
        CHECK(same(patch.data(), wPatch, 8 * E) && same(gx.data(), wGx, 4 * E) && same(gy.data(), wGy, 4 * E));
        float rowMajor[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) rowMajor[3 * i + j] = inv(i, j);
        CHECK(same(rowMajor, wInv, 36));
        CHECK(ok == (st == PS_PATCH_CONVERGED) && MatchingOnPatches::lastStatus() == st && MatchingOnPatches::lastIterations() == it);
        const double got[2] = {x, y};
        CHECK(same(got, wxy, 16));
        converged += ok;
    }
    point = -1;

    // the batch form: one call for the list
    std::vector<double> oldXY((size_t)2 * n), newXY((size_t)2 * n);
    for (int k = 0; k < n; ++k) {
        oldXY[2 * k] = pts[4 * k], oldXY[2 * k + 1] = pts[4 * k + 1];
        newXY[2 * k] = pts[4 * k + 2], newXY[2 * k + 1] = pts[4 * k + 3];
    }
    std::vector<int> iterations;
    const std::vector<int> status = mop.optimizeLocations(oldImg, newImg, oldXY, newXY, &iterations);
    CHECK((int)status.size() == n && (int)iterations.size() == n);
    for (point = 0; point < n && (int)status.size() == n; ++point) {
        const unsigned char *w = want.data() + (size_t)point * rec;
        int32_t st, it;
        std::memcpy(&st, w, 4);
        std::memcpy(&it, w + 4, 4);
        CHECK(status[point] == st && iterations[point] == it && same(&newXY[2 * point], w + 8, 16));
    }
    point = -1;
    // ... and with images whose steps differ: the same results
    std::vector<unsigned char> dense((size_t)rows * cols * cn);
    for (int r = 0; r < rows; ++r) std::memcpy(dense.data() + (size_t)r * cols * cn, newBuf.data() + (size_t)r * step, (size_t)cols * cn);
    cv::Mat newDense(rows, cols, type, dense.data());
    std::vector<double> again((size_t)2 * n);
    for (int k = 0; k < n; ++k) again[2 * k] = pts[4 * k + 2], again[2 * k + 1] = pts[4 * k + 3];
    const std::vector<int> status2 = mop.optimizeLocations(oldImg, newDense, oldXY, again);
    CHECK(status2 == status && same(again.data(), newXY.data(), again.size() * 8));

    // refusals are loud and change nothing: an even patch, a 16-bit image
    MatchingOnPatches even(12, 50, 0.04);
    std::vector<double> keep = newXY;
    CHECK(even.optimizeLocations(oldImg, newImg, oldXY, keep).empty() && same(keep.data(), newXY.data(), keep.size() * 8)); // (bytes: the list holds NaNs)
    CHECK(even.computePatch(oldImg, 20.0, 20.0).empty());
    cv::Mat deep(rows, cols, CV_16U);
    CHECK(mop.computePatch(deep, 20.0, 20.0).empty());

    if (failures) return std::printf("%d failure(s)\n", failures), 1;
    std::printf("dropin patches ok: %d points, %d converged, %d without a model\n", n, converged, noModel);
    return 0;
}
