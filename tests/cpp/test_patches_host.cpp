// test_patches_host.cpp -- ps_patches_host.h (the sequential C++ restatement of MatchingOnPatches) on cases a test wrote, for
// tests/test_patches_ref_host.py to hold to tests/patches_ref.py byte for byte.  A plain program: no HIP, no library; built
// with -ffp-contract=off and, once, under the address and undefined-behaviour sanitizers.
//
//   test_patches_host <cases.bin> <results.bin>
// cases.bin:   int32 rows, cols, channels, step, patchSize, maxIter, n, 0; double minSqrtIncrement; old image (rows x step
//              bytes); new image; n x (oldX, oldY, newX, newY) doubles
// results.bin: per point int32 status, iterations; double x, y; E doubles patch; E floats gx; E floats gy; 9 floats inverse
//              Hessian (zeros for a point without a model)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "putslam_hip.h"
#include "ps_patches_host.h"

static bool read_all(FILE *f, void *to, size_t bytes) { return bytes == 0 || fread(to, 1, bytes, f) == bytes; }

int main(int argc, char **argv)
{
    if (argc != 3) return fprintf(stderr, "usage: test_patches_host cases.bin results.bin\n"), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    int32_t head[8];
    double minInc = 0.0;
    if (!read_all(f, head, sizeof head) || !read_all(f, &minInc, 8)) return fprintf(stderr, "short header\n"), 2;
    const int rows = head[0], cols = head[1], cn = head[2], step = head[3], n = head[6];
    PsPatchParams prm{};
    prm.minSqrtIncrement = minInc;
    prm.patchSize = head[4];
    prm.maxIter = head[5];
    if (const char *why = patch_params_error(&prm)) return fprintf(stderr, "%s\n", why), 2;
    if (rows < 1 || cols < 1 || (cn != 1 && cn != 3) || step < cols * cn || n < 0) return fprintf(stderr, "bad shape\n"), 2;
    std::vector<uint8_t> oldImg((size_t)rows * step), newImg((size_t)rows * step);
    std::vector<double> pts((size_t)n * 4);
    if (!read_all(f, oldImg.data(), oldImg.size()) || !read_all(f, newImg.data(), newImg.size()) || !read_all(f, pts.data(), pts.size() * 8))
        return fprintf(stderr, "short file\n"), 2;
    fclose(f);
    const patch_host::Image io{oldImg.data(), (size_t)step, rows, cols, cn}, in{newImg.data(), (size_t)step, rows, cols, cn};
    const size_t E = (size_t)patch_elems(prm.patchSize);
    std::vector<double> patch(E), scratch(E);
    std::vector<float> gx(E), gy(E);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return perror(argv[2]), 2;
    for (int k = 0; k < n; ++k) {
        float inv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        std::fill(patch.begin(), patch.end(), 0.0);
        std::fill(gx.begin(), gx.end(), 0.f);
        std::fill(gy.begin(), gy.end(), 0.f);
        double x = pts[4 * k + 2], y = pts[4 * k + 3];
        int iterations = 0;
        const int32_t st[2] = {patch_host::align(io, in, pts[4 * k], pts[4 * k + 1], prm, x, y, iterations, patch.data(), scratch.data(),
                                                 gx.data(), gy.data(), inv),
                               0};
        const int32_t rec[2] = {st[0], iterations};
        const double xy[2] = {x, y};
        fwrite(rec, 4, 2, o);
        fwrite(xy, 8, 2, o);
        fwrite(patch.data(), 8, E, o);
        fwrite(gx.data(), 4, E, o);
        fwrite(gy.data(), 4, E, o);
        fwrite(inv, 4, 9, o);
    }
    if (fclose(o) != 0) return perror(argv[2]), 2;
    printf("patches host ok: %d points\n", n);
    return 0;
}
