// klt_host_loop.cpp -- a single-thread C++ restatement of the tracker's specification (tests/klt_ref.py):
// both pyramids with their borders, the Scharr derivatives of the previous image, the per-point walk over the levels and
// performTracking's selection.  The host loop profiles/scripts/klt_times.py times ps_perform_tracking against (g++ -O2
// -ffp-contract=off, no -march: scalar SSE2, no FMA); the two must return the same bytes.  A restatement, not OpenCV compiled.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

int reflect101(int i, int n)
{
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

struct Level {
    int rows = 0, cols = 0, es = 0; // es: elements of a stored row, (cols + 2W) * cn
    std::vector<uint8_t> img;       // (rows + 2W) x es
    std::vector<int16_t> dx, dy;    // the same elements
};

void pad_level(Level &l, const uint8_t *src, size_t step, int cn, int W)
{
    l.es = (l.cols + 2 * W) * cn;
    l.img.resize((size_t)(l.rows + 2 * W) * l.es);
    for (int y = -W; y < l.rows + W; ++y)
        for (int x = -W; x < l.cols + W; ++x)
            for (int c = 0; c < cn; ++c)
                l.img[(size_t)(y + W) * l.es + (x + W) * cn + c] = src[(size_t)reflect101(y, l.rows) * step + reflect101(x, l.cols) * cn + c];
}

void pyr_down(const Level &s, Level &d, int cn, int W)
{
    static const int k[5] = {1, 4, 6, 4, 1};
    d.rows = (s.rows + 1) / 2;
    d.cols = (s.cols + 1) / 2;
    std::vector<uint8_t> plain((size_t)d.rows * d.cols * cn);
    for (int y = 0; y < d.rows; ++y)
        for (int x = 0; x < d.cols; ++x)
            for (int c = 0; c < cn; ++c) {
                int sum = 0;
                for (int j = 0; j < 5; ++j)
                    for (int i = 0; i < 5; ++i) sum += k[j] * k[i] * s.img[(size_t)(2 * y - 2 + j + W) * s.es + (2 * x - 2 + i + W) * cn + c];
                plain[((size_t)y * d.cols + x) * cn + c] = (uint8_t)((sum + 128) >> 8);
            }
    pad_level(d, plain.data(), (size_t)d.cols * cn, cn, W);
}

void scharr(Level &l, int cn, int W)
{
    l.dx.assign(l.img.size(), 0);
    l.dy.assign(l.img.size(), 0);
    const int es = l.es;
    for (int y = 0; y < l.rows; ++y)
        for (int x = 0; x < l.cols * cn; ++x) {
            const size_t at = (size_t)(y + W) * es + W * cn + x;
            const uint8_t *p = &l.img[at];
            l.dx[at] = (int16_t)(3 * (p[-es + cn] - p[-es - cn]) + 10 * (p[cn] - p[-cn]) + 3 * (p[es + cn] - p[es - cn]));
            l.dy[at] = (int16_t)(3 * (p[es - cn] - p[-es - cn]) + 10 * (p[es] - p[-es]) + 3 * (p[es + cn] - p[-es + cn]));
        }
}

void build(std::vector<Level> &pyr, const uint8_t *img, int rows, int cols, int cn, size_t step, int W, int maxLevels, bool deriv)
{
    pyr.clear();
    pyr.emplace_back();
    pyr[0].rows = rows;
    pyr[0].cols = cols;
    pad_level(pyr[0], img, step, cn, W);
    for (int l = 0; l < maxLevels; ++l) {
        const int r = (pyr[l].rows + 1) / 2, c = (pyr[l].cols + 1) / 2;
        if (r <= W || c <= W) break;
        pyr.emplace_back();
        pyr_down(pyr[l], pyr[l + 1], cn, W);
    }
    if (deriv)
        for (Level &l : pyr) scharr(l, cn, W);
}

bool inside(float fx, float fy, int W, int cols, int rows) { return fx >= (float)-W && fx < (float)cols && fy >= (float)-W && fy < (float)rows; }

struct Wt {
    int w00, w01, w10, w11;
};
Wt weights(float a, float b)
{
    Wt k;
    k.w00 = (int)std::nearbyintf((1.f - a) * (1.f - b) * 16384.f);
    k.w01 = (int)std::nearbyintf(a * (1.f - b) * 16384.f);
    k.w10 = (int)std::nearbyintf((1.f - a) * b * 16384.f);
    k.w11 = 16384 - k.w00 - k.w01 - k.w10;
    return k;
}
template <class T> int tap(const T *p, int es, int cn, const Wt &k, int shift)
{
    const int v = (int)p[0] * k.w00 + (int)p[cn] * k.w01 + (int)p[es] * k.w10 + (int)p[es + cn] * k.w11;
    return (v + (1 << (shift - 1))) >> shift;
}

} // namespace

extern "C" {

// cv::calcOpticalFlowPyrLK on one pair; flags: 4 = use initial flow, 8 = minimal eigenvalue as the error
int klt_track_host(const uint8_t *prevImg, const uint8_t *nextImg, int rows, int cols, int cn, size_t step, const float *prevPts,
                   float *nextPts, int n, uint8_t *status, float *err, int W, int maxLevels, int maxCount, double eps, int flags,
                   double minEigThreshold)
{
    if (rows <= W || cols <= W) return -1;
    std::vector<Level> P, N;
    build(P, prevImg, rows, cols, cn, step, W, maxLevels, true);
    build(N, nextImg, rows, cols, cn, step, W, maxLevels, false);
    const int L = (int)P.size() - 1, Wcn = W * cn, wn = W * Wcn;
    maxCount = maxCount < 0 ? 0 : (maxCount > 100 ? 100 : maxCount);
    eps = !(eps > 0.0) ? 0.0 : (eps > 10.0 ? 10.0 : eps);
    const double eps2 = eps * eps;
    const float half = (float)(W - 1) * 0.5f, scale = 1.f / (float)(1 << 20), errScale = 1.f / (float)(32 * W * cn * W);
    std::vector<int16_t> I((size_t)wn), Ix((size_t)wn), Iy((size_t)wn);
    for (int i = 0; i < n; ++i) {
        float npx = (flags & 4) ? nextPts[2 * i] : 0.f, npy = (flags & 4) ? nextPts[2 * i + 1] : 0.f;
        int st = 1;
        float er = 0.f;
        for (int level = L; level >= 0; --level) {
            const Level &lp = P[level], &ln = N[level];
            const int es = lp.es;
            const float sc = (float)(1.0 / (1 << level));
            float px = prevPts[2 * i] * sc, py = prevPts[2 * i + 1] * sc, nx, ny;
            if (level == L) {
                nx = (flags & 4) ? npx * sc : px;
                ny = (flags & 4) ? npy * sc : py;
            } else {
                nx = npx * 2.f;
                ny = npy * 2.f;
            }
            npx = nx;
            npy = ny;
            px -= half;
            py -= half;
            float fx = std::floor(px), fy = std::floor(py);
            if (!inside(fx, fy, W, lp.cols, lp.rows)) {
                if (level == 0) st = 0, er = 0.f;
                continue;
            }
            Wt k = weights(px - fx, py - fy);
            size_t at = (size_t)((int)fy + W) * es + ((int)fx + W) * cn;
            float A11 = 0.f, A12 = 0.f, A22 = 0.f;
            for (int y = 0, e = 0; y < W; ++y)
                for (int x = 0; x < Wcn; ++x, ++e) {
                    const size_t o = at + (size_t)y * es + x;
                    I[e] = (int16_t)tap(&lp.img[o], es, cn, k, 9);
                    const int ix = tap(&lp.dx[o], es, cn, k, 14), iy = tap(&lp.dy[o], es, cn, k, 14);
                    Ix[e] = (int16_t)ix;
                    Iy[e] = (int16_t)iy;
                    A11 += (float)(ix * ix);
                    A12 += (float)(ix * iy);
                    A22 += (float)(iy * iy);
                }
            A11 *= scale;
            A12 *= scale;
            A22 *= scale;
            float D = A11 * A22 - A12 * A12;
            const float dd = A11 - A22;
            const float minEig = ((A22 + A11) - std::sqrt(dd * dd + 4.f * A12 * A12)) / (float)(2 * W * W);
            if (flags & 8) er = minEig;
            if ((double)minEig < minEigThreshold || D < FLT_EPSILON) {
                if (level == 0) st = 0;
                continue;
            }
            D = 1.f / D;
            nx -= half;
            ny -= half;
            float pdx = 0.f, pdy = 0.f;
            for (int j = 0; j < maxCount; ++j) {
                fx = std::floor(nx);
                fy = std::floor(ny);
                if (!inside(fx, fy, W, lp.cols, lp.rows)) {
                    if (level == 0) st = 0;
                    break;
                }
                k = weights(nx - fx, ny - fy);
                at = (size_t)((int)fy + W) * es + ((int)fx + W) * cn;
                float b1 = 0.f, b2 = 0.f;
                for (int y = 0, e = 0; y < W; ++y)
                    for (int x = 0; x < Wcn; ++x, ++e) {
                        const int diff = tap(&ln.img[at + (size_t)y * es + x], es, cn, k, 9) - I[e];
                        b1 += (float)(diff * Ix[e]);
                        b2 += (float)(diff * Iy[e]);
                    }
                b1 *= scale;
                b2 *= scale;
                const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
                nx += dx;
                ny += dy;
                npx = nx + half;
                npy = ny + half;
                if ((double)dx * dx + (double)dy * dy <= eps2) break;
                if (j > 0 && std::fabs(dx + pdx) < 0.01 && std::fabs(dy + pdy) < 0.01) {
                    npx -= dx * 0.5f;
                    npy -= dy * 0.5f;
                    break;
                }
                pdx = dx;
                pdy = dy;
            }
            if (level == 0 && st && !(flags & 8)) {
                const float qx = npx - half, qy = npy - half;
                fx = std::floor(qx);
                fy = std::floor(qy);
                if (!inside(fx, fy, W, lp.cols, lp.rows)) {
                    st = 0;
                    continue;
                }
                k = weights(qx - fx, qy - fy);
                at = (size_t)((int)fy + W) * es + ((int)fx + W) * cn;
                float s = 0.f;
                for (int y = 0, e = 0; y < W; ++y)
                    for (int x = 0; x < Wcn; ++x, ++e) s += std::fabs((float)(tap(&ln.img[at + (size_t)y * es + x], es, cn, k, 9) - I[e]));
                er = s * errScale;
            }
        }
        nextPts[2 * i] = npx;
        nextPts[2 * i + 1] = npy;
        status[i] = (uint8_t)st;
        err[i] = er;
    }
    return 0;
}

// performTracking's selection as the reference writes it (a flag per feature instead of the std::set); returns the survivors
int klt_select_host(const float *pts, const uint8_t *status, const float *err, int n, double errThr, double minDist, int32_t *keptIdx)
{
    std::vector<uint8_t> marked((size_t)n, 0);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const float dx = pts[2 * i] - pts[2 * j], dy = pts[2 * i + 1] - pts[2 * j + 1];
            if (std::sqrt((double)dx * dx + (double)dy * dy) < minDist) marked[(size_t)(err[i] > err[j] ? i : j)] = 1;
        }
    int k = 0;
    for (int i = 0; i < n; ++i)
        if (status[i] != 0 && !((double)err[i] > errThr) && !marked[(size_t)i]) keptIdx[k++] = i;
    return k;
}

} // extern "C"
