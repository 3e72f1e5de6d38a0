// The host loop that ps_detect_features replaces, as a single-thread C++ program: MatcherOpenCV::detectFeatures (reference
// src/Matcher/matcherOpenCV.cpp:118-180) for detector "FAST" by the reading of DESIGN.md section 8.10 -- the grey conversion, the
// grid of ROIs, in each ROI a row loop with a threshold table, quick rejections on the antipodal ring pairs, the run-length test
// over the ring repeated to 25 entries, the score by pairwise min / max, suppression through three row buffers, std::stable_sort
// by response and the two cuts.  A third restatement next to the two of tests/fast_ref.py, written for speed on one core: the
// control profiles/scripts/fast_times.py times the GPU against, after checking that both return the same bytes.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Kp {
    float x, y, response;
};

const int kRing[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3}, {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

int corner_score(const uint8_t *p, const int *pix, int t)
{
    int d[25];
    const int v = p[0];
    for (int k = 0; k < 25; ++k) d[k] = v - (int)p[pix[k]];
    int a0 = t;
    for (int k = 0; k < 16; k += 2) {
        int a = std::min(d[k + 1], d[k + 2]);
        a = std::min(a, d[k + 3]);
        if (a <= a0) continue;
        a = std::min(a, d[k + 4]);
        a = std::min(a, d[k + 5]);
        a = std::min(a, d[k + 6]);
        a = std::min(a, d[k + 7]);
        a = std::min(a, d[k + 8]);
        a0 = std::max(a0, std::min(a, d[k]));
        a0 = std::max(a0, std::min(a, d[k + 9]));
    }
    int b0 = -a0;
    for (int k = 0; k < 16; k += 2) {
        int b = std::max(d[k + 1], d[k + 2]);
        b = std::max(b, d[k + 3]);
        b = std::max(b, d[k + 4]);
        b = std::max(b, d[k + 5]);
        if (b >= b0) continue;
        b = std::max(b, d[k + 6]);
        b = std::max(b, d[k + 7]);
        b = std::max(b, d[k + 8]);
        b0 = std::min(b0, std::max(b, d[k]));
        b0 = std::min(b0, std::max(b, d[k + 9]));
    }
    return -b0 - 1;
}

void fast_roi(const uint8_t *img, int step, int rows, int cols, int t, bool nms, std::vector<Kp> &out)
{
    out.clear();
    if (rows < 7 || cols < 7) return;
    int pix[25];
    for (int k = 0; k < 25; ++k) pix[k] = kRing[k & 15][1] * step + kRing[k & 15][0];
    uint8_t tab[512];
    for (int i = -255; i <= 255; ++i) tab[i + 255] = (uint8_t)(i < -t ? 1 : (i > t ? 2 : 0));
    std::vector<uint8_t> buf((size_t)cols * 3, 0);
    std::vector<int> cpbuf((size_t)(cols + 1) * 3, 0);
    for (int i = 3; i < rows - 2; ++i) {
        const uint8_t *ptr = img + (size_t)i * step + 3;
        uint8_t *curr = buf.data() + (size_t)((i - 3) % 3) * cols;
        int *cornerpos = cpbuf.data() + (size_t)((i - 3) % 3) * (cols + 1);
        std::memset(curr, 0, (size_t)cols);
        int ncorners = 0;
        if (i < rows - 3) {
            for (int j = 3; j < cols - 3; ++j, ++ptr) {
                const int v = ptr[0];
                const uint8_t *tb = tab + 255 - v;
                int d = tb[ptr[pix[0]]] | tb[ptr[pix[8]]];
                if (d == 0) continue;
                d &= tb[ptr[pix[2]]] | tb[ptr[pix[10]]];
                d &= tb[ptr[pix[4]]] | tb[ptr[pix[12]]];
                d &= tb[ptr[pix[6]]] | tb[ptr[pix[14]]];
                if (d == 0) continue;
                d &= tb[ptr[pix[1]]] | tb[ptr[pix[9]]];
                d &= tb[ptr[pix[3]]] | tb[ptr[pix[11]]];
                d &= tb[ptr[pix[5]]] | tb[ptr[pix[13]]];
                d &= tb[ptr[pix[7]]] | tb[ptr[pix[15]]];
                bool found = false;
                if (d & 1) {
                    const int vt = v - t;
                    for (int k = 0, count = 0; k < 25; ++k) {
                        if ((int)ptr[pix[k]] < vt) {
                            if (++count > 8) {
                                found = true;
                                break;
                            }
                        } else
                            count = 0;
                    }
                }
                if ((d & 2) && !found) {
                    const int vt = v + t;
                    for (int k = 0, count = 0; k < 25; ++k) {
                        if ((int)ptr[pix[k]] > vt) {
                            if (++count > 8) {
                                found = true;
                                break;
                            }
                        } else
                            count = 0;
                    }
                }
                if (found) {
                    cornerpos[ncorners++] = j;
                    if (nms) curr[j] = (uint8_t)corner_score(ptr, pix, t);
                }
            }
        }
        cornerpos[cols] = ncorners; // (the count rides behind the positions)
        if (i == 3) continue;
        const uint8_t *prev = buf.data() + (size_t)((i - 4) % 3) * cols, *pprev = buf.data() + (size_t)((i - 5 + 3) % 3) * cols;
        const int *cp = cpbuf.data() + (size_t)((i - 4) % 3) * (cols + 1);
        for (int k = 0, n = cp[cols]; k < n; ++k) {
            const int j = cp[k], s = prev[j];
            if (!nms || (s > prev[j + 1] && s > prev[j - 1] && s > pprev[j - 1] && s > pprev[j] && s > pprev[j + 1] && s > curr[j - 1] &&
                         s > curr[j] && s > curr[j + 1]))
                out.push_back(Kp{(float)j, (float)(i - 1), (float)s});
        }
    }
}

bool by_response(const Kp &a, const Kp &b) { return a.response > b.response; }

} // namespace

// img rows x cols x cn bytes, rowStride bytes between rows; xy / response have room for maxFeatures entries.  Returns the count.
extern "C" int fast_detect_host(const uint8_t *img, int rows, int cols, int cn, size_t rowStride, int threshold, int nms, int gridRows,
                                int gridCols, int maxFeatures, float *xy, float *response)
{
    const int t = threshold < 0 ? 0 : (threshold > 255 ? 255 : threshold);
    std::vector<uint8_t> gray((size_t)rows * cols);
    for (int y = 0; y < rows; ++y) {
        const uint8_t *p = img + (size_t)y * rowStride;
        uint8_t *g = gray.data() + (size_t)y * cols;
        if (cn == 1)
            std::memcpy(g, p, (size_t)cols);
        else
            for (int x = 0; x < cols; ++x, p += 3) g[x] = (uint8_t)((p[0] * 4899 + p[1] * 9617 + p[2] * 1868 + 8192) >> 14);
    }
    const int maxInRoi = (int)(3ll * maxFeatures / ((long long)gridCols * gridRows));
    std::vector<Kp> raw, in;
    for (int k = 0; k < gridCols; ++k)
        for (int i = 0; i < gridRows; ++i) {
            const int x0 = k * cols / gridCols, y0 = i * rows / gridRows;
            fast_roi(gray.data() + (size_t)y0 * cols + x0, cols, rows / gridRows, cols / gridCols, t, nms != 0, in);
            std::stable_sort(in.begin(), in.end(), by_response);
            for (size_t j = 0; j < in.size() && (int)j < maxInRoi; ++j) raw.push_back(Kp{in[j].x + (float)x0, in[j].y + (float)y0, in[j].response});
        }
    std::stable_sort(raw.begin(), raw.end(), by_response);
    if ((int)raw.size() > maxFeatures) raw.resize((size_t)maxFeatures);
    for (size_t j = 0; j < raw.size(); ++j) {
        xy[2 * j] = raw[j].x;
        xy[2 * j + 1] = raw[j].y;
        response[j] = raw[j].response;
    }
    return (int)raw.size();
}
