// ps_match_l2.h -- cross-check matching of FLOAT descriptors (SURF / SIFT): cv::BFMatcher(cv::NORM_L2, true).match(query = prev,
// train = cur), the matcher MatcherOpenCV builds for those two descriptor settings (reference src/Matcher/matcherOpenCV.cpp:100-102,
// called at :198-206), for a device-resident batch of P frame pairs (ps_match_l2_f32 / ps_match_l2_device /
// ps_vo_pairs_l2_device, include/putslam_hip.h).  The semantics are restated, not compiled:
//
//   L2sqr(a, b)  float, every operation rounded separately, no FMA: eight lane accumulators over the blocks of eight elements
//                (acc0[i] += (a[j+i] - b[j+i])^2, acc1[i] += (a[j+4+i] - b[j+4+i])^2), d = ((s0 + s1) + s2) + s3 with
//                s[i] = acc0[i] + acc1[i]; then blocks of four, d += ((t0^2 + t1^2) + t2^2) + t3^2; then single elements.
//   dist         sqrtf(L2sqr), correctly rounded.  Every comparison is made on dist: different sums may share a root.
//   step 1       train row t -> the query q with the least dist < FLT_MAX, ties to the lowest q (NaN / inf never chosen).
//   step 2       query q -> the train row with the least dist among those that chose it, ties to the lowest t.
//   step 3       DMatch(q, t, 0, dist) in ascending q.
//
//   ps_l2_nn<DV>        step 1, value-exact.  One lane = one train row, the query rows are wave-uniform (scalar loads); DV = 64 /
//                       128 keeps the train row in registers, DV = 0 is any dim, the row read from memory.  grid P x tiles x
//                       qsplit: the query range may be split over work-groups, every split writes ITS key per train row --
//                       (dist bits << 32) | q, whose unsigned order is (dist, q) since dist >= +0 -- and the cross-check takes
//                       the minimum of a row's keys: no atomic between work-groups.
//   ps_l2_crosscheck    steps 2 and 3, one work-group per pair: best[q] in LDS (8 bytes a query) by ds_min_u64 on
//                       (dist bits << 32) | t -- a minimum, not an order --, the ordered compaction and, in the VO form, the depth
//                       filter and the scoring records exactly as ps_crosscheck_prep writes them (write_records).
//   ps_l2_prepare / ps_l2_mfma<D> / ps_l2_refine   dim 64 / 128, option "matcher_l2" = 1 (default): step 1 with a matrix-core
//                       prefilter in front of the value-exact code (described with its error band further down); the same keys.
#pragma once
#include "ps_glue.h"
#include "ps_match_stage.h"
#include "ps_ransac_stage.h"
#include "ps_map_match.h"
#include "ps_matcher_mfma.h"

namespace psdev {

constexpr unsigned long long kNoKeyL2 = ~0ull;
constexpr uint32_t kFltMaxBits = 0x7F7FFFFFu; // dist < FLT_MAX  <=>  bits(dist) < this, for dist >= +0 or NaN
constexpr int kL2MaxQsplit = 64;

struct L2Args {
    const float *desc;        // the frame set's descriptors
    const int32_t *nkpts;
    const int32_t *pairs;     // P x (query = previous frame, train = current frame)
    int numFrames, cap, dim;
    int rowStride;            // floats between rows
    size_t frameStride;       // floats between frames
    int tiles, qsplit;        // work-groups of kBlock train rows per pair, parts of the query range
    unsigned long long *keys; // [P][qsplit][cap]
};

// The restated L2sqr over elements a(j), b(j), j < D.  DC > 0: D = DC at compile time and every loop unrolls (the train row then
// stays in registers).
template <int DC, class A, class B> PS_D float l2sqr_restated(int Drt, A a, B b)
{
    const int D = DC > 0 ? DC : Drt;
    int j = 0;
    float d = 0.0f;
    if (D >= 8) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
        const auto block8 = [&](int k) {
            const float t0 = a(k) - b(k), t1 = a(k + 1) - b(k + 1), t2 = a(k + 2) - b(k + 2), t3 = a(k + 3) - b(k + 3);
            const float u0 = a(k + 4) - b(k + 4), u1 = a(k + 5) - b(k + 5), u2 = a(k + 6) - b(k + 6), u3 = a(k + 7) - b(k + 7);
            a0 = a0 + t0 * t0; a1 = a1 + t1 * t1; a2 = a2 + t2 * t2; a3 = a3 + t3 * t3;
            b0 = b0 + u0 * u0; b1 = b1 + u1 * u1; b2 = b2 + u2 * u2; b3 = b3 + u3 * u3;
        };
        if constexpr (DC > 0) {
#pragma unroll
            for (int k = 0; k < DC / 8; ++k) block8(8 * k);
            j = DC & ~7;
        } else {
            for (; j <= D - 8; j += 8) block8(j);
        }
        const float s0 = a0 + b0, s1 = a1 + b1, s2 = a2 + b2, s3 = a3 + b3;
        d = ((s0 + s1) + s2) + s3;
    }
    for (; j <= D - 4; j += 4) {
        const float t0 = a(j) - b(j), t1 = a(j + 1) - b(j + 1), t2 = a(j + 2) - b(j + 2), t3 = a(j + 3) - b(j + 3);
        d = d + (((t0 * t0 + t1 * t1) + t2 * t2) + t3 * t3);
    }
    for (; j < D; ++j) {
        const float t = a(j) - b(j);
        d = d + t * t;
    }
    return d;
}

// (dist bits, index) of one evaluation, kNoKeyL2 for a distance step 1 never takes (NaN, +inf, >= FLT_MAX)
PS_D unsigned long long l2_key(float sq, int index)
{
    const uint32_t bits = __float_as_uint(sqrtf(sq));
    return bits < kFltMaxBits ? ((unsigned long long)bits << 32) | (unsigned)index : kNoKeyL2;
}

template <int DV> __global__ __launch_bounds__(kBlock) void ps_l2_nn(L2Args a)
{
    const unsigned perPair = (unsigned)(a.tiles * a.qsplit);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(L / perPair);
    const int inner = (int)(L - (unsigned)p * perPair);
    const int fq = a.pairs[2 * p], ft = a.pairs[2 * p + 1];
    const int nq = map_count(a.nkpts, fq, a.numFrames, a.cap), nt = map_count(a.nkpts, ft, a.numFrames, a.cap);
    const int tile = inner / a.qsplit, qs = inner - tile * a.qsplit;
    if (tile * kBlock >= nt) return; // (the whole work-group; nt == 0 included: the frames are not touched)
    const int t = tile * kBlock + (int)threadIdx.x;
    const int q0 = (int)(((long long)nq * qs) / a.qsplit), q1 = (int)(((long long)nq * (qs + 1)) / a.qsplit);
    const float *__restrict__ trow = a.desc + (size_t)ft * a.frameStride + (size_t)(t < nt ? t : nt - 1) * a.rowStride;
    const float *__restrict__ qrow = a.desc + (size_t)(nq > 0 ? fq : ft) * a.frameStride + (size_t)q0 * a.rowStride;
    unsigned long long best = kNoKeyL2;
    if constexpr (DV > 0) {
        float r[DV];
#pragma unroll
        for (int j = 0; j < DV; ++j) r[j] = trow[j];
        for (int q = q0; q < q1; ++q, qrow += a.rowStride) {
            const unsigned long long key = l2_key(l2sqr_restated<DV>(DV, [&](int j) { return r[j]; }, [&](int j) { return qrow[j]; }), q);
            best = key < best ? key : best;
        }
    } else {
        const int D = a.dim;
        for (int q = q0; q < q1; ++q, qrow += a.rowStride) {
            const unsigned long long key = l2_key(l2sqr_restated<0>(D, [&](int j) { return trow[j]; }, [&](int j) { return qrow[j]; }), q);
            best = key < best ? key : best;
        }
    }
    if (t < nt) a.keys[((size_t)p * a.qsplit + qs) * a.cap + t] = best;
}

// ------------------------------------------------------------------------------------------
// The matrix-core prefilter (dim 64 / 128): decides, per train row, a short list of queries that can be its nearest; only the
// listed (t, q) are evaluated by the value-exact code.  No output value comes from it.
//
//   ps_l2_prepare     N work, one work-group per (frame, tile of 32 rows): the rows' squared norms n~ (NaN for a row that has a
//                     non-finite element or whose norm exceeds 2^100: such a row is always listed / swept) and the tile's
//                     fragment-major operand image  img[frame][tile][g < D / 8][lane][4 floats]: lane (r = lane & 31,
//                     h = lane >> 5) holds elements 8g + 2j + h, j < 4, of row r -- the A / B operand of v_mfma_f32_32x32x2_f32 for
//                     the k-steps 4g .. 4g + 3 (lane l holds A[l & 31][k = l >> 5] and B[k = l >> 5][l & 31]), read back as
//                     one contiguous 1-KiB load.
//   ps_l2_mfma<D>     one wave = one tile of 32 train rows, kept as B operands in registers; the query tiles stream through as A
//                     operands, D / 2 MFMAs a tile into ONE accumulator: g~(t, q), a k-ordered f32 fma chain from 0.  Train
//                     rows lie on the lanes (column = lane & 31); a lane holds the 16 queries tile_row(reg, lane >> 5).
//                         s~ = (n~t + n~q) - 2 g~,      E = kL2Band(D) (n~t + n~q) + 2^-130
//                     and the lane keeps a running  U = min(s~ + E)  over the queries it has seen and lists every q with
//                     s~ - E <= U (1 + 2^-20)  (16 places a lane, a count beyond: the row is swept exactly); after every tile
//                     the two lanes of a row exchange their U.  About ln(queries seen) entries a list beyond the true candidates.
//   ps_l2_refine      one lane = one train row: the listed queries that also pass the test against the least FINAL U of the
//                     row's lists (each entry keeps its s~ - E), evaluated by the value-exact code -- or every query, for a row
//                     with an overflowed list or a NaN norm --, the minimum by (dist, q) as ps_l2_nn writes it.
//
// THE BAND.  u = 2^-24, S = sum (t_k - q_k)^2 in real numbers, Nt = |t|^2, Nq = |q|^2, M = Nt + Nq + 2 sum |t_k q_k| <=
// 2 (Nt + Nq); every float operation on finite operands below 2^100 returns x (1 + d), |d| <= u, or, for a subnormal result, x + e,
// |e| <= 2^-150.  Relative parts first:
//   the restated L2sqr: t_k - q_k rounds once, its square once, and every square passes through at most D / 8 + 4 additions:
//       |L2sqr - S| <= g(D/8 + 7) S <= (D + 8) u M                                   [g(n) = n u / (1 - n u), S <= M];
//   n~t, n~q are sums of D rounded squares in some order (any order, fused or not): |n~ - N| <= g(D) N;
//   g~ is a chain of D fused multiply-adds from 0, one rounding each: |g~ - G| <= g(D) sum |t_k q_k|;
//   s~ = fl(fl(n~t + n~q) - 2 g~): two more roundings of quantities bounded by M (1 + g(D)):
//       |s~ - S| <= g(D) M + 2 u (1 + g(D)) M (1 + u) <= (D + 8) u M.
//   Both are below  2 (D + 8) u (Nt + Nq), and with N <= n~ (1 + 2 g(D))  below  Ehalf = 2 (D + 8) u (1 + 2^-8) (n~t + n~q).
// Absolute parts: at most 4 D + 8 operations lie between the inputs and either value: 2^-138 covers them.  kL2Band(D) =
// 4 (D + 8) u (1 + 2^-8), so E >= 2 Ehalf + 2^-130 bounds |s~ - S| + |L2sqr - S| >= |s~ - L2sqr| (and each of the two alone:
// ps_debug_l2_band's test).  THE RULE.  The winner q' of a train row has dist(q') <= dist(q) for every q; at most three
// adjacent floats share a correctly rounded square root, so L2sqr(q') <= L2sqr(q) (1 + 2^-21); with L2sqr(q) <= s~(q) + E(q),
// L2sqr(q') <= (1 + 2^-21) U for the running U of ANY subset of queries, and s~(q') - E(q') <= L2sqr(q'): q' is listed whenever
// it is looked at, whatever the order.  (The 2^-20 leaves room for the rounding of the comparison's own operations.)
// ------------------------------------------------------------------------------------------
constexpr int kL2ListLen = 16;    // places of a lane's candidate list
constexpr float kL2NormMax = 1.2676506e30f; // 2^100

PS_HD float l2_band(int D) { return 4.0f * (float)(D + 8) * 5.9604645e-08f * 1.00390625f; }

struct L2Pre {
    float4 *img;          // [numFrames][tpf][D / 8][64] operand image
    float *norms;         // [numFrames][tpf * 32]
    unsigned short *list; // [P][cap][slots][kL2ListLen] candidate queries, slot = 2 * (query part) + lane half
    float *listLo;        // ... and their s~ - E
    int32_t *count;       // [P][cap][slots] candidates met (may exceed kL2ListLen: the list overflowed)
    float *bound;         // [P][cap][slots] the list's final U (+inf: it saw nothing)
    int tpf, slots;       // tiles per frame, lists per train row
    int groups;           // work-groups of four train tiles per pair
    float *dbgS, *dbgE;   // ps_debug_l2_band: [nt][nq] of pair 0, else null
    unsigned long long *stats; // {train rows swept exactly, candidate evaluations, rows with an overflowed list} or null
};

__global__ __launch_bounds__(kBlock) void ps_l2_prepare(L2Args a, L2Pre pre)
{
    const int f = blockIdx.x / pre.tpf, tile = blockIdx.x - f * pre.tpf;
    const int n = map_count(a.nkpts, f, a.numFrames, a.cap);
    const int D = a.dim, G = D >> 3;
    const float *__restrict__ rows = a.desc + (size_t)f * a.frameStride;
    // norms: eight threads a row
    {
        const int r = tile * kTileRows + ((int)threadIdx.x >> 3), part = threadIdx.x & 7;
        float s = r < n ? 0.0f : __builtin_nanf(""); // (a row beyond the frame: never the bound, never listed)
        if (r < n) {
            const float *__restrict__ x = rows + (size_t)r * a.rowStride;
            for (int k = part; k < D; k += 8) {
                const float v = x[k];
                s += fabsf(v) <= kL2NormMax ? v * v : __builtin_nanf("");
            }
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (part == 0) pre.norms[(size_t)f * pre.tpf * kTileRows + r] = s <= kL2NormMax ? s : __builtin_nanf("");
    }
    // image: piece (g, lane) = elements 8g + 2j + h of row (lane & 31)
    float4 *__restrict__ out = pre.img + ((size_t)f * pre.tpf + tile) * G * 64;
    for (int e = threadIdx.x; e < G * 64; e += kBlock) {
        const int g = e >> 6, lane = e & 63, r = tile * kTileRows + (lane & 31), h = lane >> 5;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < n) {
            const float *__restrict__ x = rows + (size_t)r * a.rowStride + 8 * g + h;
            v = make_float4(x[0], x[2], x[4], x[6]);
        }
        out[e] = v;
    }
}

template <int D> __global__ __launch_bounds__(kBlock) void ps_l2_mfma(L2Args a, L2Pre pre)
{
    constexpr int G = D / 8;
    const unsigned perPair = (unsigned)(pre.groups * a.qsplit);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(L / perPair);
    const int inner = (int)(L - (unsigned)p * perPair);
    const int fq = a.pairs[2 * p], ft = a.pairs[2 * p + 1];
    const int nq = map_count(a.nkpts, fq, a.numFrames, a.cap), nt = map_count(a.nkpts, ft, a.numFrames, a.cap);
    const int group = inner / a.qsplit, qs = inner - group * a.qsplit;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, h = lane >> 5;
    const int tt = group * kWavesPerWG + w;
    if (tt * kTileRows >= nt || nq == 0) return; // (the wave: no barrier below)
    const int t = tt * kTileRows + (lane & 31);
    const int qtiles = (nq + kTileRows - 1) / kTileRows;
    const int qt0 = (int)(((long long)qtiles * qs) / a.qsplit), qt1 = (int)(((long long)qtiles * (qs + 1)) / a.qsplit);
    const float4 *__restrict__ imgT = pre.img + ((size_t)ft * pre.tpf + tt) * G * 64 + lane;
    const float4 *__restrict__ imgQ = pre.img + (size_t)fq * pre.tpf * G * 64 + lane;
    const float *__restrict__ normQ = pre.norms + (size_t)fq * pre.tpf * kTileRows;
    const float nT = pre.norms[(size_t)ft * pre.tpf * kTileRows + t];
    float4 b[G];
#pragma unroll
    for (int g = 0; g < G; ++g) b[g] = imgT[g * 64];
    const float band = l2_band(D);
    const int slot = 2 * qs + h;
    const size_t row = ((size_t)p * a.cap + (t < nt ? t : 0)) * pre.slots + slot;
    unsigned short *__restrict__ list = pre.list + row * kL2ListLen;
    float *__restrict__ listLo = pre.listLo + row * kL2ListLen;
    float U = __builtin_inff();
    int cnt = 0;
    for (int qt = qt0; qt < qt1; ++qt) {
        v16f_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float4 *__restrict__ aq = imgQ + (size_t)qt * G * 64;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float4 av = aq[g * 64];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b[g].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b[g].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b[g].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b[g].w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int qbase = qt * kTileRows + 8 * r4 + 4 * h; // tile_row(4 r4 + i, h) = 8 r4 + 4 h + i
            const float4 nq4 = *reinterpret_cast<const float4 *>(normQ + qbase);
            const float nqs[4] = {nq4.x, nq4.y, nq4.z, nq4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = qbase + i;
                const float nsum = nT + nqs[i];
                const float st = nsum - 2.0f * acc[4 * r4 + i];
                const float E = band * nsum + 7.3468397e-40f; // 2^-130
                if (pre.dbgS != nullptr && p == 0 && t < nt && q < nq) {
                    pre.dbgS[(size_t)t * nq + q] = st;
                    pre.dbgE[(size_t)t * nq + q] = E;
                }
                U = fminf(U, q < nq ? st + E : U); // (a NaN is skipped)
                const float thr = U + U * 9.5367432e-07f; // 2^-20
                if (!(st - E > thr) && q < nq) { // (NaN: listed)
                    if (cnt < kL2ListLen && t < nt) {
                        list[cnt] = (unsigned short)q;
                        listLo[cnt] = st - E;
                    }
                    ++cnt;
                }
            }
        }
        U = fminf(U, __shfl_xor(U, 32, 64)); // the row's other half of the tile
    }
    if (t < nt) {
        pre.count[row] = cnt;
        pre.bound[row] = U;
    }
}

__global__ __launch_bounds__(kBlock) void ps_l2_refine(L2Args a, L2Pre pre)
{
    const int p = blockIdx.x / a.tiles, tile = blockIdx.x - p * a.tiles;
    const int fq = a.pairs[2 * p], ft = a.pairs[2 * p + 1];
    const int nq = map_count(a.nkpts, fq, a.numFrames, a.cap), nt = map_count(a.nkpts, ft, a.numFrames, a.cap);
    const int t = tile * kBlock + (int)threadIdx.x;
    if (t >= nt) return;
    const int D = a.dim;
    const float *__restrict__ trow = a.desc + (size_t)ft * a.frameStride + (size_t)t * a.rowStride;
    const float *__restrict__ qrows = a.desc + (size_t)(nq > 0 ? fq : ft) * a.frameStride;
    const size_t row = ((size_t)p * a.cap + t) * pre.slots;
    const float nT = pre.norms[(size_t)ft * pre.tpf * kTileRows + t];
    bool sweep = !(nT == nT), over = false;
    for (int s = 0; s < pre.slots && nq > 0; ++s) over = over || pre.count[row + s] > kL2ListLen;
    sweep = sweep || over;
    unsigned long long best = kNoKeyL2;
    unsigned evals = 0;
    const auto eval = [&](int q) {
        const float *__restrict__ qrow = qrows + (size_t)q * a.rowStride;
        const unsigned long long key = l2_key(l2sqr_restated<0>(D, [&](int j) { return trow[j]; }, [&](int j) { return qrow[j]; }), q);
        best = key < best ? key : best;
    };
    if (sweep) {
        for (int q = 0; q < nq; ++q) eval(q);
    } else if (nq > 0) {
        // the lists were kept against their own running bounds: the least final bound thins them once more (THE RULE holds
        // for the U of any subset of queries)
        float U = __builtin_inff();
        for (int s = 0; s < pre.slots; ++s)
            if (pre.count[row + s] > 0) U = fminf(U, pre.bound[row + s]);
        const float thr = U + U * 9.5367432e-07f; // 2^-20
        for (int s = 0; s < pre.slots; ++s) {
            const int n = pre.count[row + s];
            const unsigned short *__restrict__ list = pre.list + (row + s) * kL2ListLen;
            const float *__restrict__ listLo = pre.listLo + (row + s) * kL2ListLen;
            for (int k = 0; k < n; ++k) {
                if (listLo[k] > thr) continue; // (a NaN stays)
                eval((int)list[k]);
                ++evals;
            }
        }
    }
    a.keys[(size_t)p * a.cap + t] = best;
    if (pre.stats != nullptr) {
        if (sweep) atomicAdd(&pre.stats[0], 1ull);
        if (evals) atomicAdd(&pre.stats[1], (unsigned long long)evals);
        if (over) atomicAdd(&pre.stats[2], 1ull);
    }
}

template <bool REC, int BLOCK>
__global__ __launch_bounds__(BLOCK) void ps_l2_crosscheck(L2Args a, const float *__restrict__ pts, PrepArgs pa, RecPtrs rec,
                                                          PsDMatch *__restrict__ matches, int32_t *__restrict__ numMatches,
                                                          int32_t *__restrict__ mvalid, float2 *__restrict__ cmaxOut)
{
    extern __shared__ __align__(16) unsigned long long s_l2best[]; // nq keys
    __shared__ int s_wsum[2 * (BLOCK / 64)];
    __shared__ float2 s_red[BLOCK / 64];
    const int p = blockIdx.x, cap = a.cap;
    const int fq = a.pairs[2 * p], ft = a.pairs[2 * p + 1];
    const int nq = map_count(a.nkpts, fq, a.numFrames, cap), nt = map_count(a.nkpts, ft, a.numFrames, cap);
    for (int q = threadIdx.x; q < nq; q += BLOCK) s_l2best[q] = kNoKeyL2;
    __syncthreads();
    // step 2: query q keeps the closest train row among those that chose it, ties to the lowest train index
    if (nq > 0) {
        for (int t = threadIdx.x; t < nt; t += BLOCK) {
            unsigned long long key = kNoKeyL2;
            for (int s = 0; s < a.qsplit; ++s) {
                const unsigned long long k = a.keys[((size_t)p * a.qsplit + s) * cap + t];
                key = k < key ? k : key;
            }
            if (key != kNoKeyL2) atomicMin(&s_l2best[(uint32_t)key], (key & 0xFFFFFFFF00000000ull) | (unsigned)t);
        }
    }
    __syncthreads();
    // step 3, and what ps_crosscheck_prep does with its matches
    const float *pp = REC ? pts + (size_t)(nq > 0 ? fq : 0) * pa.ptsStride : nullptr; // (a match implies both frames lie in the set)
    const float *cp = REC ? pts + (size_t)(nq > 0 && nt > 0 ? ft : 0) * pa.ptsStride : nullptr;
    PairRecords pr(pa, rec, p, REC);
    int base = 0, trip = 0;
    for (int q0 = 0; q0 < nq; q0 += BLOCK, ++trip) {
        const int q = q0 + (int)threadIdx.x;
        const unsigned long long key = q < nq ? s_l2best[q] : kNoKeyL2;
        const bool has = key != kNoKeyL2;
        const int t = (int)(uint32_t)key;
        float px = 0, py = 0, pz = 0, cx_ = 0, cy_ = 0, cz_ = 0;
        bool ok = false;
        if (REC && has) {
            px = pp[3 * q]; py = pp[3 * q + 1]; pz = pp[3 * q + 2];
            cx_ = cp[3 * t]; cy_ = cp[3 * t + 1]; cz_ = cp[3 * t + 2];
            ok = match_depth_ok(px, py, pz, cx_, cy_, cz_);
        }
        int pos, total, vpos, vtotal;
        block_scan_flags2<BLOCK, false>(has, ok, pos, total, vpos, vtotal, s_wsum, trip);
        if (has) {
            PsDMatch m;
            m.queryIdx = q;
            m.trainIdx = t;
            m.imgIdx = 0;
            m.distance = __uint_as_float((uint32_t)(key >> 32));
            matches[(size_t)p * cap + base + pos] = m;
        }
        if (REC) pr.add(ok, vpos, vtotal, base + pos, q, t, px, py, pz, cx_, cy_, cz_);
        base += total;
    }
    if (REC) pr.finish<BLOCK>(s_red, mvalid, cmaxOut);
    if (threadIdx.x == 0) numMatches[p] = base;
}

} // namespace psdev

// Host side.  Part of the device translation unit: included by ps_capi.hip behind the plan and the stages.
namespace {

struct L2Strides {
    int rowFloats = 0, ptsFloats = 0;
    size_t frameFloats = 0;
};

// THE RULES of a PsFrameSetF32 (include/putslam_hip.h).  needPts = false: the call reads no points.
int check_l2_frames(PsContext *ctx, const PsFrameSetF32 &fs, bool needPts, const char *who, L2Strides &out)
{
    const std::string w(who);
    if (!fs.desc || !fs.nkpts || (needPts && !fs.pts) || fs.numFrames < 1 || fs.maxKpts < 1 || fs.dim < 1)
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": bad frame set (null array, numFrames, maxKpts or dim < 1)").c_str());
    if (fs.dim > PS_MAX_L2_DIM) return fail(ctx, PS_ERR_UNSUPPORTED, (w + ": more than PS_MAX_L2_DIM elements per descriptor").c_str());
    if (fs.maxKpts > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, (w + ": more than PS_MAX_KPTS keypoints per frame").c_str());
    const size_t row = fs.descRowStride ? fs.descRowStride : (size_t)fs.dim * 4;
    const size_t frame = fs.descFrameStride ? fs.descFrameStride : (size_t)fs.maxKpts * row;
    const size_t pts = fs.ptsFrameStride ? fs.ptsFrameStride : (size_t)fs.maxKpts * 12;
    if ((row & 3) != 0 || row < (size_t)fs.dim * 4 || row / 4 > (size_t)INT_MAX || ((uintptr_t)fs.desc & 3) != 0)
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": descRowStride must be a multiple of 4, >= dim x 4 and below 8 GiB, desc 4-byte aligned").c_str());
    if ((frame & 3) != 0 || frame / row < (size_t)fs.maxKpts)
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": descFrameStride must be a multiple of 4 and >= maxKpts x the row stride").c_str());
    if (needPts && ((pts & 3) != 0 || pts < (size_t)fs.maxKpts * 12 || pts / 4 > (size_t)INT_MAX))
        return fail(ctx, PS_ERR_BAD_ARG, (w + ": ptsFrameStride must be a multiple of 4, >= maxKpts x 12 and below 8 GiB").c_str());
    out.rowFloats = (int)(row / 4);
    out.frameFloats = frame / 4;
    out.ptsFloats = (int)(pts / 4);
    return PS_OK;
}

// The launches for a checked set -- the sweep or the prefilter's three, then the cross-check; pl = null: matches only.
struct L2Debug { float *s, *e; }; // ps_debug_l2_band: device blocks [nt][nq] for pair 0

int run_l2_match(PsContext *ctx, const PsFrameSetF32 &fs, const L2Strides &strides, const int32_t *dPairs, int P, const Plan *pl,
                 PsDMatch *dMatches, int32_t *dNumMatches, int slot0, const L2Debug *dbg = nullptr)
{
    const int cap = fs.maxKpts;
    L2Args a{};
    a.desc = fs.desc; a.nkpts = fs.nkpts; a.pairs = dPairs;
    a.numFrames = fs.numFrames; a.cap = cap; a.dim = fs.dim;
    a.rowStride = strides.rowFloats; a.frameStride = strides.frameFloats;
    a.tiles = (cap + kBlock - 1) / kBlock;
    // few pairs, many CUs: the query range in parts of at least 16 rows (as ps_hamming_nn's)
    a.qsplit = pick_split((long long)P * a.tiles, kL2MaxQsplit, 16, cap);
    if (ctx->forceQsplit > 0) a.qsplit = ctx->forceQsplit < kL2MaxQsplit ? ctx->forceQsplit : kL2MaxQsplit;
    PS_ENSURE(ctx->l2Keys, (size_t)P * a.qsplit * cap * sizeof(unsigned long long));
    a.keys = (unsigned long long *)ctx->l2Keys.p;
    PrepArgs pa = pl ? pl->pa : PrepArgs{};
    pa.cap = cap;
    pa.ptsStride = strides.ptsFloats;
    if (pl) {
        PS_ENSURE(ctx->mvalid, (size_t)P * sizeof(int32_t));
        PS_ENSURE(ctx->cmax, (size_t)P * sizeof(float2));
        int rc = ensure_records(ctx, (size_t)P, (size_t)cap);
        if (rc != PS_OK) return rc;
    }
    const bool pref = dbg != nullptr || (ctx->matcherL2 == 1 && (fs.dim == 64 || fs.dim == 128));
    ctx->matcherL2Used = pref ? 1 : 0;
    tick(ctx, slot0, false);
    if (pref) {
        L2Pre pre{};
        pre.tpf = (cap + kTileRows - 1) / kTileRows;
        pre.groups = (pre.tpf + kWavesPerWG - 1) / kWavesPerWG;
        // few pairs: the query tiles in parts (every part keeps its own lists)
        int qsplit = pick_split((long long)P * pre.groups, 8, 4, pre.tpf);
        if (ctx->forceQsplit > 0) qsplit = ctx->forceQsplit < 8 ? ctx->forceQsplit : 8;
        pre.slots = 2 * qsplit;
        const size_t rows = (size_t)P * cap * pre.slots;
        PS_ENSURE(ctx->l2Img, (size_t)fs.numFrames * pre.tpf * kTileRows * fs.dim * sizeof(float));
        PS_ENSURE(ctx->l2Norms, (size_t)fs.numFrames * pre.tpf * kTileRows * sizeof(float));
        PS_ENSURE(ctx->l2List, rows * kL2ListLen * sizeof(unsigned short));
        PS_ENSURE(ctx->l2ListLo, rows * kL2ListLen * sizeof(float));
        PS_ENSURE(ctx->l2Count, rows * 2 * sizeof(int32_t));
        pre.img = (float4 *)ctx->l2Img.p; pre.norms = (float *)ctx->l2Norms.p;
        pre.list = (unsigned short *)ctx->l2List.p; pre.listLo = (float *)ctx->l2ListLo.p;
        pre.count = (int32_t *)ctx->l2Count.p; pre.bound = (float *)(pre.count + rows);
        if (dbg) { pre.dbgS = dbg->s; pre.dbgE = dbg->e; }
        if (ctx->l2Stats) {
            PS_ENSURE(ctx->l2Stat, 4 * sizeof(unsigned long long));
            PS_HIP(hipMemsetAsync(ctx->l2Stat.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
            pre.stats = (unsigned long long *)ctx->l2Stat.p;
        }
        hipLaunchKernelGGL(ps_l2_prepare, dim3((unsigned)fs.numFrames * (unsigned)pre.tpf), dim3(kBlock), 0, ctx->stream, a, pre);
        PS_HIP(hipGetLastError());
        // a part of the query range that holds no tile would leave its counts unwritten: they start from zero
        PS_HIP(hipMemsetAsync(pre.count, 0, rows * sizeof(int32_t), ctx->stream));
        a.qsplit = qsplit;
        const dim3 grid((unsigned)P * (unsigned)pre.groups * (unsigned)qsplit), block(kBlock);
        if (fs.dim == 64) hipLaunchKernelGGL(ps_l2_mfma<64>, grid, block, 0, ctx->stream, a, pre);
        else hipLaunchKernelGGL(ps_l2_mfma<128>, grid, block, 0, ctx->stream, a, pre);
        PS_HIP(hipGetLastError());
        a.qsplit = 1; // the refinement writes ONE key per train row
        hipLaunchKernelGGL(ps_l2_refine, dim3((unsigned)P * (unsigned)a.tiles), dim3(kBlock), 0, ctx->stream, a, pre);
    } else {
        const dim3 grid((unsigned)P * (unsigned)a.tiles * (unsigned)a.qsplit), block(kBlock);
        switch (fs.dim) {
        case 64: hipLaunchKernelGGL(ps_l2_nn<64>, grid, block, 0, ctx->stream, a); break;
        case 128: hipLaunchKernelGGL(ps_l2_nn<128>, grid, block, 0, ctx->stream, a); break;
        default: hipLaunchKernelGGL(ps_l2_nn<0>, grid, block, 0, ctx->stream, a); break;
        }
    }
    tick(ctx, slot0, true);
    PS_HIP(hipGetLastError());
    tick(ctx, slot0 + 1, false);
    const size_t lds = (size_t)cap * sizeof(unsigned long long);
    const bool wide = P <= kWidePairs; // a handful of pairs: 1024-thread work-groups shorten the per-pair serial walk
    const RecPtrs rp = pl ? rec_ptrs(ctx, pl->score) : RecPtrs{};
    int32_t *mv = (int32_t *)ctx->mvalid.p;
    float2 *cmx = (float2 *)ctx->cmax.p;
    if (pl) {
        if (wide) hipLaunchKernelGGL((ps_l2_crosscheck<true, 1024>), dim3((unsigned)P), dim3(1024), lds, ctx->stream, a, fs.pts, pa, rp, dMatches, dNumMatches, mv, cmx);
        else hipLaunchKernelGGL((ps_l2_crosscheck<true, kBlock>), dim3((unsigned)P), dim3(kBlock), lds, ctx->stream, a, fs.pts, pa, rp, dMatches, dNumMatches, mv, cmx);
    } else {
        if (wide) hipLaunchKernelGGL((ps_l2_crosscheck<false, 1024>), dim3((unsigned)P), dim3(1024), lds, ctx->stream, a, fs.pts, pa, rp, dMatches, dNumMatches, mv, cmx);
        else hipLaunchKernelGGL((ps_l2_crosscheck<false, kBlock>), dim3((unsigned)P), dim3(kBlock), lds, ctx->stream, a, fs.pts, pa, rp, dMatches, dNumMatches, mv, cmx);
    }
    tick(ctx, slot0 + 1, true);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// the cross-check keeps best[q] for up to PS_MAX_KPTS queries in LDS (128 KiB of the CU's 160 KiB)
void l2_kernel_attributes()
{
    for (const void *k : {reinterpret_cast<const void *>(&ps_l2_crosscheck<true, kBlock>), reinterpret_cast<const void *>(&ps_l2_crosscheck<false, kBlock>),
                          reinterpret_cast<const void *>(&ps_l2_crosscheck<true, 1024>), reinterpret_cast<const void *>(&ps_l2_crosscheck<false, 1024>)})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, PS_MAX_KPTS * 8);
}

} // namespace

namespace {

// One pair of host arrays through the device path: the match list (out / nout), or the prefilter's s~ and E (dbgS / dbgE, host,
// nt x nq each).
int l2_host_pair(PsContext *ctx, const float *query, int nq, size_t qstep, const float *train, int nt, size_t tstep, int dim,
                 PsDMatch *out, int *nout, float *dbgS, float *dbgE)
{
    if (nq < 0 || nt < 0 || dim < 1 || (nq > 0 && !query) || (nt > 0 && !train)) return fail(ctx, PS_ERR_BAD_ARG, "float matcher: bad argument");
    if (dim > PS_MAX_L2_DIM) return fail(ctx, PS_ERR_UNSUPPORTED, "float matcher: more than PS_MAX_L2_DIM elements per descriptor");
    const size_t row = (size_t)dim * 4;
    if ((nq > 0 && qstep < row) || (nt > 0 && tstep < row)) return fail(ctx, PS_ERR_BAD_ARG, "float matcher: row pitch below dim x 4 bytes");
    if (nq > PS_MAX_KPTS || nt > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "more than PS_MAX_KPTS rows");
    if (nq == 0 || nt == 0) return PS_OK; // BFMatcher on an empty side: no matches
    const int cap = nq > nt ? nq : nt;
    PS_ENSURE(ctx->sDesc, (size_t)2 * cap * row);
    PS_ENSURE(ctx->sNk, 4 * sizeof(int32_t));
    PS_ENSURE(ctx->sMatches, (size_t)cap * sizeof(PsDMatch));
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    const size_t dbgBytes = (size_t)nt * nq * sizeof(float);
    if (dbgS) {
        PS_ENSURE(ctx->sMisc0, dbgBytes);
        PS_ENSURE(ctx->sMisc1, dbgBytes);
    }
    uint8_t *dDesc = (uint8_t *)ctx->sDesc.p;
    PS_HIP(hipMemcpy2DAsync(dDesc, row, query, qstep, row, (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc + (size_t)cap * row, row, train, tstep, row, (size_t)nt, hipMemcpyHostToDevice, ctx->stream));
    const int32_t hostMeta[4] = {nq, nt, 0, 1}; // nkpts[2], pair (0, 1)
    PS_HIP(hipMemcpyAsync(ctx->sNk.p, hostMeta, sizeof hostMeta, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // hostMeta goes out of scope
    PsFrameSetF32 fs{};
    fs.desc = (const float *)dDesc;
    fs.nkpts = (const int32_t *)ctx->sNk.p;
    fs.numFrames = 2;
    fs.maxKpts = cap;
    fs.dim = dim;
    L2Strides strides;
    int rc = check_l2_frames(ctx, fs, false, "float matcher", strides);
    if (rc) return rc;
    const L2Debug dbg{(float *)ctx->sMisc0.p, (float *)ctx->sMisc1.p};
    rc = run_l2_match(ctx, fs, strides, (const int32_t *)ctx->sNk.p + 2, 1, nullptr, (PsDMatch *)ctx->sMatches.p, (int32_t *)ctx->sNumM.p, 0,
                      dbgS ? &dbg : nullptr);
    if (rc) return rc;
    if (dbgS) {
        PS_HIP(hipMemcpyAsync(dbgS, dbg.s, dbgBytes, hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipMemcpyAsync(dbgE, dbg.e, dbgBytes, hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
        return PS_OK;
    }
    int32_t n = 0;
    PS_HIP(hipMemcpyAsync(&n, ctx->sNumM.p, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    if (n > 0) {
        PS_HIP(hipMemcpyAsync(out, ctx->sMatches.p, (size_t)n * sizeof(PsDMatch), hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
    }
    *nout = n;
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_frameset_f32(void) { return sizeof(PsFrameSetF32); }

int ps_match_l2_f32(PsContext *ctx, const float *query, int nq, size_t qstep, const float *train, int nt, size_t tstep, int dim,
                    PsDMatch *out, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    if (nout) *nout = 0;
    if (!out || !nout) return fail(ctx, PS_ERR_BAD_ARG, "ps_match_l2_f32: null output");
    return l2_host_pair(ctx, query, nq, qstep, train, nt, tstep, dim, out, nout, nullptr, nullptr);
}

int ps_debug_l2_band(PsContext *ctx, const float *query, int nq, size_t qstep, const float *train, int nt, size_t tstep, int dim,
                     float *stilde, float *band)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    if (!stilde || !band) return fail(ctx, PS_ERR_BAD_ARG, "ps_debug_l2_band: null output");
    if (dim != 64 && dim != 128) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_debug_l2_band: the prefilter takes dim 64 and 128");
    return l2_host_pair(ctx, query, nq, qstep, train, nt, tstep, dim, nullptr, nullptr, stilde, band);
}

int ps_debug_l2_stats(PsContext *ctx, uint64_t *out3)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out3) return PS_ERR_BAD_ARG;
    out3[0] = out3[1] = out3[2] = 0;
    if (!ctx->l2Stat.p) return PS_OK;
    unsigned long long h[3] = {0, 0, 0};
    PS_HIP(hipMemcpyAsync(h, ctx->l2Stat.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 3; ++i) out3[i] = h[i];
    return PS_OK;
}

int ps_match_l2_device(PsContext *ctx, const PsFrameSetF32 *frames, const int32_t *pairs, int P, PsDMatch *matches, int32_t *numMatches)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!frames || P < 0) return fail(ctx, PS_ERR_BAD_ARG, "ps_match_l2_device: null frame set or P < 0");
    if (P == 0) return PS_OK;
    if (!pairs || !matches || !numMatches) return fail(ctx, PS_ERR_BAD_ARG, "ps_match_l2_device: null pairs or output");
    L2Strides strides;
    rc = check_l2_frames(ctx, *frames, false, "ps_match_l2_device", strides);
    if (rc) return rc;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return run_l2_match(ctx, *frames, strides, pairs, P, nullptr, matches, numMatches, 0);
}

int ps_vo_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                          const PsFrameSetF32 *frames, const int32_t *pairs, int P, const PsPairResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!frames || !out || P < 0) return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_l2_device: null frame set / output or P < 0");
    if (P == 0) return PS_OK;
    if (!pairs || !out->matches || !out->numMatches || !out->inlierMask || !out->pose || !out->stats)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_l2_device: null pairs or output");
    L2Strides strides;
    rc = check_l2_frames(ctx, *frames, true, "ps_vo_pairs_l2_device", strides);
    if (rc) return rc;
    if (cfg && cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "explicit sample streams are per call, not per batch");
    const int cap = frames->maxKpts;
    Plan pl;
    rc = make_plan(ctx, params, cfg, K, cap, cap, pl);
    if (rc) return rc;
    begin_timed_call(ctx);
    HandoffGuard handoffGuard{ctx}; // (prepare_score below may already queue a clearing: the guard stands before it)
    rc = prepare_score(ctx, pl, P, cap, false, true, frames->desc);
    if (rc) return rc;
    rc = run_l2_match(ctx, *frames, strides, pairs, P, &pl, out->matches, out->numMatches, 0);
    if (rc) return rc;
    return run_ransac_stage(ctx, pl, P, cap, out->matches, out->numMatches, cap, out->pose, out->inlierMask, out->stats, 2);
}

} // extern "C"
