// ps_map_match_l2.h -- guided map matching for FLOAT descriptors (SURF / SIFT): Matcher::matchXYZ (reference
// src/Matcher/matcher.cpp:694-746) with normType = cv::NORM_L2 on CV_32F rows (:625-628), for host arrays (ps_match_xyz_l2_f32)
// and for P (map view, frame) pairs of a device-resident batch (ps_match_xyz_l2_device / ps_map_pairs_l2_device,
// include/putslam_hip.h).  Everything but the VALUE of a candidate is ps_map_match.h's rule, and ps_map_emit is reused as it is
// (it works on staged PsDMatch rows; the descriptor pointers of its MapArgs stay null).
//
// The value (tests/map_l2_ref.py is the definition; restated from OpenCV 3.x's continuous path norm() -> normL2_32f ->
// normL2Sqr<float, double>, not compiled against an OpenCV):
//   x[k] = fl32(map[k] - cur[k]);  v[k] = (double)x[k];  s = 0.0
//   blocks of four:  s = s + (((v0 v0 + v1 v1) + v2 v2) + v3 v3);  then  s = s + v v  per tail element;  value = (float)sqrt(s)
// A product of two floats is exact in double, so the roundings are the subtraction, the additions, the square root (correctly
// rounded) and the narrowing.
//
//   ps_map_sweep_l2<F>  ps_map_sweep<F>'s decomposition and sphere / level arithmetic.  The inner loop records candidate INDICES
//                       only (kMapStash places per feature, ballot order = ascending i): a row is 256 - 2048 B and is not touched
//                       inside the hit branch.  After the sweep the wave evaluates its features' short lists:
//                         group form (dim 64 / 128, bases and strides multiples of 16 B): dim / 4 lanes per candidate, each one
//                           16-byte load per row = one block of four; the block sums are added in block order by a chain of
//                           dim / 4 double additions over cross-lane reads;
//                         plain form (every other dim or alignment): one lane per candidate, the sequential loop.
//                       Both give the same bytes.  Then best / ratio / emit as ps_map_sweep, with the NaN rule of :714-727:
//                       the first candidate is always taken, a later one only if value < bestVal -- a NaN first value leaves
//                       bestVal NaN and the feature emits nothing, a later NaN is ignored.
//                       A feature with more candidates than the stash holds is swept again from global memory, three times
//                       (least value, count, write), evaluating values on the way: slow and correct.
#pragma once
#include "ps_glue.h"
#include "ps_kernels.h"
#include "ps_map_match.h"

namespace psdev {

struct MapL2Args {
    MapArgs m;                             // ps_map_match.h's arguments; mapDesc / curDesc unused (null)
    const float *mapDesc, *curDesc;        // float rows
    size_t mapFrameFloats, curFrameFloats; // floats between views / frames
    int mapRowFloats, curRowFloats;        // floats between rows
    int dim;
    int group; // lanes per candidate of the value phase: dim / 4 (16 or 32), or 0 = one lane per candidate
};

PS_D uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_down((int)v, o, 64);
        v = other < v ? other : v;
    }
    return (uint32_t)__shfl((int)v, 0, 64);
}

// one block of four: ((v0^2 + v1^2) + v2^2) + v3^2 over the double casts of the float differences
PS_D double l2_block4(float a0, float a1, float a2, float a3, float b0, float b1, float b2, float b3)
{
    const double v0 = (double)(a0 - b0), v1 = (double)(a1 - b1), v2 = (double)(a2 - b2), v3 = (double)(a3 - b3);
    return ((v0 * v0 + v1 * v1) + v2 * v2) + v3 * v3;
}

// plain form: one lane, the whole row
PS_D float l2_value_plain(const float *__restrict__ a, const float *__restrict__ b, int dim)
{
    double s = 0.0;
    int k = 0;
    for (; k <= dim - 4; k += 4) s = s + l2_block4(a[k], a[k + 1], a[k + 2], a[k + 3], b[k], b[k + 1], b[k + 2], b[k + 3]);
    for (; k < dim; ++k) {
        const double v = (double)(a[k] - b[k]);
        s = s + v * v;
    }
    return (float)ps_sqrt(s);
}

// group form: G = dim / 4 consecutive lanes (G a power of two, a divisor of 64) hold one block each; every lane of the group
// returns the value.  Called by the whole wave; a group without a candidate (valid = false) loads nothing.
PS_D float l2_value_group(const float *__restrict__ a, const float *__restrict__ b, bool valid, int G, int lane)
{
    double blk = 0.0;
    if (valid) {
        const int g = lane & (G - 1);
        const float4 x = *reinterpret_cast<const float4 *>(a + 4 * g), y = *reinterpret_cast<const float4 *>(b + 4 * g);
        blk = l2_block4(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w);
    }
    const int base = lane & ~(G - 1);
    double s = 0.0;
    for (int k = 0; k < G; ++k) s = s + __shfl(blk, base + k, 64); // block order
    return (float)ps_sqrt(s);
}

// One wave, one map feature, the whole frame from global memory, values in the plain form.
//   MODE 0: returns the bits of the least non-NaN value among the candidates (+inf's bits if there is none);
//   MODE 1 / 2: the number of candidates within the accept ratio of bestVal, ascending i; MODE 2 writes them from out[0] on.
template <int MODE>
PS_D uint32_t map_l2_resweep(float mx, float my, float mz, int lj, const float *__restrict__ mrow, const float *__restrict__ curPos,
                             const float *__restrict__ curDesc, int curRowFloats, int dim, const int32_t *__restrict__ curLevel,
                             int ncur, float radiusBound, double acceptRatio, float bestVal, int j, PsDMatch *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    uint32_t n = 0, least = 0x7F800000u;
    for (int i0 = 0; i0 < ncur; i0 += 64) {
        const int i = i0 + lane;
        bool acc = false;
        float value = 0.f;
        if (i < ncur) {
            const float d0 = mx - curPos[3 * i], d1 = my - curPos[3 * i + 1], d2 = mz - curPos[3 * i + 2];
            const float s = d0 * d0 + (d1 * d1 + d2 * d2);
            const int li = curLevel[i];
            if (s < radiusBound && li - 1 <= lj && lj <= li + 1) {
                value = l2_value_plain(mrow, curDesc + (size_t)i * curRowFloats, dim);
                if (MODE == 0) {
                    if (value == value && __float_as_uint(value) < least) least = __float_as_uint(value);
                } else {
                    acc = acceptRatio * (double)value <= (double)bestVal;
                }
            }
        }
        if (MODE != 0) {
            const unsigned long long bal = __ballot(acc);
            if (MODE == 2 && acc) {
                PsDMatch m;
                m.queryIdx = j;
                m.trainIdx = i;
                m.imgIdx = -1; // default-constructed cv::DMatch (matcher.cpp:741)
                m.distance = value;
                out[n + __popcll(bal & ((1ull << lane) - 1ull))] = m;
            }
            n += __popcll(bal);
        }
    }
    return MODE == 0 ? wave_min_u32(least) : n;
}

template <int F>
__global__ __launch_bounds__(kMapBlock) void ps_map_sweep_l2(MapL2Args b)
{
    constexpr int CH = kMapWaves * F;
    const MapArgs &a = b.m;
    __shared__ uint4 s_tile[kMapTile];
    __shared__ int s_idx[CH * kMapStash];
    __shared__ float s_val[CH * kMapStash];
    __shared__ int s_n[CH];
    __shared__ int s_start;
    const int p = blockIdx.x / a.chunks, c = blockIdx.x - p * a.chunks;
    const int view = a.pairs[2 * p], frame = a.pairs[2 * p + 1];
    const int nmap = map_count(a.mapN, view, a.mapFrames, a.mapCap);
    const int ncur = map_count(a.curN, frame, a.curFrames, a.curCap);
    const int j0 = c * CH;
    if (j0 >= nmap || ncur == 0) { // (the whole work-group)
        if (threadIdx.x == 0) {
            a.chunkStart[(size_t)p * a.chunks + c] = 0;
            a.chunkCount[(size_t)p * a.chunks + c] = 0;
        }
        return;
    }
    const float radiusBound = a.radiusPer ? a.radiusPer[p] : a.radiusBound;
    const double acceptRatio = a.ratioPer ? a.ratioPer[p] : a.acceptRatio;
    const float *__restrict__ mapPos = a.mapPts + (size_t)view * a.mapPtsStride;
    const float *__restrict__ mapDesc = b.mapDesc + (size_t)view * b.mapFrameFloats;
    const int32_t *__restrict__ mapLevel = a.mapLevel + (size_t)view * a.mapCap;
    const float *__restrict__ curPos = a.curPts + (size_t)frame * a.curPtsStride;
    const float *__restrict__ curDesc = b.curDesc + (size_t)frame * b.curFrameFloats;
    const int32_t *__restrict__ curLevel = a.curLevel + (size_t)frame * a.curCap;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long below = (1ull << lane) - 1ull;

    // the wave's F map features: wave-uniform (a feature beyond the view gets a NaN position: no test passes)
    float mx[F], my[F], mz[F];
    int lj[F], cnt[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const int j = j0 + w * F + f;
        const bool has = j < nmap;
        const int jc = has ? j : nmap - 1;
        mx[f] = has ? mapPos[3 * jc] : __builtin_nanf("");
        my[f] = mapPos[3 * jc + 1];
        mz[f] = mapPos[3 * jc + 2];
        lj[f] = mapLevel[jc];
        cnt[f] = 0;
    }

    for (int t0 = 0; t0 < ncur; t0 += kMapTile) {
        const int nt = ncur - t0 < kMapTile ? ncur - t0 : kMapTile;
        __syncthreads(); // (the previous tile has been read)
        for (int i = threadIdx.x; i < nt; i += kMapBlock) {
            const int g = t0 + i;
            s_tile[i] = make_uint4(__float_as_uint(curPos[3 * g]), __float_as_uint(curPos[3 * g + 1]),
                                   __float_as_uint(curPos[3 * g + 2]), (uint32_t)curLevel[g]);
        }
        __syncthreads();
        for (int i0 = 0; i0 < nt; i0 += 64) {
            const int i = i0 + lane;
            const bool inb = i < nt;
            const uint4 q = s_tile[inb ? i : nt - 1];
            const float px = __uint_as_float(q.x), py = __uint_as_float(q.y), pz = __uint_as_float(q.z);
            const int li = (int)q.w;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const float d0 = mx[f] - px, d1 = my[f] - py, d2 = mz[f] - pz;
                const float s = d0 * d0 + (d1 * d1 + d2 * d2); // the reference's rounding (no contraction)
                const bool hit = inb && s < radiusBound && li - 1 <= lj[f] && lj[f] <= li + 1;
                const unsigned long long bal = __ballot(hit);
                if (bal != 0ull) { // (rare; wave-uniform)
                    if (hit) {
                        const int pos = cnt[f] + __popcll(bal & below);
                        if (pos < kMapStash) s_idx[(w * F + f) * kMapStash + pos] = t0 + i;
                    }
                    cnt[f] += __popcll(bal);
                }
            }
        }
    }
    __syncthreads(); // the lists are complete

    // the value phase: the wave's short lists
    const int G = b.group;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const int nl = cnt[f] < kMapStash ? cnt[f] : kMapStash;
        if (nl == 0) continue; // (wave-uniform)
        const int slot = (w * F + f) * kMapStash;
        const float *__restrict__ mrow = mapDesc + (size_t)(j0 + w * F + f) * b.mapRowFloats;
        if (G != 0) {
            const int per = 64 / G, cl = lane / G;
            for (int c0 = 0; c0 < nl; c0 += per) {
                const int cand = c0 + cl;
                const bool valid = cand < nl;
                const int g = valid ? s_idx[slot + cand] : 0;
                const float v = l2_value_group(mrow, curDesc + (size_t)g * b.curRowFloats, valid, G, lane);
                if (valid && (lane & (G - 1)) == 0) s_val[slot + cand] = v;
            }
        } else if (lane < nl) {
            s_val[slot + lane] = l2_value_plain(mrow, curDesc + (size_t)s_idx[slot + lane] * b.curRowFloats, b.dim);
        }
    }
    __syncthreads(); // the values are complete

    // best / ratio over the short list (or further sweeps), the feature's accepted count
    unsigned long long accMask[F];
    float bestVal[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const int j = j0 + w * F + f;
        accMask[f] = 0ull;
        bestVal[f] = 0.f;
        int n = 0;
        if (cnt[f] > 0) {
            const int slot = (w * F + f) * kMapStash;
            const int nl = cnt[f] < kMapStash ? cnt[f] : kMapStash;
            const float *__restrict__ mrow = mapDesc + (size_t)j * b.mapRowFloats;
            const float v = lane < nl ? s_val[slot + lane] : 0.f;
            const float first = s_val[slot];
            // :714-727 -- the first candidate is taken whatever its value, a later one if value < bestVal (never a NaN)
            uint32_t least = wave_min_u32(lane < nl && v == v ? __float_as_uint(v) : 0x7F800000u); // (values are >= +0)
            if (cnt[f] > kMapStash) {
                const uint32_t all = map_l2_resweep<0>(mx[f], my[f], mz[f], lj[f], mrow, curPos, curDesc, b.curRowFloats, b.dim, curLevel,
                                                       ncur, radiusBound, acceptRatio, 0.f, j, nullptr);
                least = all < least ? all : least;
            }
            bestVal[f] = first == first ? __uint_as_float(least) : first;
            if (cnt[f] <= kMapStash) {
                const bool acc = lane < nl && acceptRatio * (double)v <= (double)bestVal[f];
                accMask[f] = __ballot(acc);
                n = __popcll(accMask[f]);
            } else {
                n = (int)map_l2_resweep<1>(mx[f], my[f], mz[f], lj[f], mrow, curPos, curDesc, b.curRowFloats, b.dim, curLevel, ncur,
                                           radiusBound, acceptRatio, bestVal[f], j, nullptr);
            }
        }
        if (lane == 0) s_n[w * F + f] = n;
    }
    __syncthreads();
    int total = 0, before = 0; // accepted matches of the chunk / of the features in front of this wave's
    for (int k = 0; k < CH; ++k) {
        const int n = s_n[k];
        if (k < w * F) before += n;
        total += n;
    }
    if (threadIdx.x == 0) {
        const int start = total > 0 ? atomicAdd(&a.tmpCount[p], total) : 0;
        s_start = start;
        a.chunkStart[(size_t)p * a.chunks + c] = start;
        a.chunkCount[(size_t)p * a.chunks + c] = total;
    }
    __syncthreads();
    const int start = s_start;
    // the pair overflows its row (ps_map_emit reports it from the total): nothing of it is kept
    if (total == 0 || start < 0 || start > a.maxMatches - total) return;
    PsDMatch *__restrict__ out = a.tmp + (size_t)p * a.maxMatches + start + before;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const int j = j0 + w * F + f;
        if (cnt[f] == 0) continue;
        const int slot = (w * F + f) * kMapStash;
        if (cnt[f] <= kMapStash) {
            if ((accMask[f] >> lane) & 1ull) {
                PsDMatch m;
                m.queryIdx = j;
                m.trainIdx = s_idx[slot + lane];
                m.imgIdx = -1; // default-constructed cv::DMatch (matcher.cpp:741)
                m.distance = s_val[slot + lane];
                out[__popcll(accMask[f] & below)] = m;
            }
            out += __popcll(accMask[f]);
        } else {
            out += map_l2_resweep<2>(mx[f], my[f], mz[f], lj[f], mapDesc + (size_t)j * b.mapRowFloats, curPos, curDesc, b.curRowFloats,
                                     b.dim, curLevel, ncur, radiusBound, acceptRatio, bestVal[f], j, out);
        }
    }
}

} // namespace psdev

// Host side.  Part of the device translation unit: included by ps_capi.hip behind ps_map_match.h (run_map_match's helpers) and
// ps_match_l2.h (the rules of a PsFrameSetF32).
namespace {

struct MapL2Strides { L2Strides maps, frames; };

int check_map_batch_f32(PsContext *ctx, const PsMapBatchF32 *b, MapL2Strides &strides)
{
    if (!b || b->P < 0) return fail(ctx, PS_ERR_BAD_ARG, "float map batch: null batch or P < 0");
    if (b->P == 0) return PS_OK;
    if (!b->pairs || !b->mapLevel || !b->curLevel) return fail(ctx, PS_ERR_BAD_ARG, "float map batch: null pairs / mapLevel / curLevel");
    if (int rc = check_l2_frames(ctx, b->maps, true, "float map batch: map views", strides.maps)) return rc;
    if (int rc = check_l2_frames(ctx, b->frames, true, "float map batch: frames", strides.frames)) return rc;
    if (b->maps.dim != b->frames.dim) return fail(ctx, PS_ERR_BAD_ARG, "float map batch: maps.dim and frames.dim differ");
    if (b->maxMatches < 1) return fail(ctx, PS_ERR_BAD_ARG, "float map batch: maxMatches must lie in 1 .. 1 << 22");
    if (b->maxMatches > (1 << 22)) return fail(ctx, PS_ERR_UNSUPPORTED, "float map batch: maxMatches must lie in 1 .. 1 << 22");
    return PS_OK;
}

// The two launches for a checked batch (run_map_match's layout of the shared scratch); pl = null: matches only.
int run_map_match_l2(PsContext *ctx, const PsMapBatchF32 &b, const MapL2Strides &strides, const Plan *pl, PsDMatch *dMatches,
                     int32_t *dNumMatches, int32_t **numClamped, int slot0)
{
    const int P = b.P, F = map_features_per_wave(P, b.maps.maxKpts), CH = kMapWaves * F;
    MapL2Args l{};
    MapArgs &a = l.m;
    a.mapPts = b.maps.pts; a.curPts = b.frames.pts;
    a.mapN = b.maps.nkpts; a.curN = b.frames.nkpts;
    a.mapLevel = b.mapLevel; a.curLevel = b.curLevel;
    a.mapFrames = b.maps.numFrames; a.curFrames = b.frames.numFrames;
    a.mapCap = b.maps.maxKpts; a.curCap = b.frames.maxKpts;
    a.mapPtsStride = strides.maps.ptsFloats; a.curPtsStride = strides.frames.ptsFloats;
    a.pairs = b.pairs;
    a.radiusBound = b.radiusBound; a.acceptRatio = b.acceptRatio;
    a.radiusPer = b.radiusBoundPerPair; a.ratioPer = b.acceptRatioPerPair;
    a.maxMatches = b.maxMatches;
    a.chunks = (a.mapCap + CH - 1) / CH;
    a.chunkFeatures = CH;
    l.mapDesc = b.maps.desc; l.curDesc = b.frames.desc;
    l.mapFrameFloats = strides.maps.frameFloats; l.curFrameFloats = strides.frames.frameFloats;
    l.mapRowFloats = strides.maps.rowFloats; l.curRowFloats = strides.frames.rowFloats;
    l.dim = b.maps.dim;
    // the group form's 16-byte loads: SURF / SIFT widths, every row of either set on a 16-byte boundary
    const bool aligned = (((uintptr_t)b.maps.desc | (uintptr_t)b.frames.desc) & 15) == 0 && ((l.mapRowFloats | l.curRowFloats) & 3) == 0 &&
                         ((l.mapFrameFloats | l.curFrameFloats) & 3) == 0;
    l.group = aligned && (l.dim == 64 || l.dim == 128) ? l.dim / 4 : 0;
    // scratch: the staging rows, then [P] reserved | [P] clamped | [P][chunks] start | [P][chunks] count
    PS_ENSURE(ctx->sMatches, (size_t)P * b.maxMatches * sizeof(PsDMatch));
    PS_ENSURE(ctx->sMisc2, ((size_t)2 * P + (size_t)2 * P * a.chunks) * sizeof(int32_t));
    if (pl) {
        PS_ENSURE(ctx->mvalid, (size_t)P * sizeof(int32_t));
        PS_ENSURE(ctx->cmax, (size_t)P * sizeof(float2));
        int rc = ensure_records(ctx, (size_t)P, (size_t)b.maxMatches);
        if (rc != PS_OK) return rc;
    }
    a.tmp = (PsDMatch *)ctx->sMatches.p;
    a.tmpCount = (int32_t *)ctx->sMisc2.p;
    int32_t *clamped = a.tmpCount + P;
    a.chunkStart = clamped + P;
    a.chunkCount = a.chunkStart + (size_t)P * a.chunks;
    if (numClamped) *numClamped = clamped;
    PS_HIP(hipMemsetAsync(a.tmpCount, 0, (size_t)P * sizeof(int32_t), ctx->stream));
    tick(ctx, slot0, false);
    const dim3 grid((unsigned)P * (unsigned)a.chunks), block(kMapBlock);
    switch (F) {
    case 8: hipLaunchKernelGGL(ps_map_sweep_l2<8>, grid, block, 0, ctx->stream, l); break;
    case 4: hipLaunchKernelGGL(ps_map_sweep_l2<4>, grid, block, 0, ctx->stream, l); break;
    case 2: hipLaunchKernelGGL(ps_map_sweep_l2<2>, grid, block, 0, ctx->stream, l); break;
    default: hipLaunchKernelGGL(ps_map_sweep_l2<1>, grid, block, 0, ctx->stream, l); break;
    }
    tick(ctx, slot0, true);
    PS_HIP(hipGetLastError());
    tick(ctx, slot0 + 1, false);
    const size_t lds = ((size_t)a.chunks + 1) * sizeof(int32_t);
    const bool wide = P <= kWidePairs; // a handful of pairs: 1024-thread work-groups shorten the per-pair serial walk
    const PrepArgs pa = pl ? pl->pa : PrepArgs{};
    const RecPtrs rp = pl ? rec_ptrs(ctx, pl->score) : RecPtrs{};
    int32_t *mv = (int32_t *)ctx->mvalid.p;
    float2 *cmx = (float2 *)ctx->cmax.p;
    if (pl) {
        if (wide) hipLaunchKernelGGL((ps_map_emit<true, 1024>), dim3((unsigned)P), dim3(1024), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
        else hipLaunchKernelGGL((ps_map_emit<true, kBlock>), dim3((unsigned)P), dim3(kBlock), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
    } else {
        if (wide) hipLaunchKernelGGL((ps_map_emit<false, 1024>), dim3((unsigned)P), dim3(1024), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
        else hipLaunchKernelGGL((ps_map_emit<false, kBlock>), dim3((unsigned)P), dim3(kBlock), lds, ctx->stream, a, pa, rp, dMatches, dNumMatches, clamped, mv, cmx);
    }
    tick(ctx, slot0 + 1, true);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

} // namespace

extern "C" {

size_t ps_abi_sizeof_map_batch_f32(void) { return sizeof(PsMapBatchF32); }

int ps_match_xyz_l2_f32(PsContext *ctx, const float *mapPos, const float *mapDesc, size_t mapDescStep, const int32_t *mapLevel, int nmap,
                        const float *curPos, const float *curDesc, size_t curDescStep, const int32_t *curLevel, int ncur, int dim,
                        double sphereRadius, double acceptRatio, PsDMatch *out, int cap, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    if (nout) *nout = 0;
    if (!nout || nmap < 0 || ncur < 0 || cap < 0 || dim < 1 || (cap > 0 && !out) || (nmap > 0 && (!mapPos || !mapDesc || !mapLevel)) ||
        (ncur > 0 && (!curPos || !curDesc || !curLevel)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_match_xyz_l2_f32: bad argument");
    if (dim > PS_MAX_L2_DIM) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_match_xyz_l2_f32: more than PS_MAX_L2_DIM elements per descriptor");
    const size_t row = (size_t)dim * 4;
    if ((nmap > 0 && mapDescStep < row) || (ncur > 0 && curDescStep < row))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_match_xyz_l2_f32: row pitch below dim x 4 bytes");
    if (nmap > PS_MAX_KPTS || ncur > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_match_xyz_l2_f32: more than PS_MAX_KPTS rows");
    if (nmap == 0 || ncur == 0) return PS_OK;
    const int devCap = cap < 1 ? 1 : (cap > (1 << 22) ? (1 << 22) : cap);
    PS_ENSURE(ctx->sMisc0, (size_t)nmap * 12);
    PS_ENSURE(ctx->sMisc1, (size_t)ncur * 12);
    PS_ENSURE(ctx->sDesc, (size_t)(nmap + ncur) * row);
    PS_ENSURE(ctx->sNk, (size_t)(nmap + ncur + 4) * sizeof(int32_t));
    PS_ENSURE(ctx->sMask, (size_t)devCap * sizeof(PsDMatch)); // (the device rows of `out`: sMatches is the batch's staging)
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    uint8_t *dDesc = (uint8_t *)ctx->sDesc.p;
    int32_t *dLvl = (int32_t *)ctx->sNk.p, *dMeta = dLvl + nmap + ncur;
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, mapPos, (size_t)nmap * 12, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, curPos, (size_t)ncur * 12, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc, row, mapDesc, mapDescStep, row, (size_t)nmap, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc + (size_t)nmap * row, row, curDesc, curDescStep, row, (size_t)ncur, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(dLvl, mapLevel, (size_t)nmap * 4, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(dLvl + nmap, curLevel, (size_t)ncur * 4, hipMemcpyHostToDevice, ctx->stream));
    const int32_t hostMeta[4] = {nmap, ncur, 0, 0}; // the two counts, the pair (view 0, frame 0)
    PS_HIP(hipMemcpyAsync(dMeta, hostMeta, sizeof hostMeta, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // hostMeta goes out of scope
    PsMapBatchF32 b{};
    b.maps.desc = (const float *)dDesc; b.maps.pts = (const float *)ctx->sMisc0.p; b.maps.nkpts = dMeta;
    b.maps.numFrames = 1; b.maps.maxKpts = nmap; b.maps.dim = dim;
    b.frames.desc = (const float *)(dDesc + (size_t)nmap * row); b.frames.pts = (const float *)ctx->sMisc1.p; b.frames.nkpts = dMeta + 1;
    b.frames.numFrames = 1; b.frames.maxKpts = ncur; b.frames.dim = dim;
    b.mapLevel = dLvl; b.curLevel = dLvl + nmap;
    b.pairs = dMeta + 2;
    b.P = 1;
    b.maxMatches = devCap;
    b.radiusBound = sq_bound_f32(sphereRadius); // (float)norm < (double)radius  <=>  squared sum < bound
    b.acceptRatio = acceptRatio;
    MapL2Strides strides;
    rc = check_map_batch_f32(ctx, &b, strides);
    if (rc) return rc;
    rc = run_map_match_l2(ctx, b, strides, nullptr, (PsDMatch *)ctx->sMask.p, (int32_t *)ctx->sNumM.p, nullptr, 0);
    if (rc) return rc;
    int32_t n = 0;
    PS_HIP(hipMemcpyAsync(&n, ctx->sNumM.p, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    const int total = n < 0 ? -n : n;
    *nout = total;
    if (total > cap) return fail(ctx, PS_ERR_BAD_ARG, "ps_match_xyz_l2_f32: output capacity too small (*nout = needed)");
    if (total > 0) {
        PS_HIP(hipMemcpyAsync(out, ctx->sMask.p, (size_t)total * sizeof(PsDMatch), hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PS_OK;
}

int ps_match_xyz_l2_device(PsContext *ctx, const PsMapBatchF32 *b, PsDMatch *matches, int32_t *numMatches)
{
    int rc = bind(ctx);
    if (rc) return rc;
    MapL2Strides strides;
    rc = check_map_batch_f32(ctx, b, strides);
    if (rc) return rc;
    if (b->P == 0) return PS_OK;
    if (!matches || !numMatches) return fail(ctx, PS_ERR_BAD_ARG, "ps_match_xyz_l2_device: null output");
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return run_map_match_l2(ctx, *b, strides, nullptr, matches, numMatches, nullptr, 0);
}

int ps_map_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                           const PsMapBatchF32 *b, const PsPairResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    MapL2Strides strides;
    rc = check_map_batch_f32(ctx, b, strides);
    if (rc) return rc;
    if (!out) return fail(ctx, PS_ERR_BAD_ARG, "ps_map_pairs_l2_device: null output");
    if (b->P == 0) return PS_OK;
    if (!out->matches || !out->numMatches || !out->inlierMask || !out->pose || !out->stats)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_map_pairs_l2_device: null output");
    if (cfg && cfg->sampleIdx) return fail(ctx, PS_ERR_BAD_ARG, "explicit sample streams are per call, not per batch");
    const int P = b->P, cap = b->maxMatches;
    Plan pl;
    rc = make_plan(ctx, params, cfg, K, cap, b->frames.maxKpts, pl);
    if (rc) return rc;
    begin_timed_call(ctx);
    HandoffGuard handoffGuard{ctx}; // (prepare_score below may already queue a clearing: the guard stands before it)
    rc = prepare_score(ctx, pl, P, cap, false, true, b->maps.desc);
    if (rc) return rc;
    int32_t *clamped = nullptr;
    rc = run_map_match_l2(ctx, *b, strides, &pl, out->matches, out->numMatches, &clamped, 0);
    if (rc) return rc;
    return run_ransac_stage(ctx, pl, P, cap, out->matches, clamped, cap, out->pose, out->inlierMask, out->stats, 2);
}

} // extern "C"
