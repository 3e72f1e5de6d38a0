// ps_map_match_l2.h -- guided map matching for FLOAT descriptors (SURF / SIFT): Matcher::matchXYZ (reference
// src/Matcher/matcher.cpp:694-746) with normType = cv::NORM_L2 on CV_32F rows (:625-628), for host arrays (ps_match_xyz_l2_f32)
// and for P (map view, frame) pairs of a device-resident batch (ps_match_xyz_l2_device / ps_map_pairs_l2_device,
// include/putslam_hip.h).  The sweep, its launcher, the batch check and the entries' bodies are ps_map_match.h's; this header
// holds the VALUE of a candidate, the policy that places it in the sweep (MapL2Rows) and the batch kind (MapL2Kind).
//
// The value (tests/map_l2_ref.py is the definition; restated from OpenCV 3.x's continuous path norm() -> normL2_32f ->
// normL2Sqr<float, double>, not compiled against an OpenCV):
//   x[k] = fl32(map[k] - cur[k]);  v[k] = (double)x[k];  s = 0.0
//   blocks of four:  s = s + (((v0 v0 + v1 v1) + v2 v2) + v3 v3);  then  s = s + v v  per tail element;  value = (float)sqrt(s)
// A product of two floats is exact in double, so the roundings are the subtraction, the additions, the square root (correctly
// rounded) and the narrowing.
//
//   ps_map_sweep_l2<F>  map_sweep<F, MapL2Rows>.  The inner loop records candidate INDICES only (ballot order = ascending i):
//                       a row is 256 - 2048 B and is not touched inside the hit branch.  After the sweep the wave evaluates its
//                       features' short lists:
//                         group form (dim 64 / 128, bases and strides multiples of 16 B): dim / 4 lanes per candidate, each one
//                           16-byte load per row = one block of four; the block sums are added in block order by a chain of
//                           dim / 4 double additions over cross-lane reads;
//                         plain form (every other dim or alignment): one lane per candidate, the sequential loop.
//                       Both give the same bytes.  bestVal follows the NaN rule of :714-727: the first candidate is always
//                       taken, a later one only if value < bestVal -- a NaN first value leaves bestVal NaN and the feature
//                       emits nothing, a later NaN is ignored.
//                       A feature with more candidates than the stash holds is swept again from global memory, three times
//                       (least value, count, write), evaluating values on the way: slow and correct.
#pragma once
#include "ps_glue.h"
#include "ps_map_match.h"

namespace psdev {

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
struct MapL2Args {
    MapArgs m;
    const float *mapDesc, *curDesc;        // float rows
    size_t mapFrameFloats, curFrameFloats; // floats between views / frames
    int mapRowFloats, curRowFloats;        // floats between rows
    int dim;
    int group; // lanes per candidate of the value phase: dim / 4 (16 or 32), or 0 = one lane per candidate
};

struct MapL2Rows {
    using Args = MapL2Args;
    struct Best {}; // (nothing is evaluated during the tile loop)
    const Args &b; // (strides, dim and group are read where they are used: nothing more is live across the tile loop)
    const float *__restrict__ mapDesc, *__restrict__ curDesc;

    PS_D MapL2Rows(const Args &b, int view, int frame)
        : b(b), mapDesc(b.mapDesc + (size_t)view * b.mapFrameFloats), curDesc(b.curDesc + (size_t)frame * b.curFrameFloats)
    {
    }
    PS_D static Best none() { return {}; }
    PS_D uint32_t hit(int, int, Best &) const { return 0u; } // (the index alone; values() fills the bits in)

    // the value phase: the wave's short lists
    template <int F> PS_D void values(uint2 *lists, const int (&cnt)[F], int jw) const
    {
        const int lane = threadIdx.x & 63, G = b.group;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const int nl = cnt[f] < kMapStash ? cnt[f] : kMapStash;
            if (nl == 0) continue; // (wave-uniform)
            uint2 *list = lists + f * kMapStash;
            const float *__restrict__ mrow = mapDesc + (size_t)(jw + f) * b.mapRowFloats;
            if (G != 0) {
                const int per = 64 / G, cl = lane / G;
                for (int c0 = 0; c0 < nl; c0 += per) {
                    const int cand = c0 + cl;
                    const bool valid = cand < nl;
                    const int g = valid ? (int)list[cand].x : 0;
                    const float v = l2_value_group(mrow, curDesc + (size_t)g * b.curRowFloats, valid, G, lane);
                    if (valid && (lane & (G - 1)) == 0) list[cand].y = __float_as_uint(v);
                }
            } else if (lane < nl) {
                list[lane].y = __float_as_uint(l2_value_plain(mrow, curDesc + (size_t)(int)list[lane].x * b.curRowFloats, b.dim));
            }
        }
        __syncthreads(); // the values are complete
    }

    // :714-727 -- the first candidate is taken whatever its value, a later one if value < bestVal (never a NaN)
    PS_D float best_value(Best, const uint2 *list, int cnt, const MapSphere &s) const
    {
        const int lane = threadIdx.x & 63, nl = cnt < kMapStash ? cnt : kMapStash;
        const float v = lane < nl ? __uint_as_float(list[lane].y) : 0.f;
        const float first = __uint_as_float(list[0].y);
        uint32_t least = wave_min_u32(lane < nl && v == v ? __float_as_uint(v) : 0x7F800000u); // (values are >= +0)
        if (cnt > kMapStash) {
            const uint32_t all = map_resweep<kMapLeast>(*this, s, 0.f, nullptr); // (nothing beyond the stash has a value yet)
            least = all < least ? all : least;
        }
        return first == first ? __uint_as_float(least) : first;
    }
    PS_D float value(int j, int i) const { return l2_value_plain(mapDesc + (size_t)j * b.mapRowFloats, curDesc + (size_t)i * b.curRowFloats, b.dim); }
};

template <int F> __global__ __launch_bounds__(kMapBlock) void ps_map_sweep_l2(MapL2Args b) { map_sweep<F, MapL2Rows>(b); }

} // namespace psdev

// Host side.  Part of the device translation unit: included by ps_capi.hip behind ps_map_match.h (the launcher and the bodies of
// the entries) and ps_match_l2.h (the rules of a PsFrameSetF32).
namespace {

struct MapL2Kind {
    using Batch = PsMapBatchF32;
    using Args = MapL2Args;
    using Elem = float;
    static constexpr const char *what = "float map batch";
    static int host_rows(PsContext *ctx, int dim, bool shortPitch)
    {
        if (dim > PS_MAX_L2_DIM) return fail(ctx, PS_ERR_UNSUPPORTED, "ps_match_xyz_l2_f32: more than PS_MAX_L2_DIM elements per descriptor");
        return shortPitch ? fail(ctx, PS_ERR_BAD_ARG, "ps_match_xyz_l2_f32: row pitch below dim x 4 bytes") : PS_OK;
    }
    static void set_dim(Batch &b, int dim) { b.maps.dim = b.frames.dim = dim; }
    static MapSweeps<Args> sweeps() { return {ps_map_sweep_l2<1>, ps_map_sweep_l2<2>, ps_map_sweep_l2<4>, ps_map_sweep_l2<8>}; }
    static int sets(PsContext *ctx, const Batch &b, Args &l)
    {
        L2Strides maps, frames;
        if (int rc = check_l2_frames(ctx, b.maps, true, "float map batch: map views", maps)) return rc;
        if (int rc = check_l2_frames(ctx, b.frames, true, "float map batch: frames", frames)) return rc;
        if (b.maps.dim != b.frames.dim) return fail(ctx, PS_ERR_BAD_ARG, "float map batch: maps.dim and frames.dim differ");
        l.m.mapPtsStride = maps.ptsFloats; l.m.curPtsStride = frames.ptsFloats;
        l.mapDesc = b.maps.desc; l.curDesc = b.frames.desc;
        l.mapFrameFloats = maps.frameFloats; l.curFrameFloats = frames.frameFloats;
        l.mapRowFloats = maps.rowFloats; l.curRowFloats = frames.rowFloats;
        l.dim = b.maps.dim;
        // the group form's 16-byte loads: SURF / SIFT widths, every row of either set on a 16-byte boundary
        const bool aligned = (((uintptr_t)b.maps.desc | (uintptr_t)b.frames.desc) & 15) == 0 && ((l.mapRowFloats | l.curRowFloats) & 3) == 0 &&
                             ((l.mapFrameFloats | l.curFrameFloats) & 3) == 0;
        l.group = aligned && (l.dim == 64 || l.dim == 128) ? l.dim / 4 : 0;
        return PS_OK;
    }
};

} // namespace

extern "C" {

size_t ps_abi_sizeof_map_batch_f32(void) { return sizeof(PsMapBatchF32); }

int ps_match_xyz_l2_f32(PsContext *ctx, const float *mapPos, const float *mapDesc, size_t mapDescStep, const int32_t *mapLevel, int nmap,
                        const float *curPos, const float *curDesc, size_t curDescStep, const int32_t *curLevel, int ncur, int dim,
                        double sphereRadius, double acceptRatio, PsDMatch *out, int cap, int *nout)
{
    return match_xyz_host<MapL2Kind>(ctx, "ps_match_xyz_l2_f32", mapPos, mapDesc, mapDescStep, mapLevel, nmap, curPos, curDesc, curDescStep,
                                     curLevel, ncur, dim, sphereRadius, acceptRatio, out, cap, nout);
}

int ps_match_xyz_l2_device(PsContext *ctx, const PsMapBatchF32 *b, PsDMatch *matches, int32_t *numMatches)
{
    return match_xyz_body<MapL2Kind>(ctx, "ps_match_xyz_l2_device", b, matches, numMatches);
}

int ps_map_pairs_l2_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                           const PsMapBatchF32 *b, const PsPairResults *out)
{
    return map_pairs_body<MapL2Kind>(ctx, "ps_map_pairs_l2_device", params, cfg, K, b, out);
}

} // extern "C"
