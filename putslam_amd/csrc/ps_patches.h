// ps_patches.h -- MatchingOnPatches (reference include/putslam/Matcher/MatchingOnPatches.h, src/Matcher/MatchingOnPatches.cpp:14-246):
// the Gauss-Newton alignment of a feature's patch from an old image in a new one, to sub-pixel precision.
//
// The arithmetic is the reference's, operation by operation (include/putslam_hip.h states it; restated
// sequentially in tests/patches_ref.py and ps_patches_host.h, which the kernels are held to byte for byte): the patch as a
// bilinear form of four grey taps in double, the gradients as halved integer differences in float, the 3 x 3 Hessian and the
// mismatch vector as FLOAT sums taken in element order, Eigen's fixed-size inverse as the project reads it, the step and its two
// stopping rules.  Two tap rules (ps_patches_rule.h) decide the positions at which the reference reads outside its images.
//
// Shape (ps_klt.h's tracker): one wavefront per (pair, point), work-groups of up to four independent waves, no work-group
// barrier -- trip counts differ.  Element k of the patch lives on lane k % 64: each lane samples its elements and keeps patch
// (double), gx, gy (float) and three rows of per-element products in the wave's slice of dynamic LDS, sized from patchSize at
// launch (ps_patches_rule.h's patch_wave_bytes: 31 x 31 takes 27 KB, two such waves share a work-group's 64 KiB and two such
// work-groups a CU's 160 KiB).  The float sums are sequential by definition, so one lane per sum walks its row in element order:
// five for the Hessian (gx gx, gx gy, gy gy, and gx, gy themselves: J[2] = 1.f; H[2][2] counts to E exactly; J[a] J[b] = J[b] J[a]),
// three for the mismatch vector.  The sums come back through readlane, so the step and every decision are the same scalar on all
// lanes: lane 0 stores them.
// Two kernels on one body: ps_patch_model_rows (patch, gradients, inverse Hessian of points of one image) and ps_patch_align_rows,
// which builds the model from the pair's old slot (fused) or reads it from arrays (PS_PATCH_GIVEN_MODEL).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "ps_device_math.h"
#include "ps_glue.h"
#include "ps_patches_rule.h"

namespace psdev {

struct PatchArgs {
    const uint8_t *img;
    unsigned long long rowStride, frameStride;
    const int32_t *slots; // models: P; align: P x 2
    const double *oldPts; // x, y pairs: read and written as single doubles, so 8-byte alignment is enough
    double *newPts;
    const int32_t *counts;
    PsPatchModel model;
    uint8_t *status;
    int32_t *iterations;
    double minInc;
    int rows, cols, cn, frames, cap;
    int ps, h, E, E4, waveBytes, maxIter, flags;
};

// LDS traffic of one wave is ordered by the hardware; this keeps the compiler from moving accesses across the hand-over
PS_D void patch_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The row-sum idiom of ps_klt.h's klt_lane_sum: lanes 0 .. nsum-1 take row `lane` one element at a time in element order, from
// zero.  Sub: s = s - v (the mismatch vector), else s = s + v (the Hessian).  The rows are padded with +0 to a multiple of four:
// a sum that starts at +0 never becomes -0, so s +- 0 = s.
template <bool Sub> PS_D float patch_lane_walk(const float *rows, int E4, int lane, int nsum)
{
    float s = 0.f;
    if (lane < nsum) {
        const float4 *q = reinterpret_cast<const float4 *>(rows + lane * E4);
        for (int k = 0; k < E4 / 4; ++k) {
            const float4 v = q[k];
            if (Sub) {
                s = s - v.x;
                s = s - v.y;
                s = s - v.z;
                s = s - v.w;
            } else {
                s = s + v.x;
                s = s + v.y;
                s = s + v.z;
                s = s + v.w;
            }
        }
    }
    return s;
}
PS_D float patch_from_lane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// one channel as it is, three by CV_RGB2GRAY (ps_fast.h's rule)
PS_D int patch_grey(const uint8_t *__restrict__ p, int cn)
{
    return cn == 1 ? (int)p[0] : ((int)p[0] * 4899 + (int)p[1] * 9617 + (int)p[2] * 1868 + 8192) >> 14;
}

struct PatchWeights {
    double tl, tr, bl, br;
};
PS_D PatchWeights patch_weights(double x, double y, int ix, int iy)
{
    const double xs = x - (double)ix, ys = y - (double)iy;
    PatchWeights k;
    k.tl = (1.0 - xs) * (1.0 - ys);
    k.tr = xs * (1.0 - ys);
    k.bl = (1.0 - xs) * ys;
    k.br = xs * ys;
    return k;
}
// computePatch's element (:41-44) at p = &I[i][j]
PS_D double patch_sample(const uint8_t *__restrict__ p, size_t es, int cn, const PatchWeights &k)
{
    return ((k.tl * (double)patch_grey(p, cn) + k.tr * (double)patch_grey(p + cn, cn)) + k.bl * (double)patch_grey(p + es, cn)) +
           k.br * (double)patch_grey(p + es + cn, cn);
}

// every NaN written is the one quiet pattern (the host's 0 x inf carries the sign bit, this device's does not)
PS_D float patch_canon(float v) { return v == v ? v : __builtin_bit_cast(float, 0x7FC00000u); }
PS_D double patch_canon(double v) { return v == v ? v : __builtin_bit_cast(double, 0x7FF8000000000000ull); }

PS_D float patch_cof(float a, float b, float c, float d) { return a * b - c * d; }

// Align = false: the model pass.  One wavefront per (set or pair, point); dynamic LDS of waveBytes per wave.
template <bool Align> PS_D void patch_wave(const PatchArgs &a, unsigned char *lds)
{
    const int lane = (int)threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)blockDim.x >> 6, bpp = (a.cap + waves - 1) / waves;
    const int p = (int)blockIdx.x / bpp, i = ((int)blockIdx.x % bpp) * waves + w;
    const int n = a.counts[p];
    if (n < 0 || n > a.cap || i >= n) return;
    const size_t o = (size_t)p * a.cap + i;
    const bool given = Align && (a.flags & PS_PATCH_GIVEN_MODEL) != 0;
    const int s0 = Align ? a.slots[2 * p] : a.slots[p], s1 = Align ? a.slots[2 * p + 1] : 0;
    if ((!given && (unsigned)s0 >= (unsigned)a.frames) || (unsigned)s1 >= (unsigned)a.frames) { // a slot outside the set
        if (lane == 0) {
            a.status[o] = PS_PATCH_OLD_TAPS_OUTSIDE;
            if (Align) a.iterations[o] = 0;
        }
        return;
    }
    const int ps = a.ps, h = a.h, E = a.E, E4 = a.E4, cn = a.cn;
    const size_t es = (size_t)a.rowStride;
    double *sP = reinterpret_cast<double *>(lds + (size_t)w * a.waveBytes); // [E4]
    float *prod = reinterpret_cast<float *>(sP + E4);                       // [3][E4], then gx [E4], gy [E4]
    float *sGx = prod + 3 * E4, *sGy = sGx + E4;
    // (the pads of the five float rows are written here, once: the loops below write only e < E, so the pads the walks read stay +0
    // through every step; the pad of the patch's doubles, sP[E .. E4), is never written and never read)
    if (lane < E4 - E) prod[E + lane] = prod[E4 + E + lane] = prod[2 * E4 + E + lane] = sGx[E + lane] = sGy[E + lane] = 0.f;
    const int qstep = 64 / ps, rstep = 64 % ps, r0 = lane / ps, c0 = lane % ps;

    float v00, v01, v02, v10, v11, v12, v20, v21, v22; // the inverse Hessian, row-major
    if (!given) {
        const struct { double x, y; } op = {a.oldPts[2 * o], a.oldPts[2 * o + 1]};
        if (!(op.x >= (double)(h + 1) && op.x < (double)(a.cols - h - 1) && op.y >= (double)(h + 1) && op.y < (double)(a.rows - h - 1))) {
            if (lane == 0) { // patch_old_taps_inside
                a.status[o] = PS_PATCH_OLD_TAPS_OUTSIDE;
                if (Align) a.iterations[o] = 0;
            }
            return;
        }
        const int ix = (int)op.x, iy = (int)op.y;
        const PatchWeights k = patch_weights(op.x, op.y, ix, iy);
        const uint8_t *base = a.img + (size_t)s0 * a.frameStride + (size_t)(iy - h) * es + (size_t)(ix - h) * cn;
        for (int e = lane, r = r0, c = c0; e < E; e += 64) {
            const uint8_t *q = base + (size_t)r * es + (size_t)c * cn;
            const float gx = 0.5f * (float)(patch_grey(q + cn, cn) - patch_grey(q - cn, cn));
            const float gy = 0.5f * (float)(patch_grey(q + es, cn) - patch_grey(q - es, cn));
            const double v = patch_sample(q, es, cn, k);
            sP[e] = v;
            sGx[e] = gx;
            sGy[e] = gy;
            prod[e] = gx * gx;
            prod[E4 + e] = gx * gy;
            prod[2 * E4 + e] = gy * gy;
            if (a.model.patch) a.model.patch[o * E + e] = v;
            if (a.model.gx) a.model.gx[o * E + e] = gx;
            if (a.model.gy) a.model.gy[o * E + e] = gy;
            c += rstep;
            r += qstep;
            if (c >= ps) {
                c -= ps;
                ++r;
            }
        }
        patch_wave_sync();
        const float sH = patch_lane_walk<false>(prod, E4, lane, 5); // rows: gx gx, gx gy, gy gy, gx, gy
        const float m00 = patch_from_lane(sH, 0), m01 = patch_from_lane(sH, 1), m11 = patch_from_lane(sH, 2), m02 = patch_from_lane(sH, 3),
                    m12 = patch_from_lane(sH, 4), m22 = (float)E, m10 = m01, m20 = m02, m21 = m12;
        patch_wave_sync();
        // cof(i, j) = m(i1, j1) m(i2, j2) - m(i1, j2) m(i2, j1), indices cyclic
        const float c00 = patch_cof(m11, m22, m12, m21), c01 = patch_cof(m12, m20, m10, m22), c02 = patch_cof(m10, m21, m11, m20);
        const float c10 = patch_cof(m21, m02, m22, m01), c11 = patch_cof(m22, m00, m20, m02), c12 = patch_cof(m20, m01, m21, m00);
        const float c20 = patch_cof(m01, m12, m02, m11), c21 = patch_cof(m02, m10, m00, m12), c22 = patch_cof(m00, m11, m01, m10);
        const float det = (c00 * m00 + c10 * m10) + c20 * m20;
        const float invdet = ps_div(1.f, det);
        v00 = c00 * invdet, v01 = c10 * invdet, v02 = c20 * invdet;
        v10 = c01 * invdet, v11 = c11 * invdet, v12 = c21 * invdet;
        v20 = c02 * invdet, v21 = c12 * invdet, v22 = c22 * invdet;
        if (a.model.invHessian && lane == 0) {
            float *iv = a.model.invHessian + o * 9;
            iv[0] = patch_canon(v00), iv[1] = patch_canon(v01), iv[2] = patch_canon(v02), iv[3] = patch_canon(v10), iv[4] = patch_canon(v11);
            iv[5] = patch_canon(v12), iv[6] = patch_canon(v20), iv[7] = patch_canon(v21), iv[8] = patch_canon(v22);
        }
    } else {
        for (int e = lane; e < E; e += 64) {
            sP[e] = a.model.patch[o * E + e];
            sGx[e] = a.model.gx[o * E + e];
            sGy[e] = a.model.gy[o * E + e];
        }
        const float *iv = a.model.invHessian + o * 9;
        v00 = iv[0], v01 = iv[1], v02 = iv[2], v10 = iv[3], v11 = iv[4], v12 = iv[5];
        v20 = v21 = v22 = 0.f; // (the third row is not read: the reference sets increment[2] to 0)
        patch_wave_sync();
    }
    (void)v20, (void)v21, (void)v22;
    if (!Align) {
        if (lane == 0) a.status[o] = v00 != v00 ? PS_PATCH_NAN_HESSIAN : PS_PATCH_CONVERGED;
        return;
    }
    if (v00 != v00) {
        if (lane == 0) {
            a.status[o] = PS_PATCH_NAN_HESSIAN;
            a.iterations[o] = 0;
        }
        return;
    }
    const struct { double x, y; } start = {a.newPts[2 * o], a.newPts[2 * o + 1]};
    double x = start.x, y = start.y;
    const double mean = 0.0;
    const uint8_t *img1 = a.img + (size_t)s1 * a.frameStride;
    int status = PS_PATCH_MAX_ITERATIONS, iters = 0;
    for (int it = 0; it < a.maxIter; ++it) {
        if (x != x || y != y || x < (double)h || x > (double)(a.cols - h) || y < (double)h || y > (double)(a.rows - h)) {
            status = PS_PATCH_OUT_OF_IMAGE; // patch_gate_out
            break;
        }
        const int ix = (int)x, iy = (int)y;
        if (!(ix + h + 1 <= a.cols - 1 && iy + h + 1 <= a.rows - 1)) {
            status = PS_PATCH_NEW_TAPS_OUTSIDE; // patch_new_taps_inside
            break;
        }
        const PatchWeights k = patch_weights(x, y, ix, iy);
        const uint8_t *base = img1 + (size_t)(iy - h) * es + (size_t)(ix - h) * cn;
        for (int e = lane, r = r0, c = c0; e < E; e += 64) {
            const double v = patch_sample(base + (size_t)r * es + (size_t)c * cn, es, cn, k);
            const float diff = (float)((v - sP[e]) + mean);
            prod[e] = diff * sGx[e];
            prod[E4 + e] = diff * sGy[e];
            prod[2 * E4 + e] = diff;
            c += rstep;
            r += qstep;
            if (c >= ps) {
                c -= ps;
                ++r;
            }
        }
        patch_wave_sync();
        const float sT = patch_lane_walk<true>(prod, E4, lane, 3);
        const float t0 = patch_from_lane(sT, 0), t1 = patch_from_lane(sT, 1), t2 = patch_from_lane(sT, 2);
        patch_wave_sync();
        const float inc0 = (v00 * t0 + v01 * t1) + v02 * t2, inc1 = (v10 * t0 + v11 * t1) + v12 * t2;
        x = x + (double)inc0;
        y = y + (double)inc1;
        iters = it + 1;
        if ((double)(inc0 * inc0 + inc1 * inc1) < a.minInc) {
            const double dx = x - start.x, dy = y - start.y;
            status = dx * dx + dy * dy > (double)(h * h) ? PS_PATCH_MOVED_TOO_FAR : PS_PATCH_CONVERGED;
            break;
        }
    }
    if (lane == 0) {
        if (iters > 0) { // (no step: the position is untouched)
            a.newPts[2 * o] = patch_canon(x);
            a.newPts[2 * o + 1] = patch_canon(y);
        }
        a.status[o] = (uint8_t)status;
        a.iterations[o] = iters;
    }
}

constexpr int kPatchBlock = 256; // four waves at most (patch_block_waves)

__global__ __launch_bounds__(kPatchBlock) void ps_patch_model_rows(PatchArgs a)
{
    extern __shared__ __align__(16) unsigned char patchLds[];
    patch_wave<false>(a, patchLds);
}
__global__ __launch_bounds__(kPatchBlock) void ps_patch_align_rows(PatchArgs a)
{
    extern __shared__ __align__(16) unsigned char patchLds[];
    patch_wave<true>(a, patchLds);
}

} // namespace psdev

// Host side (part of the device translation unit, ps_capi.hip): the checks, the launch and the entry points
namespace {

// params and the image set as both calls take them; `a` resolved
int patch_check(PsContext *ctx, const PsImageSet *images, const PsPatchParams *params, int P, int capacity, const char *who, PatchArgs &a)
{
    const auto msg = [who](const char *what) { return std::string(who) + ": " + what; };
    if (const char *why = patch_params_error(params)) return fail(ctx, PS_ERR_BAD_ARG, msg(why).c_str());
    size_t row = 0, frame = 0;
    if (const char *why = patch_images_error(images, row, frame)) return fail(ctx, PS_ERR_BAD_ARG, msg(why).c_str());
    if (P < 0) return fail(ctx, PS_ERR_BAD_ARG, msg("P < 0").c_str());
    if (P > 0 && capacity < 1) return fail(ctx, PS_ERR_BAD_ARG, msg("capacity < 1").c_str());
    a = PatchArgs{};
    a.img = images->pixels;
    a.rowStride = row;
    a.frameStride = frame;
    a.rows = images->rows, a.cols = images->cols, a.cn = images->channels, a.frames = images->numFrames;
    a.cap = capacity;
    a.ps = params->patchSize;
    a.h = patch_half(a.ps);
    a.E = patch_elems(a.ps);
    a.E4 = patch_elems4(a.ps);
    a.waveBytes = (int)patch_wave_bytes(a.ps);
    a.maxIter = params->maxIter;
    a.flags = params->flags;
    a.minInc = params->minSqrtIncrement;
    return PS_OK;
}

int patch_launch(PsContext *ctx, const PatchArgs &a, int P, bool align, const char *who)
{
    const int waves = patch_block_waves(a.ps);
    const long long blocks = (long long)P * ((a.cap + waves - 1) / waves);
    if (blocks > INT_MAX) return fail(ctx, PS_ERR_BAD_ARG, (std::string(who) + ": sets x capacity beyond 2^31 work-groups").c_str());
    const size_t lds = (size_t)waves * a.waveBytes;
    if (align)
        hipLaunchKernelGGL(ps_patch_align_rows, dim3((unsigned)blocks), dim3((unsigned)waves * 64), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL(ps_patch_model_rows, dim3((unsigned)blocks), dim3((unsigned)waves * 64), lds, ctx->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// The host forms: one image (mode 0: the model pass) or one pair (1: fused, 2: given model), uploads included, synchronous.
// in*: the given model; out*: the model wanted back (modes 0 and 1)
int patch_host_form(PsContext *ctx, const char *who, int mode, const uint8_t *oldImg, const uint8_t *newImg, int rows, int cols, int channels,
                    size_t rowStride, const double *oldPts, double *newPts, int n, const PsPatchParams *prm, const double *inPatch,
                    const float *inGx, const float *inGy, const float *inInv, double *outPatch, float *outGx, float *outGy, float *outInv,
                    uint8_t *status, int32_t *iterations)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const auto msg = [who](const char *what) { return std::string(who) + ": " + what; };
    const bool needOld = mode != 2, needNew = mode != 0;
    if (const char *why = patch_params_error(prm)) return fail(ctx, PS_ERR_BAD_ARG, msg(why).c_str());
    if (prm->flags) return fail(ctx, PS_ERR_BAD_ARG, msg("the host forms take no flags").c_str());
    const uint8_t *imgs[2] = {needOld ? oldImg : newImg, newImg};
    const int frames = mode == 1 ? 2 : 1;
    PsImageSet is{};
    is.pixels = imgs[0]; // (the host array: checked for NULL only; the device copy is named below)
    is.rowStride = rowStride;
    is.numFrames = frames;
    is.rows = rows, is.cols = cols, is.channels = channels;
    PsPatchParams p = *prm;
    if (mode == 2) p.flags = PS_PATCH_GIVEN_MODEL;
    PatchArgs a;
    rc = patch_check(ctx, &is, &p, 1, n > 0 ? n : 1, who, a);
    if (rc) return rc;
    if (n < 0 || (needNew && !newImg) ||
        (n > 0 && (!status || (needOld && !oldPts) || (needNew && (!newPts || !iterations)) || (mode == 2 && (!inPatch || !inGx || !inGy || !inInv)))))
        return fail(ctx, PS_ERR_BAD_ARG, msg("null array or n < 0").c_str());
    if (n == 0) return PS_OK;
    TimingOff toff(ctx);
    const size_t N = (size_t)n, E = (size_t)a.E, imgBytes = image_bytes(rows, cols, channels, a.rowStride);
    // one block: the images | slots[2], count, 0 | oldPts | newPts | patch | gx | gy | invHessian | iterations | status
    BlockLayout lay;
    lay.take<uint8_t>(imgBytes, 16); // (the first image, at 0)
    const size_t oImg1 = lay.take<uint8_t>(frames == 2 ? imgBytes : 0, 16), oHead = lay.take<int32_t>(4, 16), oOld = lay.take<double>(2 * N, 16),
                 oNew = lay.take<double>(2 * N, 16), oPatch = lay.take<double>(N * E, 16), oGx = lay.take<float>(N * E, 16),
                 oGy = lay.take<float>(N * E, 16), oInv = lay.take<float>(9 * N, 16), oIt = lay.take<int32_t>(N, 16), oSt = lay.take<uint8_t>(N, 16);
    const DeviceBlock blk(lay.total);
    if (blk.err != hipSuccess) return fail(ctx, PS_ERR_ALLOC, "hipMalloc", blk.err);
    char *d = blk.p;
    const int32_t head[4] = {0, frames - 1, n, 0};
    PS_HIP(hipMemcpyAsync(d, imgs[0], imgBytes, hipMemcpyHostToDevice, ctx->stream));
    if (frames == 2) PS_HIP(hipMemcpyAsync(d + oImg1, imgs[1], imgBytes, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(d + oHead, head, sizeof head, hipMemcpyHostToDevice, ctx->stream));
    if (needOld) PS_HIP(hipMemcpyAsync(d + oOld, oldPts, N * 16, hipMemcpyHostToDevice, ctx->stream));
    if (needNew) PS_HIP(hipMemcpyAsync(d + oNew, newPts, N * 16, hipMemcpyHostToDevice, ctx->stream));
    if (mode == 2) {
        PS_HIP(hipMemcpyAsync(d + oPatch, inPatch, N * E * 8, hipMemcpyHostToDevice, ctx->stream));
        PS_HIP(hipMemcpyAsync(d + oGx, inGx, N * E * 4, hipMemcpyHostToDevice, ctx->stream));
        PS_HIP(hipMemcpyAsync(d + oGy, inGy, N * E * 4, hipMemcpyHostToDevice, ctx->stream));
        PS_HIP(hipMemcpyAsync(d + oInv, inInv, N * 36, hipMemcpyHostToDevice, ctx->stream));
    }
    // (a point with status 5 has no model: its rows come back as zeros, not as whatever the allocation held)
    if (mode != 2) PS_HIP(hipMemsetAsync(d + oPatch, 0, oIt - oPatch, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream)); // (head[] leaves scope, pageable sources may change)
    a.img = (const uint8_t *)d;
    a.frameStride = oImg1; // (a multiple of 16 at or above the image's bytes)
    a.slots = (const int32_t *)(d + oHead);
    a.counts = (const int32_t *)(d + oHead) + 2;
    a.oldPts = (const double *)(d + oOld);
    a.newPts = (double *)(d + oNew);
    a.status = (uint8_t *)(d + oSt);
    a.iterations = (int32_t *)(d + oIt);
    if (mode == 2 || outPatch) a.model.patch = (double *)(d + oPatch);
    if (mode == 2 || outGx) a.model.gx = (float *)(d + oGx);
    if (mode == 2 || outGy) a.model.gy = (float *)(d + oGy);
    if (mode == 2 || outInv) a.model.invHessian = (float *)(d + oInv);
    rc = patch_launch(ctx, a, 1, needNew, who);
    if (rc) return rc;
    PS_HIP(hipMemcpyAsync(status, d + oSt, N, hipMemcpyDeviceToHost, ctx->stream));
    if (needNew) {
        PS_HIP(hipMemcpyAsync(newPts, d + oNew, N * 16, hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipMemcpyAsync(iterations, d + oIt, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (outPatch) PS_HIP(hipMemcpyAsync(outPatch, d + oPatch, N * E * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (outGx) PS_HIP(hipMemcpyAsync(outGx, d + oGx, N * E * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (outGy) PS_HIP(hipMemcpyAsync(outGy, d + oGy, N * E * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (outInv) PS_HIP(hipMemcpyAsync(outInv, d + oInv, N * 36, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

} // namespace

static void patch_kernel_attributes()
{
    // two waves of the largest patch (31 x 31) keep 53 KiB
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ps_patch_model_rows), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ps_patch_align_rows), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
}

extern "C" {

size_t ps_abi_sizeof_patch_params(void) { return sizeof(PsPatchParams); }
size_t ps_abi_sizeof_patch_model(void) { return sizeof(PsPatchModel); }

int ps_patch_models(PsContext *ctx, const PsImageSet *images, const int32_t *slots, const double *pts, const int32_t *counts, int P, int capacity,
                    const PsPatchParams *params, const PsPatchModel *model, uint8_t *status)
{
    static const char *who = "ps_patch_models";
    int rc = bind(ctx);
    if (rc) return rc;
    PatchArgs a;
    rc = patch_check(ctx, images, params, P, capacity, who, a);
    if (rc) return rc;
    if (params->flags) return fail(ctx, PS_ERR_BAD_ARG, "ps_patch_models: the model pass takes no flags");
    if (P == 0) return PS_OK;
    if (!slots || !pts || !counts || !status) return fail(ctx, PS_ERR_BAD_ARG, "ps_patch_models: null array");
    a.slots = slots;
    a.oldPts = pts;
    a.counts = counts;
    if (model) a.model = *model; // (NULL: the statuses alone, as ps_patch_align takes it)
    a.status = status;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return patch_launch(ctx, a, P, false, who);
}

int ps_patch_align(PsContext *ctx, const PsImageSet *images, const int32_t *pairs, const double *oldPts, double *newPts, const int32_t *counts,
                   int P, int capacity, const PsPatchParams *params, const PsPatchModel *model, uint8_t *status, int32_t *iterations)
{
    static const char *who = "ps_patch_align";
    int rc = bind(ctx);
    if (rc) return rc;
    PatchArgs a;
    rc = patch_check(ctx, images, params, P, capacity, who, a);
    if (rc) return rc;
    if (P == 0) return PS_OK;
    const bool given = (params->flags & PS_PATCH_GIVEN_MODEL) != 0;
    if (!pairs || !newPts || !counts || !status || !iterations || (!given && !oldPts))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_patch_align: null array");
    if (given && (!model || !model->patch || !model->gx || !model->gy || !model->invHessian))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_patch_align: PS_PATCH_GIVEN_MODEL needs all four model arrays");
    a.slots = pairs;
    a.oldPts = oldPts;
    a.newPts = newPts;
    a.counts = counts;
    if (model) a.model = *model;
    a.status = status;
    a.iterations = iterations;
    TimingOff toff(ctx);
    HandoffGuard handoffGuard{ctx};
    return patch_launch(ctx, a, P, true, who);
}

int ps_compute_patch(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const double *pts, int n,
                     const PsPatchParams *params, double *patch, uint8_t *status)
{
    if (ctx && (!img || (n > 0 && !patch))) return fail(ctx, PS_ERR_BAD_ARG, "ps_compute_patch: null image or output");
    return patch_host_form(ctx, "ps_compute_patch", 0, img, nullptr, rows, cols, channels, rowStride, pts, nullptr, n, params, nullptr, nullptr,
                           nullptr, nullptr, patch, nullptr, nullptr, nullptr, status, nullptr);
}

int ps_compute_patch_gradient(PsContext *ctx, const uint8_t *img, int rows, int cols, int channels, size_t rowStride, const double *pts, int n,
                              const PsPatchParams *params, float *gx, float *gy, float *invHessian, uint8_t *status)
{
    if (ctx && !img) return fail(ctx, PS_ERR_BAD_ARG, "ps_compute_patch_gradient: null image");
    return patch_host_form(ctx, "ps_compute_patch_gradient", 0, img, nullptr, rows, cols, channels, rowStride, pts, nullptr, n, params, nullptr,
                           nullptr, nullptr, nullptr, nullptr, gx, gy, invHessian, status, nullptr);
}

int ps_optimize_location(PsContext *ctx, const uint8_t *oldImg, const double *oldPatch, const uint8_t *newImg, int rows, int cols, int channels,
                         size_t rowStride, double *newPts, int n, const float *gx, const float *gy, const float *invHessian,
                         const PsPatchParams *params, uint8_t *status, int32_t *iterations)
{
    (void)oldImg; // (optimizeLocation converts it to grey and reads it nowhere)
    return patch_host_form(ctx, "ps_optimize_location", 2, nullptr, newImg, rows, cols, channels, rowStride, nullptr, newPts, n, params, oldPatch,
                           gx, gy, invHessian, nullptr, nullptr, nullptr, nullptr, status, iterations);
}

int ps_optimize_locations(PsContext *ctx, const uint8_t *oldImg, const uint8_t *newImg, int rows, int cols, int channels, size_t rowStride,
                          const double *oldPts, double *newPts, int n, const PsPatchParams *params, uint8_t *status, int32_t *iterations)
{
    if (ctx && !oldImg) return fail(ctx, PS_ERR_BAD_ARG, "ps_optimize_locations: null image");
    return patch_host_form(ctx, "ps_optimize_locations", 1, oldImg, newImg, rows, cols, channels, rowStride, oldPts, newPts, n, params, nullptr,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, status, iterations);
}

} // extern "C"
