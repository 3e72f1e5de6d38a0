// ps_score_value.h -- the hypothesis model and the VALUE-exact inlier test of the RANSAC core: every intermediate value of
// RANSAC.cpp:251-281,325-436 is reproduced, not only the decision (the decision-exact families are ps_score_fast.h and
// ps_score_euclid.h; they hand doubtful evaluations to inlier_test()).
//
// Kernel 3  ps_ransac_score    one lane = one 3-point hypothesis: Umeyama fit + score all M matches
//
// Also here, because kernels 3 and 4 must see the same bits: ModelArgs with the parked models, gen_model, ScoreConsts, the
// shared-reciprocal division (div2_shared) with its window checks.  The launch is launch_score in ps_ransac_stage.h (it takes the Plan).
#pragma once
#include "ps_block.h" // kBlock, xcd_remap, wave_all, add_mask
#include "ps_device_math.h"

#include "../../include/putslam_hip.h"

namespace psdev {

// ------------------------------------------------------------------------------------------
// Hypothesis model: sample -> gather 3 correspondences -> float Umeyama (+ general inverse when a
// reprojection mode needs it).  Used identically by kernel 3 (all hypotheses) and kernel 4 (the
// selected one), so both see the same bits.
// ------------------------------------------------------------------------------------------
struct ModelArgs {
    uint64_t seed;
    const uint32_t *raw;     // optional explicit draws, H x 3 (device)
    const uint64_t *seedDev; // optional: the seed lives in device memory (captured graphs replay with a new seed)
    float *models;           // optional [P][modelH][12]: kernel 3 parks hypothesis models here and kernel 4 reads the
                             // winner's instead of repeating its sample -> Umeyama -> Jacobi-SVD chain (small batches:
                             // the chain is ~10 us of latency on the critical path of a single frame pair)
    int modelH;              // hypotheses per pair that have a slot: [0, modelH).  Under a long cap (USAC's 850 000) only the
                             // leading ones are parked -- the schedules end long before -- and a hypothesis beyond is swept in
                             // one piece by stage 1 and, should it win, rebuilt by kernel 4 (the rare path)
};

PS_D void store_model(const ModelArgs &ma, size_t slot, const Rigid &m)
{
    float4 *d = reinterpret_cast<float4 *>(ma.models + slot * 12);
    d[0] = make_float4(m.R[0][0], m.R[0][1], m.R[0][2], m.R[1][0]);
    d[1] = make_float4(m.R[1][1], m.R[1][2], m.R[2][0], m.R[2][1]);
    d[2] = make_float4(m.R[2][2], m.t[0], m.t[1], m.t[2]);
}
PS_D void load_model(const ModelArgs &ma, size_t slot, Rigid &m)
{
    const float4 *d = reinterpret_cast<const float4 *>(ma.models + slot * 12);
    const float4 a = d[0], b = d[1], c = d[2];
    m.R[0][0] = a.x; m.R[0][1] = a.y; m.R[0][2] = a.z; m.R[1][0] = a.w;
    m.R[1][1] = b.x; m.R[1][2] = b.y; m.R[2][0] = b.z; m.R[2][1] = b.w;
    m.R[2][2] = c.x; m.t[0] = c.y; m.t[1] = c.z; m.t[2] = c.w;
}
PS_D uint64_t base_seed(const ModelArgs &ma) { return ma.seedDev ? *ma.seedDev : ma.seed; }

PS_D bool gen_model(const float4 *__restrict__ recA, const float4 *__restrict__ recB, size_t rbase, uint32_t M,
                    const ModelArgs &ma, uint64_t pairSeed, uint32_t h, Rigid &mdl)
{
    uint32_t idx[3];
    sample_triplet(pairSeed, ma.raw, h, M, idx);
    float src[3][3], dst[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float4 A = recA[rbase + idx[j]]; // previous frame = dst
        float4 B = recB[rbase + idx[j]]; // current frame  = src   (umeyama(cur, prev), RANSAC.cpp:225-226)
        dst[j][0] = A.x; dst[j][1] = A.y; dst[j][2] = A.z;
        src[j][0] = B.x; src[j][1] = B.y; src[j][2] = B.z;
    }
    return umeyama3(src, dst, mdl);
}

struct ScoreConsts {
    float fx, fy, cx, cy;
    double boundR; // squared-domain bound of inlierThresholdReprojection (double, cv::norm)
    float bLo, bHi; // float pre-filter band around boundR: f < bLo => surely < boundR, f > bHi => surely >= boundR
};

// ---- IEEE division without the range fix-ups, two numerators sharing one reciprocal -------------
// hipcc expands a correctly rounded float a/b into
//   div_scale(b), div_scale(a), rcp, fma, fma, mul, fma, fma, fma, div_fmas, div_fixup        (11 VALU ops)
// The two div_scale ops rescale operands only when an exponent is extreme (|b| or |a| outside roughly
// 2^+-96, a quotient that would be subnormal, a subnormal denominator); div_fmas is a plain fma when no
// scaling happened and div_fixup returns its first operand unless an operand is 0 / inf / NaN or the
// quotient leaves the normal range.  Inside the window checked by div_window_ok() none of that can
// trigger, so the sequence below IS the compiler's sequence with the no-op instructions removed and
// returns the same bits.  x*fx/z and y*fy/z share z, hence one rcp + refinement for both quotients:
// 13 VALU ops instead of 22.  Outside the window the caller uses the ordinary '/' operator.
constexpr float kDivLo = 9.094947017729282e-13f; // 2^-40
constexpr float kDivHi = 1.099511627776e12f;     // 2^+40

PS_D void div2_shared(float a0, float a1, float b, float &q0, float &q1)
{
    float r0 = __builtin_amdgcn_rcpf(b);
    float e0 = __builtin_fmaf(-b, r0, 1.0f);
    float r1 = __builtin_fmaf(e0, r0, r0);
    float m0 = a0 * r1;
    float m1 = a1 * r1;
    float f0 = __builtin_fmaf(-b, m0, a0);
    float f1 = __builtin_fmaf(-b, m1, a1);
    float g0 = __builtin_fmaf(f0, r1, m0);
    float g1 = __builtin_fmaf(f1, r1, m1);
    float h0 = __builtin_fmaf(-b, g0, a0);
    float h1 = __builtin_fmaf(-b, g1, a1);
    q0 = __builtin_fmaf(h0, r1, g0);
    q1 = __builtin_fmaf(h1, r1, g1);
}

PS_D float min3_abs(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
PS_D float max3_abs(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// Wave-level forms: every comparison is balloted on its own (a ballot of a single compare IS the compare's
// SGPR result) and the masks are combined with scalar ANDs; balloting a compound predicate would first
// materialise it in a VGPR (v_cndmask + v_cmp_ne).
// HI_HOISTED: the upper end of the window has been established for every match of the pair from
// per-hypothesis norms and the pair's largest coordinate (hi_bound_holds), only the lower end is checked here.
template <bool HI_HOISTED>
PS_D bool wave_div_window_ok(float a0, float a1, float b, float c0, float c1, float d)
{
    unsigned long long m = __builtin_amdgcn_ballot_w64(min3_abs(a0, a1, b) >= kDivLo) &
                           __builtin_amdgcn_ballot_w64(min3_abs(c0, c1, d) >= kDivLo);
    if (!HI_HOISTED)
        m &= __builtin_amdgcn_ballot_w64(max3_abs(a0, a1, b) <= kDivHi) &
             __builtin_amdgcn_ballot_w64(max3_abs(c0, c1, d) <= kDivHi);
    return m == __builtin_amdgcn_ballot_w64(true);
}

// |R x + t| <= 3 max|R_ij| max|x_i| + max|t_i| for every point of the pair (coordinates bounded by cmax),
// with 1 % slack for the float roundings of the transform and of the multiplication by fx / fy: if that
// bound times max(|fx|, |fy|, 1) stays below 2^40 no numerator or denominator of this hypothesis can leave the
// window at its upper end.  NaN / inf anywhere makes the comparison false (the per-match check then applies).
PS_D bool hi_bound_holds(const Rigid &m, float cmax, float fmaxK)
{
    float r = 0.0f, t = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) r = fmaxf(r, fabsf(m.R[i][j]));
        t = fmaxf(t, fabsf(m.t[i]));
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) finite = finite && (m.R[i][j] == m.R[i][j]);
        finite = finite && (m.t[i] == m.t[i]);
    }
    const float e = (3.0f * r * cmax + t) * 1.01f;
    return finite && (e * fmaxK <= kDivHi);
}

// true when every magnitude of both (numerator, numerator, denominator) triples lies in [2^-40, 2^40]
// (a NaN operand is ignored by min3/max3; it then yields NaN on either division path: same outcome)
PS_D bool div_window_ok(float a0, float a1, float b, float c0, float c1, float d)
{
    return min3_abs(a0, a1, b) >= kDivLo && min3_abs(c0, c1, d) >= kDivLo && max3_abs(a0, a1, b) <= kDivHi &&
           max3_abs(c0, c1, d) <= kDivHi;
}

// Reference form of the inlier test of one match under one model (RANSAC.cpp:251-281,325-436): used by
// kernel 4 for the selected hypothesis.  Kernel 3 evaluates the same arithmetic through score_accumulate().
template <int MODE>
PS_D bool inlier_test(const Rigid &mdl, const Rigid &inv, const ScoreConsts &k, const float4 &A, const float4 &B,
                      const float4 &C)
{
    float ex, ey, ez;
    xform(mdl, B.x, B.y, B.z, ex, ey, ez); // estimatedOldPosition = R * features[train] + t
    bool in = true;
    if (MODE == PS_EUCLIDEAN_ERROR || MODE == PS_ADAPTIVE_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR) {
        float d0 = ex - A.x, d1 = ey - A.y, d2 = ez - A.z;
        float s = d0 * d0 + (d1 * d1 + d2 * d2);
        in = s < A.w;
    }
    if (MODE == PS_REPROJECTION_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR) {
        float nx, ny, nz;
        xform(inv, A.x, A.y, A.z, nx, ny, nz); // estimatedNewPosition = Rinv * prev[query] + tinv
        float pnu, pnv, pou, pov;
        project(nx, ny, nz, k.fx, k.fy, k.cx, k.cy, pnu, pnv);
        project(ex, ey, ez, k.fx, k.fy, k.cx, k.cy, pou, pov);
        float dxn = pnu - C.z, dyn = pnv - C.w; // predictedNew - realNew
        float dxo = pou - C.x, dyo = pov - C.y; // predictedOld - realOld
        double e0 = (double)dxn * (double)dxn + (double)dyn * (double)dyn;
        double e1 = (double)dxo * (double)dxo + (double)dyo * (double)dyo;
        in = in && (e0 < k.boundR) && (e1 < k.boundR);
    }
    return in;
}

// Kernel 3's form of the same test: cnt += inlier.  Identical values, cheaper instruction stream:
//  * the two quotients of each projected point share one reciprocal inside the checked division window
//    (div2_shared), the whole wavefront falling back to '/' otherwise;
//  * cv::norm's double comparison is settled in float outside the band [bLo, bHi] around boundR: the float
//    sums f0, f1 are within 2^-22 of the exact values and the band's half-width is 2^-21; the larger of the
//    two (as unsigned bit patterns: sums of squares are >= +0 and any NaN sorts above +inf) decides both tests
//    at once; inside the band, or on NaN, the wavefront evaluates in double;
//  * the count is updated inside each branch, so no boolean has to be carried across the branches in a VGPR.
template <int MODE, bool HI_HOISTED>
PS_D void score_accumulate(const Rigid &mdl, const Rigid &inv, const ScoreConsts &k, const float4 &A, const float4 &B,
                           const float4 &C, int &cnt)
{
    float ex, ey, ez;
    xform(mdl, B.x, B.y, B.z, ex, ey, ez);
    bool in = true;
    if (MODE == PS_EUCLIDEAN_ERROR || MODE == PS_ADAPTIVE_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR) {
        float d0 = ex - A.x, d1 = ey - A.y, d2 = ez - A.z;
        float s = d0 * d0 + (d1 * d1 + d2 * d2);
        in = s < A.w;
    }
    if (MODE == PS_REPROJECTION_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR) {
        float nx, ny, nz;
        xform(inv, A.x, A.y, A.z, nx, ny, nz);
        float pnu, pnv, pou, pov;
        const float a0 = nx * k.fx, a1 = ny * k.fy, c0 = ex * k.fx, c1 = ey * k.fy;
        if (wave_div_window_ok<HI_HOISTED>(a0, a1, nz, c0, c1, ez)) {
            float q0, q1, q2, q3;
            div2_shared(a0, a1, nz, q0, q1);
            div2_shared(c0, c1, ez, q2, q3);
            pnu = q0 + k.cx; pnv = q1 + k.cy;
            pou = q2 + k.cx; pov = q3 + k.cy;
        } else {
            pnu = a0 / nz + k.cx; pnv = a1 / nz + k.cy;
            pou = c0 / ez + k.cx; pov = c1 / ez + k.cy;
        }
        float dxn = pnu - C.z, dyn = pnv - C.w;
        float dxo = pou - C.x, dyo = pov - C.y;
        // pre-filter only (the decision inside the band is taken in double below): one product may be fused, the
        // float sums then sit within 2^-23 of the exact values, inside the 2^-22 the band allows for
        float f0 = __builtin_fmaf(dxn, dxn, dyn * dyn), f1 = __builtin_fmaf(dxo, dxo, dyo * dyo);
        uint32_t u0, u1;
        memcpy(&u0, &f0, 4);
        memcpy(&u1, &f1, 4);
        uint32_t um = u0 > u1 ? u0 : u1;
        float fm;
        memcpy(&fm, &um, 4);
        const unsigned long long mIn = __builtin_amdgcn_ballot_w64(fm < k.bLo);
        const unsigned long long mOut = __builtin_amdgcn_ballot_w64(fm > k.bHi);
        if ((mIn | mOut) == __builtin_amdgcn_ballot_w64(true)) {
            if (MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR)
                add_mask(cnt, mIn & __builtin_amdgcn_ballot_w64(in));
            else
                add_mask(cnt, mIn);
            return;
        }
        // cold side: keep the eight f64 instructions from being speculated above the branch
        asm volatile("" : "+v"(dxn), "+v"(dyn), "+v"(dxo), "+v"(dyo));
        double e0 = (double)dxn * (double)dxn + (double)dyn * (double)dyn;
        double e1 = (double)dxo * (double)dxo + (double)dyo * (double)dyo;
        in = in && (e0 < k.boundR) && (e1 < k.boundR);
    }
    cnt += in ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// Kernel 3.  RANSAC loop body of RANSAC.cpp:93-135 for ALL hypotheses at once.
// lane = hypothesis (model in VGPRs); the match records are wave-uniform and arrive through
// scalar loads.  grid = ceil(H/256) * msplit * P work-groups in XCD-aware order; msplit > 1 splits the
// match range and merges the integer counts with atomicAdd.  __launch_bounds__(256, 6): 6 waves per SIMD
// (80 VGPRs; the one-off Jacobi-SVD prologue spills 3-5 dwords) measured 2-3 % faster than 5 waves, 8 is slower.
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kBlock, 6) void ps_ransac_score(const float4 *__restrict__ recA,
                                                          const float4 *__restrict__ recB,
                                                          const float4 *__restrict__ recC,
                                                          const int32_t *__restrict__ mvalid,
                                                          const float2 *__restrict__ cmaxArr, ModelArgs ma,
                                                          ScoreConsts k, int H, int cap, int minRun, int msplit,
                                                          int32_t *__restrict__ counts)
{
    const unsigned hb = (unsigned)((H + kBlock - 1) / kBlock);
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned bx = L % hb, by = (L / hb) % (unsigned)msplit;
    const int p = (int)(L / (hb * (unsigned)msplit));
    const int M = mvalid[p];
    if (M < minRun) return; // too few matches: kernel 4 returns identity (RANSAC.cpp:77-80)
    const int h = (int)bx * kBlock + threadIdx.x;
    const size_t rbase = (size_t)p * cap;
    const int m0 = (int)(((long long)M * by) / msplit);
    const int m1 = (int)(((long long)M * (by + 1)) / msplit);

    Rigid mdl, inv;
    bool valid = false;
    if (h < H) {
        valid = gen_model(recA, recB, rbase, (uint32_t)M, ma, base_seed(ma) + (uint64_t)p, (uint32_t)h, mdl);
        if (ma.models && by == 0 && h < ma.modelH) store_model(ma, (size_t)p * ma.modelH + h, mdl);
        if (MODE == PS_REPROJECTION_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR)
            inverse_rigid_general(mdl, inv);
    }
    int cnt = 0;
    if (MODE == PS_MAHALANOBIS_ERROR) valid = false; // dead metric in the reference: scores 0
    const float4 *__restrict__ pa = recA + rbase;
    const float4 *__restrict__ pb = recB + rbase;
    const float4 *__restrict__ pc = recC + rbase;
    if (MODE == PS_EUCLIDEAN_ERROR || MODE == PS_ADAPTIVE_ERROR) {
#pragma unroll 4
        for (int m = m0; m < m1; ++m) { // straight-line body: the unrolled loop batches the scalar record loads
            float4 A = pa[m], B = pb[m];
            score_accumulate<MODE, false>(mdl, inv, k, A, B, A, cnt);
        }
    } else {
        // wave-uniform branches inside: not unrollable.  The upper end of the division window is settled here,
        // once per hypothesis, whenever the pair's coordinate bound allows it.
        const float cmax = cmaxArr[p].x;
        const float fmaxK = fmaxf(fmaxf(fabsf(k.fx), fabsf(k.fy)), 1.0f);
        const bool hoisted = wave_all(hi_bound_holds(mdl, cmax, fmaxK) && hi_bound_holds(inv, cmax, fmaxK));
        if (hoisted) {
            for (int m = m0; m < m1; ++m) {
                float4 A = pa[m], B = pb[m], C = pc[m];
                score_accumulate<MODE, true>(mdl, inv, k, A, B, C, cnt);
            }
        } else {
            for (int m = m0; m < m1; ++m) {
                float4 A = pa[m], B = pb[m], C = pc[m];
                score_accumulate<MODE, false>(mdl, inv, k, A, B, C, cnt);
            }
        }
    }
    if (h < H) {
        if (!valid) cnt = 0; // model not computed -> iteration skipped (RANSAC.cpp:107)
        if (msplit == 1)
            counts[(size_t)p * H + h] = cnt;
        else if (cnt)
            atomicAdd(&counts[(size_t)p * H + h], cnt);
    }
}

} // namespace psdev
