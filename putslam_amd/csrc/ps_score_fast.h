// ps_score_fast.h -- kernel 3 for the reprojection metric, decision-exact instead of value-exact.
//
// RANSAC::computeInlierRatioReprojection (reference src/TransformEst/RANSAC.cpp:325-375) decides, for every
// (hypothesis, match), whether two reprojection errors stay below inlierThresholdReprojection.  Only that
// DECISION has to equal the reference's; ps_ransac_score<1> (ps_score_value.h) reproduces every intermediate VALUE
// bit for bit (two rigid transforms without FMA, four IEEE quotients, two cv::norm tests: 61 VALU instructions
// per evaluation).  This kernel takes the decision from a cheap evaluation with a proven error band and hands the
// evaluations that fall inside the band to the value-exact code:
//
//   fast evaluation (21 VALU instructions, 16 of them v_pk_*_f32 over the two directions): both transforms as FMA
//   chains with the camera constants folded into the model rows (X~ = fx (R p + t)_x, ..., Z~ = (R p + t)_z) and the
//   test taken in the MULTIPLIED domain, without any division:
//       reference:  dx = fl(fl(fl(e_x fx) / e_z) + cx) - u_real,   inlier <=> dx^2 + dy^2 < boundR  (both directions)
//       here:       A~ = X~ + (cx - u_real) Z~  ~  dx * e_z,        s~ = A~^2 + B~^2  against  T^2 Z~^2,  T = sqrt(boundR)
//   (offsets c - real come from a per-match record; the reciprocal form of this kernel, 24 instructions with two
//   v_rcp_f32 and a depth floor, is kept in profiles/variants/ps_score_fast_rcp.h.txt: same speed within 1 %, 0.11 % instead
//   of 0.07 % of the evaluations parked, and it needs v_rcp_f32's 1-ulp accuracy as an assumption).
//
//   error band.  u = 2^-24.  For one hypothesis let S >= sum_j |R_ij| |p_j| + |t_i| for every row of the model and of
//   its inverse and every point of the pair (S = 1.001 (rho * cmax + tau), rho = largest row sum of |R|, tau = largest
//   |t|, cmax = the pair's largest coordinate); then |e_z| <= S.  Against the real number A* = fx E_x + (cx - u_real) E_z
//   (E = the real-valued transform):
//     reference:  dx e_z = (1+d4)[(1+d3)(1+d2) c0 + (1+d3) cx e_z - u_real e_z],  c0 = fl(e_x fx), e_x within g4 S of E_x
//                 => |dx e_z - A*| <= u S (8.03 fmaxK + 5.02 Umax + 3.02 cmaxK)      (Umax = the pair's largest |c - real|)
//     here:       A~ = fl(fma(k, Z~, X~)), X~ within 4.01 u fmaxK S of fx E_x, Z~ within 3.01 u S of E_z, k = fl(cx - u_real)
//                 => |A~ - A*|     <= u S (5.02 fmaxK + 5.03 Umax)
//   so each of the four products the comparison is about is within  E = lambda S,  lambda = 1.05 u (14 fmaxK + 11 Umax +
//   4 cmaxK), of the fast value, and |e_z - Z~| <= 8 u S.  With w = |Z~|, G = sqrt2 E + T 8 u S (triangle inequality on
//   the 2-vector (dx e_z, dy e_z) and on the right-hand side T |e_z|):
//       s~ < w (T^2 (1 - 16u) w - 2 T' G)                   =>  the reference's test passes      (certain inlier)
//       s~ > w (T'^2 w + 2 T' G) + G^2 (1 + 1e-4)           =>  it fails                          (certain outlier:
//                                                                had it passed, s~ would be below this limit)
//   with T' = T (1 + 1e-5).  Round 4 evaluates both with per-HYPOTHESIS coefficients: 2 T' G w <= T' G (eps w^2 + 1 / eps) for
//   any eps > 0, so  (T^2 (1 - 20u) - T' G eps) q - T' G / eps - G^2  and  (T'^2 + T' G eps) q + T' G / eps + G^2 (1 + 1e-4),  q = Z~^2,
//   are valid (slightly wider) limits: one packed FMA each on q, constants rounded to the safe side (rebuild()).  (Round 3 had a
//   per-match band 2 T' G |Z~| + G^2: two plain FMAs with the |.| source modifier more per evaluation.)  No depth floor is
//   needed: the errors are absolute, not divided by Z~; for |Z~| -> 0 the lower limit turns negative (never "inlier") and the
//   upper one tends to its constant term, the noise level of s~ itself (then "uncertain", not "outlier").
//   Anything else -- inside the band, NaN -- is "uncertain".
//
//   uncertain evaluations are parked as (match, lane) in a wave-private LDS queue and evaluated later by the
//   value-exact inlier_test<MODE>() (the model is parked in LDS at the start), densely packed: one lane per parked
//   evaluation instead of one whole wavefront per uncertain match.  Counts therefore equal ps_ransac_score<1>'s
//   for every hypothesis (tests: test_hypothesis_counts_bit_exact, test_score_variants_*, the fuzz slice).
//
// A wavefront whose bounds do not hold (non-finite model, S fmaxK > 2^40, threshold outside [1e-10, 1e15]) runs
// the value-exact loop of ps_score_value.h instead.
//
// The staged-scoring protocol around the sweep (StageArgs, the replay of the prefix, the frame of a pass and the walk of a work-group
// over its passes) is ps_score_pass.h's, shared with ps_score_euclid.h; ps_stage_reorder, which runs between stage 0 and stage 1 of
// either family, is at the end of this file.
#pragma once

#include "ps_score_pass.h"

namespace psdev {

struct FastConsts {
    float fmaxK;  // max(|fx|, |fy|, 1)
    float cmaxK;  // max(|cx|, |cy|)
    float thrUp;  // sqrt(boundR) (1 + 1e-5), rounded up
    float bIn0;   // boundR (1 - 20u), rounded down
    float cIn;    // 2 sqrt2 sqrt(boundR) (1 + 1e-5), rounded up
    float thr2Up; // thrUp^2, rounded up
    float cHi;    // (2 c + c^2) thrUp with c = sqrt2 (1 + 1e-5), rounded up
    int enabled;  // thresholds and camera constants inside the range the bounds were derived for
};

constexpr int kQueueCap = 256; // parked evaluations per wave (drained by the wave itself when full)

// Both folded models of one hypothesis, packed across the two directions for v_pk_fma_f32:
// .x = current point -> previous image (model), .y = previous point -> current image (inverse model).
// (twelve named pairs, not arrays of pairs: the compiler merged array neighbours into 4-vectors and took them apart again
// through scratch memory)
struct FastModel {
    v2f_t r00, r01, r02, t0; // fx * row 0, fx * t_0
    v2f_t r10, r11, r12, t1; // fy * row 1, fy * t_1
    v2f_t r20, r21, r22, t2; // row 2, t_2
};

PS_D void make_fast(const Rigid &m, const Rigid &inv, float fx, float fy, FastModel &f)
{
    f.r00 = v2f_t{fx * m.R[0][0], fx * inv.R[0][0]};
    f.r01 = v2f_t{fx * m.R[0][1], fx * inv.R[0][1]};
    f.r02 = v2f_t{fx * m.R[0][2], fx * inv.R[0][2]};
    f.r10 = v2f_t{fy * m.R[1][0], fy * inv.R[1][0]};
    f.r11 = v2f_t{fy * m.R[1][1], fy * inv.R[1][1]};
    f.r12 = v2f_t{fy * m.R[1][2], fy * inv.R[1][2]};
    f.r20 = v2f_t{m.R[2][0], inv.R[2][0]};
    f.r21 = v2f_t{m.R[2][1], inv.R[2][1]};
    f.r22 = v2f_t{m.R[2][2], inv.R[2][2]};
    f.t0 = v2f_t{fx * m.t[0], fx * inv.t[0]};
    f.t1 = v2f_t{fy * m.t[1], fy * inv.t[1]};
    f.t2 = v2f_t{m.t[2], inv.t[2]};
}

// The two limits of the reprojection test from TWO register pairs, K = (kLo, kHi) and G = (G2p, -G2p), with the halves
// broadcast by op_sel:   lower = kLo * q - G2p   (K.x, q, G.y)      upper = kHi * q + G2p   (K.y, q, G.x)
// (inline asm: left to the register allocator the broadcasts became v_mov pairs inside the hot loop in two of the builds)
PS_D v2f_t limit_lower(v2f_t K, v2f_t q, v2f_t G)
{
    v2f_t r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[0,1,1]" : "=v"(r) : "v"(K), "v"(q), "v"(G));
    return r;
}
PS_D v2f_t limit_upper(v2f_t K, v2f_t q, v2f_t G)
{
    v2f_t r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "=v"(r) : "v"(K), "v"(q), "v"(G));
    return r;
}

// The two directions are .x: predictedOld - realOld and .y: predictedNew - realNew.  Operand pairs (cur, prev) of the three
// coordinates and the offset pairs (cx - uOld, cx - uNew), (cy - vOld, cy - vNew).
// Division-free form: A~ = X~ + k Z~ ~ (predicted - real) * depth; returns s~ = A~^2 + B~^2 of the two directions and
// Z~ of the two projected depths.
PS_D v2f_t fast_sq2(const FastModel &f, v2f_t px, v2f_t py, v2f_t pz, v2f_t kx, v2f_t ky, v2f_t &Zout)
{
    const v2f_t X = pk_fma(f.r00, px, pk_fma(f.r01, py, pk_fma(f.r02, pz, f.t0)));
    const v2f_t Y = pk_fma(f.r10, px, pk_fma(f.r11, py, pk_fma(f.r12, pz, f.t1)));
    const v2f_t Z = pk_fma(f.r20, px, pk_fma(f.r21, py, pk_fma(f.r22, pz, f.t2)));
    const v2f_t Au = pk_fma(kx, Z, X);
    const v2f_t Bv = pk_fma(ky, Z, Y);
    Zout = Z;
    return pk_fma(Au, Au, Bv * Bv);
}


// Two record forms.  BIG (launches that fill the chip several times over): the packed 40-byte match record (RecPtrs::F: the
// loop is sensitive to the scalar-cache footprint of the records every wave streams).  Small launches are bound by the
// latency of ONE prologue and of cold record loads: the three 16-byte records, whose loads go out side by side.
// MODE = EUCLIDEAN_AND_REPROJECTION_ERROR (RANSAC.cpp:377-436: both reprojection errors AND the Euclidean residual below their
// thresholds) adds the Euclidean term of ps_score_euclid.h to every evaluation: the unfolded current -> previous transform as
// three FMA chains (plain instructions: only one direction has a Euclidean test), the squared residual against the same
// per-lane limits lo / hi; "inlier" needs both certain, one certain "outlier" suffices, anything else is parked and decided by
// inlier_test<2>().  40 vector instructions per evaluation instead of 61 + the Euclidean part of the value-exact kernel.
// KIND: what the launch scores (StageArgs, ps_score_pass.h).
// Registers: the library is built with the SLP vectoriser and VectorCombine off (Makefile).  With them the scalar prologue
// (sample -> Umeyama -> SVD -> general inverse) was turned into packed instructions whose aligned register pairs and
// shuffles cost 20 registers: 72 VGPRs + 12 ... 19 values per lane in scratch memory at seven waves per SIMD (0.4 GB of HBM
// traffic per 499 pairs, profiles/r03i) against 56 VGPRs, no scratch memory and eight waves without (profiles/r03l).  The
// epilogues still derive the hypothesis index again instead of keeping it across the loops.
// One pass of a work-group in the frame of ps_score_pass.h.  Around the frame: a wavefront without a hypothesis skips the sweep but
// goes on to the work-group's final drain; the pair's bound is read after the model is parked; s_cnt is this kernel's own.
template <int MODE, bool BIG, int KIND>
PS_D bool score_fast_pass(const float4 *__restrict__ recA, const float4 *__restrict__ recB, const float4 *__restrict__ recC,
                          const float4 *__restrict__ recE, const float2 *__restrict__ recF,
                          const float2 *__restrict__ pairBound, const ModelArgs &ma, const ScoreConsts &k,
                          const FastConsts &fc, const EuclidConsts &ec, const SelectArgs &sa, const StageArgs &st, int H, int cap,
                          int msplit, int32_t *__restrict__ counts, unsigned long long *__restrict__ dbg, const unsigned bx,
                          const unsigned by, const int p, const int M)
{
    constexpr bool EUCLID = MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR;
    __shared__ LdsModels s_mdl;
    __shared__ uint32_t s_q[kBlock / 64][kQueueCap];
    __shared__ int s_cnt[kBlock];
    __shared__ int s_tot[kBlock]; // kind 2, split match range: the counts of the range's parts meet here
    __shared__ int s_pref[2];
    __shared__ int s_qn[kBlock / 64]; // what each wave leaves to the work-group's final drain
    static_assert(kBlock / 64 == 4, "the final drain finds an entry's wave among four");

    const size_t rbase = (size_t)p * cap;
    int32_t *__restrict__ cout = counts + (size_t)p * H;
    constexpr bool pruned = KIND >= 1;
    PassState ps;
    if (const PassGo go = pass_begin<KIND>(ps, ma, sa, st, cout, s_tot, s_pref, msplit, bx, by, p, M)) return go == kPassDone;
    const int tid = ps.tid, lane = ps.lane, wv = ps.wv, m0 = ps.m0, m1 = ps.m1;

    // (a wavefront without a hypothesis of its own goes to the barriers of the work-group's final drain and takes its share of
    // the entries; the models-only launch has neither)
    const bool idle = wave_idle(ps);
    if (KIND == 0 && st.genOnly && idle) return false;

    const float4 *__restrict__ pa = recA + rbase;
    const float4 *__restrict__ pb = recB + rbase;
    const float4 *__restrict__ pc = recC + rbase;
    const float4 *__restrict__ pe = recE + rbase;
    const float2 *__restrict__ pf = recF + rbase * 5;
    // position of the hot record -> match of the original record arrays (stages after ps_stage_reorder; the cold paths)
    const int32_t *__restrict__ pperm = (pruned && st.perm != nullptr) ? st.perm + rbase : nullptr;
    auto orig = [&](int m) { return pperm != nullptr ? pperm[m] : m; };

    bool valid = false;
    int cnt = 0;
    int qn = 0;                      // parked evaluations of this wave (wave-uniform)
    unsigned long long parked = 0;
    bool swept = false;              // the decision-exact sweep ran (wave-uniform): its counts are in s_cnt, its statistics due
    int mFrontS = 0, mPairsS = 0, frontParkTripsS = 0; // (statistics of the sweep, reported after the final drain)
    if (!idle) { // (not indented: down to the final drain)
    Rigid mdl;
    set_identity(mdl);
    pass_model<KIND>(ps, recA, recB, rbase, ma, st, H, bx, by, p, M, mdl, valid);
    if (KIND == 0 && st.genOnly) return false; // (stage 0, first launch: models and validity only)
    lds_put_model(s_mdl, tid, mdl);
    s_cnt[tid] = 0;

    const float2 pbnd = pairBound[p];
    const float cmax = pbnd.x, umax = pbnd.y;

    // The model leaves the registers here: everything below reads it back from LDS.
    // Everything the hot loop keeps in registers per hypothesis -- the folded models and the band coefficients -- is
    // (re)built by rebuild() from the model parked in LDS: once before the loop and again after every in-loop drain, so that
    // none of it has to stay alive across the drain's register-hungry code (kept alive it was spilled to scratch on
    // every launch: 40 dwords per lane, 349 MB of writes per 499 pairs, profiles/r02d).  The size S the bounds hang on
    // comes out of the same pass (one general inverse per hypothesis, not two).
    {
        FastModel F;
        // per-hypothesis coefficients of the two limits (see rebuild), held as TWO register pairs whose halves the packed FMAs
        // broadcast through op_sel (limit_lower / limit_upper)
        v2f_t KL, GG; // KL = (kLo, kHi), GG = (G2p, -G2p)
        float S;
        float U[3][4];          // EUCLID: the unfolded model (R | t), current point -> previous frame
        float loE = 0.0f, hiE = 0.0f; // EUCLID: per-lane limits of the squared residual (ps_score_euclid.h)
        // uniform part of the band: E = lambda S, |e_z - Z~| <= 8 u S, G = (sqrt2 lambda + 8 u T') S = g S
        const float lam = 1.05f * kEpsU * (14.0f * fc.fmaxK + 11.0f * umax + 4.0f * fc.cmaxK);
        const float g = 1.4143f * lam + 8.0f * kEpsU * fc.thrUp;
        auto rebuild = [&]() {
            Rigid md, iv;
            lds_get_model(s_mdl, tid, md);
            // md: current point -> previous image (estimatedOldPosition, RANSAC.cpp:346);
            // iv: previous point -> current image (estimatedNewPosition, RANSAC.cpp:348)
            inverse_rigid_general(md, iv);
            make_fast(md, iv, k.fx, k.fy, F);
            float rho2 = 0.0f, tau2 = 0.0f;
            model_norms(md, rho2, tau2);
            model_norms(iv, rho2, tau2);
            S = (rho2 * cmax + tau2) * 1.001f;
            const float G = S * g;
            // The limits  T^2 (1 - 16u) w^2 - 2 T' G w  and  T'^2 w^2 + 2 T' G w + G^2 (1 + 1e-4)  (w = |Z~|) with the linear term
            // bounded by the quadratic one:  2 T' G w <= T' G (eps w^2 + 1 / eps)  for ANY eps > 0 (AM-GM), so
            //     lower limit >= (T^2 (1 - 16u) - T' G eps) q - T' G / eps - G^2 (1 + 1e-4),   q = Z~^2
            //     upper limit <= (T'^2          + T' G eps) q + T' G / eps + G^2 (1 + 1e-4)
            // are valid limits too -- a little wider than the exact ones except at w = 1 / eps -- and have per-HYPOTHESIS
            // coefficients: one packed FMA per limit on q, no |Z~| and no per-match band (round 3: two plain v_fma_f32 with the
            // |.| modifier per evaluation; 23 -> 21 vector instructions, 19 -> 17 per pre-tested pair of matches).
            // eps = 2 / cmax puts the tangent point in the middle of the pair's depth range; the band is 0.1 % of the
            // evaluations wide either way.  Roundings: 1e-6 / 1e-5 relative slack on every constant covers the few float
            // roundings of the constants themselves (<= 6e-8 each), the rounding of q (u) and of the limit's FMA (u).
            const float eps = 2.0f / cmax;
            const float TG = (fc.thrUp * G) * 1.00001f;
            const float cQ = (TG * eps) * 1.00001f;
            const float G2p = ((TG / eps) * 1.00001f + (G * G) * 1.0001f) * 1.00002f;
            // (kLo is negative for a band wider than the threshold: then never "certainly inside")
            KL = v2f_t{fc.bIn0 * 0.999999f - cQ, fc.thr2Up * 1.000001f + cQ};
            GG = v2f_t{G2p, -G2p};
            if (EUCLID) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) U[i][j] = md.R[i][j];
                    U[i][3] = md.t[i];
                }
                float rhoE = 0.0f, tauE = 0.0f;
                model_norms(md, rhoE, tauE);
                const float aE = ((rhoE * cmax + tauE) * 1.001f) * (12.7f * kEpsU);
                const float xl = ec.tbLo - aE;
                loE = xl > 0.0f ? (xl * xl) * (1.0f - 8.0f * kEpsU) : -1.0f;
                const float yh = ec.tbHi + aE * (1.0f + 4.0f * kEpsU);
                hiE = (yh * yh) * (1.0f + 8.0f * kEpsU);
            }
        };
        rebuild();
        // (comparisons are false for NaN: a non-finite model, cmax or umax sends the wavefront to the value-exact loop)
        const bool boundsOk = fc.enabled != 0 && S * fc.fmaxK <= kDivHi && S >= 1.0e-20f && umax <= 1.0e7f &&
                              (!EUCLID || (ec.enabled != 0 && cmax <= 1.0e15f));
        if (!wave_all(boundsOk)) {
            Rigid md, iv;
            lds_get_model(s_mdl, tid, md);
            inverse_rigid_general(md, iv);
            for (int m = m0; m < m1; ++m) {
                const int mo = orig(m);
                const float4 A = pa[mo], B = pb[mo], C = pc[mo];
                score_accumulate<MODE, false>(md, iv, k, A, B, C, cnt);
            }
        } else {
        // value-exact evaluation of the parked (match, lane) pairs, one lane each: the wave's own drain, when its queue is full
        // in the middle of the sweep (what is left at the end goes to the work-group's final drain, below)
        auto drain = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int e = lane; e < qn; e += 64) {
                const uint32_t ent = s_q[wv][e];
                const int t = wv * 64 + (int)(ent & 63u), m = orig((int)(ent >> 6));
                Rigid md, iv;
                lds_get_model(s_mdl, t, md);
                inverse_rigid_general(md, iv);
                const float4 A = pa[m], B = pb[m], C = pc[m];
                if (inlier_test<MODE>(md, iv, k, A, B, C)) atomicAdd(&s_cnt[t], 1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            parked += (unsigned long long)qn;
            qn = 0;
        };

        const unsigned long long execAll = __builtin_amdgcn_ballot_w64(true);
        // one match: its record as the five operand pairs (cur.x, prev.x) (cur.y, prev.y) (cur.z, prev.z) (cx - uOld, cx - uNew)
        // (cy - vOld, cy - vNew)
        // (held as five 64-bit scalars = the aligned register pairs the packed instructions take)
        struct Rec {
            unsigned long long q[5];
        };
        auto pair64 = [](float lo, float hi) {
            return (unsigned long long)__builtin_bit_cast(uint32_t, lo) | ((unsigned long long)__builtin_bit_cast(uint32_t, hi) << 32);
        };
        // (BIG: rp = the packed record of match m, kept as a running pointer -- recomputed from the index every trip it cost a
        // multiply, a sign extension, a 64-bit shift and a 64-bit add per record on the scalar unit, which the probe of round 4
        // showed to be nearly as loaded as the vector ALU in this loop)
        auto load_rec = [&](int m, const unsigned long long *__restrict__ rp) {
            Rec r;
            if (BIG) {
#pragma unroll
                for (int i = 0; i < 5; ++i) r.q[i] = rp[i];
            } else {
                const float4 A = pa[m], B = pb[m], E = pe[m];
                r.q[0] = pair64(B.x, A.x); r.q[1] = pair64(B.y, A.y); r.q[2] = pair64(B.z, A.z);
                r.q[3] = pair64(E.x, E.y); r.q[4] = pair64(E.z, E.w);
            }
            return r;
        };
        // decides one match for the 64 hypotheses of the wavefront: counts the certain inliers, returns the DECIDED lanes
        // (the undecided ones are worked out only when a trip has any: two scalar instructions less per evaluation)
        auto eval = [&](const Rec &r) -> unsigned long long {
            v2f_t Z;
            const v2f_t e0 = __builtin_bit_cast(v2f_t, r.q[0]), e1 = __builtin_bit_cast(v2f_t, r.q[1]),
                        e2 = __builtin_bit_cast(v2f_t, r.q[2]), e3 = __builtin_bit_cast(v2f_t, r.q[3]),
                        e4 = __builtin_bit_cast(v2f_t, r.q[4]);
            const v2f_t ss = fast_sq2(F, e0, e1, e2, e3, e4, Z);
            // the match's current and previous point (wave-uniform)
            const float cxm = e0.x, cym = e1.x, czm = e2.x, pxm = e0.y, pym = e1.y, pzm = e2.y;
            // limits  kLo Z~^2 - G2p  and  kHi Z~^2 + G2p  with the per-hypothesis coefficients of rebuild()
            const v2f_t q = Z * Z;
            const v2f_t lo = limit_lower(KL, q, GG);
            const v2f_t hi = limit_upper(KL, q, GG);
            // (scalar copies: comparisons on vector-element expressions; any NaN makes all four comparisons false)
            const float se = ss.x, sn = ss.y, loe = lo.x, lon = lo.y, hie = hi.x, hin = hi.y;
            unsigned long long mIn =
                __builtin_amdgcn_ballot_w64(se < loe) & __builtin_amdgcn_ballot_w64(sn < lon);
            unsigned long long mOut =
                __builtin_amdgcn_ballot_w64(se > hie) | __builtin_amdgcn_ballot_w64(sn > hin);
            if (EUCLID) {
                const float d0 = __builtin_fmaf(U[0][0], cxm, __builtin_fmaf(U[0][1], cym, __builtin_fmaf(U[0][2], czm, U[0][3]))) - pxm;
                const float d1 = __builtin_fmaf(U[1][0], cxm, __builtin_fmaf(U[1][1], cym, __builtin_fmaf(U[1][2], czm, U[1][3]))) - pym;
                const float d2 = __builtin_fmaf(U[2][0], cxm, __builtin_fmaf(U[2][1], cym, __builtin_fmaf(U[2][2], czm, U[2][3]))) - pzm;
                const float sE = __builtin_fmaf(d0, d0, __builtin_fmaf(d1, d1, d2 * d2));
                mIn &= __builtin_amdgcn_ballot_w64(sE < loE);
                mOut |= __builtin_amdgcn_ballot_w64(sE > hiE);
            }
            add_mask(cnt, mIn);
            return mIn | mOut;
        };
        // Stage 1 on the reordered record starts with the matches EVERY voter rejected (the wrong correspondences): nearly
        // every hypothesis rejects them too, and one direction of the test is enough to know -- current point -> previous
        // image alone.  ps_stage_reorder lays that direction's operands out two MATCHES per record (StageArgs::frontRec), so
        // one packed chain decides a pair of matches in 19 vector instructions instead of 2 x 23: a lane whose squared error is
        // above the upper limit is a certain outlier -- the values are the .x lanes of eval() bit for bit (same operations, same
        // order; the model's .x halves are broadcast), so eval() would say the same -- and every other lane (under 1 %: mostly
        // the hypotheses that were sampled from that very match) is parked for the value-exact test like an undecided one.
        // Neither the matches' full records nor the other direction are touched.
        auto bx2 = [](float v) { return v2f_t{v, v}; };
        auto not_out2 = [&](const float2 *__restrict__ fr, unsigned long long &ua, unsigned long long &ub) {
            const unsigned long long *__restrict__ e = reinterpret_cast<const unsigned long long *>(fr);
            const unsigned long long q0 = e[0], q1 = e[1], q2 = e[2], q3 = e[3], q4 = e[4];
            const v2f_t cx = __builtin_bit_cast(v2f_t, q0), cy = __builtin_bit_cast(v2f_t, q1), cz = __builtin_bit_cast(v2f_t, q2),
                        kx = __builtin_bit_cast(v2f_t, q3), ky = __builtin_bit_cast(v2f_t, q4);
            const v2f_t X = pk_fma(bx2(F.r00.x), cx, pk_fma(bx2(F.r01.x), cy, pk_fma(bx2(F.r02.x), cz, bx2(F.t0.x))));
            const v2f_t Y = pk_fma(bx2(F.r10.x), cx, pk_fma(bx2(F.r11.x), cy, pk_fma(bx2(F.r12.x), cz, bx2(F.t1.x))));
            const v2f_t Z = pk_fma(bx2(F.r20.x), cx, pk_fma(bx2(F.r21.x), cy, pk_fma(bx2(F.r22.x), cz, bx2(F.t2.x))));
            const v2f_t A = pk_fma(kx, Z, X), B = pk_fma(ky, Z, Y);
            const v2f_t ss = pk_fma(A, A, B * B);
            const v2f_t q = Z * Z;
            const v2f_t hi = limit_upper(KL, q, GG); // (eval()'s limit, bit for bit)
            const float sa = ss.x, sb = ss.y, ha = hi.x, hb2 = hi.y;
            ua = __builtin_amdgcn_ballot_w64(sa > ha); // decided = certainly out (NaN: not "above": parked)
            ub = __builtin_amdgcn_ballot_w64(sb > hb2);
        };
        // (only stage 1 sweeps the front.  profiles/r03n: stage 1 640 -> 563 us with errorVersion 1, -11 % of the scoring step
        // with errorVersion 2; the pre-test leaves 0.9 % of its trips with a lane to park.)
        constexpr bool PRE = KIND == 1;
        int mFront = m0; // matches [m0, mFront): the all-reject front of the reordered record
        // (the launch passes the front record as recE, which the packed-record build does not read otherwise: only loads
        // through a __restrict__ kernel argument become scalar loads -- through the pointer inside StageArgs they were
        // vector loads of one address by 64 lanes)
        const float2 *__restrict__ pfr = reinterpret_cast<const float2 *>(recE) + (size_t)p * ((size_t)((cap + 1) >> 1) * 5);
        if (PRE && st.frontRec != nullptr && st.prefInfo != nullptr) {
            const int f = __builtin_amdgcn_readfirstlane(st.prefInfo[ps.prefRow + 2]); // (uniform: keep the loop's branch scalar)
            mFront = f < m1 ? f : m1;
        }
        // Two matches per trip, both records requested before the first is used: a wavefront that is alone on its SIMD (the
        // stages with few hypotheses, a single pair) otherwise waits out one scalar load per match.  The undecided lanes of
        // both are parked afterwards, in ONE copy of the parking code (it holds the drain).
        const unsigned long long *__restrict__ rp = reinterpret_cast<const unsigned long long *>(pf) + 5 * (size_t)m0;
        const float2 *__restrict__ fr2 = pfr + 5 * (size_t)(m0 >> 1); // (the front record of the pair of matches m, m + 1)
        // (whole pairs only: no "is there a second match" select on the scalar unit in every trip; the odd last match of a
        // pair's last range goes to the value-exact code for every lane, below)
        const int mPairs = m0 + ((m1 - m0) & ~1);
        int frontParkTrips = 0; // trips of the pre-tested front that left a lane to the value-exact test (wave-uniform)
        for (int m = m0; m < mPairs; m += 2, rp += 10, fr2 += (PRE ? 5 : 0)) {
            unsigned long long ua, ub;
            if (PRE && m + 2 <= mFront) { // (m0 = 0 in stage 1: m is even)
                not_out2(fr2, ua, ub);
            } else {
                Rec ra = load_rec(m, rp), rb = load_rec(m + 1, rp + 5);
                // (an empty asm that takes both records: the compiler otherwise sinks the second load below the first evaluation)
                asm volatile("" : "+s"(ra.q[0]), "+s"(ra.q[1]), "+s"(ra.q[2]), "+s"(ra.q[3]), "+s"(ra.q[4]), "+s"(rb.q[0]),
                             "+s"(rb.q[1]), "+s"(rb.q[2]), "+s"(rb.q[3]), "+s"(rb.q[4]));
                ua = eval(ra);
                ub = eval(rb);
            }
            if ((ua & ub) != execAll) { // (ua, ub: the lanes eval() / the pre-test decided)
                if (PRE && m + 2 <= mFront) ++frontParkTrips; // (statistics: counted here, in the rare path, not per trip)
#pragma nounroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned long long mU = execAll & ~(j ? ub : ua);
                    if (mU == 0ull) continue;
                    const int n = __popcll(mU);
                    if (qn + n > kQueueCap) {
                        drain();
                        rebuild();
                    }
                    if (lane_in(mU)) s_q[wv][qn + lanes_below(mU)] = ((uint32_t)(m + j) << 6) | (uint32_t)lane;
                    qn += n;
                }
            }
        }
        if (mPairs < m1) { // the odd last match: every lane's evaluation is handed to the value-exact code
            const int n = __popcll(execAll);
            if (qn + n > kQueueCap) drain();
            s_q[wv][qn + lanes_below(execAll)] = ((uint32_t)mPairs << 6) | (uint32_t)lane;
            qn += n;
        }
        parked += (unsigned long long)qn; // (the statistics count entries parked, whoever evaluates them)
        swept = true;
        mFrontS = mFront, mPairsS = mPairs, frontParkTripsS = frontParkTrips;
        }
    }
    } // (!idle)

    // The final drain, ONE for the work-group.  A wave ends its sweep with a handful of entries (0.07 % of the evaluations and
    // 0.9 % of the pre-test trips are parked): drained by the wave itself they cost a whole value-exact pass -- twelve LDS
    // reads, the general inverse, three record loads, inlier_test -- with 5 ... 7 of 64 lanes busy, in every wave of every
    // launch.  Instead the waves leave their entries in s_q[wave][0 .. qn), publish qn, and after a barrier the work-group
    // takes the four queues as one list, entry e to thread e (in strides of 256): a wave whose stride holds no entry skips
    // the value-exact code.  An entry names its thread (wave * 64 + lane) and its match; the model is that thread's in
    // s_mdl, the verdict goes to that thread's s_cnt -- nothing else travels.  EVERY wave of the work-group comes here:
    // the ones without a hypothesis and the ones that took the value-exact loop publish 0 (the exits above this point are
    // uniform over the work-group).  The looping forms separate their passes by a barrier of their own, so the next pass
    // writes s_q / s_qn / s_mdl / s_cnt only after every wave has left this one's second barrier.
    if (lane == 0) s_qn[wv] = qn;
    __syncthreads();
    {
        const int n1 = __builtin_amdgcn_readfirstlane(s_qn[0]);
        const int n2 = n1 + __builtin_amdgcn_readfirstlane(s_qn[1]);
        const int n3 = n2 + __builtin_amdgcn_readfirstlane(s_qn[2]);
        const int n4 = n3 + __builtin_amdgcn_readfirstlane(s_qn[3]);
        for (int e = tid; e < n4; e += kBlock) {
            const int w = (e >= n1) + (e >= n2) + (e >= n3);                 // the wave that parked entry e ...
            const int i = e - (w == 0 ? 0 : (w == 1 ? n1 : (w == 2 ? n2 : n3))); // ... as its i-th (i < its qn <= kQueueCap)
            const uint32_t ent = s_q[w][i];
            const int t = w * 64 + (int)(ent & 63u), m = orig((int)(ent >> 6));
            Rigid md, iv;
            lds_get_model(s_mdl, t, md);
            inverse_rigid_general(md, iv);
            const float4 A = pa[m], B = pb[m], C = pc[m];
            if (inlier_test<MODE>(md, iv, k, A, B, C)) atomicAdd(&s_cnt[t], 1);
        }
    }
    __syncthreads();
    if (idle) return false;
    if (swept) {
        cnt += s_cnt[tid];
        if (dbg != nullptr && lane == 0) {
            atomicAdd(&dbg[0], parked);
            atomicAdd(&dbg[1], (unsigned long long)(m1 - m0) * 64ull);
            if (KIND == 1) { // (ps_debug_score_stats_ex: [2] / [3] = pre-test trips without / with a lane left to the value-exact test)
                const int frontTrips = mFrontS > m0 ? ((mFrontS < mPairsS ? mFrontS : mPairsS) - m0) >> 1 : 0;
                atomicAdd(&dbg[3], (unsigned long long)frontParkTripsS);
                atomicAdd(&dbg[2], (unsigned long long)(frontTrips - frontParkTripsS));
            }
        }
    }
    pass_finish<KIND>(ps, s_mdl, s_tot, cout, ma, st, H, msplit, bx, p, M, valid, cnt);
    return false;
}

// (kind 2 sweeps short lists with few wavefronts: five per SIMD are plenty, and its loop over the list keeps the kernel
// arguments alive across the passes -- at seven or eight they went to scratch memory and the inlier counter with them)
// (LOOP, kind 1 only: the work-groups walk the blocks of 256 hypotheses, score_kernel_body in ps_score_pass.h)
template <int MODE, bool BIG, int KIND = 0, bool LOOP = false>
__global__ __launch_bounds__(kBlock, (KIND == 2 || LOOP) ? 5 : 8) void ps_ransac_score_fast(
    const float4 *__restrict__ recA, const float4 *__restrict__ recB, const float4 *__restrict__ recC,
    const float4 *__restrict__ recE, const float2 *__restrict__ recF, const int32_t *__restrict__ mvalid,
    const float2 *__restrict__ pairBound,
    ModelArgs ma, ScoreConsts k, FastConsts fc, EuclidConsts ec, SelectArgs sa, StageArgs st, int H, int cap, int minRun,
    int msplit, int32_t *__restrict__ counts, unsigned long long *__restrict__ dbg)
{
    static_assert(MODE == PS_REPROJECTION_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR,
                  "the metrics with a reprojection test");
    score_kernel_body<KIND, LOOP>(mvalid, st, minRun, msplit, [&](unsigned bx, unsigned by, int p, int M) __attribute__((always_inline)) {
        return score_fast_pass<MODE, BIG, KIND>(recA, recB, recC, recE, recF, pairBound, ma, k, fc, ec, sa, st, H, cap, msplit, counts, dbg,
                                                bx, by, p, M);
    });
}

// ------------------------------------------------------------------------------------------
// Between stage 0 and stage 1: the hot record of every pair in the order that ends hypotheses soonest.
//
// A hypothesis is out once it has missed M - B0 matches.  The prefix's best hypothesis misses exactly that many; nearly
// every other hypothesis misses THOSE matches too (they are the wrong correspondences) and then a few more.  In the original
// order the wrong correspondences are spread over the whole list, and a hypothesis that ends up five inliers short of B0 is
// only out at the very end; with the matches the prefix's best hypothesis rejects moved to the front, it is out at its first
// miss among the remaining ones.  Any order is valid -- a count is a sum over all matches and the bound "count so far +
// matches left <= B0" holds for every subset -- so this changes no output, only where hypotheses stop.
// One hypothesis's verdict is a noisy guide (it rejects marginal matches others accept, which leaves those others slack):
// the nTopMax best hypotheses of the prefix VOTE, and the matches are ordered by how many of them reject each (a stable
// counting sort: all-reject first -- the wrong correspondences --, then the marginal ones, the solid ones last).
// One work-group per pair: replay the prefix, pick the voters, read their models (parked by stage 0), test every match
// value-exactly against each, sort, and write
//   F2 / G2  the hot record of the stage kernels (RecPtrs::F or ::G layout),   perm  position -> original match
// (the cold paths -- value-exact recounts, the sampler of gen_model -- keep using the original arrays through perm).
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kBlock) void ps_stage_reorder(const float4 *__restrict__ recA, const float4 *__restrict__ recB,
                                                           const float4 *__restrict__ recC, const float2 *__restrict__ recF,
                                                           const int32_t *__restrict__ mvalid, ModelArgs ma, ScoreConsts k,
                                                           SelectArgs sa, int prefix, int nTopMax, int bailGran, int bailMargin,
                                                           int H, int cap, int minRun,
                                                           const int32_t *__restrict__ counts, float2 *__restrict__ recF2,
                                                           int32_t *__restrict__ perm, int32_t *__restrict__ prefInfo,
                                                           float2 *__restrict__ frontRec, unsigned *__restrict__ bailCount)
{
    constexpr bool EUCLID_REC = MODE == PS_EUCLIDEAN_ERROR || MODE == PS_ADAPTIVE_ERROR; // hot record = RecPtrs::G
    constexpr int RF = MODE == PS_ADAPTIVE_ERROR ? 16 : 12;
    constexpr int kMaxChunks = PS_MAX_KPTS / kBlock;
    __shared__ int s_top[kReorderTopMax + 1];                              // [0] = how many, then the hypotheses
    __shared__ uint8_t s_rej[PS_MAX_KPTS];                                 // per match: how many of them reject it
    __shared__ float s_vote[kReorderTopMax][24];                           // the voters' models and their inverses
    __shared__ int s_tab[(kReorderTopMax + 2) * kMaxChunks * (kBlock / 64)]; // bucket-major counts -> start positions
    const int p = blockIdx.x;
    const int M = mvalid[p];
    if (M < minRun) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t rbase = (size_t)p * cap;
    const int32_t *__restrict__ cnts = counts + (size_t)p * H;
    if (wv == 0) {
        // the limit the prefix leaves: with every later hypothesis beyond it the stages return at once and read nothing
        int b, l, bi;
        wave_replay_prefix(cnts, prefix, sa, M, b, l, bi);
        if (lane == 0) { // what every work-group of the stages needs (stage_prefix)
            prefInfo[4 * p] = b;
            prefInfo[4 * p + 1] = l;
            prefInfo[4 * p + 2] = 0; // (the all-reject front: known after the sort)
            prefInfo[4 * p + 3] = 0; // (1: the vote was skipped, see below)
        }
        int n = 0;
        const bool idle = b > 0 && l <= prefix; // (without a record nothing can be cut: the stages sweep everything)
        // Nothing to gain from an order (option "bail", Euclidean metrics): the prefix's best hypothesis misses so many
        // matches that stage 1 sweeps the whole list whatever the order (stage_range puts its cut at M) -- hopeless data, no
        // pair accepted.  The vote (nTop value-exact tests per match) is skipped and the record is handed on in its
        // original order.  The reprojection metrics always vote: their pre-test front pays even when nothing can be abandoned.
        bool bail = false;
        if (bailGran > 0 && b > 0) {
            const int c1 = (M - b + bailMargin + bailGran - 1) & ~(bailGran - 1);
            bail = c1 >= M - M / 8; // (the rule of stage_range for the reordered sweep)
        }
        if (b > 0 && !idle && !bail) {
            // the nTopMax best counts of the prefix (first of equals first): (count, 0xFFFF - index) keys, lane i holds
            // hypotheses i, i + 64, ...
            int key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = lane + 64 * j;
                key[j] = (i < prefix && cnts[i] > 0) ? ((cnts[i] << 16) | (0xFFFF - i)) : 0;
            }
            for (; n < nTopMax; ++n) {
                int m = max(max(key[0], key[1]), max(key[2], key[3]));
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
                if (m == 0) break;
                if (lane == 0) s_top[1 + n] = 0xFFFF - (m & 0xFFFF);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (key[j] == m) key[j] = 0;
            }
        }
        if (lane == 0) {
            s_top[0] = idle ? -1 : n; // (no record: no votes, one bucket, the original order)
            if (bail) prefInfo[4 * p + 3] = 1;
            if (bailCount != nullptr) { // what the host's "nothing to gain" policy looks at (ps_capi.hip, prepare_score)
                atomicAdd(&bailCount[0], 1u);
                if (bail || b <= 0) atomicAdd(&bailCount[1], 1u);
            }
        }
    }
    __syncthreads();
    const int nTop = s_top[0];
    if (nTop < 0) return; // nothing beyond the prefix will be scored
    const float4 *__restrict__ pa = recA + rbase;
    const float4 *__restrict__ pb = recB + rbase;
    const float4 *__restrict__ pc = recC + rbase;
    // the voters' models and inverses, one thread each, side by side (one global round trip instead of one per voter)
    if (tid < nTop) {
        Rigid mdl, inv;
        load_model(ma, (size_t)p * ma.modelH + s_top[1 + tid], mdl); // parked by stage 0
        inverse_rigid_general(mdl, inv);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s_vote[tid][3 * i + j] = mdl.R[i][j];
                s_vote[tid][12 + 3 * i + j] = inv.R[i][j];
            }
            s_vote[tid][9 + i] = mdl.t[i];
            s_vote[tid][21 + i] = inv.t[i];
        }
    }
    __syncthreads();
    for (int m = tid; m < M; m += kBlock) { // (the thread's own matches)
        const float4 A = pa[m], B = pb[m], C = pc[m];
        int rej = 0;
        bool far = (MODE == PS_REPROJECTION_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR) && nTop >= 1;
        for (int t = 0; t < nTop; ++t) {
            Rigid mdl, inv;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    mdl.R[i][j] = s_vote[t][3 * i + j];
                    inv.R[i][j] = s_vote[t][12 + 3 * i + j];
                }
                mdl.t[i] = s_vote[t][9 + i];
                inv.t[i] = s_vote[t][21 + i];
            }
            rej += inlier_test<MODE>(mdl, inv, k, A, B, C) ? 0 : 1;
            if (MODE == PS_REPROJECTION_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR) {
                // FAR off in the direction stage 1's pre-test looks at (current point -> previous image): more than four
                // thresholds (a heuristic for the order only; plain float arithmetic)
                float ex, ey, ez, pu, pv;
                xform(mdl, B.x, B.y, B.z, ex, ey, ez);
                project(ex, ey, ez, k.fx, k.fy, k.cx, k.cy, pu, pv);
                const float du = pu - C.x, dv = pv - C.y;
                far = far && (du * du + dv * dv > 16.0f * (float)k.boundR);
            }
        }
        // bucket of the counting sort: 0 = every voter rejects it AND it is far off for each (the wrong correspondences
        // proper), then 1 + (nTop - rejections): rejected by all but close for some voter (marginal true correspondences:
        // in doubt for every good hypothesis), ..., accepted by all
        s_rej[m] = (uint8_t)(far && rej == nTop ? 0 : 1 + nTop - rej);
    }
    // Stable counting sort by bucket.  Counts per (bucket, chunk of 256 matches, wave) -> exclusive prefix in that order
    // -> position = start + lanes below in the same bucket.
    const int nB = nTop + 2; // buckets
    const int nChunks = (M + kBlock - 1) / kBlock;
    for (int c = 0; c < nChunks; ++c) {
        const int m = c * kBlock + tid;
        const int d = m < M ? (int)s_rej[m] : -1;
        for (int b = 0; b < nB; ++b) {
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(d == b);
            if (lane == 0) s_tab[(b * nChunks + c) * (kBlock / 64) + wv] = __popcll(bal);
        }
    }
    __syncthreads();
    if (wv == 0) {
        const int n = nB * nChunks * (kBlock / 64);
        int carry = 0;
        for (int e0 = 0; e0 < n; e0 += 64) {
            const int e = e0 + lane;
            const int v = e < n ? s_tab[e] : 0;
            int inc = v; // inclusive scan over the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(inc, o, 64);
                if (lane >= o) inc += u;
            }
            if (e < n) s_tab[e] = carry + inc - v;
            carry += __shfl(inc, 63, 64);
        }
    }
    __syncthreads();
    // matches every voter rejects and finds far off (bucket 0; empty without a voter and for the Euclidean metrics)
    const int front = s_tab[(1 * nChunks) * (kBlock / 64)];
    if (tid == 0) prefInfo[4 * p + 2] = front;
    float *__restrict__ frOut =
        (EUCLID_REC || frontRec == nullptr) ? nullptr : reinterpret_cast<float *>(frontRec) + (size_t)p * ((size_t)((cap + 1) >> 1) * 10);
    const float *__restrict__ gIn = reinterpret_cast<const float *>(recF) + (size_t)p * ((size_t)((cap + 1) >> 1) * RF);
    float *__restrict__ gOut = reinterpret_cast<float *>(recF2) + (size_t)p * ((size_t)((cap + 1) >> 1) * RF);
    for (int c = 0; c < nChunks; ++c) {
        const int m = c * kBlock + tid;
        const int d = m < M ? (int)s_rej[m] : -1;
        int pos = 0;
        for (int b = 0; b < nB; ++b) {
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(d == b);
            if (d == b) pos = s_tab[(b * nChunks + c) * (kBlock / 64) + wv] + lanes_below(bal);
        }
        if (m < M) {
            perm[rbase + pos] = m;
            if (EUCLID_REC) {
                const float *src = gIn + (size_t)(m >> 1) * RF + (m & 1);
                float *dst = gOut + (size_t)(pos >> 1) * RF + (pos & 1);
#pragma unroll
                for (int i = 0; i < RF; i += 2) dst[i] = src[i];
            } else {
                const float2 *src = recF + 5 * (rbase + m);
                float2 *dst = recF2 + 5 * (rbase + pos);
#pragma unroll
                for (int i = 0; i < 5; ++i) dst[i] = src[i];
                if (frOut != nullptr && pos < front) { // one direction's operands, two matches per record (stage 1's pre-test)
                    float *fd = frOut + (size_t)(pos >> 1) * 10 + (pos & 1);
#pragma unroll
                    for (int i = 0; i < 5; ++i) fd[2 * i] = src[i].x;
                }
            }
        }
    }
    if (EUCLID_REC && (M & 1)) { // the unwritten second half of the last pair record repeats the first (finish_pair_records)
        __syncthreads();
        if (tid == 0) {
            float *g = gOut + (size_t)(M >> 1) * RF;
            for (int i = 0; i < RF; i += 2) g[i + 1] = g[i];
        }
    }
}

} // namespace psdev
