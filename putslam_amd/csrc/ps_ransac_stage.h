// ps_ransac_stage.h -- the RANSAC core on the host side: the plan of a call (Plan, make_plan, prepare_score), the kernel-3 launch
// families with their schedule, and run_ransac_stage, which queues kernels 3 + 4 over records already in the arena;
// ps_ransac_rigid3d is the host-pointer form.  The pipeline for gfx950 (wave64, 256 CUs) starts here:
//
// Data layout in HBM (one "frame set" + one "pair batch", see include/putslam_hip.h):
//   desc   [F][cap][32 B]      binary descriptors (ORB / LDB, 256 bit)
//   pts    [F][cap][3] f32     back-projected 3-D points (Eigen::Vector3f storage)
//   keys   [P][cap]    u32     per train row: (hamming << 16) | nearest query   (scratch; all-ones again after kernel 2)
//   recA/B/C/D [P][cap] 16 B   per depth-valid match: prev xyz + squared Euclid bound |
//                              cur xyz | projections of prev and cur | indices    (scratch)
//   counts [P][H]      i32     inlier count of every hypothesis                   (scratch)
// Nothing of size N*N or H*M ever touches HBM: distances live in VGPRs, models in VGPRs.
//
// Kernel 1  ps_hamming_nn      train -> nearest query (the N x N popcount sweep)
// Kernel 2  ps_crosscheck_prep OpenCV cross-check, ordered compaction, depth filter, records
// Kernel 3  ps_ransac_score    one lane = one 3-point hypothesis: Umeyama fit + score all M matches
// Kernel 4  ps_select_refit    replay of the sequential best-model rule, refit, final inliers
//             (kernels 1 + 2: ps_match_stage.h; kernel 3: ps_score_value.h, ps_score_fast.h, ps_score_euclid.h; kernel 4: ps_select_refit.h)
//
// What kernel 2 and the other routes into RANSAC leave for kernels 3 and 4 is ps_pair_records.h's (PrepArgs, RecPtrs,
// write_records, PairRecords; the match-list kernels ps_prep_from_matches and ps_prep_match_lists).
// Host code of the device translation unit: ps_capi.hip's `using namespace psdev` stands in front of it, as for every feature header.
#pragma once
#include "ps_glue.h"
#include "ps_internal.h"
#include "ps_pair_records.h" // PrepArgs, RecPtrs; ps_prep_from_matches
#include "ps_score_euclid.h"
#include "ps_score_fast.h"
#include "ps_score_pass.h"
#include "ps_score_value.h"
#include "ps_select_refit.h"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

double sq_bound_f64(double thr)
{
    // smallest double x >= 0 with sqrt(x) >= thr  (cv::norm(Point2f) < thr  <=>  dx^2+dy^2 < x)
    if (!(thr > 0.0)) return 0.0;
    if (thr > 1.3407807929942596e154) return INFINITY;
    double x = thr * thr;
    const double tiny = 4.9406564584124654e-324;
    if (!(x > 0.0)) x = tiny;
    while (x > tiny && std::sqrt(std::nextafter(x, 0.0)) >= thr) x = std::nextafter(x, 0.0);
    while (std::sqrt(x) < thr) x = std::nextafter(x, INFINITY);
    return x;
}

int prepare_tables(PsContext *ctx, int estimator, double minRatio, int H, SelectArgs &sa)
{
    sa.ransacTab = nullptr;
    sa.ransacTabN = 0;
    sa.usacTab = nullptr;
    sa.usacTabN = 0;
    if (estimator == PS_EST_FIXED) {
        sa.iter0 = H;
        return PS_OK;
    }
    if (!(ctx->tabEstimator == estimator && ctx->tabH == H && ctx->tabMinRatio == minRatio)) {
        if (estimator == PS_EST_RANSAC) {
            std::vector<float> tab;
            int iter0 = 0;
            build_ransac_table(minRatio, H, tab, iter0, ctx->tabTiny);
            PS_ENSURE(ctx->tabR, tab.size() * sizeof(float) + 4);
            if (!tab.empty()) {
                PS_HIP(hipMemcpyAsync(ctx->tabR.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice,
                                      ctx->stream));
                PS_HIP(hipStreamSynchronize(ctx->stream)); // tab goes out of scope
            }
            ctx->tabRN = (int)tab.size();
            ctx->tabIter0 = iter0;
        } else {
            std::vector<double> tab;
            build_usac_table(H, tab);
            PS_ENSURE(ctx->tabU, tab.size() * sizeof(double) + 8);
            if (!tab.empty()) {
                PS_HIP(hipMemcpyAsync(ctx->tabU.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice,
                                      ctx->stream));
                PS_HIP(hipStreamSynchronize(ctx->stream));
            }
            ctx->tabUN = (int)tab.size();
            ctx->tabIter0 = H < (int)kUsacMaxHyp ? H : (int)kUsacMaxHyp;
        }
        ctx->tabEstimator = estimator;
        ctx->tabH = H;
        ctx->tabMinRatio = minRatio;
    }
    sa.iter0 = ctx->tabIter0;
    if (estimator == PS_EST_RANSAC) {
        sa.ransacTab = (const float *)ctx->tabR.p;
        sa.ransacTabN = ctx->tabRN;
        sa.ransacTiny = ctx->tabTiny;
    } else {
        sa.usacTab = (const double *)ctx->tabU.p;
        sa.usacTabN = ctx->tabUN;
    }
    return PS_OK;
}

int effective_mode(int errorVersion)
{
    switch (errorVersion) {
    case PS_EUCLIDEAN_ERROR:
    case PS_REPROJECTION_ERROR:
    case PS_EUCLIDEAN_AND_REPROJECTION_ERROR:
    case PS_ADAPTIVE_ERROR:
        return errorVersion;
    default:
        // MAHALANOBIS is dead in the reference (RANSAC.cpp:301-303) and unknown values print
        // "incorrect error version" and score 0 (RANSAC.cpp:134-135): both score 0 here.
        return PS_MAHALANOBIS_ERROR;
    }
}

struct Plan {
    int mode = 0;
    Scoring score = Scoring::Value; // (make_plan)
    int H = 0;        // hypotheses scored
    int minRun = 3;
    ScoreConsts sc{};
    FastConsts fc{};
    EuclidConsts ec{};
    PrepArgs pa{};
    SelectArgs sa{};
    ModelArgs ma{};
    ScoreDecision d;        // how the scoring stage runs (prepare_score; decide_score, ps_score_plan.h)
    bool bailWatch = false; // this staged call feeds the "nothing to gain" policy (PsContext::bailHost)
    int bailSlot = 0;       // ... for this kind of call (PsContext::bailTracker)
};

// directed roundings to float
float round_up(double v) { float f = (float)v; return (double)f < v ? std::nextafterf(f, INFINITY) : f; }
float round_down(double v) { float f = (float)v; return (double)f > v ? std::nextafterf(f, -INFINITY) : f; }

int make_plan(PsContext *ctx, const PsRansacParams *prm, const PsRansacConfig *cfg, const float *K, int cap,
              int trainRange, Plan &pl)
{
    if (!prm || !cfg) return fail(ctx, PS_ERR_BAD_ARG, "null params/config");
    if (prm->usedPairs != 3) return fail(ctx, PS_ERR_UNSUPPORTED, "usedPairs must be 3");
    if (cfg->numHypotheses < 1 || cfg->numHypotheses > PS_MAX_HYPOTHESES)
        return fail(ctx, PS_ERR_BAD_ARG, "numHypotheses out of range");
    if (cfg->estimator < PS_EST_RANSAC || cfg->estimator > PS_EST_FIXED)
        return fail(ctx, PS_ERR_BAD_ARG, "unknown estimator");
    pl.mode = effective_mode(prm->errorVersion);
    if (ctx->scoreFast == 0 || pl.mode == PS_MAHALANOBIS_ERROR) pl.score = Scoring::Value;
    else pl.score = (pl.mode == PS_EUCLIDEAN_ERROR || pl.mode == PS_ADAPTIVE_ERROR) ? Scoring::Euclid : Scoring::Reproj;
    float k[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (K) memcpy(k, K, sizeof k);
    pl.sc.fx = k[0]; pl.sc.fy = k[4]; pl.sc.cx = k[2]; pl.sc.cy = k[5];
    pl.sc.boundR = sq_bound_f64(prm->inlierThresholdReprojection);
    // float pre-filter band (see inlier_test): only when boundR is comfortably inside the float range
    pl.sc.bLo = -1.0f;      // never "surely inside"
    pl.sc.bHi = INFINITY;   // never "surely outside"
    if (pl.sc.boundR >= 1e-20 && pl.sc.boundR <= 1e30) {
        const double w = 4.76837158203125e-07; // 2^-21
        double lo = pl.sc.boundR * (1.0 - w), hi = pl.sc.boundR * (1.0 + w);
        float flo = (float)lo, fhi = (float)hi;
        if ((double)flo > lo) flo = std::nextafterf(flo, 0.0f);
        if ((double)fhi < hi) fhi = std::nextafterf(fhi, INFINITY);
        pl.sc.bLo = flo;
        pl.sc.bHi = fhi;
    }
    // constants of the decision-exact fast path (ps_score_fast.h); directed roundings keep every bound on its safe side
    {
        FastConsts &fc = pl.fc;
        const double fm = std::fmax(std::fmax(std::fabs((double)k[0]), std::fabs((double)k[4])), 1.0);
        const double cm = std::fmax(std::fabs((double)k[2]), std::fabs((double)k[5]));
        const double bR = pl.sc.boundR;
        fc.enabled = (bR >= 1e-12 && bR <= 1e12 && fm <= 1e6 && cm <= 1e6) ? 1 : 0; // false for NaN
        if (fc.enabled) {
            const double T = std::sqrt(bR);
            fc.fmaxK = round_up(fm);
            fc.cmaxK = round_up(cm);
            fc.thrUp = round_up(T * (1.0 + 1e-5));
            fc.bIn0 = round_down(bR * (1.0 - 20.0 * 5.9604644775390625e-08));
            fc.cIn = round_up(2.0 * std::sqrt(2.0) * T * (1.0 + 1e-5));
            const double c = std::sqrt(2.0) * (1.0 + 1e-5);
            fc.thr2Up = round_up((double)fc.thrUp * (double)fc.thrUp);
            fc.cHi = round_up((2.0 * c + c * c) * (double)fc.thrUp);
        }
    }
    // constants of the decision-exact Euclidean path (ps_score_euclid.h): the threshold in the root domain, pushed
    // 6u (7u) to the safe side; errorVersion 0 works against the exact float bound B the value-exact code compares with,
    // errorVersion 4 against thr itself (the record is normalised by the match's depth)
    {
        EuclidConsts &ec = pl.ec;
        const double thr = prm->inlierThresholdEuclidean;
        ec.enabled = (thr >= 1e-10 && thr <= 1e10) ? 1 : 0; // false for NaN
        ec.tbLo = ec.tbHi = 0.0f;
        if (ec.enabled) {
            const double u = 5.9604644775390625e-08;
            if (pl.mode == PS_ADAPTIVE_ERROR) {
                ec.tbLo = round_down(thr * (1.0 - 7.0 * u));
                ec.tbHi = round_up(thr * (1.0 + 7.0 * u));
            } else {
                const double Tb = std::sqrt((double)sq_bound_f32(thr));
                ec.tbLo = round_down(Tb * (1.0 - 6.0 * u));
                ec.tbHi = round_up(Tb * (1.0 + 6.0 * u));
            }
        }
    }
    pl.pa.fx = k[0]; pl.pa.fy = k[4]; pl.pa.cx = k[2]; pl.pa.cy = k[5];
    pl.pa.thrE = prm->inlierThresholdEuclidean;
    pl.pa.mode = pl.mode;
    pl.pa.cap = cap;
    pl.sa.estimator = cfg->estimator;
    pl.sa.mode = pl.mode;
    pl.sa.cap = cap;
    pl.sa.minMatches = (cfg->estimator == PS_EST_USAC) ? 8 : prm->minimalNumberOfMatches;
    pl.sa.minRatio = prm->minimalInlierRatioThreshold;
    pl.sa.trainRange = trainRange;
    pl.minRun = pl.sa.minMatches > 3 ? pl.sa.minMatches : 3;
    const int H = scored_hypotheses(cfg->estimator, cfg->numHypotheses, prm->minimalInlierRatioThreshold);
    pl.H = H;
    pl.sa.H = H;
    int rc = prepare_tables(ctx, cfg->estimator, prm->minimalInlierRatioThreshold, H, pl.sa);
    if (rc != PS_OK) return rc;
    if (pl.sa.iter0 > H) pl.sa.iter0 = H;
    pl.ma.seed = cfg->seed;
    pl.ma.raw = nullptr;
    pl.ma.seedDev = nullptr;
    return PS_OK;
}

// The Euclidean fast scoring kernel reads its own pair-interleaved record, kept in the block the reprojection kernels use
// for theirs (recF): kernel 2 writes one or the other.
RecPtrs rec_ptrs(PsContext *ctx, Scoring score)
{
    RecPtrs r;
    r.G = score == Scoring::Euclid ? (float *)ctx->recF.p : nullptr;
    r.A = (float4 *)ctx->recA.p; r.B = (float4 *)ctx->recB.p; r.C = (float4 *)ctx->recC.p; r.D = (int4 *)ctx->recD.p;
    r.E = (float4 *)ctx->recE.p;
    r.F = (float2 *)ctx->recF.p;
#ifdef PS_STREAM_DIAG
    r.S = (float4 *)ctx->recShadow.p; // (null unless PUTSLAM_HIP_DIAG_SHADOW_RECORDS=1: ensure_records)
#endif
    return r;
}

template <int MODE>
void launch_score(PsContext *ctx, dim3 grid, const Plan &pl, int cap, int msplit)
{
    hipLaunchKernelGGL(ps_ransac_score<MODE>, grid, dim3(kBlock), 0, ctx->stream, (const float4 *)ctx->recA.p,
                       (const float4 *)ctx->recB.p, (const float4 *)ctx->recC.p, (const int32_t *)ctx->mvalid.p,
                       (const float2 *)ctx->cmax.p, pl.ma, pl.sc, pl.H, cap, pl.minRun, msplit, (int32_t *)ctx->counts.p);
}

// The options the scoring plan reads, as they stand now (ScoreOptions, ps_score_plan.h).
ScoreOptions score_options(const PsContext *ctx)
{
    ScoreOptions o;
    o.prune = ctx->prune; o.sideBySide = ctx->sideBySide; o.reorder = ctx->reorder; o.genSplit = ctx->genSplit;
    o.singleRest = ctx->singleRest; o.pretest = ctx->pretest; o.listGroups2 = ctx->listGroups2; o.forcePrefix = ctx->forcePrefix;
    o.forceMsplit = ctx->forceMsplit; o.modelRoomMiB = ctx->modelRoomMiB; o.bail = ctx->bail; o.reorderMargin = ctx->reorderMargin;
    return o;
}

ScoreShape score_shape(const Plan &pl, int P, int cap, bool complete = false, bool adaptive = false)
{
    ScoreShape s;
    s.P = P; s.cap = cap; s.H = pl.H; s.mode = pl.mode; s.score = pl.score; s.estimator = pl.sa.estimator;
    s.complete = complete; s.adaptive = adaptive;
    return s;
}

// The "nothing to gain" policy's side of a staged call of kind `key` (BailTracker, ps_score_plan.h, is the state machine; here its
// counters: the device block, the mapped host mirror kernel 4 forwards them to).  Returns whether the call scores completely instead.
bool bail_consult(PsContext *ctx, Plan &pl, const BailKey &key)
{
    if (!ctx->bailHost) {
        const size_t nb = (size_t)BailTracker::kKinds * 2 * sizeof(unsigned);
        if (hipHostMalloc((void **)&ctx->bailHost, nb, hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer((void **)&ctx->bailHostDev, ctx->bailHost, 0) == hipSuccess) {
            memset(ctx->bailHost, 0, nb);
            if (ensure(ctx, ctx->bailCnt, nb) == PS_OK) (void)hipMemsetAsync(ctx->bailCnt.p, 0, nb, ctx->stream);
        } else {
            (void)hipGetLastError();
            ctx->bailHostDev = nullptr; // (no mapped memory here: the policy stays off)
        }
    }
    if (!(ctx->bailHostDev && ctx->bailCnt.p)) return false;
    BailTracker &t = ctx->bailTracker;
    const volatile unsigned *host = (volatile unsigned *)ctx->bailHost;
    bool recycled = false;
    const int slot = t.find(key, recycled);
    if (recycled) {
        // (the slot's counters are monotonic: what its previous kind left there is simply "seen" -- once it HAS landed:
        // a call of the previous kind may still be in flight, and counts arriving after the snapshot would read as an
        // observation of the new kind.  Recycling is rare -- more than eight kinds alternating on one context -- and
        // drains the stream first.)
        (void)hipStreamSynchronize(ctx->stream);
        t.adopt(slot, host[2 * slot], host[2 * slot + 1]);
    }
    ctx->hopeless = t.observe(slot, host[2 * slot], host[2 * slot + 1]);
    const bool veto = t.veto(slot);
    pl.bailWatch = !veto;
    pl.bailSlot = slot;
    ctx->bailSlot = slot;
    return veto;
}

// Decisions of the scoring stage that the preceding kernels need to know (decide_score, ps_score_plan.h), and the arena blocks they ask for.
// complete = true: every hypothesis is scored completely whatever the batch size (ps_debug_ransac_counts returns the counts
// themselves: the staged scoring leaves lower bounds for abandoned hypotheses)
int prepare_score(PsContext *ctx, Plan &pl, int P, int cap, bool complete = false, bool adaptive = false, const void *dataKey = nullptr)
{
    const ScoreOptions opts = score_options(ctx);
    const ScoreShape shape = score_shape(pl, P, cap, complete, adaptive);
    bool staged = wants_staged(shape, opts);
    pl.bailWatch = false;
    pl.bailSlot = 0;
    if (bail_applies(shape, opts, staged) && bail_consult(ctx, pl, bail_key(shape, dataKey))) staged = false;
    const ScoreDecision &d = pl.d = decide_score(shape, opts, staged);
    if (d.status != PS_OK)
        return fail(ctx, d.status, "complete scoring of this batch (pairs x hypotheses x matches > 2e14) would run for minutes: "
                                   "leave the staged scoring on (option \"prune\") or pass fewer pairs per call");
    Buf *const blocks[kScoreBlocks] = {&ctx->counts, &ctx->models, &ctx->survA, &ctx->survB, &ctx->survN,
                                       &ctx->validMask, &ctx->recF2, &ctx->permBuf, &ctx->prefInfo, &ctx->frontRec}; // (ScoreBlock's order)
    for (int i = 0; i < kScoreBlocks; ++i)
        if (d.bytes[i]) PS_ENSURE(*blocks[i], d.bytes[i]);
    pl.pa.zeroCounts = d.zeroCounts ? (int32_t *)ctx->counts.p : nullptr;
    pl.pa.zeroH = d.zeroH;
    pl.pa.zeroStride = pl.H;
    pl.pa.zeroSurvA = d.staged ? (int32_t *)ctx->survN.p : nullptr; // cleared by kernel 2, one counter per pair and stage
    pl.pa.zeroSurvB = d.staged ? (int32_t *)ctx->survN.p + P : nullptr;
    pl.pa.skipE = d.skipE;
    pl.pa.skipF = d.skipF;
    pl.ma.models = d.parkModels ? (float *)ctx->models.p : nullptr;
    pl.ma.modelH = d.modelH;
    ctx->lastModelH = d.parkModels ? d.modelH : 0;
    ctx->stagedP = d.staged ? P : 0;
    ctx->stagedCap = d.staged ? cap : 0;
    ctx->reorderedP = d.reorder ? P : 0;
    return PS_OK;
}

// What the kernel-3 launches of one call share (run_ransac_stage).
struct K3Call {
    PsContext *ctx;
    const Plan &pl;
    int P, cap;
    const float2 *hotF;      // the hot record of stages 1+: reordered between stage 0 and stage 1 (ps_stage_reorder) unless the option is off
    unsigned long long *dbg; // option "score_stats": the decision-exact kernels' counters, else null
};

// A launch of kernel 3 of KIND 0 (stage 0 / the complete scoring), 1 (stage 1; LOOP: looping work-groups) or 2 (stages 2+);
// a family's launcher runs it with the given StageArgs over groups x msplit x P work-groups.
template <int KIND, bool LOOP = false> struct Kind {};

template <int MODE> struct EuclidK3 {
    const K3Call &c;
    template <int KIND, bool LOOP> void operator()(Kind<KIND, LOOP>, const StageArgs &st, unsigned groups, int msplit) const
    {
        PsContext *ctx = c.ctx;
        hipLaunchKernelGGL((ps_ransac_score_euclid<MODE, KIND, LOOP>), dim3(groups * (unsigned)msplit * (unsigned)c.P), dim3(kBlock),
                           0, ctx->stream, (const float4 *)ctx->recA.p, (const float4 *)ctx->recB.p,
                           KIND >= 1 ? c.hotF : (const float2 *)ctx->recF.p, (const int32_t *)ctx->mvalid.p,
                           (const float2 *)ctx->cmax.p, c.pl.ma, c.pl.sc, c.pl.ec, c.pl.sa, st, c.pl.H, c.cap, c.pl.minRun, msplit,
                           (int32_t *)ctx->counts.p, c.dbg);
    }
};

template <int MODE> struct ReprojK3 {
    const K3Call &c;
    template <bool BIG, int KIND, bool LOOP> void launch(const StageArgs &st, unsigned groups, int msplit) const
    {
        PsContext *ctx = c.ctx;
        hipLaunchKernelGGL((ps_ransac_score_fast<MODE, BIG, KIND, LOOP>), dim3(groups * (unsigned)msplit * (unsigned)c.P),
                           dim3(kBlock), 0, ctx->stream, (const float4 *)ctx->recA.p, (const float4 *)ctx->recB.p,
                           (const float4 *)ctx->recC.p, st.frontRec ? (const float4 *)st.frontRec : (const float4 *)ctx->recE.p,
                           KIND >= 1 ? c.hotF : (const float2 *)ctx->recF.p, (const int32_t *)ctx->mvalid.p,
                           (const float2 *)ctx->cmax.p, c.pl.ma, c.pl.sc, c.pl.fc, c.pl.ec, c.pl.sa, st, c.pl.H, c.cap, c.pl.minRun,
                           msplit, (int32_t *)ctx->counts.p, c.dbg);
    }
    // more work-groups than fit at once (256 CUs x 6): the build for big launches (ps_score_fast.h) -- for stage 0 and the
    // complete scoring as prepare_score decided (ScoreDecision::big0), always for the stages after the prefix
    template <int KIND, bool LOOP> void operator()(Kind<KIND, LOOP>, const StageArgs &st, unsigned groups, int msplit) const
    {
        if constexpr (KIND == 0) {
            if (!c.pl.d.big0) return launch<false, KIND, LOOP>(st, groups, msplit);
        }
        launch<true, KIND, LOOP>(st, groups, msplit);
    }
};

// Kernel 3 of the decision-exact scoring (ps_score_fast.h, ps_score_euclid.h) through one family's launcher k3.  Staged
// scoring: stage 0 = the prefix completely, stages 1 .. lastStage = the rest with hypotheses abandoned between the launches;
// otherwise every hypothesis of [0, H) completely.
template <int MODE, class K3> void score_schedule(const K3Call &c, const K3 &k3)
{
    PsContext *ctx = c.ctx;
    const Plan &pl = c.pl;
    const ScoreDecision &d = pl.d;
    const int P = c.P;
    const ScoreOptions opts = score_options(ctx);
    const StageSchedule sch = stage_schedule(score_shape(pl, P, c.cap), opts, d);
    int32_t *const list[3] = {nullptr, (int32_t *)ctx->survA.p, (int32_t *)ctx->survB.p};
    int32_t *const count[3] = {nullptr, (int32_t *)ctx->survN.p, (int32_t *)ctx->survN.p + P};
    for (int i = 0; i < sch.n; ++i) {
        const StageLaunch &l = sch.launch[i];
        if (i == sch.reorderBefore)
            hipLaunchKernelGGL(ps_stage_reorder<MODE>, dim3((unsigned)P), dim3(kBlock), 0, ctx->stream, (const float4 *)ctx->recA.p,
                               (const float4 *)ctx->recB.p, (const float4 *)ctx->recC.p, (const float2 *)ctx->recF.p,
                               (const int32_t *)ctx->mvalid.p, pl.ma, pl.sc, pl.sa, d.prefix, ctx->reorderTop,
                               (ctx->bail != 0 && pl.score == Scoring::Euclid) ? 64 : 0, ctx->reorderMargin, pl.H, c.cap, pl.minRun,
                               (const int32_t *)ctx->counts.p, (float2 *)ctx->recF2.p, (int32_t *)ctx->permBuf.p,
                               (int32_t *)ctx->prefInfo.p, sch.pretest ? (float2 *)ctx->frontRec.p : (float2 *)nullptr,
                               pl.bailWatch ? (unsigned *)ctx->bailCnt.p + 2 * pl.bailSlot : (unsigned *)nullptr);
        StageArgs st{};
        st.stage = l.stage;
        st.hBase = l.hBase;
        st.hCount = l.hCount;
        st.genOnly = l.genOnly;
        st.listIn = list[l.listIn]; st.countIn = count[l.listIn];
        st.listOut = list[l.listOut]; st.countOut = count[l.listOut];
        if (l.validMask) st.validMask = (unsigned long long *)ctx->validMask.p;
        if (l.perm) st.perm = (const int32_t *)ctx->permBuf.p;
        if (l.perm) st.prefInfo = (const int32_t *)ctx->prefInfo.p;
        if (l.frontRec) st.frontRec = (const float2 *)ctx->frontRec.p;
        st.loopGroups = l.loopGroups;
        st.single = l.single;
        if (d.staged) {
            st.listStride = d.modelH;
            st.margin = opts.reorderMargin;
            st.gran = kReorderGran;
            st.c2div = kReorderC2div;
        }
        if (l.kind == 0) k3(Kind<0>{}, st, l.groups, l.msplit);
        else if (l.kind == 2) k3(Kind<2>{}, st, l.groups, l.msplit);
        else if (l.loop) k3(Kind<1, true>{}, st, l.groups, l.msplit);
        else k3(Kind<1>{}, st, l.groups, l.msplit);
    }
}

// Kernel 3 of one call under error MODE: the family the plan chose (Plan::score).
template <int MODE> void launch_k3(const K3Call &c)
{
    if constexpr (MODE == PS_EUCLIDEAN_ERROR || MODE == PS_ADAPTIVE_ERROR) {
        if (c.pl.score == Scoring::Euclid) return score_schedule<MODE>(c, EuclidK3<MODE>{c});
    }
    if constexpr (MODE == PS_REPROJECTION_ERROR || MODE == PS_EUCLIDEAN_AND_REPROJECTION_ERROR) {
        if (c.pl.score == Scoring::Reproj) return score_schedule<MODE>(c, ReprojK3<MODE>{c});
    }
    // counts were cleared by kernel 2 when the range is split (prepare_score)
    launch_score<MODE>(c.ctx, dim3((unsigned)((c.pl.H + kBlock - 1) / kBlock) * (unsigned)c.pl.d.msplit * (unsigned)c.P), c.pl, c.cap,
                       c.pl.d.msplit);
}

// Kernels 3 + 4 over records already in the arena.
int run_ransac_stage(PsContext *ctx, const Plan &pl, int P, int cap, const PsDMatch *dMatches,
                     const int32_t *dNumMatches, int matchStride, float *dPose, uint8_t *dMask, PsRansacStats *dStats,
                     int slot0)
{
    PS_ENSURE(ctx->counts, (size_t)P * pl.H * sizeof(int32_t));
    PS_ENSURE(ctx->idxList, (size_t)P * cap * sizeof(int32_t));
    tick(ctx, slot0, false);
    unsigned long long *dbg = nullptr;
    if (ctx->scoreStats && pl.score != Scoring::Value) {
        PS_ENSURE(ctx->dbgCnt, 8 * sizeof(unsigned long long));
        PS_HIP(hipMemsetAsync(ctx->dbgCnt.p, 0, 8 * sizeof(unsigned long long), ctx->stream));
        dbg = (unsigned long long *)ctx->dbgCnt.p;
    }
    const K3Call c{ctx, pl, P, cap, (const float2 *)(pl.d.reorder ? ctx->recF2.p : ctx->recF.p), dbg};
    switch (pl.mode) {
    case PS_EUCLIDEAN_ERROR: launch_k3<PS_EUCLIDEAN_ERROR>(c); break;
    case PS_REPROJECTION_ERROR: launch_k3<PS_REPROJECTION_ERROR>(c); break;
    case PS_EUCLIDEAN_AND_REPROJECTION_ERROR: launch_k3<PS_EUCLIDEAN_AND_REPROJECTION_ERROR>(c); break;
    case PS_ADAPTIVE_ERROR: launch_k3<PS_ADAPTIVE_ERROR>(c); break;
    default: launch_k3<PS_MAHALANOBIS_ERROR>(c); break;
    }
    tick(ctx, slot0, true);
    PS_HIP(hipGetLastError());
    SelectArgs sa = pl.sa;
    // LDS of kernel 4: the two bitmaps over train indices, then up to 48 KiB for the refit's and the re-selection's operands
    // (what is left of the 64 KiB a work-group gets without an attribute, with room for the kernel's static 1 KiB)
    const size_t bitmapBytes = (((2 * (size_t)((sa.trainRange + 31) / 32)) + 3) & ~(size_t)3) * sizeof(uint32_t);
    const size_t stageRoom = ((size_t)63 << 10) - bitmapBytes;
    sa.stageCap = cap < 1536 ? cap : 1536;
    if ((size_t)sa.stageCap * 32 > stageRoom) sa.stageCap = (int)(stageRoom / 32);
    size_t lds = bitmapBytes + (size_t)sa.stageCap * 8 * sizeof(float);
    tick(ctx, slot0 + 1, false);
    // (1024-thread work-groups were measured for this kernel too: 48 us instead of 40 for a single pair)
    hipLaunchKernelGGL(ps_select_refit<kBlock>, dim3((unsigned)P), dim3(kBlock), lds, ctx->stream,
                       (const float4 *)ctx->recA.p, (const float4 *)ctx->recB.p, (const float4 *)ctx->recC.p,
                       (const int4 *)ctx->recD.p, (const int32_t *)ctx->mvalid.p, (const int32_t *)ctx->counts.p,
                       dMatches, dNumMatches, matchStride, pl.ma, pl.sc, sa, (int32_t *)ctx->idxList.p, dPose,
                       dMask, dStats, ctx->stampsOn ? (unsigned long long *)ctx->stamps.p : (unsigned long long *)nullptr,
                       (pl.bailWatch && pl.d.reorder) ? (const unsigned *)ctx->bailCnt.p + 2 * pl.bailSlot : (const unsigned *)nullptr,
                       (pl.bailWatch && pl.d.reorder) ? ctx->bailHostDev + 2 * pl.bailSlot : (unsigned *)nullptr);
    tick(ctx, slot0 + 1, true);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

int ensure_records(PsContext *ctx, size_t P, size_t cap)
{
    const size_t n = P * cap;
    PS_ENSURE(ctx->recA, n * 16);
    PS_ENSURE(ctx->recB, n * 16);
    PS_ENSURE(ctx->recC, n * 16);
    PS_ENSURE(ctx->recD, n * 16);
    PS_ENSURE(ctx->recE, n * 16);
    // 40 B per match (reprojection kernels) or up to 64 B per match pair (Euclidean kernel, ps_score_euclid.h)
    PS_ENSURE(ctx->recF, record_f_bytes(P, cap));
#ifdef PS_STREAM_DIAG
    static const bool shadow = std::getenv("PUTSLAM_HIP_DIAG_SHADOW_RECORDS") != nullptr && std::atoi(std::getenv("PUTSLAM_HIP_DIAG_SHADOW_RECORDS")) != 0;
    if (shadow) PS_ENSURE(ctx->recShadow, n * 7 * 16);
#endif
    return PS_OK;
}

} // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
static int ransac_host_entry(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                             const float *prev, int nprev, const float *cur, int ncur, const PsDMatch *matches, int m,
                             float *pose, PsDMatch *inliers, int *ninl, uint8_t *mask, PsRansacStats *stats,
                             int32_t *countsOut)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    PsRansacStats st;
    memset(&st, 0, sizeof st);
    st.bestHypothesis = -1;
    st.numMatchesIn = m > 0 ? m : 0;
    st.pointInlierRatio = NAN;
    if (pose) identity16(pose);
    if (ninl) *ninl = 0;
    if (stats) *stats = st;
    if (!pose || !ninl || m < 0 || nprev < 0 || ncur < 0 || (m > 0 && (!matches || !prev || !cur || !inliers)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_ransac_rigid3d: bad argument");
    if (mask && m > 0) memset(mask, 0, (size_t)m);
    if (m > (1 << 22)) return fail(ctx, PS_ERR_UNSUPPORTED, "too many matches");
    for (int i = 0; i < m; ++i)
        if (matches[i].queryIdx < 0 || matches[i].queryIdx >= nprev || matches[i].trainIdx < 0 ||
            matches[i].trainIdx >= ncur)
            return fail(ctx, PS_ERR_BAD_ARG, "match index out of range");
    const int cap = m > 0 ? m : 1;
    const int trainRange = ncur <= 65536 ? ncur : 0;
    Plan pl;
    rc = make_plan(ctx, params, cfg, K, cap, trainRange, pl);
    if (rc) return rc;
    if (cfg->sampleIdx) {
        PS_ENSURE(ctx->raw, (size_t)pl.H * 3 * sizeof(uint32_t));
        PS_HIP(hipMemcpyAsync(ctx->raw.p, cfg->sampleIdx, (size_t)pl.H * 3 * sizeof(uint32_t), hipMemcpyHostToDevice,
                              ctx->stream));
        pl.ma.raw = (const uint32_t *)ctx->raw.p;
    }
    rc = prepare_score(ctx, pl, 1, cap, countsOut != nullptr);
    if (rc) return rc;
    PS_ENSURE(ctx->sMisc0, (size_t)(nprev > 0 ? nprev : 1) * 12);
    PS_ENSURE(ctx->sMisc1, (size_t)(ncur > 0 ? ncur : 1) * 12);
    PS_ENSURE(ctx->sMatches, (size_t)cap * sizeof(PsDMatch));
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    PS_ENSURE(ctx->sMask, (size_t)cap);
    PS_ENSURE(ctx->sPose, 16 * sizeof(float));
    PS_ENSURE(ctx->sStats, sizeof(PsRansacStats));
    PS_ENSURE(ctx->mvalid, sizeof(int32_t));
    PS_ENSURE(ctx->cmax, sizeof(float2));
    rc = ensure_records(ctx, 1, (size_t)cap);
    if (rc) return rc;
    if (nprev > 0) PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, prev, (size_t)nprev * 12, hipMemcpyHostToDevice, ctx->stream));
    if (ncur > 0) PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, cur, (size_t)ncur * 12, hipMemcpyHostToDevice, ctx->stream));
    if (m > 0)
        PS_HIP(hipMemcpyAsync(ctx->sMatches.p, matches, (size_t)m * sizeof(PsDMatch), hipMemcpyHostToDevice,
                              ctx->stream));
    int32_t mm = m;
    PS_HIP(hipMemcpyAsync(ctx->sNumM.p, &mm, sizeof mm, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ps_prep_from_matches, dim3(1), dim3(kBlock), 0, ctx->stream, (const float *)ctx->sMisc0.p,
                       (const float *)ctx->sMisc1.p, (const PsDMatch *)ctx->sMatches.p, m, pl.pa, rec_ptrs(ctx, pl.score),
                       (int32_t *)ctx->mvalid.p, (float2 *)ctx->cmax.p);
    PS_HIP(hipGetLastError());
    rc = run_ransac_stage(ctx, pl, 1, cap, (const PsDMatch *)ctx->sMatches.p, (const int32_t *)ctx->sNumM.p, cap,
                          (float *)ctx->sPose.p, (uint8_t *)ctx->sMask.p, (PsRansacStats *)ctx->sStats.p, 2);
    if (rc) return rc;
    std::vector<uint8_t> hmask((size_t)cap);
    PS_HIP(hipMemcpyAsync(pose, ctx->sPose.p, 16 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipMemcpyAsync(&st, ctx->sStats.p, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    if (m > 0) PS_HIP(hipMemcpyAsync(hmask.data(), ctx->sMask.p, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    if (countsOut) {
        int32_t mv = 0;
        PS_HIP(hipMemcpyAsync(&mv, ctx->mvalid.p, sizeof mv, hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
        if (mv >= pl.minRun)
            PS_HIP(hipMemcpyAsync(countsOut, ctx->counts.p, (size_t)pl.H * sizeof(int32_t), hipMemcpyDeviceToHost,
                                  ctx->stream));
        else
            memset(countsOut, 0, (size_t)pl.H * sizeof(int32_t));
    }
    PS_HIP(hipStreamSynchronize(ctx->stream));
    int n = 0;
    for (int i = 0; i < m; ++i)
        if (hmask[(size_t)i]) inliers[n++] = matches[i];
    *ninl = n;
    if (mask && m > 0) memcpy(mask, hmask.data(), (size_t)m);
    if (trainRange == 0 && m > 0) {
        // train indices beyond the device bitmap: RANSAC::pointInlierRatio (RANSAC.h:56-66) on the host lists
        std::vector<uint8_t> seen((size_t)ncur, 0);
        int ua = 0, ui = 0;
        for (int i = 0; i < m; ++i) {
            uint8_t &s = seen[(size_t)matches[i].trainIdx];
            if (!(s & 1)) { s |= 1; ++ua; }
            if (hmask[(size_t)i] && !(s & 2)) { s |= 2; ++ui; }
        }
        st.pointInlierRatio = (double)ui / (double)ua;
    }
    if (stats) *stats = st;
    return PS_OK;
}

int ps_ransac_rigid3d(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                      const float *prev, int nprev, const float *cur, int ncur, const PsDMatch *matches, int m,
                      float *pose, PsDMatch *inliers, int *ninl, uint8_t *mask, PsRansacStats *stats)
{
    return ransac_host_entry(ctx, params, cfg, K, prev, nprev, cur, ncur, matches, m, pose, inliers, ninl, mask, stats,
                             nullptr);
}

} // extern "C"
