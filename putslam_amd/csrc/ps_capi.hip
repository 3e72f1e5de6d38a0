// ps_capi.hip -- the device translation unit of libputslam_hip.so (include/putslam_hip.h): the kernels (ps_kernels.h and
// friends), the plan of a call and every launch.  PsContext itself -- stream, scratch arena, option table, stop-table builders,
// timing record -- lives in ps_context.cpp / ps_internal.h, host-only; so do the batch queue and the environment default.
// There is no CPU fallback anywhere in this file: every entry point launches the HIP kernels
// of ps_kernels.h or fails with a negative PsStatus.
//
// Top to bottom: the VO path's kernel headers, the shared host glue (ps_glue.h), the plan of a call with its schedule and stages,
// the VO and host-pointer entry points, then every further feature as ONE header (its kernels, then its host glue and entry
// points) in dependency order, and psi_kernel_attributes last.
#include "ps_kernels.h"
#include "ps_matcher_mfma.h"
#include "ps_score_pass.h"
#include "ps_score_fast.h"
#include "ps_score_euclid.h"
#include "ps_internal.h"
#include "ps_glue.h"

#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace psdev;

static_assert(kPsReorderMargin == kReorderMargin && kPsReorderTopMax == kReorderTopMax, "ps_internal.h mirrors ps_score_pass.h");
static_assert(kPlanBlock == kBlock && kPlanPrefixFixed == kPrefixFixed && kPlanPrefixAdaptive == kPrefixAdaptive && kPlanStages == kStages,
              "ps_score_plan.h mirrors ps_kernels.h / ps_score_pass.h");

namespace {

constexpr int kMfmaTT = 4;       // train tiles per wave of the MFMA matcher (ps_hamming_mfma<TT>, ps_matcher_mfma.h)

// The matcher forms that merge with atomicMin start from an all-ones keys block (see PsContext::keysCleanPtr).
int keys_clean(PsContext *ctx, size_t bytes)
{
    if (ctx->keysCleanPtr == ctx->keys.p && ctx->keysCleanBytes >= bytes) return PS_OK;
    PS_HIP(hipMemsetAsync(ctx->keys.p, 0xFF, ctx->keys.cap, ctx->stream));
    ctx->keysCleanPtr = ctx->keys.p;
    ctx->keysCleanBytes = ctx->keys.cap;
    return PS_OK;
}

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
    // hypotheses that can ever be consumed by the sequential schedule
    int H = cfg->numHypotheses;
    if (cfg->estimator == PS_EST_RANSAC) {
        int a = ransac_iterations_host(0.20), b = ransac_iterations_host(prm->minimalInlierRatioThreshold);
        int most = a > b ? a : b;
        if (most < H) H = most;
        if (H < 1) H = 1;
    } else if (cfg->estimator == PS_EST_USAC) {
        if (H > (int)kUsacMaxHyp) H = (int)kUsacMaxHyp;
    }
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

void tick(PsContext *ctx, int slot, bool stop)
{
    if (!ctx->timing || slot >= kMaxTimed || ctx->ev.empty()) return;
    (void)hipEventRecord(ctx->ev[((size_t)ctx->curCall * kMaxTimed + slot) * 2 + (stop ? 1 : 0)], ctx->stream);
    if (stop) {
        ctx->slotMask[ctx->curCall] |= 1u << slot;
        if (slot + 1 > ctx->nTimed) ctx->nTimed = slot + 1;
    }
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

// Kernel 2 with (REC) or without the scoring records, BLK threads per work-group.
template <bool REC, int BLK>
void launch_prep(PsContext *ctx, const PsFrameSet &fs, const int32_t *dPairs, int P, const PrepArgs &pa, const RecPtrs &rp,
                 PsDMatch *dMatches, int32_t *dNumMatches)
{
    hipLaunchKernelGGL((ps_crosscheck_prep<REC, BLK>), dim3((unsigned)P), dim3(BLK), (size_t)fs.maxKpts * sizeof(uint32_t), ctx->stream,
                       fs.pts, fs.nkpts, dPairs, (uint32_t *)ctx->keys.p, pa, dMatches, dNumMatches, rp, (int32_t *)ctx->mvalid.p,
                       (float2 *)ctx->cmax.p, ctx->stampsOn ? (unsigned long long *)ctx->stamps.p : (unsigned long long *)nullptr);
}

// Kernels 1 + 2 for P pairs of a device-resident frame set: kernel 2 writes the records of plan `pl`, or matches only
// (pl = null).
int run_match_stage(PsContext *ctx, const PsFrameSet &fs, const int32_t *dPairs, int P, const Plan *pl, PsDMatch *dMatches,
                    int32_t *dNumMatches, int slot0)
{
    const int cap = fs.maxKpts;
    FrameStrides strides; // (PsFrameSet, ABI 2: dense unless the frames keep descriptors and points together; no points: ps_match_hamming256)
    if (int rc = frame_strides(ctx, fs, true, fs.pts != nullptr, "frame set", strides)) return rc;
    const int fstrideDw = strides.descDwords();
    PrepArgs pa = pl ? pl->pa : PrepArgs{};
    if (!pl) pa.cap = cap;
    pa.ptsStride = strides.ptsFloats();
    PS_ENSURE(ctx->keys, (size_t)P * cap * sizeof(uint32_t));
    PS_ENSURE(ctx->mvalid, (size_t)P * sizeof(int32_t));
    PS_ENSURE(ctx->cmax, (size_t)P * sizeof(float2));
    if (pl) {
        int rc = ensure_records(ctx, (size_t)P, (size_t)cap);
        if (rc != PS_OK) return rc;
    }
    // by batch size: VALU sweep 1.85 us, MFMA sweep 0.43 us per 2000 x 2000 pair on a full chip, + ~7 us for the extra launch
    const bool useMfma = ctx->matcher == 1 || (ctx->matcher == 2 && (double)P * cap * cap > 2.0e7);
    ctx->matcherUsed = useMfma ? 1 : 0;
    const size_t keyBytes = (size_t)P * cap * sizeof(uint32_t);
    // from the matcher's launch until kernel 2 has been queued behind it the keys block is in use; kernel 2 leaves what it
    // read all-ones again, so a block that was clean before this call is clean after it
    const size_t cleanBefore = ctx->keysCleanPtr == ctx->keys.p ? ctx->keysCleanBytes : 0;
    struct KeysInUse {
        PsContext *c;
        size_t restore;
        bool done = false;
        ~KeysInUse() { c->keysCleanBytes = done ? restore : 0; }
    } keysInUse{ctx, cleanBefore};
    if (useMfma) {
        // matrix-core form: expand every pair's query frame to FP4 once, then the MFMA sweep
        constexpr int TT = kMfmaTT;
        const int tpf = (cap + kTileRows - 1) / kTileRows;
        const int groups = (tpf + kWavesPerWG * TT - 1) / (kWavesPerWG * TT);
        int qsplit = pick_split((long long)P * groups, tpf, 1, tpf);
        if (ctx->forceQsplit > 0) qsplit = ctx->forceQsplit < tpf ? ctx->forceQsplit : tpf;
        if (ctx->matcherFused) {
            // fused expansion: every work-group of a query split expands its own share of the query tiles, so a split only
            // pays when the groups do not fill the chip by themselves; the splits merge with atomicMin on an all-ones keys block
            // (kept so by kernel 2: keys_clean)
            if (ctx->forceQsplit <= 0 && (long long)P * groups >= 1024) qsplit = 1;
            if (qsplit > 1) {
                int rc = keys_clean(ctx, keyBytes);
                if (rc != PS_OK) return rc;
                keysInUse.restore = ctx->keysCleanBytes;
            }
            tick(ctx, 5, false);
            hipLaunchKernelGGL(ps_hamming_mfma_fused<TT>, dim3((unsigned)(groups * qsplit) * (unsigned)P), dim3(kBlock), 0,
                               ctx->stream, (const uint32_t *)fs.desc, fs.nkpts, dPairs, cap, fstrideDw, tpf, groups, qsplit,
                               (uint32_t *)ctx->keys.p);
            tick(ctx, 5, true);
            PS_HIP(hipGetLastError());
        } else {
        PS_ENSURE(ctx->xq, (size_t)P * tpf * kTileU4 * sizeof(uint4));
        int xchunks = tpf < 8 ? tpf : 8;
        if ((long long)P * xchunks < 1024) xchunks = tpf < 64 ? tpf : 64;
        tick(ctx, 4, false);
        hipLaunchKernelGGL(ps_expand_query_fp4, dim3((unsigned)xchunks * (unsigned)P), dim3(kBlock), 0, ctx->stream,
                           (const uint32_t *)fs.desc, fs.nkpts, dPairs, cap, fstrideDw, tpf, xchunks, (uint4 *)ctx->xq.p,
                           qsplit > 1 ? (uint32_t *)ctx->keys.p : (uint32_t *)nullptr); // also clears the keys
        tick(ctx, 4, true);
        tick(ctx, 5, false);
        hipLaunchKernelGGL(ps_hamming_mfma<TT>, dim3((unsigned)(groups * qsplit) * (unsigned)P), dim3(kBlock), 0,
                           ctx->stream, (const uint32_t *)fs.desc, fs.nkpts, dPairs, cap, fstrideDw, tpf, groups, qsplit,
                           (const uint4 *)ctx->xq.p, (uint32_t *)ctx->keys.p);
        tick(ctx, 5, true);
        PS_HIP(hipGetLastError());
        }
    } else {
        constexpr int TPL = 2;
        const int tiles = (cap + kBlock * TPL - 1) / (kBlock * TPL);
        // single pair: 500 work-groups of 16 query rows (84.1 us per pair against 84.6 with 64 splits of 31 rows and 85.6
        // with 250 of 8, profiles/r04g/ab_latency.txt)
        int qsplit = pick_split((long long)P * tiles, 128, 16, cap);
        if (ctx->forceQsplit > 0) qsplit = ctx->forceQsplit;
        if (qsplit > 1) {
            int rc = keys_clean(ctx, keyBytes);
            if (rc != PS_OK) return rc;
            keysInUse.restore = ctx->keysCleanBytes;
        }
        tick(ctx, slot0, false);
        hipLaunchKernelGGL(ps_hamming_nn<TPL>, dim3((unsigned)(tiles * qsplit) * (unsigned)P), dim3(kBlock), 0, ctx->stream,
                           (const uint4 *)fs.desc, fs.nkpts, dPairs, cap, strides.descUint4(), tiles, qsplit, (uint32_t *)ctx->keys.p);
        tick(ctx, slot0, true);
        PS_HIP(hipGetLastError());
    }
    tick(ctx, slot0 + 1, false);
    const bool wide = P <= kWidePairs; // a handful of pairs: 1024-thread work-groups shorten the per-pair serial walk
    const auto prep = pl ? (wide ? launch_prep<true, 1024> : launch_prep<true, kBlock>)
                         : (wide ? launch_prep<false, 1024> : launch_prep<false, kBlock>);
    prep(ctx, fs, dPairs, P, pa, pl ? rec_ptrs(ctx, pl->score) : RecPtrs{}, dMatches, dNumMatches);
    tick(ctx, slot0 + 1, true);
    PS_HIP(hipGetLastError());
    keysInUse.done = true;
    return PS_OK;
}

void identity16(float *T)
{
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

} // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
int ps_match_hamming256(PsContext *ctx, const uint8_t *query, int nq, size_t qstep, const uint8_t *train, int nt,
                        size_t tstep, PsDMatch *out, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    if (nout) *nout = 0;
    if (!out || !nout || nq < 0 || nt < 0 || (nq > 0 && !query) || (nt > 0 && !train))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_match_hamming256: bad argument");
    if ((nq > 0 && qstep < PS_DESC_BYTES) || (nt > 0 && tstep < PS_DESC_BYTES))
        return fail(ctx, PS_ERR_UNSUPPORTED, "descriptor rows must be 32 bytes (ORB/LDB); float descriptors are out of scope");
    if (nq > PS_MAX_KPTS || nt > PS_MAX_KPTS) return fail(ctx, PS_ERR_UNSUPPORTED, "more than PS_MAX_KPTS rows");
    if (nq == 0 || nt == 0) return PS_OK; // BFMatcher on an empty side: no matches
    int cap = nq > nt ? nq : nt;
    PS_ENSURE(ctx->sDesc, (size_t)2 * cap * 32);
    PS_ENSURE(ctx->sNk, 2 * sizeof(int32_t) + 2 * sizeof(int32_t));
    PS_ENSURE(ctx->sMatches, (size_t)cap * sizeof(PsDMatch));
    PS_ENSURE(ctx->sNumM, sizeof(int32_t));
    uint8_t *dDesc = (uint8_t *)ctx->sDesc.p;
    PS_HIP(hipMemcpy2DAsync(dDesc, 32, query, qstep, 32, (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc + (size_t)cap * 32, 32, train, tstep, 32, (size_t)nt, hipMemcpyHostToDevice,
                            ctx->stream));
    int32_t hostMeta[4] = {nq, nt, 0, 1}; // nkpts[2], pair (0,1)
    PS_HIP(hipMemcpyAsync(ctx->sNk.p, hostMeta, sizeof hostMeta, hipMemcpyHostToDevice, ctx->stream));
    PsFrameSet fs;
    fs.desc = dDesc;
    fs.pts = nullptr;
    fs.nkpts = (const int32_t *)ctx->sNk.p;
    fs.numFrames = 2;
    fs.maxKpts = cap;
    fs.descFrameStride = fs.ptsFrameStride = 0;
    rc = run_match_stage(ctx, fs, (const int32_t *)ctx->sNk.p + 2, 1, nullptr, (PsDMatch *)ctx->sMatches.p, (int32_t *)ctx->sNumM.p, 0);
    if (rc) return rc;
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

#include "ps_diag.h" // ps_debug_*: the parity tests' diagnostics (no reference counterpart)

extern "C" {

// ---------------------------------------------------------------------------------------------
int ps_match_xyz(PsContext *ctx, const float *mapPos, const uint8_t *mapDesc, size_t mapDescStep, const int32_t *mapLevel,
                 int nmap, const float *curPos, const uint8_t *curDesc, size_t curDescStep, const int32_t *curLevel, int ncur,
                 double sphereRadius, double acceptRatio, PsDMatch *out, int cap, int *nout)
{
    int rc = bind(ctx);
    if (rc) return rc;
    TimingOff toff(ctx);
    if (nout) *nout = 0;
    if (!nout || nmap < 0 || ncur < 0 || cap < 0 || (cap > 0 && !out) ||
        (nmap > 0 && (!mapPos || !mapDesc || !mapLevel)) || (ncur > 0 && (!curPos || !curDesc || !curLevel)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_match_xyz: bad argument");
    if ((nmap > 0 && mapDescStep < PS_DESC_BYTES) || (ncur > 0 && curDescStep < PS_DESC_BYTES))
        return fail(ctx, PS_ERR_UNSUPPORTED, "descriptor rows must be 32 bytes (ORB/LDB)");
    if (nmap == 0 || ncur == 0) return PS_OK;
    PS_ENSURE(ctx->sMisc0, (size_t)nmap * 12);
    PS_ENSURE(ctx->sMisc1, (size_t)ncur * 12);
    PS_ENSURE(ctx->sDesc, (size_t)(nmap + ncur) * 32);
    PS_ENSURE(ctx->sNk, (size_t)(nmap + ncur) * sizeof(int32_t));
    PS_ENSURE(ctx->sMisc2, (size_t)(2 * nmap + 2) * sizeof(int32_t));
    PS_ENSURE(ctx->sMatches, (size_t)(cap > 0 ? cap : 1) * sizeof(PsDMatch));
    uint8_t *dDesc = (uint8_t *)ctx->sDesc.p;
    int32_t *dLvl = (int32_t *)ctx->sNk.p;
    int32_t *dCnt = (int32_t *)ctx->sMisc2.p, *dOff = dCnt + nmap;
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, mapPos, (size_t)nmap * 12, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, curPos, (size_t)ncur * 12, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc, 32, mapDesc, mapDescStep, 32, (size_t)nmap, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpy2DAsync(dDesc + (size_t)nmap * 32, 32, curDesc, curDescStep, 32, (size_t)ncur, hipMemcpyHostToDevice,
                            ctx->stream));
    PS_HIP(hipMemcpyAsync(dLvl, mapLevel, (size_t)nmap * 4, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(dLvl + nmap, curLevel, (size_t)ncur * 4, hipMemcpyHostToDevice, ctx->stream));
    const float bound = sq_bound_f32(sphereRadius); // (float)norm < (double)radius  <=>  squared sum < bound
    const unsigned blocks = (unsigned)((nmap + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL(ps_match_xyz_kernel<false>, dim3(blocks), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, (const uint4 *)dDesc, dLvl, nmap, (const float *)ctx->sMisc1.p,
                       (const uint4 *)(dDesc + (size_t)nmap * 32), dLvl + nmap, ncur, bound, acceptRatio, dCnt,
                       (const int32_t *)nullptr, (PsDMatch *)nullptr, 0);
    PS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ps_exclusive_scan, dim3(1), dim3(kBlock), 0, ctx->stream, dCnt, nmap, dOff);
    PS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ps_match_xyz_kernel<true>, dim3(blocks), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, (const uint4 *)dDesc, dLvl, nmap, (const float *)ctx->sMisc1.p,
                       (const uint4 *)(dDesc + (size_t)nmap * 32), dLvl + nmap, ncur, bound, acceptRatio, dCnt,
                       (const int32_t *)dOff, (PsDMatch *)ctx->sMatches.p, cap);
    PS_HIP(hipGetLastError());
    int32_t total = 0;
    PS_HIP(hipMemcpyAsync(&total, dOff + nmap, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    *nout = total;
    int ncopy = total < cap ? total : cap;
    if (ncopy > 0) {
        PS_HIP(hipMemcpyAsync(out, ctx->sMatches.p, (size_t)ncopy * sizeof(PsDMatch), hipMemcpyDeviceToHost, ctx->stream));
        PS_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (total > cap) return fail(ctx, PS_ERR_BAD_ARG, "ps_match_xyz: output capacity too small (*nout = needed)");
    return PS_OK;
}

// ---------------------------------------------------------------------------------------------
int ps_umeyama_f32(PsContext *ctx, const float *src, const float *dst, int k, int nsets, float *T, int32_t *valid)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (k < 0 || nsets < 0 || !T || !valid || (k > 0 && nsets > 0 && (!src || !dst)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_umeyama_f32: bad argument");
    if (nsets == 0) return PS_OK;
    size_t bytes = (size_t)nsets * (k > 0 ? k : 1) * 12;
    PS_ENSURE(ctx->sMisc0, bytes);
    PS_ENSURE(ctx->sMisc1, bytes);
    PS_ENSURE(ctx->sPose, (size_t)nsets * 16 * sizeof(float));
    PS_ENSURE(ctx->sMisc2, (size_t)nsets * sizeof(int32_t));
    if (k > 0) {
        PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, src, (size_t)nsets * k * 12, hipMemcpyHostToDevice, ctx->stream));
        PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, dst, (size_t)nsets * k * 12, hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(ps_umeyama_sets, dim3((unsigned)nsets), dim3(64), 0, ctx->stream, (const float *)ctx->sMisc0.p,
                       (const float *)ctx->sMisc1.p, k, nsets, (float *)ctx->sPose.p, (int32_t *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(T, ctx->sPose.p, (size_t)nsets * 16 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipMemcpyAsync(valid, ctx->sMisc2.p, (size_t)nsets * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_kabsch_f64(PsContext *ctx, const double *A, const double *B, int n, int ld, double *T)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (T)
        for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!T || n < 0 || (n > 0 && (!A || !B || ld < n))) return fail(ctx, PS_ERR_BAD_ARG, "ps_kabsch_f64: bad argument");
    if (n == 0) return PS_OK; // kabschEst.cpp:28
    size_t bytes = (size_t)3 * ld * sizeof(double);
    PS_ENSURE(ctx->sMisc0, bytes);
    PS_ENSURE(ctx->sMisc1, bytes);
    PS_ENSURE(ctx->sMisc2, (16 + (size_t)15 * 1024) * sizeof(double)); // pose + per-wave partial sums
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, A, bytes - (size_t)(ld - n) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, B, bytes - (size_t)(ld - n) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n <= 16384) { // one wavefront: lowest latency (config 1 has 500 points)
        hipLaunchKernelGGL(ps_kabsch_f64_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double *)ctx->sMisc0.p,
                           (const double *)ctx->sMisc1.p, n, ld, (double *)ctx->sMisc2.p);
    } else { // G wavefronts, two passes over the points + a finishing wave
        int G = (n + 4095) / 4096;
        if (G > 1024) G = 1024;
        double *part = (double *)ctx->sMisc2.p + 16, *part2 = part + (size_t)6 * 1024;
        hipLaunchKernelGGL(ps_kabsch_f64_sums, dim3((unsigned)G), dim3(64), 0, ctx->stream, (const double *)ctx->sMisc0.p,
                           (const double *)ctx->sMisc1.p, n, ld, part);
        hipLaunchKernelGGL(ps_kabsch_f64_cov, dim3((unsigned)G), dim3(64), 0, ctx->stream, (const double *)ctx->sMisc0.p,
                           (const double *)ctx->sMisc1.p, n, ld, (const double *)part, part2);
        hipLaunchKernelGGL(ps_kabsch_f64_finish, dim3(1), dim3(64), 0, ctx->stream, (const double *)part,
                           (const double *)part2, G, n, (double *)ctx->sMisc2.p);
    }
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(T, ctx->sMisc2.p, 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

size_t ps_depth_view_bytes(int rows, int cols, size_t depthStep) { return depth_view_bytes(rows, cols, depthStep); }

int ps_keypoints2Dto3D(PsContext *ctx, const float *xy, int n, const uint16_t *depth, int rows, int cols,
                       size_t depthStep, const float *K, double depthImageScale, float *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n < 0 || rows <= 0 || cols <= 0 || !depth || !K || depthStep < (size_t)cols * 2 || (n > 0 && (!xy || !out)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_keypoints2Dto3D: bad argument");
    if (n == 0) return PS_OK;
    const size_t bytes = depth_view_bytes(rows, cols, depthStep); // not rows x depthStep: the last row ends after its pixels
    PS_ENSURE(ctx->sMisc0, (size_t)n * 8);
    PS_ENSURE(ctx->sMisc1, bytes);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 12);
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    PS_HIP(hipMemcpyAsync(ctx->sMisc1.p, depth, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ps_backproject, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, n, (const uint8_t *)ctx->sMisc1.p, rows, cols, depthStep, bytes, K[0],
                       K[4], K[2], K[5], depthImageScale, (float *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(out, ctx->sMisc2.p, (size_t)n * 12, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_remove_image_distortion(PsContext *ctx, const float *xy, int n, const float *K, const double *dist5, float *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n < 0 || !K || !dist5 || (n > 0 && (!xy || !out)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_remove_image_distortion: bad argument");
    if (n == 0) return PS_OK;
    PS_ENSURE(ctx->sMisc0, (size_t)n * 8);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 8);
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    DistArgs a;
    for (int i = 0; i < 5; ++i) a.k[i] = dist5[i];
    a.fx = K[0]; a.fy = K[4]; a.cx = K[2]; a.cy = K[5];
    hipLaunchKernelGGL(ps_undistort_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, n, a, (float *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(out, ctx->sMisc2.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_points3Dto2D(PsContext *ctx, const float *xyz, int n, const float *K, float *uv)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n < 0 || !K || (n > 0 && (!xyz || !uv))) return fail(ctx, PS_ERR_BAD_ARG, "ps_points3Dto2D: bad argument");
    if (n == 0) return PS_OK;
    PS_ENSURE(ctx->sMisc0, (size_t)n * 12);
    PS_ENSURE(ctx->sMisc2, (size_t)n * 8);
    PS_HIP(hipMemcpyAsync(ctx->sMisc0.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ps_project_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (const float *)ctx->sMisc0.p, n, K[0], K[4], K[2], K[5], (float *)ctx->sMisc2.p);
    PS_HIP(hipGetLastError());
    PS_HIP(hipMemcpyAsync(uv, ctx->sMisc2.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PS_HIP(hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

// ---------------------------------------------------------------------------------------------
// the 72-byte per-pair record of the multi-GPU gather (include/putslam_hip.h: ps_pack_records_device)
namespace {
__global__ void ps_pack_records_kernel(const float *__restrict__ pose, const PsRansacStats *__restrict__ stats, int valid, int pairs,
                                       float *__restrict__ rec)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= pairs) return;
    float *r = rec + (size_t)p * PS_RECORD_FLOATS;
    if (p < valid) {
        for (int i = 0; i < 16; ++i) r[i] = pose[(size_t)p * 16 + i];
        r[16] = (float)stats[p].numInliers;
        r[17] = (float)stats[p].numMatchesIn;
    } else {
        for (int i = 0; i < PS_RECORD_FLOATS; ++i) r[i] = 0.0f;
    }
}
} // namespace

int ps_pack_records_device(PsContext *ctx, void *hipStream, const float *pose, const PsRansacStats *stats, int valid, int pairs,
                           float *records)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (pairs < 0 || valid < 0 || valid > pairs || (pairs > 0 && !records) || (valid > 0 && (!pose || !stats)))
        return fail(ctx, PS_ERR_BAD_ARG, "ps_pack_records_device: bad argument");
    if (pairs == 0) return PS_OK;
    hipStream_t st = hipStream ? (hipStream_t)hipStream : ctx->stream;
    hipLaunchKernelGGL(ps_pack_records_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, pose, stats, valid, pairs, records);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// ---------------------------------------------------------------------------------------------
int ps_vo_pairs_device(PsContext *ctx, const PsRansacParams *params, const PsRansacConfig *cfg, const float *K,
                       const PsFrameSet *frames, const int32_t *pairs, int P, const PsPairResults *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!frames || !out || P < 0 || (P > 0 && !pairs)) return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_device: bad argument");
    if (P == 0) return PS_OK;
    if (!frames->desc || !frames->pts || !frames->nkpts || frames->maxKpts < 1 || frames->maxKpts > PS_MAX_KPTS)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_device: bad frame set");
    if (!out->matches || !out->numMatches || !out->inlierMask || !out->pose || !out->stats)
        return fail(ctx, PS_ERR_BAD_ARG, "ps_vo_pairs_device: null output");
    FrameStrides strides; // (checked here, before anything is planned or allocated; run_match_stage resolves them for its launches)
    rc = frame_strides(ctx, *frames, true, true, "ps_vo_pairs_device", strides);
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
    rc = run_match_stage(ctx, *frames, pairs, P, &pl, out->matches, out->numMatches, 0);
    if (rc) return rc;
    return run_ransac_stage(ctx, pl, P, cap, out->matches, out->numMatches, cap, out->pose, out->inlierMask, out->stats, 2);
}

} // extern "C"

// The further features, each header its kernels and then its host side, in dependency order
#include "ps_stream_push.h"  // ps_vo_stream_create / _push: the synchronous streaming form
#include "ps_stream_async.h" // ... and the pipelined one, on the PsVoStream of the former
#include "ps_map_match.h"    // map_sweep<F, D>, its launcher and entry bodies; ps_match_xyz_device / ps_map_pairs_device (the plan and the stages above)
#include "ps_dbscan.h"       // ps_dbscan_thin(_device)
#include "ps_exclusion.h"    // ps_exclude(_device) and the three rules (DBScan's bound)
#include "ps_map_view.h"     // ps_map_views_device / ps_frame_levels_device
#include "ps_loop_closure.h" // ps_pose_sets_device / ps_loop_pairs_device (the plan and the stages above)
#include "ps_match_l2.h"     // ps_match_l2_f32 / ps_match_l2_device / ps_vo_pairs_l2_device (the plan and the stages above)
#include "ps_map_match_l2.h" // the float policy of ps_map_match.h: ps_match_xyz_l2_f32 / ps_match_xyz_l2_device / ps_map_pairs_l2_device (ps_match_l2.h too)
#include "ps_map_store_f32.h" // ps_map_views_l2_device / ps_pose_sets_l2_device / ps_loop_pairs_l2_device (ps_map_view.h, ps_loop_closure.h, ps_match_l2.h)
#include "ps_klt.h"          // ps_klt_pyramids_* / ps_klt_track_device / ps_klt_select_device / ps_perform_tracking (ps_exclusion.h's bound)
#include "ps_fast.h"         // ps_fast_detector_* / ps_detect_features(_device) (the PsImageSet rule of all three: ps_glue.h, ps_image_rule.h)
#include "ps_orb.h"          // ps_orb_pyramids_* / ps_describe_features(_device) (ps_fast.h's stable counting sort)
#include "ps_orb_detect.h"   // ps_orb_detector_* / ps_orb_detect_frames / ps_detect_features_orb (ps_fast.h's tile body, ps_orb.h's levels)
#include "ps_frame_assembly.h" // ps_gather_keypoints / ps_assemble_frames / ps_front_end_* (the launches of ps_dbscan.h, ps_orb.h, ps_orb_detect.h)
#include "ps_track_vo.h"     // ps_ransac_match_lists / ps_assemble_tracked / ps_track_vo_pairs (the plan and the stages above, ps_klt.h's launches, ps_frame_assembly.h's body)
#include "ps_uncertainty.h"  // ps_feature_uncertainty / ps_measurement_edges / ps_compute_normals / ps_compute_rgb_gradients / ps_information_matrices (ps_frame_assembly.h's back-projection)
#include "ps_patches.h"      // ps_patch_models / ps_patch_align / ps_compute_patch(_gradient) / ps_optimize_location(s) (ps_image_rule.h's set rule)
#include "ps_track_close.h"  // ps_track_candidates / ps_track_close_* (ps_exclusion.h's predicate, ps_map_view.h's level rule, the launches of ps_orb.h and ps_frame_assembly.h)

// Launch attributes of the kernels that need them (ps_internal.h; called once per context).
extern "C" void psi_kernel_attributes(void)
{
    // the cross-check kernel keeps best[q] for up to PS_MAX_KPTS queries in LDS (64 KiB of the CU's 160 KiB)
    for (const void *k : {reinterpret_cast<const void *>(&ps_crosscheck_prep<true>), reinterpret_cast<const void *>(&ps_crosscheck_prep<false>),
                          reinterpret_cast<const void *>(&ps_crosscheck_prep<true, 1024>), reinterpret_cast<const void *>(&ps_crosscheck_prep<false, 1024>)})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, PS_MAX_KPTS * 4);
    dbscan_kernel_attributes();
    exclusion_kernel_attributes();
    l2_kernel_attributes();
    klt_kernel_attributes();
    patch_kernel_attributes();
}
