// ps_score_plan.h -- the plan of the RANSAC scoring step (kernels 3, ps_score_fast.h / ps_score_euclid.h), each decision once: staged
// or complete scoring (wants_staged), what a call's launches and arena blocks look like (decide_score), the "nothing to gain" policy's
// state machine (BailTracker), the kernel-3 launches in order (stage_schedule) and the match range of every work-group and wavefront
// of such a launch (pair_split, stage_range, group_part, wave_part: host and device, ps_score_pass.h calls them).
// Pure -- no HIP header, no runtime call, no PsContext, no pointer into the arena, no heap: ps_capi.hip's prepare_score and
// score_schedule are the shells that allocate and launch what this header decides, and tests/cpp/test_score_plan.cpp includes it
// into a plain C++ program (tests/test_score_plan_host.py; tests/golden/score_plan_parent.json holds what the code decided before
// it moved here).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "putslam_hip.h"

// (mirrors of psdev::kBlock, ps_block.h, and psdev::kPrefixFixed / kPrefixAdaptive / kStages, ps_score_pass.h: the device
// translation unit checks them with static_asserts)
constexpr int kPlanBlock = 256, kPlanPrefixFixed = kPlanBlock, kPlanPrefixAdaptive = 64, kPlanStages = 3;

constexpr int kWidePairs = 16; // batches of at most this many pairs run kernel 2 with 1024-thread work-groups
// Tuning constants of the staged scoring that were per-context knobs until round 5 (debug.list_r3 / list_g3 / reorder_c2div /
// reorder_gran); every A/B since round 3 put their other values within 1 % of these (profiles/r03n, r04b), so they are constants:
// work-groups the last stage's match range is split over; where the stages' ranges are cut (multiples of kReorderGran matches, the
// second cut at 1 / kReorderC2div of the range); stage 3 runs one looping work-group per eight possible ones (list_groups).
constexpr int kListRsplit3 = 4, kReorderGran = 64, kReorderC2div = 16;
constexpr int kGenPlainFrom = 2; // complete scoring generates its models by a launch of their own from this many pairs on (ScoreDecision::genPlain)

// ------------------------------------------------------------------------------------------
// The match ranges of kernel 3's work-groups and wavefronts (ps_score_pass.h runs them on the device, tests/cpp/test_score_plan.cpp
// on a CPU): integer arithmetic on (M, by, msplit, stage, best0, cover, part) and nothing else.
// ------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#define PS_PLAN_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define PS_PLAN_HD inline
#endif

// Kinds 0 / 1: part `by` of msplit of a pair's M matches.  The range is split on match PAIRS (the loops take two matches per trip):
// only the pair's last part can be odd.
PS_PLAN_HD void pair_split(int M, unsigned by, int msplit, int &m0, int &m1)
{
    const int npair = (M + 1) >> 1;
    m0 = 2 * (int)(((long long)npair * by) / msplit);
    m1 = 2 * (int)(((long long)npair * (by + 1)) / msplit);
    m1 = m1 < M ? m1 : M;
}

// Where the pruned stages' match ranges are cut (StageArgs, ps_score_pass.h, carries one to every launch).
struct StageCuts {
    bool reordered; // the stages sweep the record ps_stage_reorder wrote -- the matches the prefix's best hypothesis rejects first
    int single;     // 1 = stage 1 sweeps ALL matches and is the only stage after the prefix
    int gran;       // reordered: stage 1 ends on a multiple of this (a power of two) ...
    int margin;     // ... this many matches after the point where a hypothesis that rejects all the leading matches is out
    int c2div;      // reordered: stage 2 takes 1 / c2div of what stage 1 leaves
};

// Match range [lo, hi) of pruned stage `stage` (1 .. kPlanStages) for a pair with M matches whose prefix reached best0.
// Reordered: every hypothesis that is not better than the prefix's best one rejects (almost all of) the leading matches too and is
// out a few matches later.
PS_PLAN_HD void stage_range(const StageCuts &sc, int stage, int M, int best0, int &lo, int &hi)
{
    int c1 = M, c2 = M;
    if (best0 > 0 && !sc.single) {
        const int miss = M - best0; // a hypothesis is out once it has missed this many matches
        if (sc.reordered) {
            const int g1 = sc.gran - 1;
            c1 = (miss + sc.margin + g1) & ~g1;
            if (c1 >= M - M / 8) c1 = M;
            if (c1 < M) {
                // (stage 2 ends where it would with stage 1 cut at a multiple of 64, whatever stage 1's granularity)
                const int c64 = (c1 + 63) & ~63;
                const int step = ((M - c64) / sc.c2div + 63) & ~63;
                c2 = c64 + (step > 0 ? step : 64); // (never an empty stage 2: it hands the survivors on)
                if (c2 >= M - M / 16) c2 = M;
            }
        } else {
            c1 = (miss + miss / 7 + 32 + 63) & ~63;
            if (c1 >= M - M / 8) c1 = M; // nothing worth a second launch
            if (c1 < M) {
                c2 = (c1 + (M - c1) / 2 + 63) & ~63;
                if (c2 >= M - M / 16) c2 = M;
            }
        }
    }
    static_assert(kPlanStages == 3, "three pruned stages");
    lo = stage == 1 ? 0 : (stage == 2 ? c1 : c2); // (selects, not an indexed array: that would live in scratch memory)
    hi = stage == 1 ? c1 : (stage == 2 ? c2 : M);
}

// Stages 2+: hypotheses one pass of a work-group takes from the survivor list.  After the reordered stage 1 the lists are
// short and the ranges left are long: a pair with at most 64 (128) survivors is swept by ONE work-group whose four
// wavefronts each take a quarter (two halves) of the match range for the same hypotheses and add their counts up in LDS --
// a single wavefront alone on its SIMD waits out every record load (stage 3 of the bench step: 21 survivors per pair, 157 us
// that way, profiles/r03k).  Longer lists: 256 hypotheses per pass as before.  The launches carry a few work-groups per
// pair (StageArgs::hCount / 256) that loop over the list: thousands of work-groups that find nothing to do still cost
// their launch (30 ... 50 us per empty stage of 7485 work-groups).
PS_PLAN_HD int list_cover(int n) { return n <= 64 ? 64 : (n <= 128 ? 128 : kPlanBlock); }

// Part `by` of msplit of a stage's range [m0, m1), in whole blocks of 64 matches from m0 (the LAST stage may split its range over
// work-groups: their counts meet in counts[]).  A part beyond the range's end comes out with m0 >= m1.
PS_PLAN_HD void group_part(unsigned by, int msplit, int &m0, int &m1)
{
    const int blen = (((m1 - m0 + msplit - 1) / msplit) + 63) & ~63;
    m0 += (int)by * blen;
    m1 = m1 < m0 + blen ? m1 : m0 + blen;
}

// ... and within it the part of one of the kPlanBlock / cover groups of wavefronts that sweep the same `cover` hypotheses (whole
// blocks of 64 matches again; a part may be empty)
PS_PLAN_HD void wave_part(int part, int cover, int &m0, int &m1)
{
    const int parts = kPlanBlock / cover;
    const int plen = ((m1 - m0 + parts * 64 - 1) / (parts * 64)) * 64;
    m0 += part * plen;
    m1 = m1 < m0 + plen ? m1 : m0 + plen;
    m1 = m1 < m0 ? m0 : m1; // (an empty part: nothing to sweep, no odd last match either)
}

// Which kernel 3 scores a call: the value-exact ps_ransac_score (option "score" = 0, and the Mahalanobis error), else the
// decision-exact Euclidean ps_ransac_score_euclid (errorVersion 0 / 4) or reprojection ps_ransac_score_fast (1 / 2).  Kernel 2
// writes the records that family reads (rec_ptrs, PrepArgs::skipE / skipF).
enum class Scoring { Value, Euclid, Reproj };

// where the staged scoring takes over from complete scoring (wants_staged): batch size in work units = pairs x
// (ceil(H / 256) - 1) x frame capacity, threshold = base + perRow x frame capacity (profiles/r05c/staged_crossover.txt)
struct StagedFrom {
    double base, perRow;
};
// ... and where it does when the context is one of several launch chains that run side by side (option "side_by_side": the
// chains of a PsBatchQueue, the lanes of the pipelined stream): the other chains' kernels fill the gaps between the staged form's
// dependent, chip-underfilling launches, so what is left of its price is the work of the extra launches -- the crossover lies
// 2 - 5 times lower (profiles/r06u/concurrent_crossover.txt: four chains, 500 ... 4000 keypoints x H = 1024 ... 16384 x 2 ... 64
// pairs on the C++ demo's frames, 73 % inliers; profiles/r06u/bench_data_crossover.txt: bench.py's kind of data with 70 % / 40 % true
// correspondences, where the staged form abandons less -- the constants are set by the latter: batches of 32 / 64 pairs of the
// bench workload's shape gain 1.26 / 1.58 x with the reprojection error, 1.27 / 1.58 x with the Euclidean one)
// [Euclid / Reproj][fixed / adaptive schedule][alone / side by side]
constexpr StagedFrom kStagedFrom[2][2][2] = {{{{7.8e5, 250.0}, {4.5e5, 75.0}}, {{6.0e4, 0.0}, {2.4e4, 0.0}}},
                                             {{{1.3e6, 500.0}, {3.0e5, 90.0}}, {{4.5e4, 0.0}, {2.4e4, 0.0}}}};

// What is scored: P pairs of at most cap matches, H hypotheses each, under error `mode` by the kernels of `score`; complete = every
// hypothesis completely whatever the batch size (ps_debug_ransac_counts); adaptive = a batched, asynchronous entry point.
struct ScoreShape {
    int P = 0, cap = 0, H = 0, mode = 0;
    Scoring score = Scoring::Value;
    int estimator = 0;
    bool complete = false, adaptive = false;
};

// The context's options that the plan reads (PsContext, ps_internal.h: the same names), as they stood when the call began.
struct ScoreOptions {
    int prune = 1, sideBySide = 0, reorder = 2, genSplit = 1, singleRest = 1, pretest = 1, listGroups2 = 0, forcePrefix = 0, forceMsplit = 0,
        modelRoomMiB = 0, bail = 1, reorderMargin = 16;
};

inline int pick_split(long long blocksWithout, int maxSplit, int minChunkOf, int total)
{
    // Few pairs and many CUs: split the inner range so that ~8 workgroups per CU are in flight.
    const long long want = 2048;
    if (blocksWithout >= want) return 1;
    long long s = (want + blocksWithout - 1) / (blocksWithout > 0 ? blocksWithout : 1);
    if (s > maxSplit) s = maxSplit;
    while (s > 1 && total / s < minChunkOf) --s;
    return (int)(s < 1 ? 1 : s);
}

// launches of the reprojection kernels with more work-groups than this use the packed match record (ps_score_fast.h, BIG)
inline unsigned big_limit(int mode) { return mode == PS_REPROJECTION_ERROR ? 1536u : 1280u; }

// bytes of the hot record of P pairs: 40 B per match (reprojection kernels) or up to 64 B per match pair (Euclidean kernel, ps_score_euclid.h)
inline size_t record_f_bytes(size_t P, size_t cap)
{
    const size_t n = P * cap;
    return n * 40 > P * ((cap + 1) / 2) * 64 ? n * 40 : P * ((cap + 1) / 2) * 64;
}

// staged scoring: stages 1+ sweep the reordered hot record (option "reorder")
inline bool will_reorder(const ScoreShape &s, const ScoreOptions &o) { return o.reorder == 1 || (o.reorder == 2 && s.estimator == PS_EST_FIXED); }

// Cost model (round 5): the staged form trades six or seven dependent launches for the evaluations it abandons, and an
// evaluation's worth of work is a (hypothesis, match) pair -- so the batch is sized in work-groups of 256 hypotheses beyond the
// first one x rows of the frame capacity (matches <= keypoints), and the crossover is where (1 - share of evaluations left)
// of that pays for the launches: base + perRow x capacity, fitted on profiles/r05c/staged_crossover.txt over 500 ... 4000
// keypoints x H = 1024 ... 16384 (rounds 3 - 4 counted work-groups only, with constants from 2000 keypoints that DESIGN
// section 8 knew to be 2 - 14 % off on either side; adaptive schedules gain from far smaller batches than they were given).
// (the staged form is six or seven dependent launches, 0.23 ms at the least with the reprojection kernels and 0.08 ms with
// the Euclidean ones: it pays from about 48 / 16 pairs of H = 4096 on, profiles/r03p/small_batches.txt)
// (adaptive schedules: the trip limit the prefix leaves cuts most of the work whatever the batch size)
// Option "prune" = 2 takes the staged form whenever the kernels have it (tests; A/B).
inline bool wants_staged(const ScoreShape &s, const ScoreOptions &o)
{
    const int hb = (s.H + kPlanBlock - 1) / kPlanBlock;
    const double units = (double)s.P * (double)(hb - 1) * (double)s.cap;
    const StagedFrom(&sf)[2] = kStagedFrom[s.score == Scoring::Euclid ? 0 : 1][s.estimator == PS_EST_FIXED ? 0 : 1];
    double stagedFrom = sf[0].base + sf[0].perRow * (double)s.cap;
    if (o.sideBySide >= 2) {
        const double sbs = sf[1].base + sf[1].perRow * (double)s.cap;
        // (two chains hide half of one another's gaps: half way between the two crossovers, on the logarithmic scale)
        stagedFrom = o.sideBySide >= 3 ? sbs : std::sqrt(sbs * stagedFrom);
    }
    // (pruned scoring: the decision-exact kernels have it; the later stages read the models back from HBM, ps_score_pass.h)
    return !s.complete && o.prune != 0 && s.score != Scoring::Value && s.H > kPlanPrefixFixed && (o.prune == 2 || units >= stagedFrom);
}

// The arena blocks whose sizes the plan decides, in the order they are asked for.
enum ScoreBlock { kBlkCounts, kBlkModels, kBlkSurvA, kBlkSurvB, kBlkSurvN, kBlkValidMask, kBlkRecF2, kBlkPermBuf, kBlkPrefInfo, kBlkFrontRec, kScoreBlocks };

// Decisions of the scoring stage that the preceding kernels need to know: how the match range is split (kernel 2 then
// clears the counts, instead of a memset launch), whether kernel 3 parks its models for kernel 4 and which records it reads.
struct ScoreDecision {
    int status = PS_OK;     // PS_ERR_UNSUPPORTED: the batch is refused (nothing else is set)
    bool staged = false;    // hypotheses [0, prefix) completely (msplit applies to it), the rest in pruned stages
    int msplit = 1;         // work-groups the match range of kernel 3 is split over
    bool genSplit = false;  // staged scoring: stage 0 as two launches (models, then the sweep)
    bool genPlain = false;  // complete scoring with a split match range, two pairs or more: the same two launches over [0, H)
    bool reorder = false;   // staged scoring: stages 1+ sweep the reordered hot record (ps_stage_reorder)
    int prefix = 0;         // 256 (fixed schedule) or 64 (adaptive schedules)
    int lastStage = 0;      // staged scoring: 1 = ONE stage after the prefix (adaptive schedules without reordering), else kStages
    bool big0 = false;      // Scoring::Reproj: stage 0 or the complete scoring runs the build for big launches
    int modelH = 0;         // hypotheses per pair with a model slot (ModelArgs::modelH)
    bool parkModels = false; // kernel 3 parks its models (ModelArgs::models)
    bool skipE = true, skipF = true; // the reprojection kernels' record forms no launch of this call reads (PrepArgs)
    bool zeroCounts = false; // kernel 2 clears the first zeroH counts of every pair (PrepArgs)
    int zeroH = 0;
    size_t bytes[kScoreBlocks] = {}; // what every arena block has to hold; 0 = the call does not touch it
};

inline ScoreDecision decide_score(const ScoreShape &s, const ScoreOptions &o, bool staged)
{
    ScoreDecision d;
    const int P = s.P, H = s.H, cap = s.cap;
    const int hb = (H + kPlanBlock - 1) / kPlanBlock;
    // Complete scoring of a batch under a long cap is the reference's own worst case times P (850 000 iterations over every
    // match, USAC_wrapper.cpp:70): minutes of GPU time behind an asynchronous call.  It is refused -- here, before the counts
    // block (4 bytes per pair and hypothesis: hundreds of GB for such a batch) is asked for; the staged scoring (option "prune",
    // the default) takes the same batch in milliseconds whenever the schedules end early.
    if (s.adaptive && !staged && (double)P * (double)H * (double)cap > 2.0e14) {
        d.status = PS_ERR_UNSUPPORTED;
        return d;
    }
    d.staged = staged;
    // (the later stages read the models back from HBM, 48 B per hypothesis: ps_score_pass.h)
    const size_t mbytes = (size_t)P * H * 12 * sizeof(float);
    d.prefix = s.estimator == PS_EST_FIXED ? kPlanPrefixFixed : kPlanPrefixAdaptive;
    if (o.forcePrefix > 0 && s.estimator == PS_EST_FIXED) d.prefix = o.forcePrefix; // (tuning knob)
    d.bytes[kBlkCounts] = (size_t)P * H * sizeof(int32_t);
    d.msplit = pick_split((long long)P * (staged ? 1 : hb), 32, 64, cap);
    d.genSplit = staged && o.genSplit != 0 && d.msplit > 1;
    if (d.genSplit) d.msplit = d.msplit * 2 < 32 ? d.msplit * 2 : 32; // (the parts no longer repeat the prologue)
    if (o.forceMsplit > 0) d.msplit = o.forceMsplit;
    if (d.msplit <= 1) d.genSplit = false;
    d.zeroCounts = d.msplit > 1;
    d.zeroH = staged ? d.prefix : H;
    d.modelH = H;
    d.reorder = staged && will_reorder(s, o);
    // adaptive schedules without reordering: ONE stage after the prefix (all matches, hypotheses below the trip limit only)
    d.lastStage = (s.estimator != PS_EST_FIXED && !will_reorder(s, o) && o.singleRest != 0) ? 1 : kPlanStages;
    if (staged) {
        // Parked models in proportion to the work, not to the cap: under a long cap (USAC's 850 000, USAC_wrapper.cpp:70) the
        // schedules end after a handful of iterations (USAC.h:944-971), and 48 bytes per pair and cap entry would be 20 GB for
        // 499 pairs.  Only the leading hypotheses get a slot (256 MB under the adaptive schedules, 2 GiB under the fixed one,
        // whose stages do read the models back); a hypothesis beyond is swept in one piece by stage 1 and, if it wins, rebuilt
        // by kernel 4.
        const size_t room = o.modelRoomMiB > 0 ? ((size_t)o.modelRoomMiB << 20) : (s.estimator == PS_EST_FIXED ? ((size_t)2 << 30) : ((size_t)256 << 20));
        if (mbytes > room) {
            long long fit = (long long)(room / ((size_t)P * 12 * sizeof(float))) & ~(long long)(kPlanBlock - 1);
            d.modelH = (int)(fit < kPlanPrefixFixed ? kPlanPrefixFixed : fit);
        }
    }
    if ((P <= kWidePairs && mbytes <= ((size_t)64 << 20)) || staged) {
        d.bytes[kBlkModels] = (size_t)P * d.modelH * 12 * sizeof(float);
        d.parkModels = true;
    }
    // Complete scoring with the match range split over msplit work-groups repeats the sample -> SVD chain in every part (16
    // pairs, H = 4096, errorVersion 1: 23 M of the launch's 45 M instructions).  From two pairs on the models are generated
    // once by a launch of their own, as stage 0 of the staged scoring does, and the sweep reads them back: 4 to 15 % of the
    // call for 2 ... 48 pairs (profiles/r04h/ab_gen_plain.txt).  A single pair keeps one launch: the chain's latency is all
    // there is, and a second launch costs 3 - 5 us more than it saves.
    if (!staged && s.score != Scoring::Value && o.genSplit != 0 && d.msplit > 1 && P >= kGenPlainFrom && mbytes <= ((size_t)1 << 30)) {
        d.bytes[kBlkModels] = mbytes; // (complete scoring: modelH = H, every hypothesis has a slot)
        d.parkModels = true;
        d.bytes[kBlkValidMask] = (size_t)P * ((H + 63) / 64) * sizeof(unsigned long long);
        d.genPlain = true;
    }
    // which record form of the reprojection kernels the launches of this call read (kernel 2 writes only those: 16 + 40 bytes
    // per match otherwise): the packed form F for launches that fill the chip (the build for big launches, BIG) and every stage
    // after the prefix, the three-record form (A, B, E) for small ones
    d.big0 = (unsigned)d.msplit * (unsigned)P * (staged ? 1u : (unsigned)hb) > big_limit(s.mode);
    d.skipF = !(s.score == Scoring::Reproj && (staged || d.big0));
    d.skipE = !(s.score == Scoring::Reproj && !d.big0);
    if (staged) {
        if (d.lastStage > 1) // (only hypotheses with a model slot are ever listed)
            d.bytes[kBlkSurvA] = d.bytes[kBlkSurvB] = (size_t)P * d.modelH * sizeof(int32_t);
        d.bytes[kBlkSurvN] = (size_t)2 * P * sizeof(int32_t); // cleared by kernel 2, one counter per pair and stage
        if (d.genSplit) d.bytes[kBlkValidMask] = (size_t)P * ((d.prefix + 63) / 64) * sizeof(unsigned long long);
        if (d.reorder) {
            d.bytes[kBlkRecF2] = record_f_bytes((size_t)P, (size_t)cap);
            d.bytes[kBlkPermBuf] = (size_t)P * cap * sizeof(int32_t);
            d.bytes[kBlkPrefInfo] = (size_t)4 * P * sizeof(int32_t);
            d.bytes[kBlkFrontRec] = (size_t)P * ((cap + 1) / 2) * 10 * sizeof(float);
        }
    }
    return d;
}

// "Nothing to gain" policy of the staged scoring (PsContext, ps_internal.h, has the whole story): its state per KIND of call, eight
// kinds at a time.  s0 / s1 are a slot's two monotonic counters as the host last read them: pairs replayed, pairs with nothing to gain.
struct BailKey {
    int mode = -1, estimator = 0, H = 0, pclass = 0, cap = 0;
    const void *frames = nullptr;
    bool operator==(const BailKey &k) const
    {
        return mode == k.mode && estimator == k.estimator && H == k.H && pclass == k.pclass && cap == k.cap && frames == k.frames;
    }
};

// whether a call takes part in the policy at all: batched calls in the staged, reordered form, Euclidean metrics, fixed schedule
inline bool bail_applies(const ScoreShape &s, const ScoreOptions &o, bool staged)
{
    return s.adaptive && staged && will_reorder(s, o) && o.bail != 0 && s.score == Scoring::Euclid && s.estimator == PS_EST_FIXED;
}

inline BailKey bail_key(const ScoreShape &s, const void *frames)
{
    BailKey k;
    k.mode = s.mode; k.estimator = s.estimator; k.H = s.H; k.cap = s.cap; k.frames = frames;
    for (int q = s.P; q > 1; q >>= 1) ++k.pclass; // the batch-size class
    return k;
}

struct BailTracker {
    static constexpr int kKinds = 8;
    struct Kind {
        BailKey key;
        unsigned seen[2] = {0, 0};
        int hopeless = 0, calls = 0;
        unsigned long long used = 0; // (least recently used slot is recycled)
    };
    Kind kinds[kKinds];
    unsigned long long clock = 0;

    void reset() { *this = BailTracker(); }
    // the slot of this kind of call, now the most recently used one; a new kind takes the least recently used slot and starts from
    // "staged" (recycled = true: adopt() what the slot's counters hold before the first observe())
    int find(const BailKey &key, bool &recycled)
    {
        int slot = -1, lru = 0;
        for (int i = 0; i < kKinds; ++i) {
            if (kinds[i].key == key) slot = i;
            if (kinds[i].used < kinds[lru].used) lru = i;
        }
        recycled = slot < 0;
        if (recycled) {
            slot = lru;
            kinds[slot] = Kind();
            kinds[slot].key = key;
        }
        kinds[slot].used = ++clock;
        return slot;
    }
    // (the slot's counters are monotonic: what its previous kind left there is simply "seen")
    void adopt(int slot, unsigned s0, unsigned s1)
    {
        kinds[slot].seen[0] = s0;
        kinds[slot].seen[1] = s1;
    }
    // the counters as they stand now; returns whether the kind's last observation said "most pairs have nothing to gain"
    int observe(int slot, unsigned s0, unsigned s1)
    {
        Kind &b = kinds[slot];
        if (s0 != b.seen[0]) { // a new observation of this kind has landed
            const unsigned d0 = s0 - b.seen[0], d1 = s1 - b.seen[1];
            const int was = b.hopeless;
            b.hopeless = (2ull * d1 > d0) ? 1 : 0;
            if (b.hopeless != was) b.calls = 0;
            b.seen[0] = s0;
            b.seen[1] = s1;
        }
        return b.hopeless;
    }
    // complete scoring while nothing can be abandoned; every 16th call looks again
    bool veto(int slot)
    {
        Kind &b = kinds[slot];
        return b.hopeless && (++b.calls & 15) != 0;
    }
};

// One launch of kernel 3 of KIND `kind`: 0 (stage 0 / the complete scoring), 1 (stage 1; loop: looping work-groups) or 2 (stages 2+),
// over groups x msplit x P work-groups; the rest is what its StageArgs (ps_score_pass.h) holds, an arena block named by its use.
struct StageLaunch {
    int kind = 0;
    bool loop = false;
    int stage = 0, genOnly = 0, hBase = 0, hCount = 0;
    unsigned groups = 0;
    int msplit = 1;
    bool validMask = false, perm = false, frontRec = false; // (perm: the order and the prefix's (best count, trip limit), prefInfo, come together)
    int listIn = 0, listOut = 0;                            // 0 = none, 1 = survivor list A with its counters, 2 = list B
    int single = 0, loopGroups = 0;
};

// Kernel 3 of the decision-exact scoring (ps_score_fast.h, ps_score_euclid.h; the staged protocol: ps_score_pass.h).  Staged scoring: stage 0 = the prefix completely,
// stages 1 .. lastStage = the rest with hypotheses abandoned between the launches; otherwise every hypothesis of [0, H) completely.
struct StageSchedule {
    int n = 0;
    StageLaunch launch[2 + kPlanStages];
    int reorderBefore = -1; // ps_stage_reorder runs in front of this launch (stage 1), -1 = not at all
    bool pretest = false;   // ... and writes the all-reject front for stage 1's one-direction pre-test
};

inline StageSchedule stage_schedule(const ScoreShape &s, const ScoreOptions &o, const ScoreDecision &d)
{
    StageSchedule sch;
    auto groups = [](int hCount) { return (unsigned)((hCount + kPlanBlock - 1) / kPlanBlock); };
    if (!d.staged) {
        StageLaunch l; // the plain launch: every hypothesis of [0, H) completely
        l.hCount = s.H;
        l.groups = groups(s.H);
        if (d.genPlain) { // the same as two launches (ScoreDecision::genPlain): models, then the sweep
            l.validMask = true;
            l.genOnly = 1;
            sch.launch[sch.n++] = l;
            l.genOnly = 0;
        }
        l.msplit = d.msplit;
        sch.launch[sch.n++] = l;
        return sch;
    }
    // stages 2+: work-groups per pair (they loop over longer lists; after the reordered stage 1 few hypotheses are left)
    auto list_groups = [&](int stage) {
        const int listed = (s.H < d.modelH ? s.H : d.modelH) - d.prefix; // hypotheses that can be on a survivor list
        const int all = ((listed > 0 ? listed : 1) + kPlanBlock - 1) / kPlanBlock;
        // (stage 3 by default: one looping group per eight possible ones -- 1 for H = 4096, where 21 of 3840 hypotheses per
        // pair are left, 48 for the stress configuration's H = 100 000, which one group swept in 4.3 ms instead of 1.0)
        const int auto3 = all / 8 > 1 ? all / 8 : 1;
        // (stage 2 by default: every possible group with the reprojection kernels -- a fifth of the hypotheses survives stage 1
        // there --, two looping groups with the Euclidean ones, whose counts saturate: hardly anything survives and the
        // launch is mostly work-groups that find nothing, 2 - 3 % of the step at every inlier share tried,
        // profiles/r04b/ab_euclid_list_groups.txt)
        const int auto2 = s.score == Scoring::Euclid ? (all / 8 > 2 ? all / 8 : 2) : 64; // (many hypotheses: lists can be long)
        const int want = d.reorder ? (stage == 2 ? (o.listGroups2 > 0 ? o.listGroups2 : auto2) : auto3) : all;
        return want < all ? want : all;
    };
    // stage 1's one-direction pre-test on the far-off front of the reordered record: the reprojection metrics (ps_score_fast.h)
    sch.pretest = d.reorder && o.pretest != 0 && (s.mode == PS_EUCLIDEAN_AND_REPROJECTION_ERROR || s.mode == PS_REPROJECTION_ERROR);
    // Stage 1 of an adaptive schedule with a long cap (USAC's 850 000 = 3320 blocks of 256 hypotheses per pair, of which the
    // trip limit leaves a handful): one work-group per block is hundreds of thousands of work-groups that look at the limit and
    // leave -- 0.9 ms per 210 pairs.  From 64 blocks per pair on a fixed number of work-groups per pair walks the blocks and
    // stops at the first one beyond the limit (enough of them to fill the chip when the limit does stay at the cap).
    const int blocks1 = (s.H - d.prefix + kPlanBlock - 1) / kPlanBlock;
    int loopGroups = 0;
    if (s.estimator != PS_EST_FIXED && blocks1 > 64) {
        // (64 per pair at the least until round 5: 32 000 work-groups per 499 pairs that read the limit and leave, a third of the
        // scoring step under USAC's cap; 4096 in all still fill the chip when the limits do stay at the cap)
        loopGroups = (4096 + s.P - 1) / s.P;
        loopGroups = loopGroups < 4 ? 4 : loopGroups;
        loopGroups = loopGroups > blocks1 ? blocks1 : loopGroups;
    }
    // stage 0, as two launches under genSplit: models + validity, then the sweep reading them back
    StageLaunch l0;
    l0.hCount = d.prefix;
    l0.groups = groups(d.prefix);
    l0.single = d.lastStage == 1 ? 1 : 0;
    l0.validMask = d.genSplit;
    if (d.genSplit) {
        l0.genOnly = 1;
        sch.launch[sch.n++] = l0;
        l0.genOnly = 0;
    }
    l0.msplit = d.msplit;
    sch.launch[sch.n++] = l0;
    if (d.reorder) sch.reorderBefore = sch.n;
    for (int stage = 1; stage <= d.lastStage; ++stage) {
        StageLaunch l;
        l.kind = stage == 1 ? 1 : 2;
        l.stage = stage;
        l.hBase = d.prefix;
        l.single = l0.single;
        l.perm = d.reorder;
        l.listIn = stage == 1 ? 0 : stage - 1;
        l.listOut = stage == 3 ? 0 : stage;
        if (stage == 1) {
            l.loop = loopGroups > 0;
            l.loopGroups = loopGroups;
            l.hCount = s.H - d.prefix;
            l.groups = loopGroups > 0 ? (unsigned)loopGroups : groups(s.H - d.prefix);
            l.frontRec = sch.pretest;
        } else {
            l.groups = (unsigned)list_groups(stage);
            l.hCount = (int)l.groups * kPlanBlock; // work-groups per pair that sweep the survivor list
            // the last stage: work-groups its match range is split over (their counts add up in counts[]; a short survivor list
            // swept by one wavefront per SIMD pays the full latency of every record load, 0.25 us per match)
            l.msplit = (d.reorder && stage == kPlanStages) ? kListRsplit3 : 1;
        }
        sch.launch[sch.n++] = l;
    }
    return sch;
}
