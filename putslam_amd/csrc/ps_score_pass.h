// ps_score_pass.h -- the staged-scoring protocol of kernel 3, once, for the two decision-exact families: ps_ransac_score_fast
// (ps_score_fast.h, the reprojection metrics) and ps_ransac_score_euclid (ps_score_euclid.h, the Euclidean metrics).
//
// The families differ in the hot loop, the band arithmetic and how they hand doubtful evaluations to inlier_test().  Everything
// around that is here: what a launch of the staged scoring is told (StageArgs), the replay of the prefix, and the frame of one
// pass of a work-group -- whose hypotheses and which matches (pass_begin), where the model comes from (pass_model), where the counts,
// the survivors and their models go (pass_finish) -- and the walk of a work-group over its passes (score_kernel_body).  All of it is
// force-inlined: a kernel is compiled as if the frame were written out in it.  The range arithmetic itself is pure and lives in
// ps_score_plan.h, where a CPU test runs it.
#pragma once

#include "ps_score_value.h"
#include "ps_select_refit.h"
#include "ps_score_plan.h"

namespace psdev {

// Limits of the decision-exact Euclidean test (derivation: ps_score_euclid.h), used by ps_ransac_score_euclid<0/4> and by
// the Euclidean term of ps_ransac_score_fast<2>.
struct EuclidConsts {
    float tbLo;  // errorVersion 0 / 2: sqrt(B) (1 - 6u) rounded down; errorVersion 4: thr (1 - 7u) rounded down
    float tbHi;  // ... (1 + 6u) / (1 + 7u) rounded up
    int enabled; // threshold inside the range the bounds were derived for
};

constexpr float kEpsU = 5.9604644775390625e-08f; // 2^-24

typedef float v2f_t __attribute__((ext_vector_type(2)));

PS_D v2f_t pk_fma(v2f_t a, v2f_t b, v2f_t c) { return __builtin_elementwise_fma(a, b, c); }

// largest row sum of |R| and largest |t| (NaN anywhere makes the sums NaN: the caller's comparison then fails)
PS_D void model_norms(const Rigid &m, float &rho, float &tau)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float rs = (fabsf(m.R[i][0]) + fabsf(m.R[i][1])) + fabsf(m.R[i][2]);
        rho = rs > rho ? rs : (rs == rs ? rho : rs); // propagate NaN
        const float ta = fabsf(m.t[i]);
        tau = ta > tau ? ta : (ta == ta ? tau : ta);
    }
}

// The models of a work-group's 256 hypotheses parked in LDS, one column per thread: rows 0 .. 8 = R, 9 .. 11 = t.
typedef float LdsModels[12][kBlock];
PS_D void lds_put_model(LdsModels &s_mdl, int t, const Rigid &m)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s_mdl[3 * i + j][t] = m.R[i][j];
        s_mdl[9 + i][t] = m.t[i];
    }
}
PS_D void lds_get_model(const LdsModels &s_mdl, int t, Rigid &m)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) m.R[i][j] = s_mdl[3 * i + j][t];
        m.t[i] = s_mdl[9 + i][t];
    }
}

// ------------------------------------------------------------------------------------------
// Staged scoring: hypotheses that provably cannot matter are abandoned between launches.
//
// The selection of kernel 4 consumes the counts sequentially: hypothesis i matters only if its count is a RECORD,
// count_i > max_{j<i} count_j (strict '>' first-best, RANSAC.cpp:438-455; the arg-max of the fixed schedule takes the
// lowest index among equals, the same rule), and only while i is below the adaptive trip limit, which from record to
// record only shrinks (RANSAC.cpp:450-453, USAC.h:944-971).  So a large batch is scored in stages:
//   stage 0   the first 256 hypotheses of every pair (64 for the adaptive schedules, whose limit after a few dozen
//             hypotheses is usually below that already), all matches (the plain launch);
//   stage 1   every later hypothesis below the trip limit L0 the prefix leaves, matches [0, c1);
//   stage 2   the SURVIVORS of stage 1, matches [c1, c2);        stage 3   the survivors of stage 2, matches [c2, M).
// Every work-group of stages 1-3 first replays the selection over the prefix (wave_replay_prefix: the record walk of
// ps_select_refit) and gets B0 = the best count so far and L0.  After its match range a hypothesis survives if
// count so far + matches left > B0; otherwise it can no longer become a record and keeps its partial count
// (<= B0: never selected, never a record).  Survivors are appended (one atomic per wavefront) to the next stage's
// per-pair list, which the next launch reads back densely: 256 live hypotheses per work-group again, full wavefronts,
// no barrier and no re-packing inside the hot loops -- they are the plain loops.  The models travel through HBM
// (ma.models, 48 B per hypothesis), the partial counts through counts[].
//   c1 = about 1.15 (M - B0) + 32 matches: where a hypothesis without inliers has run out of chances (with 75 % inliers
//   a bad sample is abandoned after a quarter of the matches); c2 halves the rest.  With the reference's own <= 487-iteration
//   schedule L0 is typically 2 ... 30, far below the prefix: stages 1-3 return at once.
// An in-kernel form (checkpoints + re-packing of live lanes through LDS inside one launch) was built first and kept
// the wave-steps it saved (29 %) from showing up as time: barriers, rebuilds and 300 bytes of scratch per lane made the
// loop 20 % slower before anything was abandoned (profiles/r03c/README.md).
// Outputs of kernel 4 are unchanged bit for bit (tests/test_gpu_prune.py: staged vs complete vs oracle); what changes is
// the meaning of counts[] for abandoned hypotheses (a lower bound <= B0 instead of the count), which is why the
// diagnostic ps_debug_ransac_counts and small batches score completely.
// ------------------------------------------------------------------------------------------
constexpr int kPrefixFixed = kBlock; // hypotheses scored completely by stage 0: fixed schedule (arg-max over all H) ...
constexpr int kPrefixAdaptive = 64;  // ... and RANSAC / USAC schedules (the reference consumes 3 of 487 on good data)
constexpr int kStages = 3;      // pruned stages after the prefix
constexpr int kReorderTopMax = 16; // ps_stage_reorder: at most this many of the prefix's best hypotheses vote on the order
constexpr int kReorderMargin = 16; // reordered sweep: stage 1 ends this many matches (rounded up to 64) after the point where
                                   // a hypothesis that rejects all the leading matches is out

struct StageArgs {
    int stage;                 // 0 = the hypotheses [hBase, hBase + hCount) completely (the plain launch: [0, H)); 1 .. kStages
                               // = pruned stages
    int hBase, hCount;         // stage 0 / 1: the hypothesis range of this launch
    int listStride;            // entries per pair of the survivor lists (= hypotheses with a model slot: only those are listed)
    const int32_t *listIn;     // stage >= 2: survivors of the previous stage, [P][listStride] hypothesis indices ...
    const int32_t *countIn;    //             ... and how many per pair
    int32_t *listOut;          // stage < kStages: where this stage's survivors go
    int32_t *countOut;
    const int32_t *perm;       // stage >= 1 after ps_stage_reorder: [P][cap], match of the ORIGINAL record arrays at each position
                               // of the reordered hot record (null: the hot record is in the original order)
    const float2 *frontRec;    // after ps_stage_reorder (reprojection metrics): [P][cap / 2][5] the matches ALL voters reject, two
                               // per record: (cur.x) (cur.y) (cur.z) (cx - uOld) (cy - vOld) of matches 2k | 2k + 1 -- the
                               // operands of the one-direction pre-test of stage 1 (null: no pre-test)
    int margin, c2div;         // reordered sweep: where stages 1 and 2 end (stage_range)
    unsigned long long *validMask; // stage 0 in two launches (models once, then the sweep split over many work-groups): [P][hCount/64]
    int genOnly;               // 1 = this launch only generates the models of [hBase, hBase + hCount), parks them and writes
                               // validMask; 0 with validMask set = this launch reads both back instead of generating
    int single;                // 1 = stage 1 sweeps ALL matches and is the only stage after the prefix (adaptive schedules
                               // without reordering: what their trip limit leaves is little, two more launches cost more)
    int gran;                  // the stage cuts are multiples of this (64: the Euclidean kernel recounts blocks of 64 matches;
                               // 8 for the reprojection kernels, which only need even cuts)
    int loopGroups;            // stage 1 of an adaptive schedule with a long cap (USAC's 850 000: 3320 blocks of 256 hypotheses per
                               // pair, of which the trip limit leaves a handful): this many work-groups per pair take the blocks
                               // bx, bx + loopGroups, ... and stop at the first block beyond the limit (0: one work-group per block)
    const int32_t *prefInfo;   // after ps_stage_reorder: [P][4] = (best count, trip limit) the prefix leaves, how many matches at
                               // the front of the reordered record ALL voters reject, reserved (null: every work-group of
                               // the stages replays the prefix itself)
};

// Replay of the sequential selection over counts[0 .. n) by one wavefront (the rule of ps_select_refit part (1)):
// best = the best count among the consumed ones, limit = the trip limit afterwards (a.H for the fixed schedule).
// bestIdx = the hypothesis that holds `best` (the first of equals), -1 without a record.
PS_D void wave_replay_prefix(const int32_t *__restrict__ cnts, int n, const SelectArgs &a, int M, int &best, int &limit,
                             int &bestIdx)
{
    const int lane = threadIdx.x & 63;
    bestIdx = -1;
    if (a.estimator == PS_EST_FIXED) {
        // (count, lowest index first) as one key: counts are <= PS_MAX_KPTS < 2^15, prefixes <= 2^16 hypotheses
        int b = 0;
        for (int i = lane; i < n; i += 64) b = max(b, (cnts[i] << 16) | (0xFFFF - i));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b = max(b, __shfl_xor(b, o, 64));
        best = b >> 16;
        if (best > 0) bestIdx = 0xFFFF - (b & 0xFFFF);
        limit = a.H;
        return;
    }
    int pos = 0;
    best = 0;
    limit = a.iter0;
    for (;;) {
        const int lim = limit < n ? limit : n;
        unsigned found = 0xFFFFFFFFu;
        for (int i = pos + lane; i < lim; i += 64)
            if (cnts[i] > best) {
                found = (unsigned)i;
                break;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)found, o, 64);
            found = other < found ? other : found;
        }
        if (found == 0xFFFFFFFFu) break;
        best = cnts[found];
        bestIdx = (int)found;
        pos = (int)found + 1;
        limit = a.estimator == PS_EST_USAC ? usac_limit(a, (unsigned)best, (unsigned)M)
                                           : ransac_limit(a, (float)best / (float)M); // ratio as RANSAC.cpp:280
    }
}

// Match range [lo, hi) of pruned stage st.stage (1 .. kStages) for a pair with M matches whose prefix reached best0
// (ps_score_plan.h: stage_range).
PS_D void stage_range(const StageArgs &st, int M, int best0, int &lo, int &hi)
{
    ::stage_range(StageCuts{st.perm != nullptr, st.single, st.gran, st.margin, st.c2div}, st.stage, M, best0, lo, hi);
}

// hypothesis of lane 0 of the calling lane's wavefront (h is consecutive over the lanes, or 0x7FFFFFFF for an idle lane
// of a survivor list: the wave's first lane then tells whether the whole wave is idle)
PS_D int hFirstOfWave(int h, int lane) { return __builtin_amdgcn_readfirstlane(h); }

// What every work-group of a pruned stage needs before it starts: the prefix's best count and trip limit (work-group
// uniform, in SGPRs) -- wave 0 replays, the others wait.
PS_D void stage_prefix(const int32_t *__restrict__ cnts, int nPrefix, const SelectArgs &sa, int M, int *s_pref, int &best0,
                       int &hLimit, const int32_t *__restrict__ prefInfo = nullptr)
{
    if (prefInfo != nullptr) { // replayed once per pair by ps_stage_reorder (scalar loads, no barrier)
        best0 = prefInfo[0];
        hLimit = best0 > 0 ? prefInfo[1] : sa.H;
        return;
    }
    if ((threadIdx.x >> 6) == 0) {
        int b, l, bi;
        wave_replay_prefix(cnts, nPrefix, sa, M, b, l, bi);
        if ((threadIdx.x & 63) == 0) {
            s_pref[0] = b;
            s_pref[1] = l;
        }
    }
    __syncthreads();
    // (LDS loads count as divergent for the compiler: readfirstlane keeps the values in SGPRs and the branches scalar)
    best0 = __builtin_amdgcn_readfirstlane(s_pref[0]);
    // the limit only shrinks from record to record, but the FIRST record may raise it above its initial value
    // (RANSAC.cpp:30 starts from computeRANSACIteration(0.20); a first ratio below 0.2 gives more): without a record in
    // the prefix nothing can be cut
    hLimit = best0 > 0 ? __builtin_amdgcn_readfirstlane(s_pref[1]) : sa.H;
}

// Appends the hypotheses of the lanes with `alive` to the next stage's list of pair p (one atomic per wavefront).
PS_D void stage_append(bool alive, int h, int32_t *__restrict__ listOut, int32_t *__restrict__ countOut, int p, int stride)
{
    const unsigned long long am = __builtin_amdgcn_ballot_w64(alive);
    if (am == 0ull) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == __builtin_ctzll(am)) base = atomicAdd(&countOut[p], __popcll(am));
    base = __builtin_amdgcn_readlane(base, __builtin_ctzll(am));
    if (alive) listOut[(size_t)p * stride + base + lanes_below(am)] = h;
}

// The hypothesis of a lane, derived AGAIN at the end of a staged launch from values that cost no vector register in between
// (the scalar work-group offset passes through an empty asm, so that the compiler cannot keep the first derivation -- or
// the 64-bit addresses built on it -- alive across the loops: with the vectorisers on, at seven waves per SIMD, it kept
// them in scratch memory; kept for the registers it still saves).
// base = first hypothesis (or list entry) of the work-group's pass, slot = the lane's place in it.
PS_D int stage_hypothesis_again(bool list, const StageArgs &st, int base, int slot, int p, int H)
{
    asm volatile("" : "+s"(base));
    if (!list) return st.hBase + base + slot;
    const int i = base + slot;
    return i < st.countIn[p] ? st.listIn[(size_t)p * st.listStride + i] : 0x7FFFFFFF;
}

// ------------------------------------------------------------------------------------------
// One pass of a work-group: the hypotheses [hBase + bx * 256, + 256) (kinds 0 / 1) or one pass over the survivor list (kind 2).
// KIND: what the launch scores (StageArgs).  0 = the hypotheses [hBase, hBase + hCount) completely -- the plain launch over
// [0, H) and stage 0 of the staged scoring; 1 = stage 1 (generates its models, first match range); 2 = stages 2+ (models and
// hypothesis list read back, a loop over the list).
// A family's pass is: pass_begin, its own rule for a wavefront without a hypothesis (wave_idle) and its early loads, pass_model,
// lds_put_model, its sweep of [m0, m1) into the lane's count, pass_finish.  Its LDS blocks s_mdl, s_tot and s_pref are its own
// declarations, handed in.
// ------------------------------------------------------------------------------------------
struct PassState {
    int tid, lane, wv;  // the thread, its lane and its wavefront (wv: scalar)
    int h, hEnd;        // this lane scores hypothesis h if h < hEnd
    int m0, m1;         // the matches it sweeps
    int mStageEnd;      // where the stage's range ends (m1 before it was split over work-groups and wavefronts)
    int best0;          // pruned stages: the best count the prefix reached
    ptrdiff_t prefRow;  // the pair's row of StageArgs::prefInfo, as an index derived ONCE for the frame and the family (the row's
                        // address kept across the sample -> SVD chain instead, or the index derived where it is used, cost stage 1 of
                        // the reprojection kernel six and seven more scalar registers spilled into vector lanes)
    int cover, slot, part; // kind 2: hypotheses per pass, the lane's place among them, its part of the match range
};

enum PassGo {
    kPassGo,      // sweep
    kPassNothing, // this pass has nothing to do (the pass returns false)
    kPassDone     // this block and every later one has nothing to do (the pass returns true, which ends the LOOP walk)
};

// (both of the exits are uniform over the work-group)
template <int KIND>
PS_D PassGo pass_begin(PassState &ps, const ModelArgs &ma, const SelectArgs &sa, const StageArgs &st, const int32_t *cout, int *s_tot,
                       int *s_pref, int msplit, const unsigned bx, const unsigned by, const int p, const int M)
{
    constexpr bool LIST = KIND == 2; // stage >= 2: hypotheses from the survivor list, models from HBM
    constexpr bool pruned = KIND >= 1;
    int tid = threadIdx.x;
    // (kind 2 calls this in a loop: without the empty asm the compiler computes everything that hangs on the thread index --
    // a dozen LDS row addresses -- once before the loop and, short of registers, keeps it in scratch memory, the inlier
    // counter of the hot loop with it)
    if (KIND == 2) asm volatile("" : "+v"(tid));
    ps.tid = tid;
    ps.lane = tid & 63;
    ps.wv = __builtin_amdgcn_readfirstlane(tid >> 6); // (wave-uniform by construction: keep it and what hangs on it scalar)
    ps.h = st.hBase + (int)bx * kBlock + tid;
    ps.hEnd = st.hBase + st.hCount;
    pair_split(M, by, msplit, ps.m0, ps.m1);
    ps.best0 = 0;
    ps.prefRow = 4 * p;
    ps.cover = kBlock, ps.slot = tid, ps.part = 0;
    ps.mStageEnd = ps.m1;
    if (LIST) {
        s_tot[tid] = 0;
        __syncthreads(); // (a part with a short range must not add into a slot another wavefront has yet to clear)
    }
    if (pruned) { // (msplit == 1 in these stages, but for the last one's split of its range)
        int hLimit;
        stage_prefix(cout, st.hBase, sa, M, s_pref, ps.best0, hLimit, // (stage >= 1: hBase = size of the prefix)
                     st.prefInfo != nullptr ? st.prefInfo + ps.prefRow : nullptr);
        stage_range(st, M, ps.best0, ps.m0, ps.m1);
        // a block with hypotheses that have no model slot (ModelArgs::modelH: long caps) is swept in one piece: nothing of it
        // is parked or listed
        {
            const int blockEnd = st.hBase + ((int)bx + 1) * kBlock;
            if (!LIST && ma.models != nullptr && (blockEnd < ps.hEnd ? blockEnd : ps.hEnd) > ma.modelH) ps.m1 = M;
        }
        ps.mStageEnd = ps.m1;
        if (ps.m0 >= ps.m1) return kPassDone; // an earlier stage finished the pair's matches
        if (!LIST) {
            ps.hEnd = ps.hEnd < hLimit ? ps.hEnd : hLimit; // beyond the trip limit: never consumed by the selection
            if (st.hBase + (int)bx * kBlock >= ps.hEnd) return kPassDone;
        } else {
            if (msplit > 1) { // the LAST stage may split its range over work-groups too: their counts meet in counts[]
                group_part(by, msplit, ps.m0, ps.m1);
                if (ps.m0 >= ps.m1) return kPassNothing;
            }
            const int n = st.countIn[p];
            ps.cover = list_cover(n);
            ps.part = __builtin_amdgcn_readfirstlane(tid / ps.cover);
            ps.slot = tid - ps.part * ps.cover;
            const int i = (int)bx * ps.cover + ps.slot;
            ps.hEnd = 0x7FFFFFFF;
            ps.h = i < n ? st.listIn[(size_t)p * st.listStride + i] : 0x7FFFFFFF; // (h >= hEnd: idle lane)
            wave_part(ps.part, ps.cover, ps.m0, ps.m1); // this wavefront's part of the stage's match range
        }
    }
    return kPassGo;
}

// A wavefront without a hypothesis of its own has nothing to sweep -- the 64-hypothesis prefix of the adaptive schedules fills
// one of the four; a pass with a split match range has no such wavefront.  (wave-uniform)
PS_D bool wave_idle(const PassState &ps) { return ps.cover == kBlock && hFirstOfWave(ps.h, ps.lane) >= ps.hEnd; }

// Where the model comes from: the survivor list (kind 2), stage 0's first launch (its second one reads models and validity back), or
// the sampler.  Ends with the lane's model in registers and `valid` set.  The models-only launch (KIND 0 with st.genOnly) has then
// parked its models and written validMask as well: its pass is over, the caller returns.
template <int KIND>
PS_D void pass_model(const PassState &ps, const float4 *recA, const float4 *recB, const size_t rbase,
                     const ModelArgs &ma, const StageArgs &st, int H, const unsigned bx, const unsigned by, const int p, const int M,
                     Rigid &mdl, bool &valid)
{
    constexpr bool LIST = KIND == 2;
    constexpr bool pruned = KIND >= 1;
    const int h = ps.h, hEnd = ps.hEnd;
    if (LIST) {
        if (h < hEnd) {
            load_model(ma, (size_t)p * ma.modelH + h, mdl); // parked by stage 1 (only valid samples survive it; h < modelH: a
                                                            // hypothesis beyond is swept completely by stage 1 and never listed)
            valid = true;
        }
    } else if (KIND == 0 && st.validMask != nullptr && !st.genOnly) {
        // stage 0, second launch: the models were generated once by the first (the sweep is split over msplit work-groups,
        // each of which would otherwise repeat the sample -> SVD chain: 63 % of stage 0's instructions with four parts)
        const unsigned long long vm = uniform64(st.validMask[(size_t)p * ((st.hCount + 63) >> 6) + (bx * (kBlock / 64) + ps.wv)]);
        valid = h < hEnd && lane_in(vm);
        if (h < hEnd) load_model(ma, (size_t)p * ma.modelH + h, mdl); // (launches of this form have a slot for every hypothesis)
    } else {
        if (h < hEnd) valid = gen_model(recA, recB, rbase, (uint32_t)M, ma, base_seed(ma) + (uint64_t)p, (uint32_t)h, mdl);
        // (stage 1 parks only the models of its survivors, at the end: the abandoned majority is never read again)
        if (ma.models && by == 0 && !pruned) {
            const int hs = stage_hypothesis_again(false, st, (int)bx * kBlock, ps.tid, p, H);
            if (hs < hEnd && hs < ma.modelH) store_model(ma, (size_t)p * ma.modelH + hs, mdl);
        }
        if (KIND == 0 && st.genOnly) { // stage 0, first launch: models and validity only
            const unsigned long long vm = __builtin_amdgcn_ballot_w64(valid);
            if (ps.lane == 0) st.validMask[(size_t)p * ((st.hCount + 63) >> 6) + (bx * (kBlock / 64) + ps.wv)] = vm;
        }
    }
}

// The end of a pass: cnt = what the lane counted over [m0, m1).  The parts of a split range meet; the count goes to counts[]; in a
// pruned stage the hypotheses that can still become records are listed for the next one and stage 1's survivors park their models.
template <int KIND>
PS_D void pass_finish(const PassState &ps, const LdsModels &s_mdl, int *s_tot, int32_t *cout, const ModelArgs &ma,
                      const StageArgs &st, int H, int msplit, const unsigned bx, const int p, const int M, bool valid, int cnt)
{
    constexpr bool LIST = KIND == 2;
    constexpr bool pruned = KIND >= 1;
    const int hEnd = ps.hEnd, cover = ps.cover, slot = ps.slot, part = ps.part, mStageEnd = ps.mStageEnd;
    int h = ps.h;
    int tidE = ps.tid; // (a fresh copy for the epilogue's LDS addresses: kept alive across the loops they went to scratch memory)
    asm volatile("" : "+v"(tidE));
    if (LIST && cover < kBlock) { // (work-group uniform) the parts of the match range add up
        if (part > 0 && h < hEnd) atomicAdd(&s_tot[slot], cnt);
        __syncthreads();
        if (part == 0) cnt += s_tot[slot];
    }
    if (pruned) {
        h = stage_hypothesis_again(LIST, st, (int)bx * cover, slot, p, H);
        const bool mine = h < hEnd && part == 0;
        if (LIST && msplit > 1) { // (last stage, range split over work-groups: nothing survives it, the counts add up)
            if (mine && valid && cnt) atomicAdd(&cout[h], cnt);
            return;
        }
        const int cnt0 = (LIST && mine) ? cout[h] : 0; // count so far
        const int total = valid ? cnt0 + cnt : 0; // model not computed -> iteration skipped (RANSAC.cpp:107)
        if (mine) cout[h] = total;
        // still able to become a record?  (count so far + matches left > best count of the earlier hypotheses)
        const bool alive = mine && valid && total + (M - mStageEnd) > ps.best0;
        if (!LIST && ma.models && h < ma.modelH && (alive || (mine && mStageEnd >= M))) { // survivors (or: this stage was the whole sweep)
            Rigid md;
            lds_get_model(s_mdl, tidE, md);
            store_model(ma, (size_t)p * ma.modelH + h, md);
        }
        if (st.stage < kStages && mStageEnd < M) stage_append(alive, h, st.listOut, st.countOut, p, st.listStride);
        return;
    }
    h = stage_hypothesis_again(false, st, (int)bx * kBlock, ps.tid, p, H);
    if (h < hEnd) {
        if (!valid) cnt = 0; // model not computed -> iteration skipped (RANSAC.cpp:107)
        if (msplit == 1)
            cout[h] = cnt;
        else if (cnt)
            atomicAdd(&cout[h], cnt);
    }
}

// The body of a scoring kernel: which pass(es) this work-group takes.  pass(bx, by, p, M) is one pass of the family; it returns true
// when its block, and with it every later one, has nothing to do (uniform over the work-group).
// hypotheses of a launch: [hBase, hBase + hCount) (plain launch: [0, H); stages 0 / 1), or a survivor list swept by
// hCount / 256 work-groups per pair (stages 2+)
// LOOP (kind 1 only): StageArgs::loopGroups work-groups per pair walk the blocks of 256 hypotheses and stop at the first one beyond
// the trip limit.
template <int KIND, bool LOOP, class Pass>
PS_D void score_kernel_body(const int32_t *mvalid, const StageArgs &st, int minRun, int msplit, const Pass &pass)
{
    static_assert(!LOOP || KIND == 1, "the looping form is stage 1's");
    const unsigned blocks = (unsigned)((st.hCount + kBlock - 1) / kBlock);
    const unsigned hb = LOOP ? (unsigned)st.loopGroups : blocks; // work-groups per pair and part of the match range
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned bx = L % hb, by = (L / hb) % (unsigned)msplit;
    const int p = (int)(L / (hb * (unsigned)msplit));
    const int M = mvalid[p];
    if (M < minRun) return; // too few matches: kernel 4 returns identity (RANSAC.cpp:77-80)
    if (LOOP) {
        for (unsigned b = bx; b < blocks; b += hb) {
            if (b != bx) __syncthreads(); // (the pass before is done with the work-group's LDS)
            if (pass(b, by, p, M)) break; // (uniform over the work-group: the exits that return true are taken by all of its waves)
        }
    } else if (KIND == 2) {
        const int n = st.countIn[p];
        const int cover = list_cover(n);
        for (unsigned b = bx; (int)b * cover < n; b += hb) {
            if (b != bx) __syncthreads(); // (the pass before is done with the work-group's LDS)
            pass(b, by, p, M);
        }
    } else
        pass(bx, by, p, M);
}

} // namespace psdev
