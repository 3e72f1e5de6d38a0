// The scoring plan (putslam_amd/csrc/ps_score_plan.h) in a plain C++ program, no HIP and no GPU; tests/test_score_plan_host.py builds
// and runs it.
//   test_score_plan          the "nothing to gain" policy's state machine (BailTracker) held to the rule as PsContext documents it
//                            (ps_internal.h); prints what fails and returns 1, else "score plan ok"
//   test_score_plan plan     stdin: one input tuple per line (tests/score_plan_rows.py: INPUT_FIELDS); stdout: per line everything
//                            wants_staged, decide_score and stage_schedule decide for it
//   test_score_plan staged   stdin: "family estimator H cap P side_by_side" per line; stdout: wants_staged, 0 or 1
//   test_score_plan ranges   the match ranges of kernel 3's work-groups and wavefronts (pair_split, stage_range, group_part, wave_part):
//                            they tile what they split, and they are what the device code computed before the arithmetic moved into
//                            the header; prints what fails and returns 1, else "match ranges ok"
#include <cstdio>
#include <cstring>
#include <vector>

#include "ps_score_plan.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s does not hold\n", __LINE__, #cond);      \
            ++failures;                                                  \
        }                                                                \
    } while (0)

BailKey kind(int H)
{
    BailKey k;
    k.mode = PS_EUCLIDEAN_ERROR; k.estimator = PS_EST_FIXED; k.H = H; k.pclass = 7; k.cap = 2000;
    return k;
}

// A call of kind `k` as prepare_score makes it: the slot, the counters as the host reads them (cnt[slot]), the veto.
struct Host {
    BailTracker t;
    unsigned cnt[BailTracker::kKinds][2] = {};
    bool recycled = false;
    int slot = -1, hopeless = -1;
    bool call(const BailKey &k)
    {
        slot = t.find(k, recycled);
        if (recycled) t.adopt(slot, cnt[slot][0], cnt[slot][1]);
        hopeless = t.observe(slot, cnt[slot][0], cnt[slot][1]);
        return t.veto(slot);
    }
    // an observation lands in the slot: `pairs` replayed, `nothing` of them with nothing to gain
    void land(int s, unsigned pairs, unsigned nothing)
    {
        cnt[s][0] += pairs;
        cnt[s][1] += nothing;
    }
};

void test_bail_tracker()
{
    const BailKey A = kind(4096), B = kind(8192);
    {
        Host h;
        CHECK(!h.call(A) && h.recycled && h.hopeless == 0); // a new kind starts from "staged"
        const int a = h.slot;
        CHECK(!h.call(A) && !h.recycled && h.slot == a && h.hopeless == 0); // no new observation changes nothing
        h.land(a, 100, 50);                                 // 2 * d1 > d0 does not hold: half the pairs is not "most"
        CHECK(!h.call(A) && h.hopeless == 0);
        h.land(a, 100, 51);
        // while hopeless, calls 1 .. 15 are vetoed and the 16th is not -- and so on
        for (int round = 0; round < 2; ++round)
            for (int i = 1; i <= 16; ++i) {
                const bool veto = h.call(A);
                CHECK(h.hopeless == 1 && veto == (i != 16));
            }
        // no new observation changes nothing: the count goes on (three calls into the next sixteen, two observations of the same say)
        for (int i = 1; i <= 3; ++i) CHECK(h.call(A));
        h.land(a, 10, 10);
        for (int i = 4; i <= 16; ++i) CHECK(h.call(A) == (i != 16) && h.hopeless == 1);
        // an observation without 2 * d1 > d0 clears it: nothing is vetoed
        for (int i = 1; i <= 5; ++i) CHECK(h.call(A));
        h.land(a, 100, 3);
        for (int i = 0; i < 40; ++i) CHECK(!h.call(A) && h.hopeless == 0);
        // a flip restarts the count: hopeless again, fifteen vetoes from the first call on whatever was counted before
        h.land(a, 7, 4);
        for (int i = 1; i <= 16; ++i) CHECK(h.call(A) == (i != 16) && h.hopeless == 1);
        for (int i = 1; i <= 9; ++i) CHECK(h.call(A));
        h.land(a, 8, 4); // good
        CHECK(!h.call(A) && h.hopeless == 0);
        h.land(a, 8, 5); // bad: the nine calls above are forgotten
        for (int i = 1; i <= 16; ++i) CHECK(h.call(A) == (i != 16));
        // the counters wrap (they are unsigned and monotonic): differences still hold
        Host w;
        w.call(A);
        w.cnt[w.slot][0] = 0xFFFFFFF0u;
        w.cnt[w.slot][1] = 0xFFFFFFF8u;
        w.t.adopt(w.slot, w.cnt[w.slot][0], w.cnt[w.slot][1]);
        w.land(w.slot, 0x20, 0x11);
        CHECK(w.call(A) && w.hopeless == 1 && w.cnt[w.slot][0] == 0x10u);
        w.land(w.slot, 0x20, 0x10);
        CHECK(!w.call(A) && w.hopeless == 0);
    }
    { // two kinds that alternate keep independent states
        Host h;
        h.call(A);
        const int a = h.slot;
        h.call(B);
        const int b = h.slot;
        CHECK(a != b && h.recycled);
        h.land(a, 64, 64); // A: hopeless data; B: good data
        h.land(b, 64, 0);
        for (int i = 1; i <= 32; ++i) {
            CHECK(h.call(A) == ((i & 15) != 0) && h.slot == a && h.hopeless == 1 && !h.recycled);
            CHECK(!h.call(B) && h.slot == b && h.hopeless == 0 && !h.recycled);
        }
    }
    { // a ninth kind recycles the least recently used slot, reports the recycle and starts not hopeless
        Host h;
        int slotOf[BailTracker::kKinds];
        for (int i = 0; i < BailTracker::kKinds; ++i) {
            CHECK(!h.call(kind(1000 + i)) && h.recycled);
            slotOf[i] = h.slot;
            for (int j = 0; j < i; ++j) CHECK(slotOf[j] != slotOf[i]);
            h.land(h.slot, 10, 10); // every kind sees hopeless data
        }
        for (int i = BailTracker::kKinds - 1; i >= 0; --i) CHECK(h.call(kind(1000 + i)) && !h.recycled && h.slot == slotOf[i]); // kind 7 is now the oldest
        h.land(slotOf[7], 5, 5);  // (lands after kind 7's last call: the ninth kind must not take it for its own)
        CHECK(!h.call(kind(2000)) && h.recycled && h.slot == slotOf[7] && h.hopeless == 0);
        for (int i = 0; i < 20; ++i) CHECK(!h.call(kind(2000)) && !h.recycled && h.hopeless == 0);
        for (int i = 0; i < 7; ++i) CHECK(h.call(kind(1000 + i)) && !h.recycled && h.hopeless == 1); // the others keep their state
        CHECK(!h.call(kind(1007)) && h.recycled && h.slot == slotOf[7] && h.hopeless == 0); // kind 7 is new again: the ninth kind's slot is the oldest now
        // reset() forgets everything
        h.t.reset();
        for (int i = 0; i < BailTracker::kKinds; ++i) CHECK(!h.call(kind(1000 + i)) && h.recycled && h.hopeless == 0);
    }
}

// ---- the match ranges ----
// The expressions of ps_score_fast.h / ps_score_euclid.h at the commit before the arithmetic moved into ps_score_plan.h, restated.
namespace parent {
void pair_split(int M, unsigned by, int msplit, int &m0, int &m1)
{
    const int npair = (M + 1) >> 1;
    m0 = 2 * (int)(((long long)npair * by) / msplit);
    m1 = 2 * (int)(((long long)npair * (by + 1)) / msplit);
    m1 = m1 < M ? m1 : M;
}
void stage_range(int stage, bool reordered, int single, int gran, int margin, int c2div, int M, int best0, int &lo, int &hi)
{
    int c1 = M, c2 = M;
    if (best0 > 0 && !single) {
        const int miss = M - best0;
        if (reordered) {
            const int g1 = gran - 1;
            c1 = (miss + margin + g1) & ~g1;
            if (c1 >= M - M / 8) c1 = M;
            if (c1 < M) {
                const int c64 = (c1 + 63) & ~63;
                const int step = ((M - c64) / c2div + 63) & ~63;
                c2 = c64 + (step > 0 ? step : 64);
                if (c2 >= M - M / 16) c2 = M;
            }
        } else {
            c1 = (miss + miss / 7 + 32 + 63) & ~63;
            if (c1 >= M - M / 8) c1 = M;
            if (c1 < M) {
                c2 = (c1 + (M - c1) / 2 + 63) & ~63;
                if (c2 >= M - M / 16) c2 = M;
            }
        }
    }
    lo = stage == 1 ? 0 : (stage == 2 ? c1 : c2);
    hi = stage == 1 ? c1 : (stage == 2 ? c2 : M);
}
void group_part(unsigned by, int msplit, int &m0, int &m1)
{
    const int blen = (((m1 - m0 + msplit - 1) / msplit) + 63) & ~63;
    m0 += (int)by * blen;
    m1 = m1 < m0 + blen ? m1 : m0 + blen;
}
void wave_part(int part, int cover, int &m0, int &m1)
{
    const int parts = 256 / cover;
    const int plen = ((m1 - m0 + parts * 64 - 1) / (parts * 64)) * 64;
    m0 += part * plen;
    m1 = m1 < m0 + plen ? m1 : m0 + plen;
    m1 = m1 < m0 ? m0 : m1;
}
int list_cover(int n) { return n <= 64 ? 64 : (n <= 128 ? 128 : 256); }
} // namespace parent

// Kinds 0 / 1: the msplit parts tile [0, M), and every part but the last is even (the loops take two matches per trip).
void check_pair_split(int M, int msplit)
{
    int next = 0;
    for (int by = 0; by < msplit; ++by) {
        int m0, m1, q0, q1;
        pair_split(M, (unsigned)by, msplit, m0, m1);
        parent::pair_split(M, (unsigned)by, msplit, q0, q1);
        CHECK(m0 == q0 && m1 == q1);
        CHECK(m0 == next && m0 <= m1 && m1 <= M);
        CHECK(by == msplit - 1 || ((m1 - m0) & 1) == 0);
        next = m1;
    }
    CHECK(next == M);
}

// A stage's range [lo, hi) as the last stage's work-groups (msplit3 of them) and, within each, the kPlanBlock / cover groups of
// wavefronts take it: in the order (work-group, wave part) the parts follow one another from lo to hi -- pairwise disjoint, their
// union the range --, each starts on a multiple of 64 from lo, and only the last one that is not empty can be odd.
void check_parts(int lo, int hi)
{
    const int msplits[2] = {1, kListRsplit3}, covers[3] = {64, 128, kPlanBlock};
    for (int msplit3 : msplits)
        for (int cover : covers) {
            int next = lo, lastOdd = 0;
            for (int by = 0; by < msplit3; ++by) {
                int g0 = lo, g1 = hi, r0 = lo, r1 = hi;
                if (msplit3 > 1) { // (pass_begin: a work-group whose part is empty leaves)
                    group_part((unsigned)by, msplit3, g0, g1);
                    parent::group_part((unsigned)by, msplit3, r0, r1);
                    CHECK(g0 == r0 && g1 == r1);
                    if (g0 >= g1) continue;
                    CHECK(g0 == next && (g0 - lo) % 64 == 0);
                }
                for (int part = 0; part < kPlanBlock / cover; ++part) {
                    int w0 = g0, w1 = g1, q0 = g0, q1 = g1;
                    wave_part(part, cover, w0, w1);
                    parent::wave_part(part, cover, q0, q1);
                    CHECK(w0 == q0 && w1 == q1);
                    CHECK(w0 <= w1 && (w0 - lo) % 64 == 0);
                    if (w0 == w1) continue;
                    CHECK(w0 == next && w1 <= g1 && lastOdd == 0);
                    lastOdd = (w1 - w0) & 1;
                    next = w1;
                }
                CHECK(next == g1);
            }
            CHECK(next == hi);
        }
}

// Stages 1, 2, 3 tile [0, M); every stage range is split as check_parts says.  `seen`: ranges already split ((maxM + 1)^2 flags, or null).
void check_stages(int M, int best0, std::vector<char> *seen, int maxM)
{
    const int grans[2] = {8, 64};
    for (int reordered = 0; reordered < 2; ++reordered)
        for (int single = 0; single < 2; ++single)
            for (int gran : grans) {
                const StageCuts sc{reordered != 0, single, gran, ScoreOptions().reorderMargin, kReorderC2div};
                int next = 0;
                for (int stage = 1; stage <= kPlanStages; ++stage) {
                    int lo, hi, q0, q1;
                    stage_range(sc, stage, M, best0, lo, hi);
                    parent::stage_range(stage, reordered != 0, single, gran, sc.margin, sc.c2div, M, best0, q0, q1);
                    CHECK(lo == q0 && hi == q1);
                    CHECK(lo == next && lo <= hi && hi <= M);
                    next = hi;
                    if (seen != nullptr) {
                        char &flag = (*seen)[(size_t)lo * (maxM + 1) + hi];
                        if (flag) continue;
                        flag = 1;
                    }
                    check_parts(lo, hi);
                }
                CHECK(next == M);
            }
}

int run_ranges()
{
    const int maxM = 600;
    std::vector<char> seen((size_t)(maxM + 1) * (maxM + 1), 0);
    for (int M = 0; M <= maxM; ++M) {
        for (int msplit = 1; msplit <= 32; ++msplit) check_pair_split(M, msplit);
        for (int best0 = 0; best0 <= M; ++best0) check_stages(M, best0, &seen, maxM);
    }
    for (int msplit = 1; msplit <= 32; ++msplit) check_pair_split(PS_MAX_KPTS, msplit);
    for (int best0 = 0; best0 <= PS_MAX_KPTS; ++best0) check_stages(PS_MAX_KPTS, best0, nullptr, 0);
    for (int n = 0; n <= 2 * kPlanBlock; ++n) CHECK(list_cover(n) == parent::list_cover(n) && kPlanBlock % list_cover(n) == 0);
    // sizes between the two, drawn from a fixed seed
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    auto draw = [&](int n) { // 0 .. n - 1
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((x >> 33) % (unsigned long long)n);
    };
    for (int i = 0; i < 20000; ++i) {
        const int M = maxM + 1 + draw(PS_MAX_KPTS - maxM);
        check_pair_split(M, 1 + draw(32));
        check_stages(M, draw(M + 1), nullptr, 0);
    }
    if (failures) return 1;
    printf("match ranges ok\n");
    return 0;
}

int run_plan()
{
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        int family, sbs, prune, reorder, gensplit, singlerest, pretest, prefix, msplit, listg2, room, complete, adaptive, veto;
        ScoreShape s;
        if (sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &family, &s.mode, &s.estimator, &s.P, &s.cap, &s.H, &sbs, &prune,
                   &reorder, &gensplit, &singlerest, &pretest, &prefix, &msplit, &listg2, &room, &complete, &adaptive, &veto) != 19) {
            fprintf(stderr, "bad input line: %s", line);
            return 1;
        }
        s.score = family == 0 ? Scoring::Value : family == 1 ? Scoring::Euclid : Scoring::Reproj;
        s.complete = complete != 0;
        s.adaptive = adaptive != 0;
        ScoreOptions o;
        o.prune = prune; o.sideBySide = sbs; o.reorder = reorder; o.genSplit = gensplit; o.singleRest = singlerest; o.pretest = pretest;
        o.forcePrefix = prefix; o.forceMsplit = msplit; o.listGroups2 = listg2; o.modelRoomMiB = room;
        const bool wants = wants_staged(s, o), staged = wants && !veto;
        const ScoreDecision d = decide_score(s, o, staged);
        printf("%d %d %d", wants, staged, d.status);
        if (d.status != PS_OK) {
            printf("\n");
            continue;
        }
        printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d", d.msplit, d.genSplit, d.genPlain, d.reorder, d.prefix, d.lastStage, d.big0, d.modelH,
               d.parkModels, d.skipE, d.skipF, d.zeroCounts, d.zeroH);
        const ScoreBlock blocks[] = {kBlkCounts, kBlkModels, kBlkValidMask, kBlkSurvA, kBlkSurvB, kBlkSurvN, kBlkRecF2, kBlkPermBuf, kBlkPrefInfo, kBlkFrontRec};
        for (ScoreBlock b : blocks) printf(" %zu", d.bytes[b]);
        StageSchedule sch; // (the value-exact kernel is one launch without StageArgs: no schedule)
        if (s.score != Scoring::Value) sch = stage_schedule(s, o, d);
        printf(" %d %d %d", sch.n, sch.reorderBefore, sch.pretest);
        for (int i = 0; i < sch.n; ++i) {
            const StageLaunch &l = sch.launch[i];
            printf(" %d %d %d %d %d %d %u %d %d %d %d %d %d %d %d", l.kind, l.loop, l.stage, l.genOnly, l.hBase, l.hCount, l.groups, l.msplit, l.validMask,
                   l.perm, l.frontRec, l.listIn, l.listOut, l.single, l.loopGroups);
        }
        printf("\n");
    }
    return 0;
}

int run_staged()
{
    int family, sbs;
    ScoreShape s;
    ScoreOptions o;
    while (scanf("%d %d %d %d %d %d", &family, &s.estimator, &s.H, &s.cap, &s.P, &sbs) == 6) {
        s.score = family == 0 ? Scoring::Value : family == 1 ? Scoring::Euclid : Scoring::Reproj;
        o.sideBySide = sbs;
        printf("%d\n", wants_staged(s, o) ? 1 : 0);
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "plan") == 0) return run_plan();
    if (argc > 1 && strcmp(argv[1], "staged") == 0) return run_staged();
    if (argc > 1 && strcmp(argv[1], "ranges") == 0) return run_ranges();
    test_bail_tracker();
    if (failures) return 1;
    printf("score plan ok\n");
    return 0;
}
