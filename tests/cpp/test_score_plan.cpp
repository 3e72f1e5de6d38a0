// The scoring plan (putslam_amd/csrc/ps_score_plan.h) in a plain C++ program, no HIP and no GPU; tests/test_score_plan_host.py builds
// and runs it.
//   test_score_plan          the "nothing to gain" policy's state machine (BailTracker) held to the rule as PsContext documents it
//                            (ps_internal.h); prints what fails and returns 1, else "score plan ok"
//   test_score_plan plan     stdin: one input tuple per line (tests/score_plan_rows.py: INPUT_FIELDS); stdout: per line everything
//                            wants_staged, decide_score and stage_schedule decide for it
//   test_score_plan staged   stdin: "family estimator H cap P side_by_side" per line; stdout: wants_staged, 0 or 1
#include <cstdio>
#include <cstring>

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
    test_bail_tracker();
    if (failures) return 1;
    printf("score plan ok\n");
    return 0;
}
