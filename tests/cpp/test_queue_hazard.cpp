// PsBatchQueue's hazard rule (putslam_amd/csrc/ps_queue_hazard.h) in a plain C++ program, no HIP and no GPU: EVERY sequence of
//     submit a whole batch on block b | submit a split batch on block b | complete the oldest unfinished share of chain c
// up to a fixed length, for 1 .. 4 chains and up to 3 blocks, is run through the rule, and after every submit a checker that shares
// nothing with the rule -- a direct scan over all batches ever submitted -- holds the plan to the queue's promises:
//   (a) safety: every earlier share that writes the block, is not complete and intersects a new share's rows runs on that share's
//       chain or is waited for by it (its event, or a later one of the same chain: a chain completes in order);
//   (b) no needless coupling: every wait names such a share, and when all of them sit on one chain the batch follows them there
//       and no wait is queued at all;
//   (c) no needless serialising: a block with no writer in flight gets the nominal bounds.
// The program completes shares itself and only in the order a GPU could: first in, first out per chain, and a share that waits
// for another chain's event not before that event.  Then the ring: more than 64 tickets with blocks reused across the wrap, as a
// long random walk, and the recommended use (a block per chain, in turn) with its cost in events asked.  Last, the rule the queue
// had before (one remembered block per chain), to show that the checker can fail: it must be rejected first at "A x chains, B, A",
// the shortest sequence that made a batch run beside its predecessors.
// Prints what fails and returns 1; tests/test_queue_hazard_host.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ps_queue_hazard.h"

namespace {

constexpr int kRing = 64; // ps_batch_queue.cpp's kTickets

struct Wait {
    int batch, chain, waiter; // chain `waiter` of this batch waits for the event of `chain` of batch `batch`
};

struct Batch {
    int block = 0;
    bool split = false;
    int P = 0;
    int32_t bounds[kQueueMaxChains + 1] = {};
    bool done[kQueueMaxChains] = {}; // (a share of no pairs counts as done)
    std::vector<Wait> waits;
};

char blockKeys[8];

struct World {
    int chains = 0, wholeP = 0, splitP = 0;
    std::vector<Batch> hist; // everything ever submitted: what the checker scans
    std::string trace;       // the operations so far, for the failure text

    bool nonempty(const Batch &b, int c) const { return b.bounds[c + 1] > b.bounds[c]; }
    bool inflight(const Batch &b, int c) const { return nonempty(b, c) && !b.done[c]; }

    // the oldest unfinished share of chain c, if the GPU could finish it now: -1 when there is none or it still waits
    int completable(int c) const
    {
        for (size_t m = 0; m < hist.size(); ++m) {
            if (!inflight(hist[m], c)) continue;
            for (const Wait &w : hist[m].waits)
                if (w.waiter == c && !hist[w.batch].done[w.chain]) return -1;
            return (int)m;
        }
        return -1;
    }
};

// ---- the rule under test, driven the way ps_batch_queue_submit drives it: a ring of records, ages, the slot being reused left out
struct NewRule {
    struct Slot {
        long long seq = -1;
        QueueBatchRecord rec;
    };
    Slot ring[kRing];
    long long asked = 0;

    void plan(const World &w, int block, int P, bool split, Batch &out)
    {
        const int C = w.chains;
        const long long seq = (long long)w.hist.size();
        int32_t nominal[kQueueMaxChains + 1];
        queue_nominal_bounds(C, P, seq, split ? 0 : 0x7fffffff, 450, nominal);
        QueuePlan p;
        const int older = (int)(seq < kRing - 1 ? seq : kRing - 1);
        queue_hazard_plan(
            C, nominal, (const void *)&blockKeys[block], older,
            [&](int age) -> const QueueBatchRecord * {
                const Slot &s = ring[(seq - age) % kRing];
                return s.seq == seq - age ? &s.rec : nullptr;
            },
            [&](int age, int chain) {
                ++asked;
                const Batch &b = w.hist[(size_t)(seq - age)];
                if (!w.nonempty(b, chain)) {
                    std::printf("the rule asked for an event that was never recorded: %s\n", w.trace.c_str());
                    std::exit(1);
                }
                return (bool)b.done[chain];
            },
            p);
        for (int i = 0; i <= C; ++i) out.bounds[i] = p.bounds[i];
        for (int i = 0; i < p.nwaits; ++i) out.waits.push_back(Wait{(int)(seq - p.waits[i].age), p.waits[i].chain, p.waits[i].waiter});
        Slot &s = ring[seq % kRing];
        s.seq = seq;
        s.rec.block = (const void *)&blockKeys[block];
        for (int i = 0; i <= C; ++i) s.rec.bounds[i] = p.bounds[i];
        for (int i = 0; i < kQueueMaxChains; ++i) s.rec.used[i] = i < C && p.bounds[i + 1] > p.bounds[i];
    }
    void undo(const World &w) { ring[w.hist.size() % kRing].seq = -1; } // (the walks that undo never wrap)
};

// ---- the rule the queue had before: the block and the number of the last whole batch per chain; split batches are not looked at
struct OldRule {
    int lastOut[kQueueMaxChains];
    long long lastSeq[kQueueMaxChains];
    struct Saved {
        int out[kQueueMaxChains];
        long long seq[kQueueMaxChains];
    };
    std::vector<Saved> saved;
    OldRule()
    {
        for (int i = 0; i < kQueueMaxChains; ++i) lastOut[i] = -1, lastSeq[i] = -1;
    }
    void plan(const World &w, int block, int P, bool split, Batch &out)
    {
        Saved sv;
        for (int i = 0; i < kQueueMaxChains; ++i) sv.out[i] = lastOut[i], sv.seq[i] = lastSeq[i];
        saved.push_back(sv);
        const int C = w.chains;
        const long long seq = (long long)w.hist.size();
        queue_nominal_bounds(C, P, seq, split ? 0 : 0x7fffffff, 450, out.bounds);
        if (C < 2 || split) return;
        int mine = (int)(seq % C);
        for (int j = 0; j < C; ++j) {
            if (j == mine || lastOut[j] != block || lastSeq[j] < 0) continue;
            if (!w.hist[(size_t)lastSeq[j]].done[j]) {
                queue_whole_on(C, j, P, out.bounds);
                mine = j;
                break;
            }
        }
        lastOut[mine] = block;
        lastSeq[mine] = seq;
    }
    void undo(const World &)
    {
        for (int i = 0; i < kQueueMaxChains; ++i) lastOut[i] = saved.back().out[i], lastSeq[i] = saved.back().seq[i];
        saved.pop_back();
    }
};

// ---- the checker: the new batch is w.hist.back().  Returns what is wrong, or nullptr.
const char *check(const World &w)
{
    const int C = w.chains;
    const int n = (int)w.hist.size() - 1;
    const Batch &nb = w.hist[(size_t)n];
    const int P = nb.P;
    // the nominal bounds, written out again
    int32_t nominal[kQueueMaxChains + 1] = {};
    for (int i = 0; i <= C; ++i) {
        if (C == 1) nominal[i] = i ? P : 0;
        else if (!nb.split) nominal[i] = i <= n % C ? 0 : P;
        else if (C == 2) nominal[i] = i == 0 ? 0 : i == 1 ? P * 450 / 1000 : P;
        else nominal[i] = (int32_t)((long long)P * i / C);
    }
    // the bounds cover [0, P) in order; they are the nominal ones or the whole batch on one chain
    if (nb.bounds[0] != 0 || nb.bounds[C] != P) return "bounds do not cover the batch";
    int shares = 0;
    bool isNominal = true;
    for (int i = 0; i < C; ++i) {
        if (nb.bounds[i + 1] < nb.bounds[i]) return "bounds not ascending";
        shares += nb.bounds[i + 1] > nb.bounds[i];
        isNominal = isNominal && nb.bounds[i + 1] == nominal[i + 1];
    }
    if (!isNominal && shares != 1) return "neither the nominal bounds nor whole on one chain";
    if (!nb.split && shares != 1) return "a whole batch was split";

    auto intersects = [](int32_t alo, int32_t ahi, int32_t blo, int32_t bhi) { return alo < bhi && blo < ahi && alo < ahi && blo < bhi; };
    // every wait names a share of an earlier batch on this block, in flight, on another chain, whose rows meet the waiter's
    for (const Wait &x : nb.waits) {
        if (x.batch < 0 || x.batch >= n || x.chain < 0 || x.chain >= C || x.waiter < 0 || x.waiter >= C) return "(b) a wait out of range";
        const Batch &e = w.hist[(size_t)x.batch];
        if (n - x.batch >= kRing) return "(b) a wait for a ticket that left the ring";
        if (e.block != nb.block) return "(b) a wait for another block's batch";
        if (x.chain == x.waiter) return "(b) a chain waits for itself";
        if (!w.inflight(e, x.chain)) return "(b) a wait for a complete share";
        if (!intersects(e.bounds[x.chain], e.bounds[x.chain + 1], nb.bounds[x.waiter], nb.bounds[x.waiter + 1])) return "(b) a wait for rows the waiter does not write";
    }
    // (a), and on the way the chains that hold a writer in flight whose rows meet the batch's
    bool writerOn[kQueueMaxChains] = {};
    int writers = 0, writerChain = -1;
    for (int m = 0; m < n; ++m) {
        const Batch &e = w.hist[(size_t)m];
        if (e.block != nb.block) continue;
        for (int c = 0; c < C; ++c) {
            if (!w.inflight(e, c) || !intersects(e.bounds[c], e.bounds[c + 1], 0, P)) continue;
            if (!writerOn[c]) writerOn[c] = true, ++writers, writerChain = c;
            for (int i = 0; i < C; ++i) {
                if (i == c || !intersects(e.bounds[c], e.bounds[c + 1], nb.bounds[i], nb.bounds[i + 1])) continue;
                bool ordered = false;
                for (const Wait &x : nb.waits) ordered = ordered || (x.waiter == i && x.chain == c && x.batch >= m);
                if (!ordered) return "(a) a share runs beside an earlier writer of its rows";
            }
        }
    }
    if (writers == 0 && (!isNominal || !nb.waits.empty())) return "(c) no writer in flight, but not the nominal bounds";
    if (writers == 1) {
        if (!nb.waits.empty()) return "(b) all writers on one chain, but a wait was queued";
        if (!nb.split && nb.bounds[writerChain + 1] - nb.bounds[writerChain] != P) return "(b) all writers on one chain, but the batch did not follow them";
    }
    return nullptr;
}

struct Result {
    long long sequences = 0, submits = 0;
    int failedAt = 0; // length of the first sequence the checker rejected (0: none)
    std::string first, why;
};

template <class Rule> struct Walk {
    World w;
    Rule rule;
    int blocks = 0, maxLen = 0;
    bool splits = true, stopAtFailure = false;
    Result r;

    bool submit(int block, bool split) // false: the checker rejected the plan
    {
        Batch b;
        b.block = block;
        b.split = split;
        b.P = split ? w.splitP : w.wholeP;
        rule.plan(w, block, b.P, split, b);
        for (int c = 0; c < kQueueMaxChains; ++c) b.done[c] = !(c < w.chains && b.bounds[c + 1] > b.bounds[c]);
        w.hist.push_back(b);
        ++r.submits;
        const char *bad = check(w);
        if (bad && !r.failedAt) {
            r.failedAt = (int)w.trace.size();
            r.first = w.trace;
            r.why = bad;
        }
        return !bad;
    }

    void go(int len)
    {
        ++r.sequences;
        if (len == maxLen || (stopAtFailure && r.failedAt)) return;
        for (int b = 0; b < blocks; ++b)
            for (int s = 0; s < (splits ? 2 : 1); ++s) {
                w.trace.push_back((char)((s ? 'a' : 'A') + b));
                if (submit(b, s != 0)) go(len + 1); // (what follows a rejected plan proves nothing)
                w.hist.pop_back();
                rule.undo(w);
                w.trace.pop_back();
            }
        for (int c = 0; c < w.chains; ++c) {
            const int m = w.completable(c);
            if (m < 0) continue;
            w.hist[(size_t)m].done[c] = true;
            w.trace.push_back((char)('0' + c));
            go(len + 1);
            w.trace.pop_back();
            w.hist[(size_t)m].done[c] = false;
        }
    }
};

int failures = 0;

void exhaustive(int chains, int blocks, int maxLen, int wholeP, int splitP)
{
    Walk<NewRule> k;
    k.w.chains = chains, k.w.wholeP = wholeP, k.w.splitP = splitP;
    k.blocks = blocks, k.maxLen = maxLen;
    k.go(0);
    if (k.r.failedAt) {
        std::printf("chains %d, blocks %d, pairs %d / %d: \"%s\": %s\n", chains, blocks, wholeP, splitP, k.r.first.c_str(), k.r.why.c_str());
        ++failures;
    }
}

// more than 64 tickets: a long random walk over the same operations, blocks reused across the wrap of the ring; before a submit
// takes a slot again the batch that held it is complete (ps_batch_queue_submit waits for it), and so is everything older
void ring_walk(int chains, int blocks, unsigned seed, int steps)
{
    Walk<NewRule> k;
    k.w.chains = chains, k.w.wholeP = 7, k.w.splitP = 12;
    k.blocks = blocks;
    unsigned long long x = seed * 2654435761ull + 1;
    auto rnd = [&](int n) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((x >> 33) % (unsigned)n);
    };
    int mood = 0;
    for (int s = 0; s < steps && !k.r.failedAt; ++s) {
        if (s % 97 == 0) mood = rnd(3); // stretches with few completions fill the ring, stretches with many drain it
        if (rnd(4) <= mood) {
            const int n = (int)k.w.hist.size();
            if (n >= kRing)
                for (int m = 0; m <= n - kRing; ++m)
                    for (int c = 0; c < chains; ++c) k.w.hist[(size_t)m].done[c] = true;
            k.w.trace = "ring walk, batch " + std::to_string(n);
            k.submit(rnd(blocks), rnd(3) == 0);
        } else {
            const int c = rnd(chains), m = k.w.completable(c);
            if (m >= 0) k.w.hist[(size_t)m].done[c] = true;
        }
    }
    if (k.r.failedAt || (int)k.w.hist.size() < 3 * kRing) {
        std::printf("ring walk, chains %d, blocks %d, seed %u, %d batches: %s\n", chains, blocks, seed, (int)k.w.hist.size(),
                    k.r.failedAt ? k.r.why.c_str() : "too few batches to wrap");
        ++failures;
    }
}

// a host that does what the header recommends -- `chains` blocks in turn, so every block stays on one chain -- with the ring full of
// batches in flight: the nominal bounds, and ONE event asked per submit (the predecessor on the block), not one per ticket
void blocks_in_turn_cost_one_query(int chains)
{
    Walk<NewRule> k;
    k.w.chains = chains, k.w.wholeP = 5, k.w.splitP = 12;
    k.blocks = chains;
    for (int n = 0; n < 4 * kRing && !k.r.failedAt; ++n) {
        if (n >= kRing)
            for (int c = 0; c < chains; ++c) k.w.hist[(size_t)(n - kRing)].done[c] = true;
        k.w.trace = "blocks in turn, batch " + std::to_string(n);
        k.submit(n % chains, false);
        const Batch &b = k.w.hist.back();
        if (b.bounds[n % chains + 1] - b.bounds[n % chains] != b.P || !b.waits.empty()) k.r.failedAt = 1, k.r.why = "left its chain";
    }
    if (k.r.failedAt || k.rule.asked > 4 * kRing) {
        std::printf("blocks in turn, chains %d: %s, %lld events asked for %d submits\n", chains, k.r.why.c_str(), k.rule.asked, 4 * kRing);
        ++failures;
    }
}

// the rule the queue had before must be rejected, and first where it went wrong: whole batches only, no completion needed
void old_rule_is_rejected(int chains)
{
    const std::string want = std::string((size_t)chains, 'A') + "BA";
    for (int len = 1; len <= (int)want.size(); ++len) {
        Walk<OldRule> k;
        k.w.chains = chains, k.w.wholeP = 5, k.w.splitP = 12;
        k.blocks = 3, k.maxLen = len, k.splits = false, k.stopAtFailure = true;
        k.go(0);
        const bool expect = len == (int)want.size();
        if ((k.r.failedAt != 0) != expect || (expect && (k.r.first != want || k.r.why.compare(0, 3, "(a)") != 0))) {
            std::printf("the old rule at %d chains, length %d: expected %s, got \"%s\" %s\n", chains, len,
                        expect ? ("the first rejection at " + want).c_str() : "no rejection", k.r.first.c_str(), k.r.why.c_str());
            ++failures;
        }
    }
}

} // namespace

int main(int argc, char **argv)
{
    // the length of the sequences at 4 chains and 3 blocks (about 10^7 of them at 7); never below 6, the shortest failure of the old rule there
    const int len4 = argc > 1 ? std::atoi(argv[1]) : 7;
    if (len4 < 6) {
        std::printf("length at 4 chains must be at least 6\n");
        return 1;
    }
    // whole batches of 5 pairs against split ones of 12: a whole batch meets some chains' shares of a split one and not others;
    // 11 against 12: it meets all but a part of the last
    const int sizes[2][2] = {{5, 12}, {11, 12}};
    for (int chains = 1; chains <= 4; ++chains)
        for (int blocks = 1; blocks <= 3; ++blocks)
            for (int s = 0; s < 2; ++s) exhaustive(chains, blocks, chains == 4 ? len4 : 7, sizes[s][0], sizes[s][1]);
    for (int chains = 1; chains <= 4; ++chains)
        for (int blocks = 1; blocks <= 3; ++blocks)
            for (unsigned seed = 1; seed <= 3; ++seed) ring_walk(chains, blocks, seed, 4000);
    for (int chains = 1; chains <= kQueueMaxChains; ++chains) blocks_in_turn_cost_one_query(chains);
    for (int chains = 2; chains <= 4; ++chains) old_rule_is_rejected(chains);
    if (failures) return 1;
    std::printf("queue hazard ok\n");
    return 0;
}
